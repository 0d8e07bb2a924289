#!/usr/bin/env python3
"""Throughput of DSD -> PCM on one GPU: 256 DSD64 stereo streams x 10 s -> 88.2 kHz, and the same at D = 8 and
D = 64.  Both routes -- the table kernel and the plain per-bit kernel -- in ALTERNATING pairs (fast, plain, fast, plain, ...), HIP
events around each launch, after back-to-back launches until the clock has settled; beside them csrc/dsd_pcm_core.h on 16 host
threads (tools/dsd_pcm_cpu.cpp, over a slice of the workload: it is per bit).  Writes profiles/dsd_pcm_summary.md and prints one JSON
line per case.  "int8 ops" are the multiply-adds the specification asks for (2 * N per output value) against the nominal dense int8
peak -- the table route performs none of them, so the figure is how far the arithmetic's own roofline is, not an occupancy of
the matrix pipe.
Usage: python tools/bench_dsd_pcm.py [--streams 256] [--seconds 10] [--pairs 5] [--out profiles/dsd_pcm_summary.md]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("DSD64 -> 88.2 kHz", 2822400, 88200, 16), ("DSD64 -> 352.8 kHz", 2822400, 352800, 8), ("DSD128 -> 88.2 kHz", 5644800, 88200, 16)]
MSG_FRAMES = 512
INT8_PEAK_TOPS = 4600.0                  # nominal dense int8 peak of the part, tera-ops
HBM_TBPS = 8.0


def cpu_rate(D, T, coef, threads):
    build = os.path.join(ROOT, "tools", "build")
    os.makedirs(build, exist_ok=True)
    exe, src = os.path.join(build, "dsd_pcm_cpu"), os.path.join(ROOT, "tools", "dsd_pcm_cpu.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", src, "-o", exe])
    path = os.path.join(build, f"coef_{D}x{T}.bin")
    coef.astype("<i4").tofile(path)
    out = subprocess.check_output([exe, str(D), str(T), path, str(2 * threads), str(max(256, 2 ** 21 // (D * T))), str(threads)], text=True)
    return float(out.split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--sustain", type=float, default=1.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsd_pcm_summary.md"))
    a = ap.parse_args()
    from ohpipeline_amd import capi
    ctx = capi.Context(0)
    clock = ctx.shader_clock_mhz()
    rows, lines = [], []
    for name, dsd_rate, pcm_rate, T in CASES:
        D, coef = capi.dsd_pcm_design(dsd_rate, pcm_rate, T, 14.0, 20000.0, 1.0)
        N = D * T
        frames = int(a.seconds * pcm_rate) // MSG_FRAMES * MSG_FRAMES
        chunks = frames * D // 16
        stream_bytes, out_bytes = chunks * 4, frames * 6
        one = np.random.default_rng(D).integers(0, 256, size=stream_bytes, dtype=np.uint8)
        d_src, d_dst = ctx.malloc(stream_bytes * a.streams), ctx.malloc(out_bytes * a.streams)
        for s in range(a.streams):                                          # (every stream the same seeded bits, each in its own memory)
            ctx.copy_h2d(capi.C.c_void_p(d_src.value + s * stream_bytes), one)
        ctx.sync()
        per = frames // MSG_FRAMES
        d = np.zeros(a.streams * per, dtype=capi.DSD_PCM_MSG_DESC)
        s_idx, m_idx = np.divmod(np.arange(d.size, dtype=np.uint64), np.uint64(per))
        out0 = m_idx * np.uint64(MSG_FRAMES)
        first = np.maximum((out0.astype(np.int64) + 1) * D - N, 0) // 16
        last = ((out0.astype(np.int64) + MSG_FRAMES) * D - 1) // 16 + 1
        d["src_chunk0"], d["src_chunks"] = first, last - first
        d["src_offset"] = s_idx * np.uint64(stream_bytes) + first.astype(np.uint64) * np.uint64(4)
        d["out_frame0"], d["n_frames"] = out0, MSG_FRAMES
        d["dst_offset"] = s_idx * np.uint64(out_bytes) + out0 * np.uint64(6)
        d["sample_block_words"], d["dst_endian"] = 2, capi.ENDIAN_BIG
        d["flags"] = np.where(m_idx % 8 == 0, capi.FLAG_RAMP, 0)
        d["ramp_start"] = np.where(m_idx % 8 == 0, capi.RAMP_MAX, 0)
        filt = ctx.dsd_pcm_create(D, T, coef)
        ctx.set_kernel_variant(1)
        b_plain = ctx.dsd_pcm_batch(filt, d, stream_bytes * a.streams, out_bytes * a.streams)
        ctx.set_kernel_variant(0)
        b_fast = ctx.dsd_pcm_batch(filt, d, stream_bytes * a.streams, out_bytes * a.streams)
        assert ctx.dsd_pcm_batch_paths(b_fast)["fast_descs"] == d.size and ctx.dsd_pcm_batch_paths(b_plain)["plain_descs"] == d.size
        ctx.dsd_pcm_run(b_plain, d_src, d_dst)
        ctx.sync()
        print(f"# {name}: {d.size} messages, first plain launch done", flush=True)
        t1 = time.perf_counter()
        while time.perf_counter() - t1 < a.sustain:
            for _ in range(4):
                ctx.dsd_pcm_run(b_fast, d_src, d_dst)
            ctx.sync()
        ev = [(ctx.event(), ctx.event(), ctx.event(), ctx.event()) for _ in range(a.pairs)]
        for e in ev:
            ctx.record(e[0]); ctx.dsd_pcm_run(b_fast, d_src, d_dst); ctx.record(e[1])
            ctx.record(e[2]); ctx.dsd_pcm_run(b_plain, d_src, d_dst); ctx.record(e[3])
        ctx.sync()
        fast = [ctx.elapsed_ms(e[0], e[1]) for e in ev]
        plain = [ctx.elapsed_ms(e[2], e[3]) for e in ev]
        for e in ev:
            for x in e:
                ctx.event_destroy(x)
        total = a.streams * frames
        algo_bytes = ctx.batch_info(b_fast)["src_bytes_touched"] + ctx.batch_info(b_fast)["dst_bytes_written"]
        cpu = cpu_rate(D, T, coef, a.threads)
        f_ms, p_ms = float(np.median(fast)), float(np.median(plain))
        row = dict(case=name, D=D, T=T, streams=a.streams, frames_per_stream=frames, fast_ms=round(f_ms, 3), plain_ms=round(p_ms, 3),
                   fast_ms_all=[round(v, 3) for v in fast], plain_ms_all=[round(v, 3) for v in plain],
                   fast_wins_every_pair=bool(all(x < y for x, y in zip(fast, plain))),
                   fast_frames_per_s=round(total / f_ms * 1e3), plain_frames_per_s=round(total / p_ms * 1e3), cpu_frames_per_s=round(cpu),
                   int8_tops_equiv=round(total * 2 * 2 * N / f_ms / 1e9, 2), frac_of_int8_peak=round(total * 2 * 2 * N / f_ms / 1e9 / INT8_PEAK_TOPS, 5),
                   tbps=round(algo_bytes / f_ms / 1e9, 4), frac_of_8TBps=round(algo_bytes / f_ms / 1e9 / HBM_TBPS, 5), shader_clock_mhz=round(clock, 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
        ctx.batch_destroy(b_fast); ctx.batch_destroy(b_plain); ctx.dsd_pcm_destroy(filt)
        ctx.free(d_src); ctx.free(d_dst)
    name_of = ctx.name().strip()
    ctx.close()
    lines.append("# DSD -> PCM: measurement\n")
    lines.append(f"`python tools/bench_dsd_pcm.py` on {name_of}, shader clock {rows[0]['shader_clock_mhz']} MHz; {a.streams} stereo streams x {a.seconds:g} s in messages of "
                 f"{MSG_FRAMES} frames (every eighth ramped), {a.pairs} alternating pairs (fast, plain), medians; device time from HIP events.\n")
    lines.append("| case | D x T | fast ms / launch (all) | plain ms / launch (all) | fast frames/s | plain frames/s | CPU core, "
                 f"{a.threads} threads, frames/s | fast: spec int8 ops/s vs {INT8_PEAK_TOPS:g} T nominal | fast: bytes vs 8 TB/s | fast wins every pair |")
    lines.append("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        lines.append(f"| {r['case']} | {r['D']} x {r['T']} | {r['fast_ms']} ({', '.join(map(str, r['fast_ms_all']))}) | {r['plain_ms']} ({', '.join(map(str, r['plain_ms_all']))}) | "
                     f"{r['fast_frames_per_s']:.3e} | {r['plain_frames_per_s']:.3e} | {r['cpu_frames_per_s']:.3e} | {r['int8_tops_equiv']} T = {r['frac_of_int8_peak']} | "
                     f"{r['tbps']} TB/s = {r['frac_of_8TBps']} | {'yes' if r['fast_wins_every_pair'] else 'NO'} |")
    lines.append("\nThe int8 column counts the multiply-adds the specification asks for (2 N per output value); the table route performs none of them "
                 "(N / 8 look-ups per value), so it says how far the filter's own arithmetic roofline is, not how busy the matrix pipe is. "
                 "The CPU column is `csrc/dsd_pcm_core.h` per bit (tools/dsd_pcm_cpu.cpp) over a slice of the workload.\n")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
