"""bench_ts.py -- the transport stream demultiplexer and the ADTS frame table on the device (ohgpu_ts_batch_run, ohgpu_adts_batch_run,
DESIGN.md 5.22): what parse, tables-and-sums and gather cost, and map and chain behind them.

`--streams` streams (256) of one segment of `--seconds` seconds (10) each: ADTS frames of 1024 samples at 44.1 kHz, `--frames-per-pes`
to a PES packet, the tables again every few PES packets, a packet of another PID now and then (tests/ts_cases.py's segment muxer);
every stream is the same bytes at its own place and phase in the source arena.  After `--warmup` runs, `--runs` runs of both batches
on one stream: each phase from device events (medians).  The gather is set against a device-to-device copy of the bytes it delivers,
timed from device events in this same process (the library's own pass-through: a PCM batch that changes nothing); `--host-leg` sets the whole against
tools/ts_host_cpu.cpp, this project's core on `--host-threads` CPU threads (a host pass a caller no longer makes, not the reference's
container).  Every stream's run and frame count are checked against the muxer's.  One JSON line.

    python tools/bench_ts.py --host-leg [--plain] [--out profiles/ts_summary.md]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_leg(one, n_streams, threads):
    build = os.path.join(ROOT, "tools", "build")
    os.makedirs(build, exist_ok=True)
    exe, text = os.path.join(build, "ts_host_cpu"), os.path.join(ROOT, "tools", "ts_host_cpu.cpp")
    core = os.path.join(ROOT, "ohpipeline_amd", "csrc", "ts_packet_core.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(text), os.path.getmtime(core)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", text, "-o", exe])
    with tempfile.NamedTemporaryFile(suffix=".ts") as f:
        f.write(one)
        f.flush()
        delivered, frames, ms = subprocess.run([exe, f.name, str(n_streams), str(threads), "5"], capture_output=True, text=True, timeout=900, check=True).stdout.split()
    return int(delivered), int(frames), float(ms)


def copy_ms(ctx, n_streams, nbytes, warmup, runs):
    """A device-to-device copy of n_streams runs of nbytes in this process, from device events, median of `runs`: the library's own
    pass-through -- a PCM batch of one message a stream that changes nothing (32-bit little-endian mono to the same), which the line
    kernel serves as a plain copy through 16-byte loads and stores."""
    from ohpipeline_amd import capi
    frames, slot = nbytes // 4, (nbytes + 255) // 256 * 256
    descs = np.zeros(n_streams, dtype=capi.MSG_DESC)
    for i in range(n_streams):
        d = descs[i]
        d["src_offset"], d["dst_offset"], d["n_frames"], d["attenuation"] = i * slot, i * slot, frames, capi.UNITY_ATTENUATION
        d["channels"], d["src_bits"], d["src_endian"], d["dst_bits"], d["dst_endian"] = 1, 32, capi.ENDIAN_LITTLE, 32, capi.ENDIAN_LITTLE
    d_a, d_b = ctx.malloc(n_streams * slot), ctx.malloc(n_streams * slot)
    ctx.memset(d_a, 0x5A, n_streams * slot)
    b = ctx.pcm_batch(descs, n_streams * slot, n_streams * slot)
    e0, e1 = ctx.event(), ctx.event()
    times = []
    try:
        for k in range(warmup + runs):
            ctx.record(e0)
            ctx.pcm_run(b, d_a, d_b)
            ctx.record(e1)
            ctx.sync()
            times.append(ctx.elapsed_ms(e0, e1))
    finally:
        ctx.batch_destroy(b)
        ctx.event_destroy(e0)
        ctx.event_destroy(e1)
        ctx.free(d_a)
        ctx.free(d_b)
    return float(np.median(times[warmup:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--frames-per-pes", type=int, default=6)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--host-leg", action="store_true")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import ts_cases as TC
    from ohpipeline_amd import capi
    n_frames = int(args.seconds * 44100 / 1024)
    packets, es = TC.segment(TC.Lcg(44100), n_frames, frames_per_pes=args.frames_per_pes, tables_every=8, payload=(300, 440))
    one = b"".join(packets)
    n, size, room = args.streams, len(one), len(packets) * 184
    slot, out_slot = (size + 255) // 256 * 256 + 48, (room + 255) // 256 * 256 + 48
    src = np.zeros(n * slot + 16, dtype=np.uint8)
    ts = np.zeros(n, dtype=capi.TS_STREAM_DESC)
    ad = np.zeros(n, dtype=capi.ADTS_STREAM_DESC)
    for i in range(n):
        a = i * slot + i % 16
        src[a:a + size] = np.frombuffer(one, dtype=np.uint8)
        ts[i]["src_offset"], ts[i]["src_bytes"], ts[i]["dst_offset"], ts[i]["dst_capacity"] = a, size, i * out_slot + (i * 5) % 16, room
        ad[i]["src_offset"], ad[i]["src_bytes"], ad[i]["flags"] = ts[i]["dst_offset"], len(es), capi.ADTS_RECOGNISE
    capi.ts_batch_check(ts, 0, src.size, n * out_slot + 16)
    with capi.Context(0) as ctx:
        d_src, d_dst = ctx.upload(src), ctx.malloc(n * out_slot + 16)
        ctx.set_kernel_variant(1 if args.plain else 0)
        try:
            b = ctx.ts_batch(ts, 0, src.size, n * out_slot + 16)
            a = ctx.adts_batch(ad, 0, n * out_slot + 16)
        finally:
            ctx.set_kernel_variant(0)
        phases, walls = [], []
        try:
            for k in range(args.warmup + args.runs):
                t0 = time.perf_counter()
                ctx.ts_run(b, d_src, d_dst)
                ctx.adts_run(a, d_dst)
                tres, _ = ctx.ts_results(b, n, 0)
                ares, _ = ctx.adts_results(a, n, 0)
                walls.append((time.perf_counter() - t0) * 1e3)
                phases.append(ctx.ts_phase_ms(b) + ctx.adts_phase_ms(a))
            allocs = ctx.device_allocations()
            ctx.ts_run(b, d_src, d_dst)
            ctx.adts_run(a, d_dst)
            ctx.ts_results(b, n, 0)
            steady = ctx.device_allocations() == allocs
            got = ctx.download(d_dst, n * out_slot + 16)
            paths = ctx.ts_paths(b)
        finally:
            ctx.batch_destroy(b)
            ctx.batch_destroy(a)
            ctx.free(d_src)
            ctx.free(d_dst)
        device = ctx.name()
        d2d = copy_ms(ctx, n, len(es), args.warmup, args.runs)
    want = np.frombuffer(es, dtype=np.uint8)
    ok = bool(np.all(tres["status"] == capi.TS_OK) and np.all(tres["bytes_delivered"] == want.size) and np.all(ares["frames"] == n_frames))
    for i in range(n):
        o = int(ts[i]["dst_offset"])
        ok = ok and np.array_equal(got[o:o + want.size], want)
    ms = np.median(np.array(phases[args.warmup:]), axis=0)
    out = dict(bench="ts", device=device, route=paths["route"], streams=n, stream_bytes=size, packets_a_stream=len(packets), frames_a_stream=n_frames,
               source_mb=round(n * size / 1e6, 1), delivered_mb=round(n * want.size / 1e6, 1), parse_ms=round(float(ms[0]), 4), sums_ms=round(float(ms[1]), 4),
               gather_ms=round(float(ms[2]), 4), adts_map_ms=round(float(ms[3]), 4), adts_chain_ms=round(float(ms[4]), 4),
               run_and_results_ms=round(float(np.median(walls[args.warmup:])), 4), copy_same_bytes_ms=round(d2d, 4),
               gather_over_copy=round(float(ms[2]) / d2d, 3) if d2d > 0 else None, gather_tbps=round(2 * n * want.size / (float(ms[2]) * 1e-3) / 1e12, 4) if ms[2] > 0 else None,
               check=ok, steady_state_allocates_nothing=steady)
    if args.host_leg:
        delivered, frames, host_ms = host_leg(one, n, args.host_threads)
        out["host_leg"] = dict(own_core_on_cpu_ms=round(host_ms, 2), threads=args.host_threads, matches=delivered == want.size and frames == n_frames,
                               note="this project's core on the CPU (demux and chain, serial text): a host pass the caller no longer makes, not the reference")
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n```\n" + line + "\n```\n")


if __name__ == "__main__":
    main()
