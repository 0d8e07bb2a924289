"""bench_ohm_rx.py -- the Songcast receiver on the device (ohgpu_ohm_rx_batch_run): what parse, sequence and gather cost.

`--streams` streams of `--frames` 5 ms stereo S24 / 48 kHz frames: 1440 audio bytes behind a 62-byte header (a 4-byte codec name), every
datagram at a multiple of 16 of the source arena -- 256 x 1400 frames are 516 MB of payload in and as much out, well past the caches.
Two shapes: `in_order`, and `mixed`, where a seeded 1 % of the frames arrive up to 150 places late, each with a resent copy behind it.
Per shape, after `--warmup` runs, `--runs` runs: each phase from device events (medians), datagrams per second over the three phases,
the gather's algorithmic bytes (payload read + payload written) per second, as a fraction of 8 TB/s and of the copy ceiling for the
same bytes in the same session: `--run-copy` runs tools/micro/run_copy (built from run_copy.hip: its header has the line) as a
child process for the payload's bytes each way, before this process opens the device, and takes its best float4 copy; `--copy-tbps`
takes a figure by hand instead.  Every stream's run is checked against the payloads in frame order.  `--host-leg` adds, for the
in-order shape, tools/ohm_rx_host_cpu.cpp on `--host-threads` threads: the oracle's parse (oracle/ohp_songcast.h) of every datagram
plus a memcpy of every payload -- a host pass a caller no longer makes, not the reference.  One JSON line.

    hipcc --offload-arch=gfx950 -O3 -o tools/micro/run_copy tools/micro/run_copy.hip
    python tools/bench_ohm_rx.py --streams 256 --frames 1400 --run-copy --host-leg [--out profiles/ohm_rx_summary.md]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

AUDIO, CODEC = 1440, b"PCM "
GRAM = 58 + len(CODEC) + AUDIO
SLOT = (GRAM + 15) // 16 * 16


def copy_ceiling(payload_bytes):
    """the best float4 copy of tools/micro/run_copy for payload_bytes each way, TB/s (a child process of its own)"""
    exe = os.path.join(ROOT, "tools", "micro", "run_copy")
    if not os.path.exists(exe):
        raise SystemExit("--run-copy: build tools/micro/run_copy first (the line is in run_copy.hip's header)")
    out = subprocess.run([exe, "40", str(payload_bytes // 16 * 16)], capture_output=True, text=True, timeout=300, check=True).stdout
    return float(next(l for l in out.splitlines() if l.startswith("best ")).split()[1])


def host_leg(n_streams, n_frames, threads):
    """tools/ohm_rx_host_cpu.cpp: the oracle's parse and a memcpy of every payload on `threads` threads, median of 5, milliseconds"""
    build = os.path.join(ROOT, "tools", "build")
    os.makedirs(build, exist_ok=True)
    exe, text, oracle = os.path.join(build, "ohm_rx_host_cpu"), os.path.join(ROOT, "tools", "ohm_rx_host_cpu.cpp"), os.path.join(ROOT, "oracle")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(text):
        import oracle_lib
        oracle_lib.build()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-I", oracle, text, "-o", exe, "-L", oracle, "-lohp_oracle", "-Wl,-rpath,$ORIGIN/../../oracle"])
    return float(subprocess.run([exe, str(n_streams), str(n_frames), str(threads), "5"], capture_output=True, text=True, timeout=600, check=True).stdout.split()[-1])


def datagram_template(stream, frame, flags):
    import ohm_textbook as OT
    sh = OT.stream_header(0, 48000, 48000 * 48, 0, 24, 2, CODEC)
    return np.frombuffer(OT.audio_frame(flags, 240, frame, 0, 4800, frame * 240, sh, bytes(AUDIO)), dtype=np.uint8).copy()


def build(n_streams, n_frames, mixed, seed=1):
    """-> (source arena, stream table, datagram table, per stream the slot of every frame's first copy)"""
    from ohpipeline_amd import capi
    rng = np.random.default_rng(seed)
    orders = []
    for i in range(n_streams):
        order = list(range(n_frames))
        copies = set()
        if mixed:
            for f in rng.choice(np.arange(1, n_frames), size=max(1, n_frames // 100), replace=False):
                order.remove(int(f))
                order.insert(min(len(order), int(f) + int(rng.integers(2, 150))), int(f))
                copies.add(int(f))
        arrival = []
        for f in order:
            arrival.append((f, False))
            if f in copies:
                arrival.append((f, True))
        orders.append(arrival)
    total = sum(len(a) for a in orders)
    src = np.zeros(total * SLOT, dtype=np.uint8)
    slots = src.reshape(total, SLOT)
    head = datagram_template(0, 0, 2)[:GRAM - AUDIO]
    slots[:, :head.size] = head
    slots[:, head.size:GRAM] = rng.integers(0, 256, size=(total, AUDIO), dtype=np.uint8)
    streams = np.zeros(n_streams, dtype=capi.OHM_RX_STREAM)
    grams = np.zeros(total, dtype=capi.OHM_RX_DATAGRAM)
    grams["src_offset"] = np.arange(total, dtype=np.uint64) * SLOT
    grams["bytes"] = GRAM
    first_of, q, at = [], 0, 0
    for i, arrival in enumerate(orders):
        frames = np.array([f for f, _ in arrival], dtype=np.uint32)
        resent = np.array([c for _, c in arrival], dtype=bool)
        rows = slots[q:q + len(arrival)]
        rows[:, 9] = np.where(resent, 2 | 8, 2)
        rows[:, 12:16] = frames.astype(">u4").view(np.uint8).reshape(-1, 4)
        rows[:, 28:36] = (frames.astype(np.uint64) * 240).astype(">u8").view(np.uint8).reshape(-1, 8)
        s = streams[i]
        s["first_datagram"], s["n_datagrams"], s["dst_offset"], s["dst_capacity"] = q, len(arrival), at, len(arrival) * (GRAM - 58)
        s["last_sample_start"], s["stream_msg_due"] = 0xffffffff, 1
        where = np.zeros(n_frames, dtype=np.int64)
        for k in range(len(arrival) - 1, -1, -1):
            if not resent[k]:
                where[frames[k]] = q + k
        first_of.append(where)
        q += len(arrival)
        at += int(s["dst_capacity"]) + 16
    return src, streams, grams, first_of, at


def measure(ctx, label, n_streams, n_frames, mixed, args):
    from ohpipeline_amd import capi
    src, streams, grams, first_of, dst_bytes = build(n_streams, n_frames, mixed)
    capi.ohm_rx_batch_check(streams, grams, src.size, dst_bytes)
    d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
    b = ctx.ohm_rx_batch(streams, grams, src.size, dst_bytes)
    phases, walls = [], []
    try:
        for k in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            ctx.ohm_rx_run(b, d_src, d_dst)
            sres, _ = ctx.ohm_rx_results(b, n_streams, 0)
            walls.append((time.perf_counter() - t0) * 1e3)
            phases.append(ctx.ohm_rx_phase_ms(b))
        allocs = ctx.device_allocations()
        ctx.ohm_rx_run(b, d_src, d_dst)
        ctx.ohm_rx_results(b, n_streams, 0)
        steady = ctx.device_allocations() == allocs
        got = ctx.download(d_dst, dst_bytes)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    ok = bool(np.all(sres["n_output"] == n_frames) and np.all(sres["n_pending"] == 0))
    slots = src.reshape(-1, SLOT)
    for i in range(n_streams):
        want = slots[first_of[i], GRAM - AUDIO:GRAM].reshape(-1)
        o = int(streams[i]["dst_offset"])
        ok = ok and np.array_equal(got[o:o + want.size], want)
    ms = np.median(np.array(phases[args.warmup:]), axis=0)
    payload = n_streams * n_frames * AUDIO
    gather_tbps = 2 * payload / (ms[2] * 1e-3) / 1e12
    out = dict(shape=label, streams=n_streams, frames=n_frames, datagrams=int(grams.size), payload_mb=round(payload / 1e6, 1),
               parse_ms=round(float(ms[0]), 4), sequence_ms=round(float(ms[1]), 4), gather_ms=round(float(ms[2]), 4),
               run_and_results_ms=round(float(np.median(walls[args.warmup:])), 4), datagrams_per_s=round(grams.size / (float(ms.sum()) * 1e-3)),
               sequence_ns_per_datagram=round(float(ms[1]) * 1e6 / grams.size, 2), gather_algorithmic_tbps=round(gather_tbps, 3),
               gather_frac_of_8TBps=round(gather_tbps / 8.0, 4), gather_frac_of_copy=round(gather_tbps / args.copy_tbps, 4) if args.copy_tbps else None,
               check=ok, steady_state_allocates_nothing=steady)
    if args.host_leg and not mixed:
        out["host_leg"] = dict(oracle_parse_and_memcpy_ms=round(host_leg(n_streams, n_frames, args.host_threads), 2), threads=args.host_threads,
                               note="the oracle's parse and memcpy: a host pass the caller no longer makes, not the reference")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1400)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copy-tbps", type=float, default=0.0)
    ap.add_argument("--run-copy", action="store_true")
    ap.add_argument("--host-leg", action="store_true")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from ohpipeline_amd import capi
    if args.run_copy:
        args.copy_tbps = copy_ceiling(args.streams * args.frames * AUDIO)
    with capi.Context(0) as ctx:
        result = dict(bench="ohm_rx", device=ctx.name(), copy_ceiling_tbps=args.copy_tbps or None, shapes=[measure(ctx, "in_order", args.streams, args.frames, False, args),
                                                                 measure(ctx, "mixed_1pct_late", args.streams, args.frames, True, args)])
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n```\n" + line + "\n```\n")


if __name__ == "__main__":
    main()
