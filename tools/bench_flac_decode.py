"""bench_flac_decode.py -- the device FLAC decoder (ohgpu_flac_batch_run) against the host decode it stands in for.

Encodes bench_flac.py's sixteen programmes with the reference's libFLAC 1.2.1 (oracle/_ref, tests/flac_ref.py), lays `--streams`
streams of `--seconds` seconds (stream s plays programme s % 16) into one source arena and decodes them on the device into TInt32
planes: `--sustain` seconds of back-to-back runs first, as bench.py does, then `--steps` timed runs (wall clock around run + results,
the call's host synchronisation and sort included; and each phase from device events).  In the same process the same streams are
decoded by libFLAC on 16 threads -- the figure config 5's `host_decode` reports -- and every stream's device output is checked against
the MD5 in its STREAMINFO.  Prints one JSON line.

    python tools/bench_flac_decode.py --streams 256 --seconds 10
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_flac import PROGRAMMES, RATE, programme  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sustain", type=float, default=1.0)
    ap.add_argument("--variant", type=int, default=0, help="1: the plain route")
    ap.add_argument("--host-threads", type=int, default=16)
    args = ap.parse_args()

    from concurrent.futures import ThreadPoolExecutor

    import flac_ref as F
    from ohpipeline_amd import capi
    if not F.available():
        raise SystemExit("needs oracle/_ref/libflac_ref.so (built by __graft_entry__.build() where the reference tree exists)")
    frames = int(round(args.seconds * RATE))
    encoded = []
    for k in range(PROGRAMMES):
        bits = 16 if k % 2 == 0 else 24
        data = F.encode(programme(k, frames, bits), bits, RATE)
        info, audio = capi.flac_streaminfo(data)
        encoded.append((data, info, audio))
    descs = np.zeros(args.streams, dtype=capi.FLAC_STREAM_DESC)
    parts, at = [], 0
    for s in range(args.streams):
        data, info, audio = encoded[s % PROGRAMMES]
        d = descs[s]
        d["src_offset"], d["src_bytes"] = at, len(data) - audio
        d["dst_offset"], d["dst_plane_stride"] = s * 2 * frames * 4, frames * 4
        d["max_samples"], d["sample_rate"], d["blocksize"], d["max_blocksize"] = frames, RATE, info["max_blocksize"], info["max_blocksize"]
        d["channels"], d["bits"], d["flags"] = 2, info["bits"], capi.FLAC_FLAG_AT_FRAME
        parts.append(np.frombuffer(data, dtype=np.uint8)[audio:])
        at += len(data) - audio
    src = np.concatenate(parts)
    dst_bytes = args.streams * 2 * frames * 4
    total = args.streams * frames

    with capi.Context(0) as ctx:
        ctx.set_kernel_variant(args.variant)
        d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
        ctx.memset(d_dst, 0, dst_bytes)
        b = ctx.flac_batch(descs, src.size, dst_bytes)
        t0, sustained = time.perf_counter(), 0
        while sustained == 0 or time.perf_counter() - t0 < args.sustain:
            ctx.flac_run(b, d_src, d_dst)
            res = ctx.flac_results(b, args.streams)
            sustained += 1
        allocs = ctx.device_allocations()
        walls, phases = [], []
        for _ in range(args.steps):
            t = time.perf_counter()
            ctx.flac_run(b, d_src, d_dst)
            res = ctx.flac_results(b, args.streams)
            walls.append(time.perf_counter() - t)
            phases.append(ctx.flac_phase_ms(b))
        steady = ctx.device_allocations() == allocs
        out = ctx.download(d_dst, dst_bytes).view("<i4").reshape(args.streams, 2, frames)
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
        name = ctx.name()
    ok = bool((res["status"] == capi.FLAC_OK).all() and (res["samples"] == frames).all())
    md5_ok = 0
    for s in range(args.streams):
        info = encoded[s % PROGRAMMES][1]
        nb = info["bits"] // 8
        le = np.ascontiguousarray(out[s].T).view(np.uint8).reshape(-1, 4)[:, :nb]
        md5_ok += hashlib.md5(np.ascontiguousarray(le).tobytes()).digest() == info["md5"]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(args.host_threads) as ex:
        host = list(ex.map(lambda s: F.decode(encoded[s % PROGRAMMES][0])[1], range(args.streams)))
    host_s = time.perf_counter() - t0
    assert all(host)

    wall = float(np.median(walls))
    ph = np.median(np.array(phases), axis=0)
    cands, rejected = int(res["candidates"].sum()), int(res["candidates_rejected"].sum())
    print(json.dumps({
        "what": "FLAC decode, file bytes -> TInt32 planes", "device": name, "route": "plain" if args.variant == 1 else "tuned",
        "streams": args.streams, "seconds": args.seconds, "frames_total": total, "encoded_bytes": int(src.size),
        "flac_frames": int(res["frames"].sum()), "candidates": cands, "candidates_rejected_share": round(rejected / max(cands, 1), 6),
        "device_run_ms": round(wall * 1e3, 3), "device_frames_per_s_M": round(total / wall / 1e6, 1),
        "phase_ms": {"scan": round(float(ph[0]), 3), "probe": round(float(ph[1]), 3), "chain": round(float(ph[2]), 3), "restore": round(float(ph[3]), 3)},
        "phase_frames_per_s_G": {k: round(total / (float(v) * 1e-3) / 1e9, 2) if v > 0 else None for k, v in zip(("scan", "probe", "chain", "restore"), ph)},
        "host_decode": {"decoder": "libFLAC 1.2.1 of the reference tree (oracle/_ref)", "threads": args.host_threads, "seconds": round(host_s, 3),
                        "frames_per_s_M": round(total / host_s / 1e6, 2)},
        "device_over_host": round((total / wall) / (total / host_s), 2),
        "md5_ok_streams": int(md5_ok), "all_ok": bool(ok and md5_ok == args.streams), "steady_state_allocates_nothing": bool(steady),
        "sustain_runs": sustained, "steps": args.steps}))
    return 0 if ok and md5_ok == args.streams else 1


if __name__ == "__main__":
    sys.exit(main())
