"""bench_vorbis.py -- the Vorbis decoder on the device (ohgpu_vorbis_batch_run): what head, entropy, synthesis and store
cost.

`--streams` streams (64), each the same random-valid stereo stream of tests/vorbis_cases.py (blocks of 256 and 2048, 70 packets) at its
own place in the arenas.  After `--warmup` runs, `--runs` runs: each phase from device events (medians).  The synthesis phase is set
against a device-to-device copy of the bytes it moves (a spectrum row read and written, a block written: 8 bytes a coefficient and 4 a
block sample), timed in this same process by tools/bench_ts.py's pass-through.  `--host-leg` sets the whole against tools/vorbis_host_cpu.cpp, the
core's serial text (its transform is the direct form) on `--host-threads` CPU threads: a host pass a caller no longer makes, not the
reference's decoder.  Every stream's sample count is checked against the model's.  One JSON line.

    python tools/bench_vorbis.py --host-leg [--plain] [--out profiles/vorbis_summary.md]
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def host_leg(st, n_streams, threads):
    build = os.path.join(ROOT, "tools", "build")
    os.makedirs(build, exist_ok=True)
    exe, text = os.path.join(build, "vorbis_host_cpu"), os.path.join(ROOT, "tools", "vorbis_host_cpu.cpp")
    core = os.path.join(ROOT, "ohpipeline_amd", "csrc", "vorbis_core.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(text), os.path.getmtime(core)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off", "-Wall", text, "-o", exe])
    case = struct.pack("<I", len(st.ident)) + st.ident + struct.pack("<I", len(st.setup)) + st.setup + struct.pack("<I", len(st.packets))
    for p in st.packets:
        case += struct.pack("<I", len(p)) + p
    with tempfile.NamedTemporaryFile(suffix=".case") as f:
        f.write(case)
        f.flush()
        samples, _, ms = subprocess.run([exe, f.name, str(n_streams), str(threads), "3"], capture_output=True, text=True, timeout=900, check=True).stdout.split()
    return int(samples), float(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--shape", default="stereo_256_2048")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--host-leg", action="store_true")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import vorbis_cases as VC
    import vorbis_frames as VF
    from bench_ts import copy_ms
    from ohpipeline_amd import capi

    st = VC.stream(args.shape)
    recs, _, pcm = VC.expected(args.shape)
    blob, descs, packets, src, dst_bytes, infos = VF.batch_tables(capi, [st] * args.streams)
    moved = sum(st.model.channels * (r[2] // 2 * 8 + r[2] * 4) for r in recs if r[0] == 0)
    with capi.Context(0) as ctx:
        ctx.set_kernel_variant(1 if args.plain else 0)
        b = ctx.vorbis_batch(descs, packets, blob, src.size, dst_bytes)
        ctx.set_kernel_variant(0)
        d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
        phases = []
        for k in range(args.warmup + args.runs):
            ctx.vorbis_run(b, d_src, d_dst)
            phases.append(ctx.vorbis_phase_ms(b))
        res, _ = ctx.vorbis_results(b, descs.size, packets.size)
        assert (res["samples"] == pcm.shape[1]).all()
        med = np.median(np.array(phases[args.warmup:]), axis=0)
        copy = copy_ms(ctx, args.streams, (moved + 3) // 4 * 4 // 2, args.warmup, args.runs)     # (a copy reads and writes: half the bytes each way)
        route = ctx.batch_paths(b)["vorbis_route"]
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
        out = dict(device=ctx.name(), streams=args.streams, shape=args.shape, route=route, packets=int(packets.size), samples_per_stream=int(pcm.shape[1]),
                   head_ms=float(med[0]), entropy_ms=float(med[1]), synthesis_ms=float(med[2]), store_ms=float(med[3]), synthesis_bytes=int(moved * args.streams),
                   copy_of_synthesis_bytes_ms=copy, synthesis_over_copy=float(med[2] / copy) if copy > 0 else None)
    if args.host_leg:
        samples, ms = host_leg(st, args.streams, args.host_threads)
        assert samples == pcm.shape[1]
        device = out["head_ms"] + out["entropy_ms"] + out["synthesis_ms"] + out["store_ms"]
        out.update(host_threads=args.host_threads, host_ms=ms, device_ms=device, host_over_device=ms / device)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n```json\n" + json.dumps(out, indent=1) + "\n```\n")


if __name__ == "__main__":
    main()
