"""bench_ogg.py -- the Ogg page layer on the device (ohgpu_ogg_batch_run): what find, verify, chain and gather cost,
and Ogg FLAC through the fused call beside native FLAC.

Demux leg: `--streams` streams of Ogg FLAC, each the frames of a committed fixture (tests/golden/flac, `--fixture`) as packets,
`--repeat` times over, in pages of `--segments` segments (17 segments are the 4 KiB pages an encoder writes); every stream is the same
bytes at its own place in the source arena (the checksums are made in Python, once).  After `--warmup` runs, `--runs` runs: each
phase from device events (medians); bytes per second over the four phases for the algorithm's bytes -- the source read once and
the run written once -- as a fraction of the copy ceiling for the same bytes in the same session (`--run-copy` runs
tools/micro/run_copy as a child process before this process opens the device; `--copy-tbps` takes a figure by hand); the verify
phase's source bytes per second on its own.  Every stream's run is checked against the packets' bytes.  `--host-leg`:
tools/ogg_host_cpu.cpp, this project's own core on `--host-threads` CPU threads (walk, serial checksums, memcpy) -- a host pass a
caller no longer makes, not the reference's library.  `--links`: every stream is that input twice, the second copy under a serial of
its own -- a chain of two links --, walked with OHGPU_OGG_FOLLOW_LINKS and the magic "\x7fFLAC".
Fused leg: `--lanes` lanes, each one fixture once as Ogg FLAC from its first audio page, through ohgpu_ogg_flac_process_host, beside
ohgpu_flac_process_host over the same frames in native framing, alternating, host clock round each call (both end in a wait); the
PCM of both must be equal (`--lanes 0` leaves the leg out, for a counter run).  One JSON line.

    hipcc --offload-arch=gfx950 -O3 -o tools/micro/run_copy tools/micro/run_copy.hip
    python tools/bench_ogg.py --run-copy --host-leg [--out profiles/ogg_summary.md]
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


def copy_ceiling(nbytes):
    """the best float4 copy of tools/micro/run_copy for nbytes each way, TB/s (a child process of its own)"""
    exe = os.path.join(ROOT, "tools", "micro", "run_copy")
    if not os.path.exists(exe):
        raise SystemExit("--run-copy: build tools/micro/run_copy first (the line is in run_copy.hip's header)")
    out = subprocess.run([exe, "40", str(nbytes // 16 * 16)], capture_output=True, text=True, timeout=300, check=True).stdout
    return float(next(l for l in out.splitlines() if l.startswith("best ")).split()[1])


def host_leg(one, n_streams, threads):
    build = os.path.join(ROOT, "tools", "build")
    os.makedirs(build, exist_ok=True)
    exe, text = os.path.join(build, "ogg_host_cpu"), os.path.join(ROOT, "tools", "ogg_host_cpu.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(text):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", text, "-o", exe])
    with tempfile.NamedTemporaryFile(suffix=".ogg") as f:
        f.write(one)
        f.flush()
        delivered, ms = subprocess.run([exe, f.name, str(n_streams), str(threads), "5"], capture_output=True, text=True, timeout=900, check=True).stdout.split()
    return int(delivered), float(ms)


def one_stream(fixture, repeat, segments, links=False):
    import flac_cases as FC
    import ogg_cases as GC
    fx = FC.fixture(fixture)
    packets, _, n_meta = GC.flac_packets(fx)
    audio = packets[n_meta:] * repeat
    pages, run = [], b""
    for serial in (0x464C, 0x464D)[:2 if links else 1]:
        pages += GC.mux(packets[:1], serial, 0, eos=False) + GC.mux(packets[1:n_meta] + audio, serial, 1, max_segments=segments, bos=False)
        run += b"fLaC" + b"".join(packets[:n_meta])[13:] + b"".join(audio)
    return b"".join(pages), run


def demux_leg(ctx, args):
    from ohpipeline_amd import capi
    one, run = one_stream(args.fixture, args.repeat, args.segments, args.links)
    n, size = args.streams, len(one)
    slot = (size + 255) // 256 * 256 + 48                             # (streams at different alignments mod 16 and mod 256)
    src = np.zeros(n * slot, dtype=np.uint8)
    descs = np.zeros(n, dtype=capi.OGG_STREAM_DESC)
    for i in range(n):
        a = i * slot + i % 16
        src[a:a + size] = np.frombuffer(one, dtype=np.uint8)
        descs[i]["src_offset"], descs[i]["src_bytes"], descs[i]["dst_offset"], descs[i]["dst_capacity"] = a, size, i * slot + (i * 5) % 16, size
        descs[i]["serial"], descs[i]["flags"] = 0x464C, capi.OGG_FLAC_MAPPING
        if args.links:
            descs[i]["flags"] |= capi.OGG_FOLLOW_LINKS
            magic = descs[i:i + 1].view(capi.OGG_STREAM_DESC_LINKS)
            magic["link_magic_bytes"], magic["link_magic"][0, :5] = 5, np.frombuffer(b"\x7fFLAC", dtype=np.uint8)
    capi.ogg_batch_check(descs, 0, src.size, src.size)
    d_src, d_dst = ctx.upload(src), ctx.malloc(src.size)
    b = ctx.ogg_batch(descs, 0, src.size, src.size)
    phases, walls = [], []
    try:
        for k in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            ctx.ogg_run(b, d_src, d_dst)
            res, _ = ctx.ogg_results(b, n, 0)
            walls.append((time.perf_counter() - t0) * 1e3)
            phases.append(ctx.ogg_phase_ms(b))
        allocs = ctx.device_allocations()
        ctx.ogg_run(b, d_src, d_dst)
        ctx.ogg_results(b, n, 0)
        steady = ctx.device_allocations() == allocs
        got = ctx.download(d_dst, src.size)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    want = np.frombuffer(run, dtype=np.uint8)
    ok = bool(np.all(res["status"] == capi.OGG_OK) and np.all(res["bytes_delivered"] == want.size))
    ok = ok and bool(np.all(res.view(capi.OGG_STREAM_RESULT_LINKS)["links"] == (1 if args.links else 0)))
    for i in range(n):
        o = int(descs[i]["dst_offset"])
        ok = ok and np.array_equal(got[o:o + want.size], want)
    ms = np.median(np.array(phases[args.warmup:]), axis=0)
    moved = n * (size + want.size)
    tbps = moved / (float(ms.sum()) * 1e-3) / 1e12
    out = dict(streams=n, links_followed=bool(args.links), stream_bytes=size, source_mb=round(n * size / 1e6, 1), pages=int(res["pages"].sum()), packets=int(res["packets"].sum()),
               find_ms=round(float(ms[0]), 4), verify_ms=round(float(ms[1]), 4), chain_ms=round(float(ms[2]), 4), gather_ms=round(float(ms[3]), 4),
               run_and_results_ms=round(float(np.median(walls[args.warmup:])), 4), algorithmic_tbps=round(tbps, 4),
               frac_of_copy=round(tbps / args.copy_tbps, 4) if args.copy_tbps else None,
               verify_source_tbps=round(n * size / (float(ms[1]) * 1e-3) / 1e12, 4), gather_tbps=round(2 * n * want.size / (float(ms[3]) * 1e-3) / 1e12, 4),
               check=ok, steady_state_allocates_nothing=steady)
    if args.host_leg:
        delivered, host_ms = host_leg(one, n, args.host_threads)
        out["host_leg"] = dict(own_core_on_cpu_ms=round(host_ms, 2), threads=args.host_threads, delivered_matches=delivered == want.size,
                               note="this project's core on the CPU (walk, serial checksums, memcpy): a host pass the caller no longer makes, not the reference")
    return out


def fused_leg(ctx, args):
    import flac_cases as FC
    import test_gpu_ogg_flac_to_driver as T
    fx = FC.fixture(args.fixture)
    lane = T.audio_lane(fx, args.segments)
    tick = T.Tick([lane] * args.lanes)
    case = FC.whole(fx, packed=True)
    from ohpipeline_amd import capi
    d = np.zeros(args.lanes, dtype=capi.FLAC_STREAM_DESC)
    audio = np.frombuffer(fx.data[fx.audio:], dtype=np.uint8)
    slot, out_slot = (audio.size + 15) // 16 * 16, (fx.samples * T.frame_bytes(fx) + 3) // 4 * 4
    nsrc, ndst = np.zeros(slot * args.lanes, dtype=np.uint8), np.zeros(out_slot * args.lanes, dtype=np.uint8)
    for i in range(args.lanes):
        nsrc[i * slot:i * slot + audio.size] = audio
        d[i]["src_offset"], d[i]["src_bytes"], d[i]["dst_offset"], d[i]["max_samples"], d[i]["sample_rate"] = i * slot, audio.size, i * out_slot, fx.samples, case.rate
        d[i]["blocksize"], d[i]["max_blocksize"], d[i]["channels"], d[i]["bits"], d[i]["flags"] = case.blocksize, case.max_blocksize, case.channels, case.bits, case.flags
    fused, native = [], []
    for k in range(args.warmup + args.runs):
        t0 = time.perf_counter()
        tick.run(ctx, frames_capacity=0)
        fused.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        res = ctx.flac_process_host(d, nsrc, ndst)
        native.append((time.perf_counter() - t0) * 1e3)
    ok = bool(np.all(tick.fres["samples"] == fx.samples) and np.all(res["samples"] == fx.samples))
    for i in range(args.lanes):
        ok = ok and tick.pcm(i) == ndst[i * out_slot:i * out_slot + fx.samples * T.frame_bytes(fx)].tobytes()
    return dict(lanes=args.lanes, fixture=args.fixture, ogg_bytes_a_lane=len(lane[1]), native_bytes_a_lane=int(audio.size),
                fused_ogg_flac_ms=round(float(np.median(fused[args.warmup:])), 3), native_flac_ms=round(float(np.median(native[args.warmup:])), 3), pcm_equal=ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--lanes", type=int, default=256)
    ap.add_argument("--fixture", default="s16_stereo_44k1_b1152_l5")
    ap.add_argument("--repeat", type=int, default=32)
    ap.add_argument("--segments", type=int, default=17)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copy-tbps", type=float, default=0.0)
    ap.add_argument("--run-copy", action="store_true")
    ap.add_argument("--host-leg", action="store_true")
    ap.add_argument("--links", action="store_true")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from ohpipeline_amd import capi
    if args.run_copy:
        one, run = one_stream(args.fixture, args.repeat, args.segments, args.links)
        args.copy_tbps = copy_ceiling(args.streams * (len(one) + len(run)) // 2)
    with capi.Context(0) as ctx:
        result = dict(bench="ogg", device=ctx.name(), copy_ceiling_tbps=args.copy_tbps or None, demux=demux_leg(ctx, args), ogg_flac=fused_leg(ctx, args) if args.lanes else None)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n```\n" + line + "\n```\n")


if __name__ == "__main__":
    main()
