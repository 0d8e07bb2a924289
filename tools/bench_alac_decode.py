"""bench_alac_decode.py -- the device Apple Lossless decoder (ohgpu_alac_batch_run), both routes.

`--streams` streams of `--seconds` seconds of 44.1 kHz stereo 16-bit, made by tiling the packets of the committed encoder-made
fixture tests/golden/alac/stereo16_fl4096 (packets are independent, so any sequence of them is a stream; every stream has its own
copy of the bytes and starts at another packet).  Two batches over the same arenas -- the three fused phases over the transposed
scratch, and the plain route (created under kernel variant 1) -- run in ALTERNATING pairs after `--sustain` seconds of back-to-back
runs: wall clock around run + results, and each phase from device events.  Every stream's planes are checked against the PCM the
fixture was encoded from.  Beside them csrc/alac_packet_core.h on `--host-threads` host threads over a slice of the streams
(tools/alac_core_cpu.cpp): the project's own core compiled for the CPU, NOT the reference's decoder, which is not part of this repository.  Prints one JSON line and writes `--out`.

    python tools/bench_alac_decode.py --streams 256 --seconds 10 [--out profiles/alac_decode_summary.md]
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIXTURE = "stereo16_fl4096"
PHASES = ("entropy", "predict", "store")


def cpu_rate(descs, table, src, dst_bytes, threads):
    build = os.path.join(ROOT, "tools", "build")
    os.makedirs(build, exist_ok=True)
    exe, text = os.path.join(build, "alac_core_cpu"), os.path.join(ROOT, "tools", "alac_core_cpu.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(text):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", text, "-o", exe])
    blob = [struct.pack("<IIQQ", len(descs), len(table), src.size, dst_bytes)]
    for d in descs:
        blob.append(struct.pack("<QQIIIIHBBBBBBQ", int(d["dst_offset"]), int(d["dst_plane_stride"]), int(d["first_packet"]), int(d["n_packets"]),
                                int(d["frame_length"]), int(d["sample_rate"]), int(d["max_run"]), int(d["bit_depth"]), int(d["pb"]), int(d["mb"]),
                                int(d["kb"]), int(d["channels"]), int(d["flags"]), 0))
    for s, d in enumerate(descs):
        for k in range(int(d["n_packets"])):
            p = table[int(d["first_packet"]) + k]
            blob.append(struct.pack("<QIIIIQ", int(p["src_offset"]), int(p["bytes"]), s, k, 0, 0))
    path = os.path.join(build, "alac_job.bin")
    with open(path, "wb") as f:
        f.write(b"".join(blob))
        f.write(src.tobytes())
    out = subprocess.check_output([exe, path, str(threads)], text=True)
    os.remove(path)
    return float(out.split()[0])


def workload(capi, fx, streams, per_stream, first_stream=0):
    """descs, packet table, source arena, destination bytes for `streams` streams of `per_stream` packets"""
    cfg, full = fx["cfg"], [p for k, p in enumerate(fx["packets"]) if k < len(fx["packets"]) - 1]
    fl, ch = cfg["frame_length"], cfg["channels"]
    descs = np.zeros(streams, dtype=capi.ALAC_STREAM_DESC)
    table = np.zeros(streams * per_stream, dtype=capi.ALAC_PACKET)
    plane = per_stream * fl * 4
    parts, at = [], 0
    for s in range(streams):
        for k in ("frame_length", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "sample_rate"):
            descs[s][k] = cfg[k]
        descs[s]["first_packet"], descs[s]["n_packets"], descs[s]["dst_offset"], descs[s]["dst_plane_stride"] = s * per_stream, per_stream, s * ch * plane, plane
        for k in range(per_stream):
            p = full[(first_stream + s + k) % len(full)]
            table[s * per_stream + k]["src_offset"], table[s * per_stream + k]["bytes"] = at, len(p)
            parts.append(p)
            at += len(p)
    return descs, table, np.frombuffer(b"".join(parts), dtype=np.uint8), streams * ch * plane


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--sustain", type=float, default=1.0)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-streams", type=int, default=32, help="the slice of the streams the CPU build decodes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alac_decode_summary.md"))
    args = ap.parse_args()

    import alac_cases as AC
    from ohpipeline_amd import capi
    fx = AC.load_fixture(FIXTURE)
    cfg = fx["cfg"]
    fl, ch, rate = cfg["frame_length"], cfg["channels"], cfg["sample_rate"]
    per_stream = -(-int(round(args.seconds * rate)) // fl)
    descs, table, src, dst_bytes = workload(capi, fx, args.streams, per_stream)
    total = args.streams * per_stream * fl
    n_full = len(fx["packets"]) - 1
    pcm = np.array(fx["samples"], dtype=np.int32)[:n_full * fl].reshape(n_full, fl, ch)
    expected = [np.concatenate([pcm[(r + k) % n_full] for k in range(per_stream)]).T for r in range(n_full)]     # [rotation][channel][sample]

    with capi.Context(0) as ctx:
        d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
        ctx.memset(d_dst, 0, dst_bytes)
        batches = {}
        for route, variant in (("fused", 0), ("plain", 1)):
            ctx.set_kernel_variant(variant)
            batches[route] = ctx.alac_batch(descs, table, src.size, dst_bytes)
            assert ctx.batch_paths(batches[route])["alac_route"] == (capi.ALAC_ROUTE_PLAIN if variant else capi.ALAC_ROUTE_FUSED)
        ctx.set_kernel_variant(0)
        t0, sustained = time.perf_counter(), 0
        while sustained == 0 or time.perf_counter() - t0 < args.sustain:
            ctx.alac_run(batches["fused"], d_src, d_dst)
            ctx.alac_results(batches["fused"], args.streams, len(table))
            sustained += 1
        allocs = ctx.device_allocations()
        walls, phases, ok = {"fused": [], "plain": []}, {"fused": [], "plain": []}, True
        checked = {}
        for _ in range(args.pairs):
            for route in ("fused", "plain"):
                if route not in checked:
                    ctx.memset(d_dst, 0, dst_bytes)
                    ctx.sync()
                t = time.perf_counter()
                ctx.alac_run(batches[route], d_src, d_dst)
                sres, pres = ctx.alac_results(batches[route], args.streams, len(table))
                walls[route].append(time.perf_counter() - t)
                phases[route].append(ctx.alac_phase_ms(batches[route]))
                ok = ok and bool((pres["status"] == capi.ALAC_OK).all() and (sres["samples"] == per_stream * fl).all())
                if route not in checked:               # every stream's planes against the PCM that was encoded, once per route
                    out = ctx.download(d_dst, dst_bytes).view("<i4").reshape(args.streams, ch, per_stream * fl)
                    checked[route] = sum(bool(np.array_equal(out[s], expected[s % n_full])) for s in range(args.streams))
        steady = ctx.device_allocations() == allocs
        for b in batches.values():
            ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
        name = ctx.name()

    host_streams = min(args.host_streams, args.streams)
    hd, ht, hs, hb = workload(capi, fx, host_streams, per_stream)
    host_rate = cpu_rate(hd, ht, hs, hb, args.host_threads)

    result = {"what": "Apple Lossless decode, packets -> TInt32 planes", "device": name, "streams": args.streams, "seconds": args.seconds,
              "samples_total": total, "packets": int(len(table)), "encoded_bytes": int(src.size), "frame_length": fl}
    for route in ("fused", "plain"):
        wall = float(np.median(walls[route]))
        ph = np.median(np.array(phases[route]), axis=0)
        result[route] = {"run_ms": round(wall * 1e3, 3), "samples_per_s_M": round(total / wall / 1e6, 1),
                         "phase_ms": {k: round(float(v), 3) for k, v in zip(PHASES, ph)}, "streams_equal_to_the_encoded_pcm": int(checked[route])}
    result["fused_over_plain"] = round(result["plain"]["run_ms"] / result["fused"]["run_ms"], 2)
    result["binding_phase_fused"] = max(PHASES, key=lambda k: result["fused"]["phase_ms"][k])
    result["host_core"] = {"what": "csrc/alac_packet_core.h compiled for the CPU (not the reference's decoder)", "threads": args.host_threads,
                           "streams": host_streams, "samples_per_s_M": round(host_rate / 1e6, 2)}
    result["device_over_host_core"] = round(total / (result["fused"]["run_ms"] * 1e-3) / host_rate, 1)
    all_ok = bool(ok and all(checked[r] == args.streams for r in checked))
    result.update({"all_ok": all_ok, "steady_state_allocates_nothing": bool(steady), "sustain_runs": sustained, "pairs": args.pairs})
    print(json.dumps(result))

    lines = ["# Apple Lossless decode on the device (`tools/bench_alac_decode.py`)", "",
             f"{args.streams} streams x {args.seconds:g} s of 44.1 kHz stereo 16-bit ({len(table)} packets of {fl} samples, {src.size / 1e6:.1f} MB of packets, "
             f"{total / 1e6:.1f} M samples per channel), tiled from `tests/golden/alac/{FIXTURE}`; {name}; medians of {args.pairs} alternating pairs "
             f"after {sustained} sustain runs.", "",
             "| route | run + results, ms | M samples/s | entropy ms | predict ms | store ms | streams equal to the encoded PCM |", "|---|---|---|---|---|---|---|"]
    for route in ("fused", "plain"):
        r = result[route]
        lines.append(f"| {route} | {r['run_ms']} | {r['samples_per_s_M']} | {r['phase_ms']['entropy']} | {r['phase_ms']['predict']} | {r['phase_ms']['store']} | "
                     f"{r['streams_equal_to_the_encoded_pcm']} / {args.streams} |")
    lines += ["", f"Fused over plain: {result['fused_over_plain']}x (plain run time / fused run time); the fused route's longest phase is **{result['binding_phase_fused']}**. "
              "The plain route is one kernel: its time is reported under entropy.", "",
              f"`csrc/alac_packet_core.h` compiled for the CPU on {args.host_threads} threads over {host_streams} of the streams: {result['host_core']['samples_per_s_M']} M samples/s "
              f"(device fused route: {result['device_over_host_core']}x).  That is the project's own core, not the reference's decoder: the reference's decoder is not part of this repository, "
              "so no figure for it is given.", "", f"Steady state allocates nothing: {steady}.  Everything OK: {all_ok}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
