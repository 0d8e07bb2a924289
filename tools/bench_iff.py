"""PCM files on the device (ohgpu_iff_*): 256 stereo files of a few seconds each, per sample width and byte order.

Per case -- WAV 16, 24, 32 and 32 under a 24-bit limit; AIFF 16, 24 and 32 under a 24-bit limit -- one batch, both phases from
ohgpu_iff_batch_phase_ms (device events), and the convert phase's algorithmic bytes per second: the audio read once and the run written
once.  That is stated as a fraction of the copy ceiling for the same number of bytes in the same session (`--run-copy` runs
tools/micro/run_copy as a child process, before this process opens the device, for the mean of the bytes read and written by the
16-, 24- and 32 -> 24-bit cases; `--copy-tbps` takes figures by hand).  Order of measurement: every batch is run until 0.5 s of launches
have passed (the clock the chip holds under this load), then the cases take turns, `--rounds` times round the whole list, and the
medians are reported with the lowest and highest.  The plain route runs once per case for comparison.  The first and the last
stream of every case are checked against tests/iff_textbook.py.

    hipcc --offload-arch=gfx950 -O3 -o tools/micro/run_copy tools/micro/run_copy.hip
    python tools/bench_iff.py --run-copy [--out profiles/iff_summary.md]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [("WAV 16 (little)", "wav", 2, 24), ("WAV 24 (little)", "wav", 3, 24), ("WAV 32 -> 24 (little)", "wav", 4, 24), ("WAV 32 (little)", "wav", 4, 32),
         ("AIFF 16 (big)", "aiff", 2, 24), ("AIFF 24 (big)", "aiff", 3, 24), ("AIFF 32 -> 24 (big)", "aiff", 4, 24)]


def copy_ceiling(nbytes):
    """the best float4 copy of tools/micro/run_copy for nbytes each way, TB/s (a child process of its own)"""
    exe = os.path.join(ROOT, "tools", "micro", "run_copy")
    if not os.path.exists(exe):
        raise SystemExit("--run-copy: build tools/micro/run_copy first (the line is in run_copy.hip's header)")
    out = subprocess.run([exe, "40", str(nbytes // 16 * 16)], capture_output=True, text=True, timeout=300, check=True).stdout
    return float(next(l for l in out.splitlines() if l.startswith("best ")).split()[1])


def traffic(streams, frames, sample_bytes, limit):
    """(bytes read, bytes written) by the convert phase of a case"""
    return streams * frames * 2 * sample_bytes, streams * frames * 2 * min(sample_bytes, limit // 8)


def make_case(capi, IC, kind, sample_bytes, limit, streams, frames):
    top_first = IC.samples(frames, 2, sample_bytes, 5 + sample_bytes)
    w = IC.wav(top_first, 2, before_fmt=[IC.junk(b"JUNK", 3)]) if kind == "wav" else IC.aiff(top_first, 2, before=[IC.junk(b"NAME", 3)], ssnd_offset=1)
    out_frame = 2 * min(sample_bytes, limit // 8)
    stride_src, stride_dst = (len(w.data) + 15) // 16 * 16 + 16, (frames * out_frame + 15) // 16 * 16 + 16
    descs = np.zeros(streams, dtype=capi.IFF_STREAM_DESC)
    src = np.zeros(streams * stride_src, dtype=np.uint8)
    one = np.frombuffer(w.data, dtype=np.uint8)
    for i in range(streams):
        at = i * stride_src + (3 * i) % 16                                  # files and runs at every address mod 16
        src[at:at + one.size] = one
        d = descs[i]
        d["src_offset"], d["src_bytes"], d["dst_offset"], d["dst_bytes_capacity"] = at, one.size, i * stride_dst + (5 * i) % 16, frames * out_frame
        d["dst_frame_capacity"], d["max_bit_depth"] = frames, limit
    return w, descs, src, streams * stride_dst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--run-copy", action="store_true")
    ap.add_argument("--copy-tbps", default="", help="comma-separated figures for the 16-, 24- and 32 -> 24-bit cases")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    frames = int(args.seconds * 44100)
    ceilings = {}
    if args.run_copy:
        for sample_bytes in (2, 3, 4):
            r, w = traffic(args.streams, frames, sample_bytes, 24)
            ceilings[(sample_bytes, 24)] = copy_ceiling((r + w) // 2)
    elif args.copy_tbps:
        for sample_bytes, v in zip((2, 3, 4), args.copy_tbps.split(",")):
            ceilings[(sample_bytes, 24)] = float(v)

    import iff_cases as IC
    import iff_textbook as IX
    from ohpipeline_amd import capi
    rows, plain_rows, ok, steady = [], [], True, True
    with capi.Context(0) as ctx:
        name = ctx.name()
        live = []
        for label, kind, sample_bytes, limit in CASES:
            w, descs, src, dst_bytes = make_case(capi, IC, kind, sample_bytes, limit, args.streams, frames)
            d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
            ctx.memset(d_dst, 0xA5, dst_bytes)
            ctx.sync()
            batch = ctx.iff_batch(descs, src.size, dst_bytes)
            assert ctx.batch_paths(batch)["iff_route"] == capi.IFF_ROUTE_FUSED
            live.append(dict(label=label, w=w, descs=descs, src=src, dst_bytes=dst_bytes, d_src=d_src, d_dst=d_dst, batch=batch, sample_bytes=sample_bytes, limit=limit,
                             walk=[], convert=[]))
        sustain = 0
        for c in live:                                                       # warm-up: every shape, until the chip holds its clock under this load
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.5:
                for _ in range(8):
                    ctx.iff_run(c["batch"], c["d_src"], c["d_dst"])
                ctx.sync()
                sustain += 8
        allocs = ctx.device_allocations()
        for _ in range(args.rounds):                                         # the cases take turns
            for c in live:
                ctx.iff_run(c["batch"], c["d_src"], c["d_dst"])
                walk, convert = ctx.iff_phase_ms(c["batch"])
                c["walk"].append(walk)
                c["convert"].append(convert)
        steady = ctx.device_allocations() == allocs
        for c in live:
            results = ctx.iff_results(c["batch"], args.streams)
            out_bytes = min(c["sample_bytes"], c["limit"] // 8)
            good = all(int(r["status"]) == capi.IFF_OK and int(r["frames_written"]) == frames for r in results)
            for i in (0, args.streams - 1):
                d = c["descs"][i]
                got = ctx.download(C.c_void_p(c["d_dst"].value + int(d["dst_offset"])), frames * 2 * out_bytes)
                good = good and got.tobytes() == IX.read(c["w"].data, max_bit_depth=c["limit"])["pcm"]
            ok = ok and good
            r, wr = traffic(args.streams, frames, c["sample_bytes"], c["limit"])
            ms = statistics.median(c["convert"])
            tbps = (r + wr) / ms / 1e9
            ceiling = ceilings.get((c["sample_bytes"], c["limit"]))
            rows.append(dict(case=c["label"], walk_ms=round(statistics.median(c["walk"]), 4), convert_ms=round(ms, 4), convert_ms_min=round(min(c["convert"]), 4),
                             convert_ms_max=round(max(c["convert"]), 4), read_mb=round(r / 1e6, 1), written_mb=round(wr / 1e6, 1), tbps=round(tbps, 3),
                             copy_tbps=ceiling, ratio=round(tbps / ceiling, 3) if ceiling else None, checked=good))
            ctx.batch_destroy(c["batch"])
        ctx.set_kernel_variant(1)
        for c in live:                                                       # the plain route: one launch, a lane a stream, for comparison
            batch = ctx.iff_batch(c["descs"], c["src"].size, c["dst_bytes"])
            assert ctx.batch_paths(batch)["iff_route"] == capi.IFF_ROUTE_PLAIN
            ctx.iff_run(batch, c["d_src"], c["d_dst"])
            plain_rows.append(dict(case=c["label"], ms=round(ctx.iff_phase_ms(batch)[0], 3)))
            ctx.batch_destroy(batch)
            ctx.free(c["d_src"])
            ctx.free(c["d_dst"])
        ctx.set_kernel_variant(0)
    result = dict(device=name, streams=args.streams, frames=frames, rounds=args.rounds, sustain_runs=sustain, cases=rows, plain=plain_rows, steady_state_allocates_nothing=steady,
                  everything_checked=ok)
    print(json.dumps(result))
    if args.out:
        lines = [f"# PCM files on the device (`tools/bench_iff.py`)", "",
                 f"{args.streams} stereo files x {args.seconds:g} s at 44.1 kHz ({frames} frames each), files and runs at every address mod 16, written by `tests/iff_cases.py`; "
                 f"{name}; medians of {args.rounds} rounds in which the cases take turns, after {sustain} sustain runs; times from device events "
                 "(`ohgpu_iff_batch_phase_ms`).  Bytes per second count the audio read once and the run written once.  The copy is `tools/micro/run_copy`'s best float4 "
                 "copy of the same number of bytes each way, in a child process of the same session.", "",
                 "| case | walk ms | convert ms (lowest .. highest) | read MB | written MB | convert TB/s | copy TB/s, same session | ratio | first and last stream equal to the model |",
                 "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['case']} | {r['walk_ms']} | {r['convert_ms']} ({r['convert_ms_min']} .. {r['convert_ms_max']}) | {r['read_mb']} | {r['written_mb']} | {r['tbps']} | "
                         f"{r['copy_tbps'] if r['copy_tbps'] else 'not measured'} | {r['ratio'] if r['ratio'] else 'not measured'} | {r['checked']} |")
        lines += ["", "The plain route (one launch, a lane a stream, byte by byte), one run each: " + ", ".join(f"{p['case']} {p['ms']} ms" for p in plain_rows) + ".", "",
                  f"Steady state allocates nothing: {steady}.  Everything checked: {ok}.", ""]
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
