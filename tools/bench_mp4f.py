"""Fragmented MPEG-4 on the device (ohgpu_mp4f_*): 256 streams of fLaC in 4-second fragments of 4096-sample frames in one
batch, the files at every address mod 16 and gathered to every address mod 16, sized so that the arenas exceed the 256 MiB last-level
cache.  The frames are arithmetic patterns of a FLAC frame's usual size (nothing decodes them here: the layer moves bytes).

Figures from one process:
  phases   the six phases of the batch (ohgpu_mp4f_batch_phase_ms, device events), medians with the lowest and highest;
  gather   the gather phase's bytes a second -- the samples' bytes read once and written once, as run_copy counts its read plus its
           write -- beside
  copy     tools/micro/run_copy's best float4 copy of the same number of bytes each way (`--run-copy` runs it as a child process
           before this process opens the device; `--copy-tbps` takes a figure by hand);
  plain    the same job through the plain route (kernel variant 1: one launch, a lane a stream), as a baseline;
  host     the same job through the core's serial text on `--host-threads` (16) host threads: tools/mp4f_serial.cpp, built here with
           g++ -O2 and run as a child process before this process opens the device, the medians of `--runs` wall times.
Order of measurement: both batches are warmed up (`--warmup` runs each, at least 3), then they take turns, `--runs` times (at least
10).  The first and the last stream are checked against the muxer's own record (tests/mp4f_cases.py) -- every run row, the first and last
sample rows, the gathered bytes -- and the plain route's destination arena against the phases'.

    hipcc --offload-arch=gfx950 -O3 -o tools/micro/run_copy tools/micro/run_copy.hip
    python tools/bench_mp4f.py --run-copy [--out profiles/mp4f_summary.md]
"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RATE, BLOCK, FRAGMENT_SECONDS = 44100, 4096, 4


def copy_ceiling(nbytes):
    """the best float4 copy of tools/micro/run_copy for nbytes each way, TB/s (a child process of its own)"""
    exe = os.path.join(ROOT, "tools", "micro", "run_copy")
    if not os.path.exists(exe):
        raise SystemExit("--run-copy: build tools/micro/run_copy first (the line is in run_copy.hip's header)")
    out = subprocess.run([exe, "40", str(nbytes // 16 * 16)], capture_output=True, text=True, timeout=300, check=True).stdout
    return float(next(l for l in out.splitlines() if l.startswith("best ")).split()[1])


def host_baseline(data, streams, threads, runs, want):
    """tools/mp4f_serial.cpp over `streams` copies of the file -> the runs' wall times in ms"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe, path = os.path.join(tmp, "mp4f_serial"), os.path.join(tmp, "file.mp4")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "mp4f_serial.cpp"), "-o", exe])
        with open(path, "wb") as f:
            f.write(data)
        out = subprocess.run([exe, path, str(streams), str(threads), str(runs)], capture_output=True, text=True, timeout=900, check=True).stdout.splitlines()
    gathered, ok, first, last = (int(v) for v in out[1].split())
    weighted = int((want.astype(np.uint64) * (np.arange(want.size, dtype=np.uint64) % 65521 + 1)).sum())
    assert gathered == want.size * streams and ok == streams and first == last == weighted, out[1]
    return [float(v) for v in out[0].split()]


def make_file(FC, minutes, frame_bytes, seed):
    rng = np.random.default_rng(seed)
    per_fragment = FRAGMENT_SECONDS * RATE // BLOCK
    fragments, frame = [], 0
    for k in range(int(minutes * 60) // FRAGMENT_SECONDS):
        sizes = rng.integers(frame_bytes * 3 // 4, frame_bytes * 5 // 4, per_fragment)
        samples = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in sizes]
        fragments.append(FC.fragment([FC.run(samples, [BLOCK] * per_fragment, fields="size")], tfhd_duration=BLOCK, tfdt=(1, frame), styp=True, sequence=k + 1))
        frame += BLOCK * per_fragment
    return FC.mux(FC.init_segment(info=FC.streaminfo(max_block=BLOCK, total=frame)), fragments)


def spread(values):
    return f"{statistics.median(values):.4f} ({min(values):.4f} .. {max(values):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--minutes", type=float, default=2.0, help="of audio a stream")
    ap.add_argument("--host-threads", type=int, default=16, help="of the host baseline (at most 16; 0: leave it out)")
    ap.add_argument("--frame-bytes", type=int, default=6000, help="the mean size of a 4096-sample frame")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--run-copy", action="store_true")
    ap.add_argument("--copy-tbps", type=float, default=0.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.runs < 10 or args.warmup < 3:
        raise SystemExit("at least 10 runs after at least 3 warm-ups")
    import mp4f_cases as FC
    m = make_file(FC, args.minutes, args.frame_bytes, 7)
    audio = sum(m.sizes)
    copy_tbps = copy_ceiling(audio * args.streams) if args.run_copy else args.copy_tbps
    from ohpipeline_amd import capi
    n = args.streams
    descs = np.zeros(n, dtype=capi.MP4F_STREAM_DESC)
    file_bytes = np.frombuffer(m.data, dtype=np.uint8)
    stride_src, stride_dst = (len(m.data) + 15) // 16 * 16 + 16, (audio + 15) // 16 * 16 + 16
    src = np.zeros(n * stride_src + 16, dtype=np.uint8)
    for i in range(n):
        d = descs[i]
        d["src_offset"], d["src_bytes"], d["codecs"], d["flags"] = i * stride_src + i % 16, len(m.data), capi.MP4F_CODEC_FLAC, capi.MP4F_GATHER
        d["packet_first"], d["packet_capacity"], d["run_first"], d["run_capacity"] = i * m.n, m.n, i * len(m.runs), len(m.runs)
        d["dst_offset"], d["dst_capacity"] = i * stride_dst + (i // 16) % 16, audio
        src[int(d["src_offset"]):int(d["src_offset"]) + len(m.data)] = file_bytes
    dst_bytes = n * stride_dst + 16
    n_packets, n_runs = n * m.n, n * len(m.runs)
    capi.mp4f_batch_check(descs, n_packets, n_runs, src.size, dst_bytes)
    want = np.frombuffer(b"".join(m.data[a:a + s] for a, s in zip(m.offsets, m.sizes)), dtype=np.uint8)
    host = host_baseline(m.data, args.streams, min(args.host_threads, 16), args.runs, want) if args.host_threads > 0 else []
    with capi.Context(0) as ctx:
        d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
        batches = {}
        for name, variant in (("phases", 0), ("plain", 1)):
            ctx.set_kernel_variant(variant)
            batches[name] = ctx.mp4f_batch(descs, n_packets, n_runs, src.size, dst_bytes)
        ctx.set_kernel_variant(0)
        arenas = {}
        for name, b in batches.items():
            ctx.memset(d_dst, 0xa5, dst_bytes)
            for _ in range(args.warmup):
                ctx.mp4f_run(b, d_src, d_dst)
            res, runs, packets, samples = ctx.mp4f_results(b, n, n_packets, n_runs)
            arenas[name] = ctx.download(d_dst, dst_bytes).copy()
            for i in (0, n - 1):
                assert int(res[i]["status"]) == capi.MP4F_OK and int(res[i]["samples_available"]) == m.n and int(res[i]["bytes_gathered"]) == audio, (name, i, res[i])
                base = int(descs[i]["src_offset"])
                mine = runs[i * len(m.runs):(i + 1) * len(m.runs)]
                assert [(int(r["data_offset"]) - base, int(r["first_frame"]), int(r["first_sample"]), int(r["samples"]), int(r["bytes"])) for r in mine] == m.runs
                for s in (0, m.n - 1):
                    assert (int(packets[i * m.n + s]["src_offset"]) - base, int(packets[i * m.n + s]["bytes"])) == (m.offsets[s], m.sizes[s])
                    assert (int(samples[i * m.n + s]["first_frame"]), int(samples[i * m.n + s]["frames"])) == (m.first_frames[s], m.frames[s])
                at = int(descs[i]["dst_offset"])
                assert np.array_equal(arenas[name][at:at + audio], want), (name, i)
        assert np.array_equal(arenas["phases"], arenas["plain"]), "the two routes' destination arenas differ"
        ms = {name: [] for name in batches}
        for _ in range(args.runs):
            for name, b in batches.items():
                ctx.mp4f_run(b, d_src, d_dst)
                ms[name].append(ctx.mp4f_phase_ms(b))
        for b in batches.values():
            ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
        device = ctx.name().strip()
        if device.startswith("("):                                       # (no marketing name: the architecture alone)
            device = device.strip("()")
    phases = list(zip(*ms["phases"]))
    names = ("walk", "run sums", "carries", "expand", "finish", "gather")
    gather = statistics.median(phases[5])
    moved = 2.0 * audio * n
    gather_tbps = moved / (gather * 1e-3) / 1e12
    total = [sum(run) for run in ms["phases"]]
    plain = [run[0] for run in ms["plain"]]
    lines = [f"# Fragmented MPEG-4 demultiplexer ({device})", "",
             f"{n} streams of {args.minutes:g} min of {BLOCK}-sample frames in {FRAGMENT_SECONDS}-second fragments: {len(m.runs)} runs and {m.n} samples a stream, "
             f"{len(m.data) / 1e6:.2f} MB a file, {audio * n / 1e9:.3f} GB gathered; {args.runs} runs after {args.warmup} warm-ups, medians (lowest .. highest).", "",
             "| phase | ms |", "|---|---|"]
    lines += [f"| {name} | {spread(values)} |" for name, values in zip(names, phases)]
    lines += [f"| all six | {spread(total)} |", f"| plain route (one launch) | {spread(plain)} |"] + \
            ([f"| the core's serial text on {min(args.host_threads, 16)} host threads (wall) | {spread(host)} |"] if host else []) + ["",
              f"gather: {gather_tbps:.3f} TB/s (read + write)" + (f"; run_copy's best float4 copy of as many bytes: {copy_tbps:.3f} TB/s; ratio {gather_tbps / copy_tbps:.2f}" if copy_tbps else ""),
              f"phases' route against the plain route: {statistics.median(plain) / statistics.median(total):.1f} x" +
              (f"; against the host threads: {statistics.median(host) / statistics.median(total):.1f} x" if host else "")]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
