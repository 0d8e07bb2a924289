"""DSD files on the device (ohgpu_dsd_file_*): 256 DSF and 256 DFF streams of DSD64 in one batch, files at every
address mod 16, sized so that the arenas exceed the 256 MiB last-level cache.

Three figures from one process, and the ratio of each pair:
  file     the convert phase of the file batch (ohgpu_dsd_file_batch_phase_ms, device events): the audio read through the byte funnel;
  packer   the existing ohgpu_dsd_batch_run over the same audio placed 16-byte aligned (device events round the launch): the code the
           file layer does not change, on its wide path;
  copy     tools/micro/run_copy's best float4 copy of the same number of bytes each way (`--run-copy` runs it as a child process
           before this process opens the device; `--copy-tbps` takes a figure by hand).
Order of measurement: both batches are warmed up (`--warmup` runs each, at least 3), then they take turns, `--runs` times (at least
10), and the medians are reported with the lowest and highest.  Bytes per second count the audio read once plus the sample
blocks written once, as run_copy counts its read plus its write.  The first and the last stream of either kind are checked against tests/dsd_file_textbook.py on a prefix, and the file
batch's whole destination against the packer's.

    hipcc --offload-arch=gfx950 -O3 -o tools/micro/run_copy tools/micro/run_copy.hip
    python tools/bench_dsd_file.py --run-copy [--out profiles/dsd_file_summary.md]
    python tools/bench_dsd_file.py --copy-tbps T --audio-phase 0      # every stream's audio at one address mod 16
"""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, P = 2, 0                          # the pipeline's plain DSD format: a sample block of two words, no padding
RATE = 2822400                       # DSD64


def copy_ceiling(nbytes):
    """the best float4 copy of tools/micro/run_copy for nbytes each way, TB/s (a child process of its own)"""
    exe = os.path.join(ROOT, "tools", "micro", "run_copy")
    if not os.path.exists(exe):
        raise SystemExit("--run-copy: build tools/micro/run_copy first (the line is in run_copy.hip's header)")
    out = subprocess.run([exe, "40", str(nbytes // 16 * 16)], capture_output=True, text=True, timeout=300, check=True).stdout
    return float(next(l for l in out.splitlines() if l.startswith("best ")).split()[1])


def make_files(FX, pairs, seed):
    """One DSF and one DFF file of `pairs` plane pairs' worth of audio (2048 chunks a pair), the audio random bytes: the headers are the
    tests' writer's, the audio is laid in behind them as it is (the benchmark measures bytes moved, the check below what they become)."""
    rng = np.random.default_rng(seed)
    chunks = pairs * 2048
    audio = rng.integers(0, 256, 4 * chunks, dtype=np.uint8).tobytes()
    head = FX.dsf(b"", b"").data                                        # 92 bytes: DSD, fmt, the data chunk's header
    head = bytearray(head)
    head[12:20] = struct.pack("<Q", len(head) + len(audio))
    head[28 + 36:28 + 44] = struct.pack("<Q", 16 * chunks)
    head[-8:] = struct.pack("<Q", 12 + len(audio))
    dsf = bytes(head) + audio
    head = bytearray(FX.dff(b"", b"", rate=RATE).data)                  # ... FRM8, FVER, PROP, the DSD chunk's header
    head[4:12] = struct.pack(">Q", len(head) - 12 + len(audio))
    head[-8:] = struct.pack(">Q", len(audio))
    dff = bytes(head) + audio
    return dsf, dff, chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256, help="streams of each kind")
    ap.add_argument("--pairs", type=int, default=160, help="DSF plane pairs a stream (2048 chunks, 8 KiB of audio, 11.6 ms of DSD64 each)")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--run-copy", action="store_true")
    ap.add_argument("--copy-tbps", type=float, default=0.0)
    ap.add_argument("--audio-phase", type=int, default=-1, help="every stream's audio at this address mod 16 (default: the files at every address mod 16)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.runs < 10 or args.warmup < 3:
        raise SystemExit("at least 10 runs after at least 3 warm-ups")
    import dsd_file_textbook as FX
    dsf, dff, chunks = make_files(FX, args.pairs, 7)
    audio_bytes = 4 * chunks
    each_way = 2 * args.streams * audio_bytes                           # the batch's audio, read once; (W, P) = (2, 0) writes as many
    moved = 2 * each_way                                                # read plus written: what run_copy's rate counts too
    ceiling = copy_ceiling(each_way) if args.run_copy else (args.copy_tbps or None)

    from ohpipeline_amd import capi
    n = 2 * args.streams
    files = [dsf if i % 2 == 0 else dff for i in range(n)]
    stride_src = (max(len(dsf), len(dff)) + 15) // 16 * 16 + 16
    stride_dst = (audio_bytes + 15) // 16 * 16
    descs = np.zeros(n, dtype=capi.DSD_FILE_STREAM_DESC)
    src = np.zeros(n * stride_src, dtype=np.uint8)
    aligned = np.zeros(n * stride_dst, dtype=np.uint8)                  # the same audio, every run at a multiple of 16: the packer's source
    packer = np.zeros(n, dtype=capi.DSD_DESC)
    heads = [capi.dsd_file_head(f[:4096], W, P) for f in (dsf, dff)]
    for i, f in enumerate(files):
        off = int(heads[i % 2]["data_offset"])
        at = i * stride_src + ((3 * i) % 16 if args.audio_phase < 0 else (args.audio_phase - off) % 16)   # files at every address mod 16
        one = np.frombuffer(f, dtype=np.uint8)
        src[at:at + one.size] = one
        d = descs[i]
        d["src_offset"], d["src_bytes"], d["dst_offset"], d["dst_bytes_capacity"] = at, one.size, i * stride_dst, audio_bytes
        d["sample_block_words"], d["pad_bytes_per_chunk"] = W, P
        aligned[i * stride_dst:i * stride_dst + audio_bytes] = one[off:off + audio_bytes]
        p = packer[i]
        p["src_offset"], p["dst_offset"], p["n_chunks"], p["kind"] = i * stride_dst, i * stride_dst, chunks, capi.DSD_FILE_KIND_DSF if i % 2 == 0 else capi.DSD_FILE_KIND_DFF
        p["sample_block_words"], p["pad_bytes_per_chunk"] = W, P
    dst_bytes = n * stride_dst
    phases = sorted({(int(d["src_offset"]) + int(heads[i % 2]["data_offset"])) % 16 for i, d in enumerate(descs)})

    file_ms, walk_ms, packer_ms = [], [], []
    with capi.Context(0) as ctx:
        name = ctx.name()
        d_src, d_aligned, d_dst, d_dst2 = ctx.upload(src), ctx.upload(aligned), ctx.malloc(dst_bytes), ctx.malloc(dst_bytes)
        for d in (d_dst, d_dst2):
            ctx.memset(d, 0xA5, dst_bytes)
        ctx.sync()
        fb = ctx.dsd_file_batch(descs, src.size, dst_bytes)
        pb = ctx.dsd_batch(packer, aligned.size, dst_bytes)
        assert ctx.batch_paths(fb)["dsd_file_route"] == capi.DSD_FILE_ROUTE_FUSED
        paths = ctx.dsd_batch_paths(pb)
        assert paths["wide_descs"] == n and paths["generic_descs"] == 0, paths
        e0, e1 = ctx.event(), ctx.event()
        for _ in range(args.warmup):
            ctx.dsd_file_run(fb, d_src, d_dst)
            ctx.dsd_run(pb, d_aligned, d_dst2)
        ctx.sync()
        allocs = ctx.device_allocations()
        for _ in range(args.runs):                                          # the two take turns
            ctx.dsd_file_run(fb, d_src, d_dst)
            walk, convert = ctx.dsd_file_phase_ms(fb)
            walk_ms.append(walk)
            file_ms.append(convert)
            ctx.record(e0)
            ctx.dsd_run(pb, d_aligned, d_dst2)
            ctx.record(e1)
            ctx.sync()
            packer_ms.append(ctx.elapsed_ms(e0, e1))
        steady = ctx.device_allocations() == allocs
        results = ctx.dsd_file_results(fb, n)
        got, want = ctx.download(d_dst, dst_bytes), ctx.download(d_dst2, dst_bytes)
        same = bool(np.array_equal(got, want))                              # the file layer's bytes are the packer's
        good = all(int(r["status"]) == capi.DSD_FILE_OK and int(r["chunks_written"]) == chunks for r in results)
        for i in (0, 1, n - 2, n - 1):                                      # ... and the model's, on each kind's first chunks
            m = FX.read(files[i][:int(heads[i % 2]["data_offset"]) + 3 * 8192], W, P)
            good = good and m["chunks_written"] >= 4096 and got[i * stride_dst:i * stride_dst + 4 * 4096].tobytes() == m["blocks"][:4 * 4096]
        ctx.set_kernel_variant(1)
        plain = ctx.dsd_file_batch(descs, src.size, dst_bytes)
        ctx.dsd_file_run(plain, d_src, d_dst)
        plain_ms = ctx.dsd_file_phase_ms(plain)[0]
        ctx.set_kernel_variant(0)
        for b in (fb, pb, plain):
            ctx.batch_destroy(b)
        for e in (e0, e1):
            ctx.event_destroy(e)
        for d in (d_src, d_aligned, d_dst, d_dst2):
            ctx.free(d)

    def row(ms):
        med = statistics.median(ms)
        return dict(ms=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), tbps=round(moved / med / 1e9, 3))
    f, p = row(file_ms), row(packer_ms)
    result = dict(device=name, streams_of_each_kind=args.streams, chunks_per_stream=chunks, mb_each_way=round(each_way / 1e6, 1), source_phases=phases, runs=args.runs,
                  warmup=args.warmup, walk_ms=round(statistics.median(walk_ms), 4), file_convert=f, aligned_packer=p, copy_tbps=ceiling,
                  file_over_packer=round(f["ms"] / p["ms"], 3), file_over_copy=round(f["tbps"] / ceiling, 3) if ceiling else None,
                  packer_over_copy=round(p["tbps"] / ceiling, 3) if ceiling else None, plain_route_ms=round(plain_ms, 3), same_bytes_as_the_packer=same,
                  steady_state_allocates_nothing=steady, everything_checked=good and same)
    print(json.dumps(result))
    if args.out:
        nm = "not measured"
        lines = ["# DSD files on the device (`tools/bench_dsd_file.py`)", "",
                 f"{args.streams} DSF and {args.streams} DFF streams of DSD64 in one batch, {chunks} chunks ({audio_bytes / 1e6:.2f} MB of audio, {chunks * 16 / RATE:.2f} s) each, "
                 f"(W, P) = ({W}, {P}); {each_way / 1e6:.0f} MB read and as many written a run, so neither arena fits the 256 MiB last-level cache; files at every address mod 16 "
                 f"(audio phases {phases}); {name}; medians of {args.runs} runs in which the two batches take turns, after {args.warmup} warm-up runs each; times from device events.  "
                 "The packer is `ohgpu_dsd_batch_run` over the same audio placed 16-byte aligned (every descriptor on its wide path); the copy is `tools/micro/run_copy`'s best "
                 "float4 copy of the same number of bytes each way, in a child process of the same session.", "",
                 "| what | ms (lowest .. highest) | TB/s |", "|---|---|---|",
                 f"| file batch, convert phase (`ohgpu_dsd_file_batch_phase_ms`) | {f['ms']} ({f['ms_min']} .. {f['ms_max']}) | {f['tbps']} |",
                 f"| aligned packer (`ohgpu_dsd_batch_run`) | {p['ms']} ({p['ms_min']} .. {p['ms_max']}) | {p['tbps']} |",
                 f"| copy of the same bytes | | {ceiling if ceiling else nm} |", "",
                 f"Ratios: file convert / aligned packer (time) {result['file_over_packer']}; file convert / copy (rate) {result['file_over_copy'] or nm}; "
                 f"aligned packer / copy (rate) {result['packer_over_copy'] or nm}.  The walk phase: {result['walk_ms']} ms.  The plain route (one launch, a lane a stream, byte by "
                 f"byte), one run: {result['plain_route_ms']} ms.", "",
                 f"The file batch's destination equals the packer's: {same}.  Steady state allocates nothing: {steady}.  Everything checked: {good and same}.", ""]
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
