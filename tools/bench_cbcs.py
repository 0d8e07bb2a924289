"""The second protected fragmented MPEG-4 family on the device (ohgpu_cbcs_*), in the shape of tools/bench_cenc.py (whose
file maker, tools/bench_mp4f.py's, this imports): `--streams` streams of `--minutes` of 4096-sample fLaC frames in one batch, the files at
every address mod 16, the clear runs written to every address mod 16.  The frames are random bytes laid out unencrypted under protection
boxes that say otherwise: the layer moves and decrypts bytes, nothing decodes them here, and what a cipher makes of random bytes costs
what it makes of cipher text.  Each job's plain route must write the phases' route's arena.

Four jobs, each with its six phase times (ohgpu_cbcs_batch_phase_ms, device events; medians with the lowest and highest after `--warmup`
runs) and its decrypt-gather's payload bytes a second:
  cbcs 0:0            whole samples, every whole block through the inverse cipher
  cbcs 1:9            whole samples, one block in ten
  cenc                whole samples, counter mode
  cenc, subsamples    two entries a sample (9 clear bytes, the rest but 4 protected; 4 clear bytes)
And the one comparison that matters: ohgpu_cbcs_* against ohgpu_cenc_* on the same bytes -- the whole-sample `cenc` job -- in the same
process, in alternating pairs; both families must write the same arena.  The figure is the median of the pairs' ratios with their spread.

    python tools/bench_cbcs.py [--out profiles/cbcs_summary.md]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("walk", "run sums", "carries", "expand", "finish", "decrypt-gather")


def spread(values):
    return f"{statistics.median(values):.4f} ({min(values):.4f} .. {max(values):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--minutes", type=float, default=1.0, help="of audio a stream")
    ap.add_argument("--frame-bytes", type=int, default=6000, help="the mean size of a 4096-sample frame")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.runs < 10 or args.warmup < 3:
        raise SystemExit("at least 10 runs after at least 3 warm-ups")
    import bench_mp4f
    import cbcs_cases as BC
    import mp4f_cases as FC
    from ohpipeline_amd import capi
    clear = bench_mp4f.make_file(FC, args.minutes, args.frame_bytes, 7)
    samples = [clear.data[a:a + s] for a, s in zip(clear.offsets, clear.sizes)]
    per = bench_mp4f.FRAGMENT_SECONDS * bench_mp4f.RATE // bench_mp4f.BLOCK
    counts = [min(per, clear.n - k) for k in range(0, clear.n, per)]
    two = lambda i, size: [(9, size - 13), (4, 0)]
    how = {"cbcs 0:0": dict(iv_size=16, listed=False), "cbcs 1:9": dict(pattern=(1, 9), constant_iv=bytes(range(16)), senc=None),
           "cenc": dict(scheme=BC.CENC, iv_size=8, listed=False), "cenc, subsamples": dict(scheme=BC.CENC, iv_size=8, layout=two)}
    files = {name: BC.build(None, samples=samples, durations=[bench_mp4f.BLOCK] * clear.n, counts=counts, init=dict(info=FC.streaminfo(max_block=bench_mp4f.BLOCK)),
                            protect_samples=False, **options) for name, options in how.items()}
    n, audio = args.streams, sum(clear.sizes)
    stride_dst = (audio + 15) // 16 * 16 + 16
    dst_bytes = n * stride_dst + 16
    rows, table = [], {}
    with capi.Context(0) as ctx:
        d_dst = ctx.malloc(dst_bytes)
        for name, m in files.items():
            stride_src = (len(m.data) + 15) // 16 * 16 + 16
            src = np.zeros(n * stride_src + 16, dtype=np.uint8)
            descs = np.zeros(n, dtype=capi.CBCS_STREAM_DESC)
            for i in range(n):
                d = descs[i]
                d["src_offset"], d["src_bytes"], d["codecs"], d["flags"] = i * stride_src + i % 16, len(m.data), capi.MP4F_CODEC_FLAC, capi.MP4F_GATHER
                d["packet_first"], d["packet_capacity"], d["run_first"], d["run_capacity"] = i * m.n, m.n, i * len(m.runs), len(m.runs)
                d["dst_offset"], d["dst_capacity"] = i * stride_dst + (i // 16) % 16, audio
                d["subsample_first"], d["subsample_capacity"] = i * m.subsamples, m.subsamples
                d["key_flags"], d["kid"], d["key"] = capi.CENC_HAVE_KEY, np.frombuffer(m.kid, dtype=np.uint8), np.frombuffer(BC.key_of(i), dtype=np.uint8)
                src[int(d["src_offset"]):int(d["src_offset"]) + len(m.data)] = np.frombuffer(m.data, dtype=np.uint8)
            n_packets, n_runs, n_subs = n * m.n, n * len(m.runs), n * m.subsamples
            d_src = ctx.upload(src)
            batches, arenas = {}, {}
            for route, variant in (("phases", 0), ("plain", 1)):
                ctx.set_kernel_variant(variant)
                batches[route] = ctx.cbcs_batch(descs, n_packets, n_runs, n_subs, src.size, dst_bytes)
            ctx.set_kernel_variant(0)
            if name == "cenc":                                                # the sibling family on the same bytes
                sibling_descs = np.zeros(n, dtype=capi.CENC_STREAM_DESC)
                for k in capi.CENC_STREAM_DESC.names:
                    sibling_descs[k] = descs[k]
                batches["sibling"] = ctx.cenc_batch(sibling_descs, n_packets, n_runs, src.size, dst_bytes)
            for route, b in batches.items():
                ctx.memset(d_dst, 0xa5, dst_bytes)
                for _ in range(args.warmup if route != "plain" else 1):
                    (ctx.cenc_run if route == "sibling" else ctx.cbcs_run)(b, d_src, d_dst)
                res = (ctx.cenc_results if route == "sibling" else ctx.cbcs_results)(b, n, n_packets, n_runs)[0]
                head = res["mp4f"] if route == "sibling" else res["cenc"]["mp4f"]
                assert (head["status"] == capi.MP4F_OK).all() and (head["samples_available"] == m.n).all() and (head["bytes_gathered"] == audio).all(), (name, route)
                arenas[route] = ctx.download(d_dst, dst_bytes).copy()
            assert all(np.array_equal(arenas["phases"], a) for a in arenas.values()), f"{name}: the routes' (or the families') destination arenas differ"
            blocks = int(res["blocks"][0]) if "sibling" in batches else int(ctx.cbcs_results(batches["phases"], n, n_packets, n_runs)[0]["cenc"]["blocks"][0])
            ms, sibling_ms = [], []
            for _ in range(args.runs):                                        # alternating pairs where there is a sibling
                ctx.cbcs_run(batches["phases"], d_src, d_dst)
                ms.append(ctx.cbcs_phase_ms(batches["phases"]))
                if "sibling" in batches:
                    ctx.cenc_run(batches["sibling"], d_src, d_dst)
                    sibling_ms.append(ctx.cenc_phase_ms(batches["sibling"]))
            ctx.cbcs_run(batches["plain"], d_src, d_dst)
            plain_ms = ctx.cbcs_phase_ms(batches["plain"])[0]
            for b in batches.values():
                ctx.batch_destroy(b)
            ctx.free(d_src)
            phases = list(zip(*ms))
            crypt = statistics.median(phases[5])
            table[name] = phases
            rows.append(f"| {name} | {m.subsamples} | {blocks * n / 1e6:.2f} | {spread(phases[5])} | {audio * n / (crypt * 1e-3) / 1e9:.0f} | {spread([sum(r) for r in ms])} | {plain_ms:.2f} |")
            if sibling_ms:
                ratios = [a[5] / b[5] for a, b in zip(ms, sibling_ms)]
                totals = [sum(a) / sum(b) for a, b in zip(ms, sibling_ms)]
                pair = (spread([r[5] for r in sibling_ms]), spread(ratios), spread(totals), audio * n / (statistics.median([r[5] for r in sibling_ms]) * 1e-3) / 1e9)
        ctx.free(d_dst)
        device = ctx.name().strip().strip("()")
    lines = [f"# Protected fragmented MPEG-4, `cbcs` and subsamples: decrypt-gather ({device})", "",
             f"{n} streams of {args.minutes:g} min of {bench_mp4f.BLOCK}-sample frames in {bench_mp4f.FRAGMENT_SECONDS}-second fragments, a key a stream: {clear.n} samples and "
             f"{audio / 1e6:.2f} MB of payload a stream, {audio * n / 1e9:.3f} GB a batch; {args.runs} runs after {args.warmup} warm-ups; medians (lowest .. highest), ms.", "",
             "| job | entries a stream | M cipher blocks | decrypt-gather ms | GB/s of payload | all six phases ms | plain route ms (one run) |", "|---|---|---|---|---|---|---|"] + rows
    lines += ["", "| phase | " + " | ".join(table) + " |", "|---|" + "---|" * len(table)]
    lines += [f"| {phase} | " + " | ".join(spread(table[name][k]) for name in table) + " |" for k, phase in enumerate(NAMES)]
    lines += ["", f"ohgpu_cbcs_* against ohgpu_cenc_* on the same bytes (whole-sample `cenc`, the same arena from both), {args.runs} alternating pairs: the sibling's decrypt-gather "
              f"{pair[0]} ms ({pair[3]:.0f} GB/s of payload); ratio of the decrypt-gather phases, new family over old, {pair[1]}; ratio of all six phases {pair[2]}."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
