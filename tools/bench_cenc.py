"""Protected fragmented MPEG-4 on the device (ohgpu_cenc_*): 256 streams of two minutes of 4096-sample fLaC frames under
256 keys in one batch, the shape of tools/bench_mp4f.py (whose file maker this imports): the files at every address mod 16, the clear
runs written to every address mod 16, the arenas larger than the 256 MiB last-level cache.  The frames are arithmetic patterns of a
FLAC frame's usual size: the layer moves and decrypts bytes, nothing decodes them here.

Figures from one process:
  phases   the six phases of the protected batch (ohgpu_cenc_batch_phase_ms, device events), medians with the lowest and highest after
           a sustain of `--warmup` runs;
  decrypt-gather
           the last phase's payload bytes a second, beside
  gather   ohgpu_mp4f_*'s clear gather of the same samples (the clear file, the same session, the batches taking turns), and beside
           RAOP's CBC decryption (profiles/raop_summary.md: 523 GB/s of payload, as many table reads a block);
  plain    the same job through the plain route (kernel variant 1: one launch, a lane a stream), as a baseline;
  host     libcrypto's AES-128-CTR (EVP, through ctypes) over the same samples on `--host-threads` (16) host threads, wall time --
           where the machine has libcrypto; the figure is left out where it has not.
The files are encrypted with libcrypto where the machine has it (8-byte IVs: the counter starts at 0 and never wraps, so a library's
counter mode and the section's agree), each stream under its own key and kid; without libcrypto every stream carries stream 0's bytes,
encrypted once by the tests' model, under one key.  The first and the last stream are checked against the clear samples, the plain
route's destination arena against the phases'.
  fused    the fused call to PCM (ohgpu_cenc_flac_process_host) beside the clear fused call (ohgpu_mp4f_flac_process_host), wall time of
           the host-buffer calls: the big job's frames are patterns that do not decode, so this one figure takes `--fused-lanes` (256)
           lanes of a committed FLAC fixture (tests/golden/flac, cut into fragments, encrypted once by the tests' model, one key) -- a
           small job, mostly the calls' fixed cost; the PCM of both must be equal.

    python tools/bench_cenc.py [--out profiles/cenc_summary.md]
"""
import argparse
import ctypes
import ctypes.util
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RAOP_GBPS = 523.0          # profiles/raop_summary.md: the CBC decrypt phase, payload bytes a second


class Libcrypto:
    """AES-128-CTR through EVP; None where the machine has no libcrypto"""

    @staticmethod
    def load():
        name = ctypes.util.find_library("crypto")
        try:
            lib = ctypes.CDLL(name) if name else None
            if lib is None or not hasattr(lib, "EVP_aes_128_ctr"):
                return None
        except OSError:
            return None
        lib.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
        lib.EVP_aes_128_ctr.restype = ctypes.c_void_p
        lib.EVP_EncryptInit_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
        lib.EVP_EncryptUpdate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int]
        lib.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
        out = Libcrypto()
        out.lib = lib
        return out

    def crypt_samples(self, key, ivs, buf, places, sizes):
        """in place: every sample [place, + size) of the uint8 array buf under its IV (8 bytes: the counter block's first half)"""
        lib = self.lib
        ctx, cipher, n = lib.EVP_CIPHER_CTX_new(), lib.EVP_aes_128_ctr(), ctypes.c_int(0)
        base = buf.ctypes.data
        for iv, at, size in zip(ivs, places, sizes):
            lib.EVP_EncryptInit_ex(ctx, cipher, None, key, iv + bytes(8))
            lib.EVP_EncryptUpdate(ctx, base + at, ctypes.byref(n), base + at, size)
        lib.EVP_CIPHER_CTX_free(ctx)


def spread(values):
    return f"{statistics.median(values):.4f} ({min(values):.4f} .. {max(values):.4f})"


def fused_job(capi, data, lanes, clear, key, kid):
    """the descriptors of one fused fLaC call over `lanes` copies of a fragmented fixture, filled from the head as a caller would"""
    head = capi.mp4f_head(data) if clear else capi.cenc_head(data)["mp4f"]
    info = head["flac"]
    rows, runs = len(data) // 8, len(data) // 16
    pcm = (int(info["total_samples"]) * int(info["channels"]) * (int(info["bits"]) // 8) + 3) // 4 * 4
    stride = (len(data) + 15) // 16 * 16
    descs = np.zeros(lanes, dtype=capi.MP4F_STREAM_DESC if clear else capi.CENC_STREAM_DESC)
    flac = np.zeros(lanes, dtype=capi.FLAC_STREAM_DESC)
    src = np.zeros(lanes * stride, dtype=np.uint8)
    for i in range(lanes):
        d, f = descs[i], flac[i]
        d["src_offset"], d["src_bytes"], d["codecs"], d["flags"] = i * stride, len(data), 3, capi.MP4F_GATHER
        d["packet_first"], d["packet_capacity"], d["run_first"], d["run_capacity"] = i * rows, rows, i * runs, runs
        d["dst_offset"], d["dst_capacity"] = i * stride, len(data)
        if not clear:
            d["key_flags"], d["kid"], d["key"] = capi.CENC_HAVE_KEY, np.frombuffer(kid, dtype=np.uint8), np.frombuffer(key, dtype=np.uint8)
        f["src_offset"], f["dst_offset"], f["max_samples"] = i * stride, i * pcm, int(info["total_samples"])
        f["sample_rate"], f["max_blocksize"], f["blocksize"] = int(info["sample_rate"]), int(info["max_blocksize"]), int(info["max_blocksize"])
        f["channels"], f["bits"], f["flags"] = int(info["channels"]), int(info["bits"]), capi.FLAC_FLAG_AT_FRAME | capi.FLAC_OUT_PACKED_BE
        src[i * stride:i * stride + len(data)] = np.frombuffer(data, dtype=np.uint8)
    return descs, flac, lanes * rows, lanes * runs, src, lanes * stride, np.zeros(lanes * pcm, dtype=np.uint8)


def fused_times(ctx, capi, CC, FC, lanes, runs, warmup):
    """-> (protected ms, clear ms, lanes' PCM bytes): wall times of the two fused calls over the same fixture, the calls taking turns"""
    name = "s16_stereo_44k1_b1152_l5"
    jobs = {"protected": (ctx.cenc_flac_process_host, fused_job(capi, CC.flac_file(name, per_fragment=3).data, lanes, False, CC.KEY, CC.KID)),
            "clear": (ctx.mp4f_flac_process_host, fused_job(capi, FC.flac_file(name, per_fragment=3).data, lanes, True, None, None))}
    ms = {k: [] for k in jobs}
    for turn in range(warmup + runs):
        for k, (call, (descs, flac, n_packets, n_runs, src, mid, dst)) in jobs.items():
            t0 = time.perf_counter()
            out = call(descs, flac, n_packets, n_runs, src, mid, dst)
            if turn >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            assert all(int(r["samples"]) == int(flac[0]["max_samples"]) for r in out[4]), k
    assert np.array_equal(jobs["protected"][1][6], jobs["clear"][1][6]) and jobs["clear"][1][6].any(), "the fused calls' PCM differs"
    return ms["protected"], ms["clear"], jobs["clear"][1][6].size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--minutes", type=float, default=2.0, help="of audio a stream")
    ap.add_argument("--host-threads", type=int, default=16, help="of the libcrypto baseline (at most 16; 0: leave it out)")
    ap.add_argument("--frame-bytes", type=int, default=6000, help="the mean size of a 4096-sample frame")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fused-lanes", type=int, default=256, help="lanes of the fused calls' job (0: leave it out)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.runs < 10 or args.warmup < 3:
        raise SystemExit("at least 10 runs after at least 3 warm-ups")
    import bench_mp4f
    import cenc_cases as CC
    import mp4f_cases as FC
    from ohpipeline_amd import capi
    clear = bench_mp4f.make_file(FC, args.minutes, args.frame_bytes, 7)
    samples = [clear.data[a:a + s] for a, s in zip(clear.offsets, clear.sizes)]
    per = bench_mp4f.FRAGMENT_SECONDS * bench_mp4f.RATE // bench_mp4f.BLOCK
    fragments, frame = [], 0
    for k in range(0, clear.n, per):
        fragments.append(FC.fragment([FC.run(samples[k:k + per], [bench_mp4f.BLOCK] * len(samples[k:k + per]), fields="size")], tfhd_duration=bench_mp4f.BLOCK, tfdt=(1, frame),
                                     styp=True, sequence=k // per + 1))
        frame += bench_mp4f.BLOCK * per
    crypto = Libcrypto.load()
    init = CC.protected_init(info=FC.streaminfo(max_block=bench_mp4f.BLOCK, total=frame), sinf_options=dict(kid=CC.kid_of(0), iv_size=8))
    m = CC.mux(init, fragments, key=CC.key_of(0), kid=CC.kid_of(0), iv_size=8, protect=crypto is None)       # (with libcrypto: laid out clear, encrypted below)
    assert m.sizes == clear.sizes and m.n == clear.n
    audio, n = sum(m.sizes), args.streams
    kid_at = m.data.index(CC.kid_of(0))
    descs = np.zeros(n, dtype=capi.CENC_STREAM_DESC)
    plain_descs = np.zeros(n, dtype=capi.MP4F_STREAM_DESC)
    stride_src, stride_dst = (len(m.data) + 15) // 16 * 16 + 16, (audio + 15) // 16 * 16 + 16
    src, clear_src = np.zeros(n * stride_src + 16, dtype=np.uint8), np.zeros(n * stride_src + 16, dtype=np.uint8)
    file_bytes, clear_bytes = np.frombuffer(m.data, dtype=np.uint8), np.frombuffer(clear.data, dtype=np.uint8)
    keys = []
    for i in range(n):
        key, kid = (CC.key_of(i), CC.kid_of(i)) if crypto else (CC.key_of(0), CC.kid_of(0))
        keys.append(key)
        for d, length in ((descs[i], len(m.data)), (plain_descs[i], len(clear.data))):
            d["src_offset"], d["src_bytes"], d["codecs"], d["flags"] = i * stride_src + i % 16, length, capi.MP4F_CODEC_FLAC, capi.MP4F_GATHER
            d["packet_first"], d["packet_capacity"], d["run_first"], d["run_capacity"] = i * m.n, m.n, i * len(m.runs), len(m.runs)
            d["dst_offset"], d["dst_capacity"] = i * stride_dst + (i // 16) % 16, audio
        descs[i]["key_flags"], descs[i]["kid"], descs[i]["key"] = capi.CENC_HAVE_KEY, np.frombuffer(kid, dtype=np.uint8), np.frombuffer(key, dtype=np.uint8)
        at = int(descs[i]["src_offset"])
        src[at:at + len(m.data)] = file_bytes
        src[at + kid_at:at + kid_at + 16] = np.frombuffer(kid, dtype=np.uint8)
        clear_src[at:at + len(clear.data)] = clear_bytes
    host_ms = []
    if crypto:
        places = [[int(descs[i]["src_offset"]) + o for o in m.offsets] for i in range(n)]
        with ThreadPoolExecutor(max_workers=16) as pool:                       # the encryption: every stream under its own key
            list(pool.map(lambda i: crypto.crypt_samples(keys[i], m.ivs, src, places[i], m.sizes), range(n)))
        if args.host_threads > 0:                                             # the baseline: the same samples decrypted on the host, into a copy
            threads = min(args.host_threads, 16)
            with ThreadPoolExecutor(max_workers=threads) as pool:
                for _ in range(max(3, args.runs // 3)):
                    work = src.copy()
                    t0 = time.perf_counter()
                    list(pool.map(lambda i: crypto.crypt_samples(keys[i], m.ivs, work, places[i], m.sizes), range(n)))
                    host_ms.append((time.perf_counter() - t0) * 1e3)
            at = int(descs[n - 1]["src_offset"]) + m.offsets[-1]
            assert work[at:at + m.sizes[-1]].tobytes() == samples[-1], "libcrypto's decryption of its own encryption"
    dst_bytes = n * stride_dst + 16
    n_packets, n_runs = n * m.n, n * len(m.runs)
    capi.cenc_batch_check(descs, n_packets, n_runs, src.size, dst_bytes)
    want = np.frombuffer(b"".join(samples), dtype=np.uint8)
    with capi.Context(0) as ctx:
        d_src, d_clear, d_dst = ctx.upload(src), ctx.upload(clear_src), ctx.malloc(dst_bytes)
        batches = {}
        for name, variant in (("phases", 0), ("plain", 1)):
            ctx.set_kernel_variant(variant)
            batches[name] = ctx.cenc_batch(descs, n_packets, n_runs, src.size, dst_bytes)
        ctx.set_kernel_variant(0)
        sibling = ctx.mp4f_batch(plain_descs, n_packets, n_runs, src.size, dst_bytes)
        arenas = {}
        for name, b in batches.items():
            ctx.memset(d_dst, 0xa5, dst_bytes)
            for _ in range(args.warmup):
                ctx.cenc_run(b, d_src, d_dst)
            res, runs, packets, rows = ctx.cenc_results(b, n, n_packets, n_runs)
            arenas[name] = ctx.download(d_dst, dst_bytes).copy()
            for i in (0, n - 1):
                r = res[i]
                assert int(r["mp4f"]["status"]) == capi.MP4F_OK and int(r["mp4f"]["samples_available"]) == m.n and int(r["mp4f"]["bytes_gathered"]) == audio, (name, i, r)
                assert int(r["is_protected"]) == 1 and int(r["blocks"]) == sum((s + 15) // 16 for s in m.sizes)
                at = int(descs[i]["dst_offset"])
                assert np.array_equal(arenas[name][at:at + audio], want), (name, i)
                assert (int(packets[i * m.n + 1]["src_offset"]), int(packets[i * m.n + 1]["bytes"])) == (at + m.sizes[0], m.sizes[1])
        assert np.array_equal(arenas["phases"], arenas["plain"]), "the two routes' destination arenas differ"
        for _ in range(args.warmup):
            ctx.mp4f_run(sibling, d_clear, d_dst)
        ms = {name: [] for name in batches}
        clear_ms = []
        for _ in range(args.runs):
            for name, b in batches.items():
                ctx.cenc_run(b, d_src, d_dst)
                ms[name].append(ctx.cenc_phase_ms(b))
            ctx.mp4f_run(sibling, d_clear, d_dst)
            clear_ms.append(ctx.mp4f_phase_ms(sibling))
        for b in list(batches.values()) + [sibling]:
            ctx.batch_destroy(b)
        fused = fused_times(ctx, capi, CC, FC, args.fused_lanes, args.runs, args.warmup) if args.fused_lanes > 0 else None
        for p in (d_src, d_clear, d_dst):
            ctx.free(p)
        device = ctx.name().strip()
        if device.startswith("("):
            device = device.strip("()")
    phases = list(zip(*ms["phases"]))
    names = ("walk", "run sums", "carries", "expand", "finish", "decrypt-gather")
    crypt = statistics.median(phases[5])
    gather = statistics.median([run[5] for run in clear_ms])
    payload = audio * n
    total = [sum(run) for run in ms["phases"]]
    plain = [run[0] for run in ms["plain"]]
    lines = [f"# Protected fragmented MPEG-4: decrypt-gather ({device})", "",
             f"{n} streams of {args.minutes:g} min of {bench_mp4f.BLOCK}-sample frames in {bench_mp4f.FRAGMENT_SECONDS}-second fragments under {len(set(keys))} keys: {len(m.runs)} runs and "
             f"{m.n} samples a stream, {len(m.data) / 1e6:.2f} MB a file, {payload / 1e9:.3f} GB of payload, {payload // 16 * 1e-6:.1f} M keystream blocks; "
             f"{args.runs} runs after {args.warmup} warm-ups, the batches taking turns; medians (lowest .. highest).", "",
             "| phase | ms |", "|---|---|"]
    lines += [f"| {name} | {spread(values)} |" for name, values in zip(names, phases)]
    lines += [f"| all six | {spread(total)} |", f"| ohgpu_mp4f_*'s clear gather of the same samples | {spread([run[5] for run in clear_ms])} |",
              f"| plain route (one launch, the cipher serial) | {spread(plain)} |"]
    lines += [f"| libcrypto AES-128-CTR on {min(args.host_threads, 16)} host threads (wall) | {spread(host_ms)} |"] if host_ms else \
             ["| libcrypto on host threads | not taken: " + ("left out by --host-threads 0" if crypto else "this machine has no libcrypto") + " |"]
    lines += ["", f"decrypt-gather: {payload / (crypt * 1e-3) / 1e9:.0f} GB/s of payload ({2 * payload / (crypt * 1e-3) / 1e12:.3f} TB/s read + write); the clear gather: "
              f"{payload / (gather * 1e-3) / 1e9:.0f} GB/s of payload; ratio {crypt / gather:.2f} x the clear gather's time; RAOP's CBC decrypt (profiles/raop_summary.md): "
              f"{RAOP_GBPS:.0f} GB/s of payload, ratio {payload / (crypt * 1e-3) / 1e9 / RAOP_GBPS:.2f}",
              f"phases' route against the plain route: {statistics.median(plain) / statistics.median(total):.1f} x" +
              (f"; the decrypt-gather phase against libcrypto on the host threads: {statistics.median(host_ms) / crypt:.0f} x" if host_ms else ""),
              (f"the fused calls to PCM, {args.fused_lanes} lanes of a committed FLAC fixture ({fused[2] / 1e6:.2f} MB of PCM, equal from both), wall ms of the host-buffer "
               f"calls: ohgpu_cenc_flac_process_host {spread(fused[0])}, ohgpu_mp4f_flac_process_host {spread(fused[1])}; a small job, mostly the calls' fixed cost"
               if fused else "the fused calls to PCM: left out by --fused-lanes 0")]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
