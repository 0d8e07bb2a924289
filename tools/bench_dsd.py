#!/usr/bin/env python3
"""Throughput of the DSD packers, the pass-through and DSD silence on one GPU: back-to-back launches first until the
clock has settled, then HIP events around each timed launch, algorithmic bytes (read once + written once) against the 8 TB/s HBM
peak.  One JSON line per case.  The descriptors are 16-byte aligned, as arenas and DecodedAudio cells are: the wide path.
Usage: python tools/bench_dsd.py [--descs 262144] [--chunks 768] [--case N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--descs", type=int, default=262144)
    ap.add_argument("--chunks", type=int, default=768, help="chunks per descriptor (3072 file bytes: tools/bench_fmt.py's default descriptor is 2880 in, 2880 out); a multiple of 8")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sustain", type=float, default=1.0, help="seconds of back-to-back launches before the timed ones (untimed), so that they see the clock the chip holds under this load")
    ap.add_argument("--case", type=int, default=-1, help="run only this case (profiling runs)")
    a = ap.parse_args()
    from ohpipeline_amd import capi
    ctx = capi.Context(0)
    n, c = a.descs, a.chunks
    assert c % 8 == 0 and c > 0
    cases = [(f"{name} ({W},{P})", kind, W, P, 0) for name, kind in (("DSF packer", capi.DSD_DSF), ("DFF packer", capi.DSD_DFF), ("raw packer", capi.DSD_RAW))
             for W, P in ((2, 0), (6, 2))]
    cases += [("playable pass-through (6,2)", capi.DSD_PASS, 6, 2, 0), ("silence (6,2)", capi.DSD_PASS, 6, 2, capi.DSD_FLAG_SILENCE)]
    if a.case >= 0:
        cases = cases[a.case:a.case + 1]
    # one source arena of seeded bytes and one destination arena serve every case
    plans = []
    for name, kind, W, P, flags in cases:
        # a DSF descriptor is a whole pair of 4096-byte planes (2048 chunks), as a packer converts them; the same bytes in all
        ck = 2048 if kind == capi.DSD_DSF else c
        nk = max(1, n * c // ck)
        in_b, out_b = capi.dsd_layout(kind, W, P, ck)
        plans.append((name, kind, W, P, flags, ck, nk, 0 if flags else (in_b + 15) // 16 * 16, out_b))
    src = np.random.default_rng(1).integers(0, 256, size=max(16, max(p[6] * p[7] for p in plans)), dtype=np.uint8)
    dst_bytes = max(p[6] * p[8] for p in plans)
    d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
    clock = ctx.shader_clock_mhz()
    for name, kind, W, P, flags, c, n, in_slot, out_b in plans:
        d = np.zeros(n, dtype=capi.DSD_DESC)
        d["kind"], d["flags"], d["sample_block_words"], d["pad_bytes_per_chunk"], d["n_chunks"] = kind, flags, W, P, c
        d["src_offset"] = np.arange(n, dtype=np.uint64) * in_slot
        d["dst_offset"] = np.arange(n, dtype=np.uint64) * out_b
        b = ctx.dsd_batch(d, src.size, dst_bytes)
        paths = ctx.dsd_batch_paths(b)
        assert paths == {"wide_descs": n, "generic_descs": 0, "launches": 1}, paths
        ctx.dsd_run(b, d_src, d_dst)
        ctx.sync()
        t1 = time.perf_counter()
        while time.perf_counter() - t1 < a.sustain:                         # steady state first, by the clock (bench.py does the same)
            for _ in range(16):
                ctx.dsd_run(b, d_src, d_dst)
            ctx.sync()
        ev = [(ctx.event(), ctx.event()) for _ in range(a.steps)]
        for e0, e1 in ev:
            ctx.record(e0); ctx.dsd_run(b, d_src, d_dst); ctx.record(e1)
        ctx.sync()
        times = [ctx.elapsed_ms(e0, e1) for e0, e1 in ev]
        ms = sum(times) / len(times)
        algo = n * ((0 if flags else (c * (4 + P) if kind == capi.DSD_PASS else c * 4)) + out_b)
        print(json.dumps(dict(kernel=name, ms_avg=round(ms, 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4),
                              gbps=round(algo / ms / 1e6, 1), frac_of_8TBps=round(algo / ms / 1e6 / 8000.0, 4), descs=n, chunks=c,
                              shader_clock_mhz=round(clock, 1))))
        for e0, e1 in ev:
            ctx.event_destroy(e0); ctx.event_destroy(e1)
        ctx.batch_destroy(b)
    ctx.free(d_src); ctx.free(d_dst)
    ctx.close()


if __name__ == "__main__":
    main()
