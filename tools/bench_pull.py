"""Measures the pulled resampler and prints one JSON line.

bulk:    256 streams of stereo S24, 44.1 -> 48 kHz, 10 s each, every stream at its own pull in +-200 ppm, as ONE batch of
         ohgpu_src_pull_batch_run: kernel time from device events (median of --steps after --warmup), the share of 8 TB/s from the
         algorithmic bytes (every input frame read once, every output frame written once: bench.py's formula), a sample of the
         messages checked byte for byte against tests/src_pull_model.py -- and, from the same input in the same process, the
         fixed-ratio resampler's batch (ohgpu_src_batch_run_timed) as the baseline.
cadence: 256 PullableSampleRateConverter lanes behind one driver thread, one 5 ms input message per lane per tick, all read with
         ONE PlayableBatch::Run per tick (libohhost.so): median microseconds per tick, beside the same with SampleRateConverter
         lanes; two pulled lanes' whole output checked against the model.

    python tools/bench_pull.py [--streams 256] [--seconds 10] [--steps 20] [--warmup 3] [--ticks 200] [--bulk-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import src_pull_model as PM                      # noqa: E402
from ohpipeline_amd import capi, hostmodel       # noqa: E402

RATE_IN, RATE_OUT, CH, FB = 44100, 48000, 2, 6
T, S, BETA_PULL, BETA_FIXED, F_PASS = 32, 8, 8.0, 9.0, 20000.0
MSG_FRAMES = 4800
HBM_PEAK_GBPS = 8000.0


def timed(ctx, run, steps, warmup):
    e0, e1 = ctx.event(), ctx.event()
    for _ in range(warmup):
        run(None)
    ms = []
    for _ in range(steps):
        run((e0, e1))
        ms.append(ctx.elapsed_ms(e0, e1))
    ctx.event_destroy(e0)
    ctx.event_destroy(e1)
    return float(np.median(ms)), ms


def bulk(ctx, args):
    rng = np.random.default_rng(2024)
    n, in_frames = args.streams, RATE_IN * args.seconds
    src = np.frombuffer(rng.bytes(n * in_frames * FB), dtype=np.uint8)
    d_src = ctx.upload(src)
    ppm = rng.uniform(-200.0, 200.0, n)
    # ---- pulled: each stream's outputs, MSG_FRAMES a message, every message reading the stream's whole input
    descs, dst_bytes = [], 0
    for s in range(n):
        step = PM.step_of(RATE_IN, RATE_OUT, PM.multiplier_of(ppm[s]))
        total = ((((in_frames - 1) << 32) + PM.MASK32) // step) + 1          # every output whose input has arrived
        pos, frac = 0, 0
        for j0 in range(0, total, MSG_FRAMES):
            cnt = min(MSG_FRAMES, total - j0)
            descs.append((s * in_frames * FB, 0, in_frames, pos, step, dst_bytes, frac, cnt))
            dst_bytes += cnt * FB
            pos, frac = PM.advance(pos, frac, step, cnt)
    d = np.zeros(len(descs), dtype=capi.SRC_PULL_MSG_DESC)
    cols = ("src_offset", "src_frame0", "src_frames", "pos_frame", "step", "dst_offset", "pos_frac", "n_frames")
    arr = np.array(descs, dtype=np.uint64)
    for i, c in enumerate(cols):
        d[c] = arr[:, i]
    d["attenuation"], d["channels"], d["src_bits"], d["src_endian"], d["dst_bits"], d["dst_endian"] = 256, CH, 24, PM.ENDIAN_LITTLE, 24, PM.ENDIAN_BIG
    table = capi.src_pull_design(RATE_IN, RATE_OUT, T, S, BETA_PULL, F_PASS, 0.001)
    flt = ctx.src_pull_create(T, S, table)
    d_dst = ctx.malloc(dst_bytes)
    b = ctx.src_pull_batch(flt, d, src.size, dst_bytes)
    info = ctx.batch_info(b)

    def run_pull(ev):
        if ev:
            ctx.record(ev[0])
        ctx.src_pull_run(b, d_src, d_dst)
        if ev:
            ctx.record(ev[1])
    pull_ms, _ = timed(ctx, run_pull, args.steps, args.warmup)
    alg = info["in_frames"] * FB + info["out_frames"] * FB
    out = ctx.download(d_dst, dst_bytes)
    sample = rng.choice(len(d), size=min(12, len(d)), replace=False)
    ok = True
    for i in sample:
        want = PM.message_bytes(table, S, d[i], src, capi.ramp_table())
        o = int(d[i]["dst_offset"])
        ok = ok and np.array_equal(out[o:o + want.size], want)
    ctx.batch_destroy(b)
    ctx.free(d_dst)
    ctx.src_pull_destroy(flt)
    pulled = {"kernel_ms": round(pull_ms, 4), "algorithmic_bytes": int(alg), "gbps": round(alg / (pull_ms * 1e-3) / 1e9, 1),
              "share_of_8tbps": round(alg / (pull_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 3), "messages": int(len(d)),
              "out_frames": int(info["out_frames"]), "check": f"bit-exact vs model ({len(sample)} messages)" if ok else "MISMATCH"}
    # ---- fixed ratio, the same input: the library's production resampler batch
    L_, M_, coef = capi.src_design(RATE_IN, RATE_OUT, T, BETA_FIXED, F_PASS)
    fixed_flt = ctx.src_create(L_, M_, T, coef)
    out_total = (in_frames * L_ + M_ - 1) // M_
    n_msgs = (out_total + MSG_FRAMES - 1) // MSG_FRAMES
    fd = np.zeros(n * n_msgs, dtype=capi.SRC_MSG_DESC)
    first = np.arange(n_msgs) * MSG_FRAMES
    for s in range(n):
        sl = slice(s * n_msgs, (s + 1) * n_msgs)
        fd["src_offset"][sl], fd["src_frames"][sl], fd["out_frame0"][sl] = s * in_frames * FB, in_frames, first
        fd["dst_offset"][sl], fd["n_frames"][sl] = (s * out_total + first) * FB, np.minimum(MSG_FRAMES, out_total - first)
    fd["ramp_start"], fd["ramp_end"], fd["attenuation"] = capi.RAMP_MAX, capi.RAMP_MAX, 256
    fd["channels"], fd["src_bits"], fd["src_endian"], fd["dst_bits"], fd["dst_endian"] = CH, 24, PM.ENDIAN_LITTLE, 24, PM.ENDIAN_BIG
    fixed_dst = n * out_total * FB
    d_dst = ctx.malloc(fixed_dst)
    fb = ctx.src_batch(fixed_flt, fd, src.size, fixed_dst)
    finfo = ctx.batch_info(fb)

    def run_fixed(ev):
        ctx.src_run(fb, d_src, d_dst, events=ev)
    fixed_ms, _ = timed(ctx, run_fixed, args.steps, args.warmup)
    falg = finfo["in_frames"] * FB + finfo["out_frames"] * FB
    fixed = {"kernel": ctx.src_kernel_name(fb), "kernel_ms": round(fixed_ms, 4), "gbps": round(falg / (fixed_ms * 1e-3) / 1e9, 1),
             "share_of_8tbps": round(falg / (fixed_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 3)}
    ctx.batch_destroy(fb)
    ctx.free(d_dst)
    ctx.src_destroy(fixed_flt)
    ctx.free(d_src)
    return {"what": f"{n} streams x {args.seconds} s stereo S24, {RATE_IN} -> {RATE_OUT} Hz, pulls in +-200 ppm, one batch",
            "pulled": pulled, "fixed_ratio": fixed}


def cadence(args):
    n, ticks = args.streams, args.ticks
    in_per_tick = RATE_IN // 200
    rng = np.random.default_rng(7)
    lane_stride = (ticks + 1) * in_per_tick * FB
    src = np.frombuffer(rng.bytes(n * lane_stride), dtype=np.uint8)
    out = np.zeros(n * 4096, dtype=np.uint8)
    res = {}
    for kind in ("fixed_ratio", "pulled"):
        t_us, kept = [], {0: [], n - 1: []}
        with hostmodel.LiveDriver(0, n, RATE_IN, RATE_OUT, CH, 24, True, 24, pulled=(kind == "pulled")) as live:
            mults = [PM.multiplier_of(p) for p in rng.uniform(-200.0, 200.0, n)]
            if kind == "pulled":
                for lane in range(n):
                    live.pull_clock(lane, mults[lane])
            for k in range(ticks):
                t0 = time.perf_counter()
                nbytes = live.tick(src[k * in_per_tick * FB:], lane_stride, in_per_tick, out, 4096)
                t_us.append((time.perf_counter() - t0) * 1e6)
                for lane in kept:
                    kept[lane].append(out[lane * 4096:lane * 4096 + int(nbytes[lane])].copy())
            st = live.stats()
        r = {"tick_us": {"median": round(float(np.median(t_us[10:])), 1), "p99": round(float(np.percentile(t_us[10:], 99)), 1)},
             "resampler_calls_per_tick": round(st["src_calls"] / ticks, 3), "device_allocations": st["device_allocs"]}
        if kind == "pulled":
            table = capi.src_pull_design(RATE_IN, RATE_OUT, T, S, BETA_PULL, F_PASS, 0.001)
            ok = True
            for lane, parts in kept.items():
                got = np.concatenate(parts)
                step = PM.step_of(RATE_IN, RATE_OUT, mults[lane])
                x = PM.decode_s24(src[lane * lane_stride:lane * lane_stride + ticks * in_per_tick * FB], CH, 24, PM.ENDIAN_LITTLE)
                n_out = got.size // FB
                have = ticks * in_per_tick                                   # every output whose input has arrived, no more
                ok = ok and n_out == ((((have - 1) << 32) + PM.MASK32) // step) + 1
                want = PM.pack(PM.resample(table, S, x, 0, 0, 0, step, n_out), 24, PM.ENDIAN_BIG)
                ok = ok and np.array_equal(got, want)
            r["check"] = "bit-exact vs model (2 lanes)" if ok else "MISMATCH"
        res[kind] = r
    res["ratio_pulled_to_fixed"] = round(res["pulled"]["tick_us"]["median"] / res["fixed_ratio"]["tick_us"]["median"], 3)
    res["what"] = f"{n} lanes behind one driver thread, one 5 ms message per lane per tick, one PlayableBatch::Run per tick, {ticks} ticks"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--bulk-only", action="store_true")
    args = ap.parse_args()
    with capi.Context(0) as ctx:
        result = {"metric": "pulled resampler", "device": ctx.name(), "bulk": bulk(ctx, args)}
    if not args.bulk_only:
        result["cadence"] = cadence(args)
    result["targets"] = {"bulk_share_min": 0.30, "cadence_ratio_max": 1.5}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
