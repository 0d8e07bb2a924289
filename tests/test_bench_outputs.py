"""bench.py's plain line, its --full line and --dump-outputs: what a plain run prints, that --full still carries the baseline
and the bit-exact check, and that the dumped samples are the destination arena's (decoded and positioned as documented) --
on the GPU against the CPU oracle, on the CPU through a stand-in context."""
import argparse
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from ohpipeline_amd import capi  # noqa: E402

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


class FakeCtx:
    def __init__(self, arena):
        self.arena = arena

    def download(self, dptr, nbytes, stream=None):
        assert nbytes == self.arena.size
        return self.arena.copy()


def encode(values, bits, endian):
    """Signed integers -> the arena's bytes, one sample after another."""
    bps = bits // 8
    u = values.astype(np.int64) & ((1 << bits) - 1)
    b = np.stack([(u >> (8 * k)) & 0xFF for k in range(bps)], axis=1).astype(np.uint8)     # little endian
    return (b[:, ::-1] if endian == capi.ENDIAN_BIG else b).reshape(-1)


def fake_group(rate_in, channels, streams, out_total, bits, endian):
    return types.SimpleNamespace(rate_in=rate_in, channels=channels, stream_ids=list(range(streams)), out_total=out_total,
                                 dst_bits=bits, dst_endian=endian, dst_bytes=streams * out_total * channels * bits // 8, d_dst=None)


@pytest.mark.parametrize("bits,endian", [(24, capi.ENDIAN_BIG), (16, capi.ENDIAN_LITTLE), (32, capi.ENDIAN_BIG)])
def test_dump_outputs_decodes_every_sample_of_a_small_output(tmp_path, bits, endian):
    g = fake_group(44100, 2, 3, 1000, bits, endian)
    rng = np.random.default_rng(7)
    want = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), 3 * 1000 * 2)
    want[:4] = [-(1 << (bits - 1)), (1 << (bits - 1)) - 1, -1, 0]
    bench.dump_outputs(capi, FakeCtx(encode(want, bits, endian)), [g], str(tmp_path))
    vals = np.load(tmp_path / "g0_44100hz_2ch.npy")
    idx = np.load(tmp_path / "g0_44100hz_2ch_index.npy")
    assert vals.dtype == (np.float32 if bits <= 24 else np.float64) and idx.dtype == np.float64
    assert np.array_equal(idx, np.arange(want.size)) and np.array_equal(vals.astype(np.int64), want)


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLES", 1000)
    groups = [fake_group(44100, 2, 4, 2000, 24, capi.ENDIAN_BIG), fake_group(96000, 6, 2, 1500, 24, capi.ENDIAN_BIG)]
    rng = np.random.default_rng(11)
    wants = [rng.integers(-(1 << 23), 1 << 23, len(g.stream_ids) * g.out_total * g.channels) for g in groups]
    for run in ("a", "b"):
        for k, (g, want) in enumerate(zip(groups, wants)):
            bench.dump_outputs(capi, FakeCtx(encode(want, 24, capi.ENDIAN_BIG)), [g], str(tmp_path / run), prefix=f"{k}_")
    kept = 0
    for k, (g, want) in enumerate(zip(groups, wants)):
        name = f"{k}_g0_{g.rate_in}hz_{g.channels}ch"
        idx = np.load(tmp_path / "a" / (name + "_index.npy"))
        vals = np.load(tmp_path / "a" / (name + ".npy"))
        assert np.array_equal(idx, np.load(tmp_path / "b" / (name + "_index.npy")))
        assert np.array_equal(vals, np.load(tmp_path / "b" / (name + ".npy")))
        pos = idx.astype(np.int64)
        assert idx.size == 1000 and (np.diff(pos) > 0).all() and pos[0] >= 0 and pos[-1] < want.size
        assert np.array_equal(vals.astype(np.int64), want[pos])
        kept += idx.size
    assert kept == 2000


def run_bench(*extra, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--seconds", "0.25", "--streams", "4", "--sustain", "0", *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_oracles_output(tmp_path):
    import oracle_lib as O
    res = run_bench("--dump-outputs", str(tmp_path))
    assert all(k in res for k in HEADLINE_KEYS)
    assert res["steps"] == 3 and res["value"] > 0 and res["ms_per_step"] > 0 and res["unit"] == "Msamples/s"
    assert res["higher_is_better"] is True and res["dtype"] in ("int32", "f64")
    frames = 4 * int(round(0.25 * 44100))
    assert abs(res["value"] * res["ms_per_step"] * 1e3 / frames - 1.0) < 0.01       # (both figures are rounded)
    for k in ("cpu_baseline", "check", "configs", "end_to_end", "cadence", "plan_ms"):
        assert k not in res, k
    # the same groups, on the CPU oracle: the dumped values are its output at the dumped positions
    args = argparse.Namespace(config=3, streams=4, seconds=0.25, rate_in=44100, channels=2, src_bits=24)
    (g,), _ = bench.build_groups(capi, args, 0, 1)
    ref = O.Src(g.rate_in, bench.RATE_OUT, g.taps, bench.BETA, bench.F_PASS)
    want = np.zeros(g.dst_bytes, dtype=np.uint8)
    assert ref.process_batch(g.oracle_descs.view(O.SRC_MSG_DESC), g.src, want) == 0
    b = want.reshape(-1, 3).astype(np.int64)
    want_vals = (b[:, 0] << 16) | (b[:, 1] << 8) | b[:, 2]
    want_vals = np.where(want_vals >= 1 << 23, want_vals - (1 << 24), want_vals)
    vals = np.load(tmp_path / "g0_44100hz_2ch.npy")
    idx = np.load(tmp_path / "g0_44100hz_2ch_index.npy")
    assert vals.dtype == np.float32 and np.array_equal(idx, np.arange(want_vals.size))
    assert np.array_equal(vals.astype(np.int64), want_vals)


@pytest.mark.gpu
def test_full_run_keeps_the_baseline_and_the_check():
    res = run_bench("--full")
    assert all(k in res for k in HEADLINE_KEYS) and res["steps"] == 3
    assert res["check"] == "bit-exact vs oracle" and res["cpu_baseline"]["value"] > 0
    assert res["plan_ms"] > 0 and "cadence" in res and "end_to_end" in res
