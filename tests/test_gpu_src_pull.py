"""GPU checks of the pulled resampler: ohgpu_src_pull_batch_run bit-exact against the numpy model
(tests/src_pull_model.py) over every layout class, ramps, stream starts, both tap counts, pulls and pull changes, message sizes and a
256-stream batch run three times; refusals before any launch; and an FFT check of the audio it makes."""
import numpy as np
import pytest

import src_pull_model as PM
from ohpipeline_amd import capi
from src_pull_cases import S, Arena, expected, stream       # (the builders: shared with the far-offset and far-position tests)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ramp_table():
    return capi.ramp_table()


_filters = {}


def pulled_filter(ctx, rate_in, rate_out, T, max_pull=0.001):
    key = (rate_in, rate_out, T, max_pull)
    if key not in _filters:
        table = capi.src_pull_design(rate_in, rate_out, T, S, 8.0 if T == 32 else 9.0, 20000.0, max_pull)
        _filters[key] = (table, ctx.src_pull_create(T, S, table))
    return _filters[key]


def run(ctx, flt, descs, src, dst_bytes, times=1):
    d_src, d_dst = ctx.upload(src), ctx.malloc(max(dst_bytes, 1))
    ctx.memset(d_dst, 0, max(dst_bytes, 1))
    b = ctx.src_pull_batch(flt, descs, src.size, dst_bytes)
    outs = []
    for _ in range(times):
        ctx.src_pull_run(b, d_src, d_dst)
        outs.append(ctx.download(d_dst, dst_bytes))
    info = ctx.batch_info(b)
    ctx.batch_destroy(b)
    ctx.free(d_src)
    ctx.free(d_dst)
    return outs, info


@pytest.mark.parametrize("T", [32, 64])
def test_every_layout_class(ctx, ramp_table, T):
    """1-8 channels x 8/16/24/32-bit sources x 16/24/32-bit destinations, both byte orders, ramps, ZERO_LSB32, stream starts."""
    table, flt = pulled_filter(ctx, 44100, 48000, T)
    rng = np.random.default_rng(T)
    a = Arena()
    step = PM.step_of(44100, 48000, PM.multiplier_of(300))
    i = 0
    for ch in range(1, 9):
        for sb in (8, 16, 24, 32):
            for db in (16, 24, 32):
                for se, de in ((PM.ENDIAN_LITTLE, PM.ENDIAN_BIG), (PM.ENDIAN_BIG, PM.ENDIAN_LITTLE)):
                    i += 1
                    flags = (PM.FLAG_RAMP if i % 3 == 0 else 0) | (PM.FLAG_ZERO_LSB32 if i % 2 == 0 else 0)
                    stream(a, rng, ch, sb, se, db, de, T, [step] * 3, [int(rng.integers(1, 120)) for _ in range(3)], 400,
                           flags_of=lambda m, f=flags: f, ramps_of=lambda m: (16384, 8000) if m == 0 else (8000, 0))
    src, descs = a.arrays()
    (got,), info = run(ctx, flt, descs, src, a.dst_bytes)
    assert info["n_msgs"] == len(descs) and info["out_frames"] == int(descs["n_frames"].sum())
    assert np.array_equal(got, expected(table, descs, src, a.dst_bytes, ramp_table))


@pytest.mark.parametrize("rate_in,T,max_pull,ppms", [(44100, 32, 0.001, (-500, 0, 500)), (48000, 32, 0.001, (-500, 0, 500)),
                                                     (44100, 64, 0.001, (-500, 0, 500)), (48000, 64, 0.02, (-20000, 20000))])
def test_pulls_and_pull_changes(ctx, ramp_table, rate_in, T, max_pull, ppms):
    """Stereo (the stereo kernel): every stream at its own fixed pull, and one whose pull changes between consecutive messages;
    messages of 1-700 frames in random order; stream starts."""
    table, flt = pulled_filter(ctx, rate_in, 48000, T, max_pull)
    rng = np.random.default_rng(rate_in + T)
    a = Arena()
    for ppm in ppms:
        st = PM.step_of(rate_in, 48000, PM.multiplier_of(ppm))
        sizes = [int(v) for v in rng.permutation(np.r_[1, 2, 3, 700, rng.integers(1, 701, 8)])]
        stream(a, rng, 2, 24, PM.ENDIAN_LITTLE, 24, PM.ENDIAN_BIG, T, [st] * len(sizes), sizes, 6000)
    changing = [PM.step_of(rate_in, 48000, PM.multiplier_of(int(p))) for p in rng.choice(ppms, 24)]
    stream(a, rng, 2, 24, PM.ENDIAN_LITTLE, 24, PM.ENDIAN_BIG, T, changing, [int(v) for v in rng.integers(1, 701, 24)], 12000,
           flags_of=lambda m: PM.FLAG_RAMP if m % 4 == 1 else 0, ramps_of=lambda m: (16384 - 600 * m, 15000 - 600 * m))
    src, descs = a.arrays()
    (got,), _ = run(ctx, flt, descs, src, a.dst_bytes)
    assert np.array_equal(got, expected(table, descs, src, a.dst_bytes, ramp_table))


def test_stereo_kernel_every_depth_and_byte_order(ctx, ramp_table):
    """A batch of stereo messages only (the stereo instantiation): 8/16/24/32-bit sources in both byte orders into 16/24/32-bit
    destinations in both byte orders, ramped and not, ZERO_LSB32, stream starts."""
    table, flt = pulled_filter(ctx, 44100, 48000, 32)
    rng = np.random.default_rng(2)
    a = Arena()
    step = PM.step_of(44100, 48000, PM.multiplier_of(-300))
    i = 0
    for sb in (8, 16, 24, 32):
        for se in (PM.ENDIAN_LITTLE, PM.ENDIAN_BIG):
            for db in (16, 24, 32):
                for de in (PM.ENDIAN_LITTLE, PM.ENDIAN_BIG):
                    i += 1
                    flags = (PM.FLAG_RAMP if i % 3 == 0 else 0) | (PM.FLAG_ZERO_LSB32 if i % 2 == 0 else 0)
                    stream(a, rng, 2, sb, se, db, de, 32, [step] * 3, [int(rng.integers(1, 300)) for _ in range(3)], 1000,
                           flags_of=lambda m, f=flags: f, ramps_of=lambda m: (16384, 8000) if m == 0 else (8000, 0))
    src, descs = a.arrays()
    assert np.all(descs["channels"] == 2)
    (got,), _ = run(ctx, flt, descs, src, a.dst_bytes)
    assert np.array_equal(got, expected(table, descs, src, a.dst_bytes, ramp_table))


@pytest.mark.parametrize("rate_in,T,ch", [(96000, 64, 2), (96000, 64, 8), (44100, 64, 8), (44100, 32, 8), (192000, 32, 6)])
def test_downsampling_and_windows_that_cut_tiles(ctx, ramp_table, rate_in, T, ch):
    """Downsampling, and messages of several hundred outputs whose tiles are cut short by the LDS window (eight channels hold
    256 frames at T = 32 and 192 at T = 64) rather than by the 256 lanes."""
    table, flt = pulled_filter(ctx, rate_in, 48000, T)
    rng = np.random.default_rng(rate_in + T + ch)
    a = Arena()
    for ppm in (-1000, 0, 1000):
        st = PM.step_of(rate_in, 48000, PM.multiplier_of(ppm))
        sizes = [int(v) for v in rng.integers(300, 900, 4)]
        stream(a, rng, ch, 24, PM.ENDIAN_LITTLE, 24, PM.ENDIAN_BIG, T, [st] * 4, sizes, 4 * 900 * (rate_in // 48000 + 1) + 200,
               flags_of=lambda m: PM.FLAG_RAMP if m == 1 else 0, ramps_of=lambda m: (16384, 0))
    src, descs = a.arrays()
    assert len(descs) >= 9 and descs["n_frames"].max() >= 300
    (got,), _ = run(ctx, flt, descs, src, a.dst_bytes)
    assert np.array_equal(got, expected(table, descs, src, a.dst_bytes, ramp_table))


def test_256_streams_each_with_its_own_pull_three_runs(ctx, ramp_table):
    """A period of 256 streams, each message's input window packed back to back (src_frame0 > 0), run three times."""
    table, flt = pulled_filter(ctx, 44100, 48000, 32)
    rng = np.random.default_rng(256)
    a = Arena()
    for k in range(256):
        st = PM.step_of(44100, 48000, PM.multiplier_of(int(rng.integers(-1000, 1001))))
        pos, frac = int(rng.integers(0, 1 << 30)), int(rng.integers(0, 1 << 32))
        n = int(rng.integers(200, 260))
        first, frames = PM.window(pos, frac, st, n, 32)
        off = a.add_input(rng.integers(0, 256, size=frames * 6, dtype=np.uint8))
        a.add_msg(off, first, frames, pos, frac, st, n, 2, 24, PM.ENDIAN_LITTLE, 24, PM.ENDIAN_BIG,
                  PM.FLAG_RAMP if k % 5 == 0 else 0, (16384, 0))
    src, descs = a.arrays()
    outs, _ = run(ctx, flt, descs, src, a.dst_bytes, times=3)
    want = expected(table, descs, src, a.dst_bytes, ramp_table)
    for got in outs:
        assert np.array_equal(got, want)


def test_refusals_before_any_launch(ctx):
    table, flt = pulled_filter(ctx, 44100, 48000, 32)
    rng = np.random.default_rng(9)
    a = Arena()
    stream(a, rng, 2, 24, PM.ENDIAN_LITTLE, 24, PM.ENDIAN_BIG, 32, [PM.step_of(44100, 48000)] * 2, [100, 100], 400)
    src, descs = a.arrays()

    def refused(descs_, src_bytes, dst_bytes, code):
        with pytest.raises(capi.OhGpuError) as e:
            ctx.src_pull_batch(flt, descs_, src_bytes, dst_bytes)
        assert e.value.code == code, capi.last_error()

    refused(descs, src.size, a.dst_bytes - 1, capi.ERR_BOUNDS)                 # output beyond the destination arena
    refused(descs, src.size - 16, a.dst_bytes, capi.ERR_BOUNDS)                # input beyond the source arena
    first, frames = PM.window(int(descs[1]["pos_frame"]), int(descs[1]["pos_frac"]), int(descs[1]["step"]), 100, 32)
    bad = descs.copy(); bad[1]["src_frames"] = first + frames - 1
    refused(bad, src.size, a.dst_bytes, capi.ERR_BOUNDS)                       # the buffer ends before the message's last frame
    bad = descs.copy(); bad[1]["src_frame0"] = first + 1; bad[1]["src_frames"] = frames - 1
    refused(bad, src.size, a.dst_bytes, capi.ERR_BOUNDS)                       # history missing in front
    bad = descs.copy(); bad[0]["src_frame0"] = 1; bad[0]["src_frames"] = 300
    refused(bad, src.size, a.dst_bytes, capi.ERR_BOUNDS)                       # a stream start needs the buffer from frame 0
    bad = descs.copy(); bad[0]["step"] = 0
    refused(bad, src.size, a.dst_bytes, capi.ERR_INVALID)
    bad = descs.copy(); bad[0]["step"] = capi.SRC_PULL_MAX_STEP + 1
    refused(bad, src.size, a.dst_bytes, capi.ERR_INVALID)
    bad = descs.copy(); bad[0]["pos_frac"] = (1 << 32) - 1; bad[0]["step"] = capi.SRC_PULL_MAX_STEP; bad[0]["n_frames"] = (1 << 32) - 1
    refused(bad, 1 << 62, 1 << 62, capi.ERR_INVALID)                           # n_frames * step overflows
    bad = descs.copy(); bad[0]["dst_bits"] = 8
    refused(bad, src.size, a.dst_bytes, capi.ERR_UNSUPPORTED)
    bad = descs.copy(); bad[0]["attenuation"] = 128
    refused(bad, src.size, a.dst_bytes, capi.ERR_UNSUPPORTED)
    bad = descs.copy(); bad[0]["flags"] = capi.FLAG_SRC_PLANAR32
    refused(bad, src.size, a.dst_bytes, capi.ERR_UNSUPPORTED)
    # the two kinds of filter do not mix
    L_, M_, coef = capi.src_design(44100, 48000, 32, 9.0, 20000.0)
    fixed = ctx.src_create(L_, M_, 32, coef)
    with pytest.raises(capi.OhGpuError) as e:
        ctx.src_pull_batch(fixed, descs, src.size, a.dst_bytes)
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.OhGpuError) as e:
        ctx.src_batch(flt, np.zeros(0, dtype=capi.SRC_MSG_DESC), 0, 0)
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.OhGpuError) as e:
        ctx.src_pull_destroy(fixed)
    assert e.value.code == capi.ERR_INVALID
    ctx.src_destroy(fixed)
    # a refused process_host call leaves the destination as it was
    dst = np.full(a.dst_bytes, 0x5A, dtype=np.uint8)
    with pytest.raises(capi.OhGpuError):
        ctx.src_pull_process_host(flt, descs, src[:-16], dst)
    assert np.all(dst == 0x5A)
    # ... and the one that is not refused writes the model's bytes
    ctx.src_pull_process_host(flt, descs, src, dst)
    assert np.array_equal(dst, expected(table, descs, src, a.dst_bytes, capi.ramp_table()))


def _tone_level_db(y, f, rate):
    """Amplitude of the tone at f Hz in dB of full scale (Blackman-Harris window, evaluated at the exact frequency), and the
    largest other spectral line below 20 kHz relative to it."""
    n = y.size
    t = np.arange(n)
    w = 0.35875 - 0.48829 * np.cos(2 * np.pi * t / n) + 0.14128 * np.cos(4 * np.pi * t / n) - 0.01168 * np.cos(6 * np.pi * t / n)
    amp = np.abs(np.sum(y * w * np.exp(-2j * np.pi * f * t / rate))) * 2 / w.sum()
    spec = np.abs(np.fft.rfft(y * w)) * 2 / w.sum()
    freqs = np.arange(spec.size) * rate / n
    keep = (freqs < 20000.0) & (np.abs(freqs - f) > 8 * rate / n) & (freqs > 8 * rate / n)
    return 20 * np.log10(amp / (1 << 23)), 20 * np.log10(spec[keep].max() / amp)


def test_audio_tones_come_out_at_the_pulled_frequency(ctx):
    """997 Hz and 15 kHz at -1 dBFS through 44.1 -> 48 and 48 -> 48 kHz at -500, 0 and +500 ppm, S24 in and out."""
    level = 10 ** (-1 / 20) * ((1 << 23) - 1)
    for rate_in in (44100, 48000):
        table, flt = pulled_filter(ctx, rate_in, 48000, 32)
        a = Arena()
        cases = []
        for f in (997.0, 15000.0):
            for ppm in (-500, 0, 500):
                in_frames = int(rate_in * 1.6)
                x = np.round(level * np.sin(2 * np.pi * f * np.arange(in_frames) / rate_in)).astype(np.int64)
                data = ((x[:, None].repeat(2, axis=1) & 0xFFFFFF)[..., None] >> np.array([0, 8, 16])) & 0xFF   # S24LE stereo
                off = a.add_input(data.astype(np.uint8).reshape(-1))
                st = PM.step_of(rate_in, 48000, PM.multiplier_of(ppm))
                first_out = a.dst_bytes
                pos, frac = 0, 0
                for _ in range(300):
                    a.add_msg(off, 0, in_frames, pos, frac, st, 240, 2, 24, PM.ENDIAN_LITTLE, 24, PM.ENDIAN_LITTLE)
                    pos, frac = PM.advance(pos, frac, st, 240)
                cases.append((f, ppm, first_out))
        src, descs = a.arrays()
        (got,), _ = run(ctx, flt, descs, src, a.dst_bytes)
        for f, ppm, first in cases:
            raw = got[first:first + 300 * 240 * 6].reshape(-1, 2, 3).astype(np.int64)
            y = raw[:, 0, 0] | (raw[:, 0, 1] << 8) | (raw[:, 0, 2] << 16)
            y = np.where(y >= 1 << 23, y - (1 << 24), y).astype(np.float64)[4800:4800 + 65536]     # past the stream start
            f_out = f * (PM.step_of(rate_in, 48000, PM.multiplier_of(ppm)) / 2.0 ** 32) * 48000 / rate_in   # the pulled frequency
            tone_db, spur_db = _tone_level_db(y, f_out, 48000.0)
            assert abs(tone_db - (-1.0)) <= 0.01, (rate_in, f, ppm, tone_db)
            assert spur_db <= -80.0, (rate_in, f, ppm, spur_db)
