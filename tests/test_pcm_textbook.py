"""tests/pcm_textbook.py (the PCM message path from its definition, plain Python integers) held to the CPU oracle byte for byte,
and to the fixture tests/golden/pcm_textbook.json.  The oracle and the kernels were written from the same reading of the
reference; the model is a second reading, so a misreading the two share shows up here (CPU) or in test_gpu_pcm_textbook.py.

Model-side matrix (the model costs microseconds per subsample): every source depth x destination depth x byte order on each side
x channels {1,2,3,5,6,8} x {ramped, plain, silent, attenuated} is crossed IN FULL; the 7 ramp endpoint pairs and the 11 frame
counts rotate through those 1536 cells so that every (ramp, count) pair appears in twenty of them, and one depth pair (24 -> 24)
carries the full ramp x count x channels cross.  The large sizes are test_gpu_pcm_textbook.py's, where the oracle carries them.

Readings of the reference that the written definition leaves open (resolved by Msg.cpp, recorded here):
  * Msg.cpp:2736-2751 (ApplyAttenuation): `(TInt)sample16 * iAttenuation / kUnityAttenuation` -- iAttenuation is a TUint, so the
    product and the division are UNSIGNED.  "The /256 with C truncation" is therefore the truncation of an unsigned quotient, which
    for a negative sample is floor(s * att / 256) modulo 2^16, NOT the signed truncation toward zero.  Model and oracle agree;
    test_attenuation_every_s16_value also states how often the signed reading would differ.
  * Msg.cpp:2874-2893 (MsgPlayableSilence::ReadBlock): the six-channel constant is a BYTE array of 32 bytes used at every depth,
    so 8/16/24-bit six-channel silence carries 0x10..0x70 too (at 16 bits: in the low byte of subsamples 3, 5, 7, ...), and the
    pattern restarts at every cell of 9216 bytes rounded down to whole frames.  Model and oracle agree.
  * Msg.cpp:835: `iLoopCount * iTotalRamp` is TInt arithmetic and the division truncates toward zero: an up-ramp (negative
    iTotalRamp) rounds the other way than a down-ramp.  Model and oracle agree.
No disagreement between model and oracle was met.
"""
import hashlib
import itertools
import json
import os
import subprocess
import sys

import numpy as np

import oracle_lib as O
import pcm_textbook as PT

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "pcm_textbook.json")
GENERATOR = os.path.join(HERE, "golden", "make_pcm_textbook_fixtures.py")

LE, BE = O.ENDIAN_LITTLE, O.ENDIAN_BIG
kMax = O.RAMP_MAX
DEPTHS = [8, 16, 24, 32]
CHANNELS = [1, 2, 3, 5, 6, 8]
RAMPS = [(kMax, 0), (0, kMax), (kMax, kMax), (0, 0), (8191, 8190), (5, 5), (kMax, kMax - 32)]     # down, up, flat, flat, ..., one table step
COUNTS = [1, 2, 3, 4, 5, 127, 128, 129, 511, 512, 513]
KINDS = ["ramped", "plain", "silence", "attenuated"]
ATTENUATIONS = [0, 1, 64, 255, 77]


def test_constants_agree_with_the_oracle_binding():
    assert (PT.ENDIAN_LITTLE, PT.ENDIAN_BIG) == (O.ENDIAN_LITTLE, O.ENDIAN_BIG)
    assert (PT.FLAG_RAMP, PT.FLAG_SILENCE, PT.FLAG_ZERO_LSB32) == (O.FLAG_RAMP, O.FLAG_SILENCE, O.FLAG_ZERO_LSB32)
    assert (PT.RAMP_MAX, PT.UNITY_ATTENUATION, PT.CELL_BYTES) == (O.RAMP_MAX, O.UNITY_ATTENUATION, O.MAX_BYTES)
    assert PT.ramp_table() == O.ramp_table().tolist()


def oracle_message(d, src):
    d = np.array([d], dtype=O.MSG_DESC)
    d["dst_offset"] = 0
    n = int(d["n_frames"][0]) * int(d["channels"][0]) * int(d["dst_bits"][0]) // 8
    dst = np.full(n + 8, 0xA5, dtype=np.uint8)
    assert O.msg_process_batch(d, src, dst) == 0
    assert (dst[n:] == 0xA5).all()
    return dst[:n].tobytes()


def desc(src_offset, n, ramp, att, ch, sbits, se, dbits, de, flags):
    return np.array([(src_offset, 0, n, ramp[0], ramp[1], att, ch, sbits, se, dbits, de, flags)], dtype=O.MSG_DESC)[0]


def kind_fields(kind, sbits, k):
    """(flags, attenuation) of cell k.  Attenuation exists for 16-bit audio only (Msg.cpp:2741 asserts): the other depths' fourth
    kind is ramped with ZERO_LSB32."""
    zero = O.FLAG_ZERO_LSB32 if k % 3 == 0 else 0
    if kind == "ramped":
        return O.FLAG_RAMP | zero, 256
    if kind == "plain":
        return zero, 256
    if kind == "silence":
        return O.FLAG_SILENCE | zero, 256
    if sbits == 16:
        return (O.FLAG_RAMP if k % 2 else 0) | zero, ATTENUATIONS[k % len(ATTENUATIONS)]
    return O.FLAG_RAMP | O.FLAG_ZERO_LSB32, 256


def test_model_equals_oracle_over_the_format_matrix():
    rng = np.random.default_rng(20260101)
    src = rng.integers(0, 256, size=513 * 8 * 4 + 16, dtype=np.uint8)
    src[:64] = np.frombuffer(bytes([0x7f, 0xff, 0xff, 0xff, 0x80, 0, 0, 0, 0xff, 0xff, 0xff, 0xff, 0x80, 0x00, 0x7f, 0xff] * 4), dtype=np.uint8)
    seen = set()
    cells = itertools.product(DEPTHS, DEPTHS, [LE, BE], [LE, BE], CHANNELS, KINDS)
    for k, (sbits, dbits, se, de, ch, kind) in enumerate(cells):
        ramp, n = RAMPS[k % 7], COUNTS[(k // 7) % 11]
        seen.add((ramp, n))
        flags, att = kind_fields(kind, sbits, k)
        d = desc(k % 13, n, ramp, att, ch, sbits, se, dbits, de, flags)
        got, want = PT.process_message(d, src), oracle_message(d, src)
        assert got == want, (sbits, dbits, se, de, ch, kind, ramp, n, att, flags)
    assert k + 1 == 1536 and len(seen) == len(RAMPS) * len(COUNTS)


def test_model_equals_oracle_every_ramp_at_every_count_and_channel_count():
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, size=513 * 8 * 3 + 16, dtype=np.uint8)
    for ramp, n, ch in itertools.product(RAMPS + [(100, 101), (12345, 54), (17, 16001)], COUNTS, CHANNELS):
        d = desc(n % 5, n, ramp, 256, ch, 24, LE if n % 2 else BE, 24, BE, O.FLAG_RAMP)
        assert PT.process_message(d, src) == oracle_message(d, src), (ramp, n, ch)


def test_attenuation_every_s16_value():
    """All 65536 values x {0, 1, 64, 255, 256}: the model's scalar expression against the oracle's buffer call."""
    vals = np.arange(65536, dtype=np.uint32)
    be = np.stack([(vals >> 8).astype(np.uint8), (vals & 0xff).astype(np.uint8)], axis=1).reshape(-1)
    signed_reading_differs = 0
    for att in (0, 1, 64, 255, 256):
        err, got = O.apply_attenuation(be, 16, att)
        assert err == 0
        got16 = (got[0::2].astype(np.int64) << 8 | got[1::2]).tolist()
        for v in range(65536):
            s32 = PT.wrap16(v) << 16
            want = s32 if att == 256 else PT.attenuate(s32, att)
            assert (want >> 16) & 0xFFFF == got16[v], (v, att)
            signed_reading_differs += ((want >> 16) != PT.trunc_div(PT.wrap16(v) * att, 256))
    assert signed_reading_differs > 0          # (the two readings are different operations: see the module docstring)


def test_ramp_product_every_top16_value_times_every_table_entry():
    """All 65536 x 512 products.  The model's definition, vectorised in int64 -- low 16 bits of (s16 * multiplier) >> 15 -- against
    the oracle's RampApplicator run on a flat ramp that selects each table entry in turn; the scalar model is tied to the vector
    form on a stride of the same values."""
    table = np.array(PT.ramp_table(), dtype=np.int64)
    s16 = np.arange(-32768, 32768, dtype=np.int64)
    u16 = (s16 & 0xFFFF).astype(np.uint32)
    be = np.stack([(u16 >> 8).astype(np.uint8), (u16 & 0xff).astype(np.uint8)], axis=1).reshape(-1)
    for idx in range(512):
        ramp = kMax - 32 * idx
        assert PT.ramp_index(PT.ramp_value(12345, 65536, ramp, ramp)) == idx
        want = ((s16 * table[idx]) >> 15) & 0xFFFF
        err, got = O.ramp_apply(be, 16, 1, ramp, ramp)
        assert err == 0
        got16 = got[0::2].astype(np.int64) << 8 | got[1::2]
        assert np.array_equal(got16, want), idx
        for j in range(idx, 65536, 4099):
            v = PT.ramp_subsample(int(s16[j]) << 16, 16, 1, 0, int(table[idx]))
            assert (v >> 16) & 0xFFFF == int(want[j]), (idx, j)


def test_ramp_index_of_every_ramp_value():
    """min(511, (16384 - ramp + 16) >> 5) for every ramp value 0..16384 against a one-frame message through the oracle."""
    table = PT.ramp_table()
    src = np.array([0x40, 0x00], dtype=np.uint8)
    for ramp in range(0, kMax + 1):
        err, got = O.ramp_apply(src, 16, 1, ramp, 0)
        assert err == 0
        assert (int(got[0]) << 8 | int(got[1])) == (0x4000 * table[PT.ramp_index(ramp)]) >> 15, ramp


def test_silence_longer_than_a_cell():
    """The id bytes restart at every cell (9216 bytes rounded down to whole frames), at every depth."""
    src = np.zeros(1, dtype=np.uint8)
    for sbits, ch, dbits in itertools.product(DEPTHS, [2, 5, 6], [16, 32]):
        frame = ch * sbits // 8
        n = O.MAX_BYTES // frame + 5
        d = desc(0, n, (kMax, 0), 256, ch, sbits, BE, dbits, LE if ch == 5 else BE, O.FLAG_SILENCE)
        got = PT.process_message(d, src)
        assert got == oracle_message(d, src), (sbits, ch, dbits)
        # (only a 32-bit subsample's id byte is its fourth: a 16-bit destination drops it there and keeps it at the other depths)
        assert any(got) == (ch == 6 and not (sbits == 32 and dbits == 16)), (sbits, ch, dbits)


def test_batch_writes_messages_where_they_belong():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, size=4000, dtype=np.uint8)
    rows, dp = [], 3
    for k in range(12):
        n, ch, sbits, dbits = 5 + 7 * k, CHANNELS[k % 6], DEPTHS[k % 4], DEPTHS[(k + 1) % 4]
        rows.append((k * 11, dp, n, 9000, 300 + k, 256, ch, sbits, LE, dbits, BE, O.FLAG_RAMP if k % 2 else 0))
        dp += n * ch * dbits // 8 + (k % 3)
    descs = np.array(rows, dtype=O.MSG_DESC)
    want = np.full(dp + 4, 0xA5, dtype=np.uint8)
    assert O.msg_process_batch(descs, src, want) == 0
    got = PT.process_batch(descs, src, np.full(dp + 4, 0xA5, dtype=np.uint8))
    assert np.array_equal(got, want)


def test_golden_fixture():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_pcm_textbook_fixtures as G
    finally:
        sys.path.pop(0)
    with open(FIXTURE) as f:
        fx = json.load(f)
    src = G.arena()
    assert hashlib.sha256(src).hexdigest() == fx["arena_sha256"]
    arena = np.frombuffer(src, dtype=np.uint8)
    assert len(fx["messages"]) == 40
    for m in fx["messages"]:
        d = {k: m[k] for k in O.MSG_DESC.names}
        out = PT.process_message(d, src)
        assert len(out) == m["bytes"] and hashlib.sha256(out).hexdigest() == m["sha256"], m
        if "hex" in m:
            assert out.hex() == m["hex"]
        rec = np.array([tuple(m[k] for k in O.MSG_DESC.names)], dtype=O.MSG_DESC)[0]
        assert oracle_message(rec, arena) == out, m            # ... and the oracle gives the pinned bytes too


def test_fixture_generator_check_mode():
    r = subprocess.run([sys.executable, GENERATOR, "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
