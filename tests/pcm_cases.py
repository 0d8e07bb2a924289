"""What the PCM message path's GPU tests share (tests/test_gpu_pcm_textbook.py, tests/test_gpu_far_offsets.py): the kinds of message
and the path each is planned onto, the batch builder, and the expected destination arena -- tests/pcm_textbook.py for messages the
model is fast enough for, the oracle that tests/test_pcm_textbook.py ties to it for larger ones.  TEST INFRASTRUCTURE ONLY."""
import hashlib

import numpy as np

import oracle_lib as O
import pcm_textbook as PT

LE, BE = O.ENDIAN_LITTLE, O.ENDIAN_BIG
kMax = O.RAMP_MAX
DEPTHS = [8, 16, 24, 32]
ENDIANS = [(BE, BE), (LE, BE), (BE, LE), (LE, LE)]
MODEL_MAX_SUB = 520            # subsamples per message the pure-Python model serves; beyond that the oracle (tied to it on the CPU)
FILL = 0xA5
PLAIN, RAMPED, ATTENUATED, SILENT = "plain", "ramped", "attenuated", "silent"


_WANT = {}


def expected(descs, src, dst_bytes):
    """(kept per input: `vctx` runs every test twice on the same seeded bytes, and the model is slow)"""
    key = hashlib.sha256(descs.tobytes() + src.tobytes() + dst_bytes.to_bytes(8, "little")).digest()
    if key not in _WANT:
        _WANT[key] = _expected(descs, src, dst_bytes)
    return _WANT[key]


def _expected(descs, src, dst_bytes):
    dst = np.full(dst_bytes, FILL, dtype=np.uint8)
    for d in descs:
        n_sub = int(d["n_frames"]) * int(d["channels"])
        if n_sub <= MODEL_MAX_SUB:
            out = np.frombuffer(PT.process_message(d, src), dtype=np.uint8)
            dst[int(d["dst_offset"]):int(d["dst_offset"]) + out.size] = out
        else:
            one = np.array([d], dtype=O.MSG_DESC)
            assert O.msg_process_batch(one, src if src.size else np.zeros(1, np.uint8), dst) == 0
    return dst


def path_of(sbits, dbits, kind):
    if sbits == 8 or dbits == 8 or kind == SILENT:
        return "staged_chunks"
    return "group_chunks" if kind == PLAIN else "heavy_chunks"


def fields(kind, sbits, k=0):
    """(flags, attenuation, ramp) of a message of `kind`; attenuation exists at 16 bits only (validate_msg, Msg.cpp:2741)."""
    ramp = [(kMax, 0), (0, kMax), (8191, 8190), (12345, 54), (17, 16001)][k % 5]
    if kind == PLAIN:
        return (O.FLAG_ZERO_LSB32 if k % 4 == 1 else 0), 256, ramp
    if kind == RAMPED:
        return O.FLAG_RAMP | (O.FLAG_ZERO_LSB32 if k % 4 == 2 else 0), 256, ramp
    if kind == SILENT:
        return O.FLAG_SILENCE, 256, ramp
    assert sbits == 16
    return (O.FLAG_RAMP if k % 2 else 0), [100, 0, 1, 255, 64][k % 5], ramp


def pack(rng, msgs, sbits, se, dbits, de, src_lead=0, dst_lead=3, src_gap=0, dst_gap=0, dst_tail=5):
    """msgs: [(n_frames, channels, kind)].  Messages back to back in both arenas (plus the gaps asked for), a guard of dst_lead
    bytes before the first and dst_tail after the last."""
    rows, sp, dp = [], src_lead, dst_lead
    for k, (n, ch, kind) in enumerate(msgs):
        flags, att, ramp = fields(kind, sbits, k)
        rows.append((sp, dp, n, ramp[0], ramp[1], att, ch, sbits, se, dbits, de, flags))
        sp += n * ch * sbits // 8 + src_gap
        dp += n * ch * dbits // 8 + dst_gap
    src = rng.integers(0, 256, size=sp, dtype=np.uint8)
    return np.array(rows, dtype=O.MSG_DESC), src, dp + dst_tail
