#!/usr/bin/env python3
"""Writes tests/golden/pcm_textbook.json: what tests/pcm_textbook.py gives for forty descriptors over a seeded source arena (the
output's SHA-256, and the output itself where it is at most 48 bytes) and what tests/flywheel_textbook.py gives for two requests
(SHA-256 and the first two frames).  It uses the models only: no oracle, no library, no device -- so an edit that moves a model
AND the oracle together is noticed.
    python tests/golden/make_pcm_textbook_fixtures.py           # (re)write the file
    python tests/golden/make_pcm_textbook_fixtures.py --check   # regenerate in memory; exit 1 unless byte-identical
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import flywheel_textbook as FT  # noqa: E402
import pcm_textbook as PT  # noqa: E402

OUT = os.path.join(HERE, "pcm_textbook.json")
ARENA_BYTES = 4096
DEPTHS = (8, 16, 24, 32)
RAMPS = ((16384, 0), (0, 16384), (16384, 16384), (0, 0), (8191, 8190), (5, 5), (16384, 16352), (100, 101))
FRAMES = (1, 2, 3, 7, 42, 43, 64)
CHANNELS = (1, 2, 3, 5, 6, 8)


def lcg_bytes(seed, n):
    """SURVEY.md 8d's generator (x = x * 1664525 + 1013904223 mod 2^32), the top byte of each state."""
    x, out = seed & 0xFFFFFFFF, bytearray()
    for _ in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append(x >> 24)
    return bytes(out)


def arena():
    return lcg_bytes(0x9E3779B9, ARENA_BYTES)


def descriptors():
    out = []
    for k in range(40):
        sbits, dbits = DEPTHS[k % 4], DEPTHS[(k // 4 + k) % 4]
        ch, n = CHANNELS[k % 6], FRAMES[k % 7]
        start, end = RAMPS[k % 8]
        kind = ("ramp", "plain", "silence", "ramp", "attenuated")[k % 5]
        flags = {"ramp": PT.FLAG_RAMP, "plain": 0, "silence": PT.FLAG_SILENCE, "attenuated": PT.FLAG_RAMP if k % 2 else 0}[kind]
        if k % 3 == 0:
            flags |= PT.FLAG_ZERO_LSB32
        att = (0, 1, 64, 255, 77)[(k // 5) % 5] if (kind == "attenuated" and sbits == 16) else 256
        out.append({"src_offset": (k * 37) % 1000, "dst_offset": 0, "n_frames": n, "ramp_start": start, "ramp_end": end,
                    "attenuation": att, "channels": ch, "src_bits": sbits, "src_endian": 1 + (k // 2) % 2,
                    "dst_bits": dbits, "dst_endian": 1 + (k // 3) % 2, "flags": flags})
    return out


def flywheel_requests():
    """(name, training bytes, channel_bytes, in_samples, sample_rate, channels, out_frames, block_frames)"""
    reqs = []
    for name, seed, rate, ch, in_samples, extra, out_frames, block in (("noise_44k1_stereo", 11, 44100, 2, 44, 0, 100, 44),
                                                                       ("noise_192k_3ch", 12, 192000, 3, 192, 8, 401, 192)):
        raw = lcg_bytes(seed, ch * (in_samples + extra) * 4)
        reqs.append((name, raw, (in_samples + extra) * 4, in_samples, rate, ch, out_frames, block))
    return reqs


def fixture():
    src = arena()
    msgs = []
    for d in descriptors():
        out = PT.process_message(d, src)
        entry = dict(d)
        entry["sha256"] = hashlib.sha256(out).hexdigest()
        entry["bytes"] = len(out)
        if len(out) <= 48:
            entry["hex"] = out.hex()
        msgs.append(entry)
    fly = []
    for name, raw, cb, ins, rate, ch, outf, block in flywheel_requests():
        y = FT.flywheel_ramp(raw, cb, ins, rate, ch, outf, block)
        fly.append({"name": name, "sample_rate": rate, "channels": ch, "in_samples": ins, "channel_bytes": cb, "out_frames": outf,
                    "block_frames": block, "sha256": hashlib.sha256(y).hexdigest(), "first_frames_hex": y[:8 * ch].hex()})
    return {"about": "tests/pcm_textbook.py and tests/flywheel_textbook.py on seeded inputs "
                     "(tests/golden/make_pcm_textbook_fixtures.py)",
            "arena_sha256": hashlib.sha256(src).hexdigest(), "messages": msgs, "flywheel": fly}


def text(fx):
    lines = ['{"about": %s, "arena_sha256": %s, "messages": [' % (json.dumps(fx["about"]), json.dumps(fx["arena_sha256"]))]
    for i, m in enumerate(fx["messages"]):
        lines.append(" " + json.dumps(m, separators=(",", ":")) + ("," if i + 1 < len(fx["messages"]) else ""))
    lines.append('], "flywheel": [')
    for i, f in enumerate(fx["flywheel"]):
        lines.append(" " + json.dumps(f, separators=(",", ":")) + ("," if i + 1 < len(fx["flywheel"]) else ""))
    lines.append("]}")
    return "\n".join(lines) + "\n"


def main():
    fx = fixture()
    new = text(fx)
    assert json.loads(new) == fx
    if "--check" in sys.argv[1:]:
        with open(OUT) as f:
            old = f.read()
        if old != new:
            print(f"{OUT} differs from what the models give now", file=sys.stderr)
            return 1
        print("ok:", OUT)
        return 0
    with open(OUT, "w") as f:
        f.write(new)
    print("wrote", OUT, len(new), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
