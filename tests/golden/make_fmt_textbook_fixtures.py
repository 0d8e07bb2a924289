#!/usr/bin/env python3
"""Writes tests/golden/fmt_textbook.json: the SHA-256 of what tests/fmt_textbook.py gives for a few seeded batches that mix the
three layout-changing kinds (whole destination arena, 0xA5 where nothing is written).  Hashes and seeds only, no audio.  It uses
the model only: no oracle, no library, no device -- so an edit that moves the model AND the oracle together is noticed.
tests/test_gpu_fmt_textbook.py runs the same batches on the device.
    python tests/golden/make_fmt_textbook_fixtures.py           # (re)write the file
    python tests/golden/make_fmt_textbook_fixtures.py --check   # regenerate in memory; exit 1 unless byte-identical
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import fmt_textbook as FT  # noqa: E402

OUT = os.path.join(HERE, "fmt_textbook.json")
FILL = 0xA5
FRAMES = (1, 2, 3, 5, 44, 63, 64, 65, 240, 513)
SEEDS = {"mixed_a": 0x0F0F1234, "mixed_b": 0x13572468, "mixed_c": 0x2468ACE1}


class Lcg:
    """SURVEY.md 8d's generator (x = x * 1664525 + 1013904223 mod 2^32), the top byte of each state."""

    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFF

    def byte(self):
        self.x = (self.x * 1664525 + 1013904223) & 0xFFFFFFFF
        return self.x >> 24

    def below(self, n):
        return self.byte() % n

    def bytes(self, n):
        return bytes(self.byte() for _ in range(n))


def batch(seed, align16, n_descs=24):
    """(descriptors as dicts, source arena, destination arena bytes): kinds, depths, channel counts 1..10, frame counts and both
    arenas' offsets from the generator; outputs in separate slots with 0..3 bytes of lead and 5 of gap.  a14's plane strides are
    multiples of 16 when `align16` (the staged kernel's condition) and any multiple of 4 otherwise."""
    g = Lcg(seed)
    descs, src, dp = [], bytearray(), 0
    for k in range(n_descs):
        kind = (FT.UNPACK_PLANAR, FT.SENDER_PACK, FT.FLAC_PACK)[g.below(3)]
        ch, n = 1 + g.below(10), FRAMES[g.below(len(FRAMES))]
        d = {"src_offset": 0, "dst_offset": dp + g.below(4), "src_plane_stride": 0, "dst_plane_stride": 0, "n_frames": n, "kind": kind,
             "channels": ch, "src_bits": 0, "dst_bits": 0}
        if kind == FT.FLAC_PACK:
            src += g.bytes((-len(src)) % 4 + 4 * g.below(4))
            stride = 4 * (n + g.below(4))
            if align16:
                stride = (stride + 15) // 16 * 16
            d.update(src_offset=len(src), src_plane_stride=stride, src_bits=32, dst_bits=(8, 16, 24)[g.below(3)])
            src += g.bytes((ch - 1) * stride + 4 * n)
            out = n * ch * d["dst_bits"] // 8
        else:
            sb = 1 + g.below(4)
            src += g.bytes(g.below(5))
            d.update(src_offset=len(src), src_bits=8 * sb)
            src += g.bytes(n * ch * sb)
            if kind == FT.UNPACK_PLANAR:
                d["dst_plane_stride"] = 4 * n + g.below(7)
                out = (ch - 1) * d["dst_plane_stride"] + 4 * n
            else:
                out = n * min(ch, 2) * min(sb, 3)
        descs.append(d)
        dp = d["dst_offset"] + out + 5
    return descs, bytes(src), dp


def batches():
    return {name: batch(seed, name != "mixed_c") for name, seed in SEEDS.items()}


def fixture():
    out = []
    for name, (descs, src, dst_bytes) in batches().items():
        got = FT.batch_bytes(descs, src, dst_bytes, FILL)
        out.append({"name": name, "seed": SEEDS[name], "descriptors": len(descs), "kinds": [d["kind"] for d in descs],
                    "src_bytes": len(src), "src_sha256": hashlib.sha256(src).hexdigest(), "dst_bytes": dst_bytes,
                    "dst_sha256": hashlib.sha256(got).hexdigest()})
    return {"about": "tests/fmt_textbook.py on seeded batches that mix the three kinds (tests/golden/make_fmt_textbook_fixtures.py)",
            "fill": FILL, "batches": out}


def text(fx):
    lines = ['{"about": %s, "fill": %d, "batches": [' % (json.dumps(fx["about"]), fx["fill"])]
    for i, b in enumerate(fx["batches"]):
        lines.append(" " + json.dumps(b, separators=(",", ":")) + ("," if i + 1 < len(fx["batches"]) else ""))
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
            print(f"{OUT} differs from what the model gives now", file=sys.stderr)
            return 1
        print("ok:", OUT)
        return 0
    with open(OUT, "w") as f:
        f.write(new)
    print("wrote", OUT, len(new), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
