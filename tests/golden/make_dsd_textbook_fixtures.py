#!/usr/bin/env python3
"""Writes tests/golden/dsd_textbook.json: the SHA-256 of what tests/dsd_textbook.py gives for a few seeded batches that mix the DSD
kinds (whole destination arena, 0xA5 where nothing is written), and the first bytes of each descriptor's output in hex, so that a
reader can see a chunk.  Seeds, hashes and a few dozen bytes, no audio.  It uses the model only: no library, no device.
tests/test_gpu_dsd_textbook.py runs the same batches on the device, tests/test_dsd_textbook.py checks that the file is current.
    python tests/golden/make_dsd_textbook_fixtures.py           # (re)write the file
    python tests/golden/make_dsd_textbook_fixtures.py --check   # regenerate in memory; exit 1 unless byte-identical
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dsd_textbook as DT  # noqa: E402

OUT = os.path.join(HERE, "dsd_textbook.json")
FILL = 0xA5
FORMATS = ((1, 0), (2, 0), (6, 2), (8, 4), (12, 8))
BLOCKS = (1, 2, 3, 7, 16, 65, 130, 513)
SEEDS = {"aligned": 0x0D5D0001, "ragged": 0x0D5D0002, "tails": 0x0D5D0003}


class Lcg:
    """x = x * 1664525 + 1013904223 mod 2^32, the top byte of each state."""

    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFF

    def byte(self):
        self.x = (self.x * 1664525 + 1013904223) & 0xFFFFFFFF
        return self.x >> 24

    def below(self, n):
        return self.byte() % n

    def bytes(self, n):
        return bytes(self.byte() for _ in range(n))


def batch(name, seed, n_descs=14):
    """(descriptors as dicts, source arena, destination arena bytes).  "aligned": every offset a multiple of 16; "ragged": any
    offset; "tails": DSF and DFF only, chunk counts that end inside a block, any offset."""
    g = Lcg(seed)
    descs, src, dp = [], bytearray(), 0
    for k in range(n_descs):
        W, P = FORMATS[g.below(len(FORMATS))]
        per_block = W - P
        kind = (DT.DSF, DT.DFF)[g.below(2)] if name == "tails" else (DT.PASS, DT.DSF, DT.DFF, DT.RAW)[g.below(4)]
        silence = name != "tails" and g.below(6) == 0
        n = BLOCKS[g.below(len(BLOCKS))] * per_block
        if name == "tails" and per_block > 1:
            n += 1 + g.below(per_block - 1)
        if name == "aligned":
            src += g.bytes((-len(src)) % 16)
            dp += (-dp) % 16
        else:
            src += g.bytes(g.below(5))
            dp += g.below(4)
        need, out = DT.layout(kind, W, P, n, silence)
        descs.append({"src_offset": len(src), "dst_offset": dp, "n_chunks": n, "kind": kind, "flags": DT.FLAG_SILENCE if silence else 0,
                      "sample_block_words": W, "pad_bytes_per_chunk": P})
        src += g.bytes(need)
        dp += out + 5
    return descs, bytes(src), dp


def batches():
    return {name: batch(name, seed) for name, seed in SEEDS.items()}


def fixture():
    out = []
    for name, (descs, src, dst_bytes) in batches().items():
        got = DT.batch_bytes(descs, src, dst_bytes, FILL)
        sizes = [DT.layout(d["kind"], d["sample_block_words"], d["pad_bytes_per_chunk"], d["n_chunks"], bool(d["flags"]))[1] for d in descs]
        heads = [got[d["dst_offset"]:d["dst_offset"] + min(size, 2 * (4 + d["pad_bytes_per_chunk"]))].hex() for d, size in zip(descs, sizes)]
        out.append({"name": name, "seed": SEEDS[name], "descriptors": descs, "heads": heads,
                    "src_bytes": len(src), "src_sha256": hashlib.sha256(src).hexdigest(), "dst_bytes": dst_bytes,
                    "dst_sha256": hashlib.sha256(got).hexdigest()})
    return {"about": "tests/dsd_textbook.py on seeded batches that mix the DSD kinds (tests/golden/make_dsd_textbook_fixtures.py)",
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
