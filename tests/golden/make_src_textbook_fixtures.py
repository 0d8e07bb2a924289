#!/usr/bin/env python3
"""Writes tests/golden/src_textbook.json: for four of ohgpu_src_design's filters, the Q28 table's SHA-256 (int32 LE) and, for the two
seeded inputs of tests/src_textbook.py (fixture_input), the SHA-256 of the textbook model's whole S24 output (int32 LE, frames x
2 channels) and its first 64 frames verbatim.  It uses the model and the library's host-side design only: no oracle, no device.
    python tests/golden/make_src_textbook_fixtures.py           # (re)write the file
    python tests/golden/make_src_textbook_fixtures.py --check   # regenerate in memory; exit 1 unless byte-identical
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import src_textbook as TB  # noqa: E402
from ohpipeline_amd import capi  # noqa: E402

OUT = os.path.join(HERE, "src_textbook.json")
FILTERS = [(44100, 48000, 32), (96000, 48000, 64), (48000, 44100, 32), (32000, 48000, 32)]
BETA, F_PASS = 9.0, 20000.0


def sha256_i32(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def fixture():
    filters = []
    for rin, rout, T in FILTERS:
        L, M, coef = capi.src_design(rin, rout, T, BETA, F_PASS)
        entry = {"rate_in": rin, "rate_out": rout, "T": T, "L": L, "M": M, "beta": BETA, "f_pass": F_PASS,
                 "coef_sha256": sha256_i32(coef), "inputs": []}
        for kind in TB.FIXTURE_INPUTS:
            x = TB.fixture_input(kind, coef, L, M, T)
            y = TB.resample(coef, L, M, T, x, 0, 0, TB.out_frames(L, M, x.shape[0]))
            entry["inputs"].append({"kind": kind, "in_frames": int(x.shape[0]), "out_frames": int(y.shape[0]),
                                    "s24_sha256": sha256_i32(y), "first_64": y[:64].tolist()})
        filters.append(entry)
    return {"about": "ohgpu_src_design tables and the textbook model's S24 output for two seeded inputs "
                     "(tests/src_textbook.py, tests/golden/make_src_textbook_fixtures.py)", "filters": filters}


def text(fx):
    # one line per record: small, and a diff shows which number moved
    lines = ['{"about": %s, "filters": [' % json.dumps(fx["about"])]
    for i, f in enumerate(fx["filters"]):
        head = {k: v for k, v in f.items() if k != "inputs"}
        lines.append(" {%s, \"inputs\": [" % json.dumps(head)[1:-1])
        for j, inp in enumerate(f["inputs"]):
            lines.append("  " + json.dumps(inp, separators=(",", ":")) + ("," if j + 1 < len(f["inputs"]) else ""))
        lines.append(" ]}" + ("," if i + 1 < len(fx["filters"]) else ""))
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
            print(f"{OUT} differs from what the model and the library's designs give now", file=sys.stderr)
            return 1
        print("ok:", OUT)
        return 0
    with open(OUT, "w") as f:
        f.write(new)
    print("wrote", OUT, len(new), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
