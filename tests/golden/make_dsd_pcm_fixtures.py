"""Writes tests/golden/dsd_pcm_textbook.json from tests/dsd_pcm_textbook.py: per design the SHA-256 of its Q28 coefficients (little-
endian int32) and the bound sum|coef| / 2^30; per case the seed and the model's first 64 output frames (as packed bytes).  Also
the audio-domain property's measured values (tests/test_dsd_pcm_textbook.py) with the bounds the test holds them to.

    python tests/golden/make_dsd_pcm_fixtures.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import dsd_pcm_cases as DC                  # noqa: E402
import dsd_pcm_textbook as DP               # noqa: E402

CASES = [((8, 8), 0, (2, 0), None, 2), ((8, 8), 1001, (8, 4), (16384, 0), 1), ((16, 24), 7, (6, 2), (0, 16384), 2),
         ((16, 24), 1001, (2, 0), None, 1), ((32, 16), 0, (6, 2), (12345, 54), 2), ((32, 16), 1001, (8, 4), None, 2),
         ((64, 16), 0, (2, 0), None, 1), ((64, 16), 7, (6, 2), (17, 16001), 2)]


def sine_property():
    """A 1 kHz sine at half modulation through a second-order modulator, 2^17 bits, D = 32, T = 16: (fitted amplitude / 2^23,
    residual in dBFS) of the model's output, the filter's edges left out."""
    from test_dsd_pcm_textbook import sine_through_the_model
    return sine_through_the_model()


def main():
    designs = {}
    for key, (dsd_rate, pcm_rate, T) in DC.DESIGNS.items():
        coef = DC.coef(key)
        designs[f"{key[0]}x{key[1]}"] = {"dsd_rate": dsd_rate, "pcm_rate": pcm_rate, "T": T, "beta": DC.BETA, "f_pass": DC.F_PASS, "gain": 1.0,
                                        "coef_sha256": hashlib.sha256(coef.astype("<i4").tobytes()).hexdigest(),
                                        "sum_abs_over_2_30": float(np.abs(coef).sum()) / (1 << 30), "sum": int(coef.sum())}
    cases = []
    for k, (key, out0, fmt, ramp, endian) in enumerate(CASES):
        seed = 9600 + k
        case = DC.Batch(key, seed).add(out0, 64, fmt, "noise", ramp, endian).finish("fixture")
        cases.append({"D": key[0], "T": key[1], "seed": seed, "out_frame0": out0, "format": list(fmt), "ramp": list(ramp) if ramp else None,
                      "dst_endian": endian, "first_64_frames": case.want().tolist()})
    amplitude, residual_db = sine_property()
    out = {"fill": DC.FILL, "designs": designs, "cases": cases,
           "sine": {"amplitude_over_2_23": amplitude, "residual_dbfs": residual_db,
                    "bounds": {"amplitude_low": 0.4995, "amplitude_high": 0.5005, "residual_dbfs_max": round(residual_db + 1.0, 1)}}}
    with open(os.path.join(HERE, "dsd_pcm_textbook.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
