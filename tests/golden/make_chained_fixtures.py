"""Writes the chained files of tests/chained_cases.py into tests/golden/vorbis: each as NAME.ogg.gz, and chains.json with, per
file and link, the serial, where the link begins, its packets, channels, rate, block sizes, samples and the MD5 of the model's PCM
(tests/vorbis_textbook.py) as interleaved big-endian 16-bit frames.  tests/test_chained_fixtures.py holds the generators and the
models to these files: run this only when a chain or a model is meant to change.

    python tests/golden/make_chained_fixtures.py
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import chained_cases as KC  # noqa: E402


def main():
    out = os.path.join(HERE, "vorbis")
    table = {}
    for chain in KC.CHAINS:
        with open(os.path.join(out, chain + ".ogg.gz"), "wb") as f:
            f.write(gzip.compress(KC.ogg(chain), 9, mtime=0))
        table[chain] = KC.table_entry(chain)
    with open(os.path.join(out, "chains.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
