"""Writes tests/golden/vorbis: every stream of tests/vorbis_cases.py (SHAPES and TREMOR_SHAPES) as an Ogg file, gzipped, and streams.json
with, per stream, its channels, packets and samples and the MD5 of the model's PCM (tests/vorbis_textbook.py) as interleaved big-endian
16-bit frames.  tests/test_vorbis_fixtures.py holds the generators and the model to these files: run this only when a stream or the
model is meant to change.

    python tests/golden/make_vorbis_fixtures.py
"""
import gzip
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vorbis_cases as VC  # noqa: E402


def main():
    out = os.path.join(HERE, "vorbis")
    os.makedirs(out, exist_ok=True)
    table = {}
    for name in list(VC.SHAPES) + list(VC.TREMOR_SHAPES):
        st, (recs, _, pcm) = VC.stream(name), VC.expected(name)
        with open(os.path.join(out, name + ".ogg.gz"), "wb") as f:
            f.write(gzip.compress(VC.ogg(name), 9, mtime=0))
        table[name] = dict(channels=st.model.channels, packets=len(st.packets), samples=int(pcm.shape[1]), pcm_md5=hashlib.md5(VC.pcm_s16be(pcm)).hexdigest())
    with open(os.path.join(out, "streams.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
