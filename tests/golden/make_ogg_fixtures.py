"""Makes tests/golden/ogg/: thirteen sessions muxed and read back by the reference tree's own page library, through
tools/gen_ogg_golden.c (compiled into a temporary directory against <reference>/thirdparty/libogg).  The byte streams are committed
gzipped (their packets are arithmetic patterns: the two sessions with packets over 64 KiB shrink to a few kilobytes), the records as
sessions.json.  Runs only where the reference tree exists; no test runs it.

    python tests/golden/make_ogg_fixtures.py /path/to/reference
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ogg = os.path.join(sys.argv[1], "thirdparty", "libogg")
    out_dir = os.path.join(HERE, "ogg")
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gen_ogg_golden")
        subprocess.check_call(["gcc", "-O1", "-w", "-I", os.path.join(ogg, "include"), "-o", exe, os.path.join(ROOT, "tools", "gen_ogg_golden.c"),
                               os.path.join(ogg, "src", "framing.c"), os.path.join(ogg, "src", "bitwise.c")])
        subprocess.check_call([exe, tmp])
        with open(os.path.join(tmp, "sessions.json")) as f:
            index = json.load(f)
        for name, rec in index["sessions"].items():
            with open(os.path.join(tmp, name + ".ogg"), "rb") as f:
                raw = f.read()
            assert len(raw) == rec["bytes"]
            with open(os.path.join(out_dir, name + ".ogg.gz"), "wb") as f:
                f.write(gzip.compress(raw, 9, mtime=0))
            print(name, len(raw), "bytes,", len(rec["events"]), "events")
        with open(os.path.join(out_dir, "sessions.json"), "w") as f:
            f.write("{\"sessions\": {\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in index["sessions"].items()) + "\n}}\n")


if __name__ == "__main__":
    main()
