"""Makes tests/golden/alac/: Apple Lossless packets from the reference tree's own encoder (alac_encode_driver.cpp beside this file,
compiled into a temporary directory against <reference>/thirdparty/apple_alac/codec).  The PCM comes from tests/alac_cases.py, by
integer arithmetic from a seed, so only the packets, the cookie and the PCM's SHA-256 are committed.  Runs only where the reference
tree exists; no test runs it.

    python tests/golden/make_alac_fixtures.py /path/to/reference
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import alac_cases  # noqa: E402

CODEC_SOURCES = ["EndianPortable.c", "ALACBitUtilities.c", "ALACEncoder.cpp", "ag_enc.c", "ag_dec.c", "dp_enc.c", "matrix_enc.c"]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    codec = os.path.join(sys.argv[1], "thirdparty", "apple_alac", "codec")
    out_dir = os.path.join(HERE, "alac")
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "alac_encode_driver")
        subprocess.check_call(["g++", "-O1", "-w", "-I", codec, "-o", exe, os.path.join(HERE, "alac_encode_driver.cpp")]
                              + [os.path.join(codec, s) for s in CODEC_SOURCES])
        for name, (bits, channels, rate, frame_length, frames, kind, seed, fast) in alac_cases.FIXTURES.items():
            pcm = alac_cases.pcm_bytes(alac_cases.fixture_samples(name), bits)
            pcm_path, bin_path, meta_path = (os.path.join(tmp, name + ext) for ext in (".pcm", ".bin", ".meta"))
            with open(pcm_path, "wb") as f:
                f.write(pcm)
            subprocess.check_call([exe, str(bits), str(channels), str(rate), str(frame_length), "1" if fast else "0", pcm_path, bin_path, meta_path])
            with open(meta_path) as f:
                lines = f.read().split()
            with open(bin_path, "rb") as f:
                blob = f.read()
            sizes = [int(x) for x in lines[1:]]
            assert sum(sizes) == len(blob)
            meta = dict(name=name, cookie=lines[0], packet_sizes=sizes, rate=rate, channels=channels, bits=bits, frame_length=frame_length,
                        frames=frames, pcm_kind=kind, pcm_seed=seed, fast_mode=fast, pcm_sha256=alac_cases.sha256(pcm))
            with open(os.path.join(out_dir, name + ".bin"), "wb") as f:
                f.write(blob)
            with open(os.path.join(out_dir, name + ".json"), "w") as f:
                json.dump(meta, f, indent=1)
                f.write("\n")
            print(name, len(blob), "bytes in", len(sizes), "packets")


if __name__ == "__main__":
    main()
