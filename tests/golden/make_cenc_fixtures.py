"""Makes tests/golden/cenc/*.json: AES-128 counter-mode keystreams from the machine's `openssl` (never from the model under test), for
triples whose counter does not wrap -- there a library's 128-bit increment and the section's 64-bit one agree --; the three counter
blocks of the wrapping case, each from a single-block ECB call; and SP 800-38A F.5.1.  Run by hand where openssl is; the tests read
the files and need no tool.

    python tests/golden/make_cenc_fixtures.py"""
import json
import os
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cenc")


def openssl(mode, key, data, iv=None):
    cmd = ["openssl", "enc", mode, "-K", key.hex(), "-nopad"] + (["-iv", iv.hex()] if iv is not None else [])
    return subprocess.run(cmd, input=data, capture_output=True, check=True).stdout


def lcg(seed):
    x = seed
    while True:
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        yield (x >> 33) & 0xff


def main():
    os.makedirs(HERE, exist_ok=True)
    rng = lcg(20264)
    triples = []
    lengths = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 100, 255, 256, 257, 1008, 1024, 1040, 2049]
    for k, n in enumerate(lengths):
        key = bytes(next(rng) for _ in range(16))
        iv = bytes(next(rng) for _ in range(8 if k % 2 else 16))
        if len(iv) == 16:
            iv = iv[:8] + bytes([iv[8] & 0x7f]) + iv[9:]          # the low half stays far from its wrap
        stream = openssl("-aes-128-ctr", key, bytes(n), iv + bytes(16 - len(iv)))
        triples.append(dict(key=key.hex(), iv=iv.hex(), length=n, keystream=stream.hex()))
    with open(os.path.join(HERE, "keystreams.json"), "w") as f:
        json.dump(dict(source="openssl enc -aes-128-ctr over zeros; an 8-byte IV is the counter block's first half, the second zero", triples=triples), f, indent=1)
    key = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
    counters = ["0001020304050607fffffffffffffffe", "0001020304050607ffffffffffffffff", "00010203040506070000000000000000"]
    blocks = [dict(counter=c, block=openssl("-aes-128-ecb", key, bytes.fromhex(c)).hex()) for c in counters]
    with open(os.path.join(HERE, "wrap.json"), "w") as f:
        json.dump(dict(source="openssl enc -aes-128-ecb, one block a call", key=key.hex(), iv=counters[0], blocks=blocks), f, indent=1)
    plain = bytes.fromhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e5130c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710")
    iv = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
    with open(os.path.join(HERE, "sp800_38a_f51.json"), "w") as f:
        json.dump(dict(source="SP 800-38A F.5.1 (CTR-AES128.Encrypt), through openssl enc -aes-128-ctr", key=key.hex(), iv=iv.hex(), plaintext=plain.hex(),
                       ciphertext=openssl("-aes-128-ctr", key, plain, iv).hex()), f, indent=1)


if __name__ == "__main__":
    main()
