"""Makes tests/golden/cbcs/*.json with the machine's `openssl enc -aes-128-cbc -nopad`, never with the model (tests/cbcs_textbook.py) or
the product: the fixtures are what holds the model's inverse cipher and its pattern rule to an implementation neither shares text with.

    python tests/golden/make_cbcs_fixtures.py          (needs /usr/bin/openssl; rewrites the three files)

  sp800_38a_f2.json   SP 800-38A F.2.1 / F.2.2's key, IV and four plaintext blocks through openssl: the cipher text it gives
  chains.json         CBC over 1, 2, 63, 64 and 65 blocks for three keys, each under a 16-byte IV; and one under an 8-byte IV that is
                      zero-extended before openssl sees it
  patterns.json       crypt:skip patterns over parts of several lengths: the blocks the pattern encrypts are taken out, encrypted by ONE
                      openssl CBC call, and put back between the skipped blocks and in front of the tail, which stay as they are"""
import json
import os
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cbcs")
OPENSSL = "/usr/bin/openssl"


def cbc_encrypt(key, iv, plain):
    assert len(plain) % 16 == 0 and len(iv) == 16
    if not plain:
        return b""
    p = subprocess.run([OPENSSL, "enc", "-aes-128-cbc", "-nopad", "-K", key.hex(), "-iv", iv.hex()], input=plain, capture_output=True, check=True)
    assert len(p.stdout) == len(plain)
    return p.stdout


def lcg_bytes(seed, n):
    out, x = bytearray(), seed
    for _ in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out.append(x >> 56)
    return bytes(out)


def pattern_encrypt(key, iv, plain, crypt, skip):
    whole = len(plain) // 16
    mine = [b for b in range(whole) if crypt == 0 or skip == 0 or b % (crypt + skip) < crypt]
    cipher = cbc_encrypt(key, iv, b"".join(plain[16 * b:16 * b + 16] for b in mine))
    out = bytearray(plain)
    for k, b in enumerate(mine):
        out[16 * b:16 * b + 16] = cipher[16 * k:16 * k + 16]
    return bytes(out)


def main():
    os.makedirs(HERE, exist_ok=True)
    key = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
    iv = bytes(range(16))
    plain = bytes.fromhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e5130c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710")
    files = {"sp800_38a_f2.json": dict(key=key.hex(), iv=iv.hex(), plain=plain.hex(), cipher=cbc_encrypt(key, iv, plain).hex())}
    chains = []
    for k in range(3):
        ckey = key if k == 0 else lcg_bytes(100 + k, 16)
        for blocks in (1, 2, 63, 64, 65):
            civ, cplain = lcg_bytes(200 + 7 * k + blocks, 16), lcg_bytes(300 + 11 * k + blocks, 16 * blocks)
            chains.append(dict(key=ckey.hex(), iv=civ.hex(), plain=cplain.hex(), cipher=cbc_encrypt(ckey, civ, cplain).hex()))
    short = lcg_bytes(400, 8)
    cplain = lcg_bytes(401, 16 * 5)
    chains.append(dict(key=key.hex(), iv=short.hex(), plain=cplain.hex(), cipher=cbc_encrypt(key, short + bytes(8), cplain).hex()))
    files["chains.json"] = chains
    patterns = []
    for n, (crypt, skip) in enumerate(((0, 0), (1, 0), (1, 9), (1, 1), (5, 5), (15, 15))):
        period = crypt + skip
        for blocks in sorted({max(crypt - 1, 0), crypt, period, period + 1, 2 * period + 1}):
            for tail in (0, 7):
                pkey, piv = lcg_bytes(500 + n, 16), lcg_bytes(600 + n + blocks, 16)
                pplain = lcg_bytes(700 + 13 * n + blocks + tail, 16 * blocks + tail)
                patterns.append(dict(key=pkey.hex(), iv=piv.hex(), crypt=crypt, skip=skip, plain=pplain.hex(), cipher=pattern_encrypt(pkey, piv, pplain, crypt, skip).hex()))
    files["patterns.json"] = patterns
    for name, content in files.items():
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(content, f, indent=0)
            f.write("\n")


if __name__ == "__main__":
    main()
