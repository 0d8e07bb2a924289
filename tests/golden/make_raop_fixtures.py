"""Makes tests/golden/raop_textbook.json: a handful of RAOP sessions -- key, IV, fmtp string and the full RTP datagrams -- wrapping the
packets of the committed Apple Lossless fixtures that fit a datagram, encrypted as a RAOP sender encrypts them (AES-128-CBC over the
whole blocks of each packet from the session's IV, the tail in the clear).

The encryption is the SYSTEM's libcrypto (AES_set_encrypt_key + AES_cbc_encrypt through ctypes), not tests/raop_textbook.py and not
the library: the golden file is independent of both implementations, and both must reproduce it.  Keys, IVs and the RTP fields come
from a fixed-seed generator.  Run from the repository root:  python tests/golden/make_raop_fixtures.py
"""
import ctypes
import ctypes.util
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import alac_cases as AC          # noqa: E402
import raop_textbook as R        # noqa: E402

SESSIONS = ("stereo16_noise_fl256", "mono16_fl256", "stereo16_silence_fl256", "mono24_noise_fl256")


def libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        raise SystemExit("no libcrypto on this machine")
    lib = ctypes.CDLL(name)
    lib.AES_set_encrypt_key.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
    lib.AES_cbc_encrypt.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    return lib


def encrypt(lib, key, iv, plain):
    schedule = ctypes.create_string_buffer(256)                 # AES_KEY: 60 words and a count
    assert lib.AES_set_encrypt_key(key, 128, schedule) == 0
    whole = len(plain) // 16 * 16
    out = ctypes.create_string_buffer(max(whole, 1))
    ivec = ctypes.create_string_buffer(bytes(iv), 16)
    if whole:
        lib.AES_cbc_encrypt(bytes(plain[:whole]), out, whole, schedule, ivec, 1)
    return out.raw[:whole] + bytes(plain[whole:])


def main():
    lib = libcrypto()
    rng = AC.Lcg(20260)
    sessions = []
    for name in SESSIONS:
        fx = AC.load_fixture(name)
        key = bytes(rng.next() & 0xff for _ in range(16))
        iv = bytes(rng.next() & 0xff for _ in range(16))
        seq, timestamp, ssrc = rng.next() & 0xffff, rng.next() * 512 + rng.next() % 512, rng.next() * 512 + 7
        datagrams, stream = [], b""
        for k, packet in enumerate(fx["packets"]):
            payload = encrypt(lib, key, iv, packet)
            d = R.make_datagram(seq + k, timestamp + k * fx["cfg"]["frame_length"], ssrc, payload, marker=k == 0)
            assert len(d) <= R.MAX_DATAGRAM, (name, len(d))
            datagrams.append(d.hex())
            stream += payload
        sessions.append(dict(fixture=name, key=key.hex(), iv=iv.hex(), fmtp=R.make_fmtp(fx["cfg"]), datagrams=datagrams,
                             ciphertext_sha256=hashlib.sha256(stream).hexdigest()))
    with open(os.path.join(HERE, "raop_textbook.json"), "w") as f:
        json.dump(dict(sessions=sessions), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
