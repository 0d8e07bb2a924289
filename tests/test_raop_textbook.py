"""The plain-Python RAOP model (tests/raop_textbook.py) against the published answers and, where the machine has one, the system's
libcrypto: FIPS-197's two worked examples in both directions, SP 800-38A's CBC-AES128 decryption vector, S-box spot values, round
trips, RAOP's packet rule against AES_cbc_encrypt followed by the reference's tail copy for every length 0..96 and a few hundred
fixed-seed (key, IV, length) cases, the committed sessions (made by libcrypto, not by the model), the datagram and fmtp parses, and the
library's host-only fmtp parser against the model's."""
import ctypes
import ctypes.util
import hashlib

import pytest

import alac_cases as AC
import raop_cases as RC
import raop_textbook as R

H = bytes.fromhex


def test_sbox_spot_values():
    assert R.SBOX[0x00] == 0x63 and R.SBOX[0x01] == 0x7c and R.SBOX[0x53] == 0xed and R.SBOX[0xff] == 0x16      # FIPS-197 figure 7, 4.2's example
    assert R.INV_SBOX[0x63] == 0x00 and R.INV_SBOX[0x00] == 0x52 and R.INV_SBOX[0xed] == 0x53
    assert sorted(R.SBOX) == list(range(256))
    assert R.gmul(0x57, 0x83) == 0xc1 and R.gmul(0x57, 0x13) == 0xfe                                                  # FIPS-197 4.2, 4.2.1


@pytest.mark.parametrize("key, plain, cipher", [
    ("000102030405060708090a0b0c0d0e0f", "00112233445566778899aabbccddeeff", "69c4e0d86a7b0430d8cdb78070b4c55a"),     # FIPS-197 C.1
    ("2b7e151628aed2a6abf7158809cf4f3c", "3243f6a8885a308d313198a2e0370734", "3925841d02dc09fbdc118597196a0b32"),     # FIPS-197 appendix B
])
def test_fips_197_examples_both_ways(key, plain, cipher):
    keys = R.key_expansion(H(key))
    assert R.encrypt_block(keys, H(plain)) == H(cipher)
    assert R.decrypt_block(keys, H(cipher)) == H(plain)


def test_key_expansion_last_word_of_appendix_a1():
    assert bytes(R.key_expansion(H("2b7e151628aed2a6abf7158809cf4f3c"))[10][12:]) == H("b6630ca6")


SP_KEY, SP_IV = H("2b7e151628aed2a6abf7158809cf4f3c"), H("000102030405060708090a0b0c0d0e0f")
SP_CIPHER = H("7649abac8119b246cee98e9b12e9197d5086cb9b507219ee95db113a917678b273bed6b8e3c1743b7116e69e222295163ff1caa1681fac09120eca307586e1a7")
SP_PLAIN = H("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e5130c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710")


def test_sp_800_38a_f22_cbc_aes128_decrypt():
    assert R.decrypt_packet(SP_KEY, SP_IV, SP_CIPHER) == SP_PLAIN
    assert R.encrypt_packet(SP_KEY, SP_IV, SP_PLAIN) == SP_CIPHER
    # RAOP's rule on top: a tail goes through as sent, a short packet is all tail, an empty one is nothing
    assert R.decrypt_packet(SP_KEY, SP_IV, SP_CIPHER + b"tail") == SP_PLAIN + b"tail"
    assert R.decrypt_packet(SP_KEY, SP_IV, b"fifteen bytes..") == b"fifteen bytes.." and R.decrypt_packet(SP_KEY, SP_IV, b"") == b""


def test_round_trips():
    rng = AC.Lcg(77)
    for n in (0, 1, 15, 16, 17, 47, 48, 100, 1028):
        key, iv, plain = RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16), RC.rand_bytes(rng, n)
        sent = R.encrypt_packet(key, iv, plain)
        assert len(sent) == n and sent[n // 16 * 16:] == plain[n // 16 * 16:]
        assert R.decrypt_packet(key, iv, sent) == plain
        if n >= 32:
            assert sent[:16] != plain[:16] and R.decrypt_packet(key, bytes(16), sent)[16:] == plain[16:]      # the IV reaches the first block only


def libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    lib = ctypes.CDLL(name)
    if not hasattr(lib, "AES_set_decrypt_key") or not hasattr(lib, "AES_cbc_encrypt"):
        return None
    lib.AES_set_decrypt_key.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
    lib.AES_cbc_encrypt.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    return lib


def reference_decrypt(lib, key, iv, data):
    """RaopAudioDecryptor::Decrypt: AES_cbc_encrypt(..., AES_DECRYPT) over ALL the bytes with a fresh copy of the IV, then the last
    bytes % 16 copied over from the input"""
    schedule = ctypes.create_string_buffer(256)
    assert lib.AES_set_decrypt_key(bytes(key), 128, schedule) == 0
    out = ctypes.create_string_buffer(len(data) + 16)
    ivec = ctypes.create_string_buffer(bytes(iv), 16)
    lib.AES_cbc_encrypt(bytes(data), out, len(data), schedule, ivec, 0)
    rest = len(data) % 16
    got = bytearray(out.raw[:len(data)])
    if rest:
        got[len(data) - rest:] = data[len(data) - rest:]
    return bytes(got)


def test_the_packet_rule_is_libcryptos_cbc_and_the_references_tail_copy():
    lib = libcrypto()
    if lib is None:
        pytest.skip("no libcrypto with AES_set_decrypt_key and AES_cbc_encrypt on this machine")
    rng = AC.Lcg(4711)
    assert reference_decrypt(lib, SP_KEY, SP_IV, SP_CIPHER) == SP_PLAIN
    cases = [(RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16), n) for n in range(97)]
    cases += [(RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16), rng.next() % 1461) for _ in range(300)]
    for key, iv, n in cases:
        data = RC.rand_bytes(rng, n)
        assert R.decrypt_packet(key, iv, data) == reference_decrypt(lib, key, iv, data), (key.hex(), iv.hex(), n)


def test_the_model_reproduces_the_committed_sessions():
    """the golden file was made by libcrypto from the Apple Lossless fixtures' packets: the model must get those packets back"""
    assert [s["fixture"] for s in RC.sessions()] == ["stereo16_noise_fl256", "mono16_fl256", "stereo16_silence_fl256", "mono24_noise_fl256"]
    assert len({s["key"] for s in RC.sessions()}) == 4
    sizes = set()
    for s in RC.sessions():
        assert hashlib.sha256(b"".join(s["payloads"])).hexdigest() == s["sha256"]
        assert [R.decrypt_packet(s["key"], s["iv"], p) for p in s["payloads"]] == s["fx"]["packets"]
        assert [R.encrypt_packet(s["key"], s["iv"], p) for p in s["fx"]["packets"]] == s["payloads"]
        assert {k: v for k, v in s["cfg"].items()} == {k: s["fx"]["cfg"][k] for k in s["cfg"]}
        heads = [R.parse_datagram(d) for d in s["datagrams"]]
        assert [h["seq"] for h in heads] == [(heads[0]["seq"] + k) & 0xffff for k in range(len(heads))] and len({h["ssrc"] for h in heads}) == 1
        assert all(len(d) <= R.MAX_DATAGRAM for d in s["datagrams"])
        sizes |= {len(p) for p in s["payloads"]}
    assert {1028, 44, 32} <= sizes                        # 64 blocks and a tail; two blocks and a tail; whole blocks only


def test_datagram_parse():
    d = R.make_datagram(0xfffe, 0x01020304, 0xa1b2c3d4, b"payload")
    assert R.parse_datagram(d) == dict(seq=0xfffe, timestamp=0x01020304, ssrc=0xa1b2c3d4, payload=b"payload")
    assert R.parse_datagram(bytes([0x00, 0x00]) + d[2:])["payload"] == b"payload"          # version and payload type are not looked at
    assert R.parse_datagram(d[:12])["payload"] == b""
    for bad in (b"", d[:3], d[:4], d[:11], bytes(R.MAX_DATAGRAM + 1)):
        with pytest.raises(R.InvalidRaopPacket):
            R.parse_datagram(bad)
    assert len(R.parse_datagram(bytes(R.MAX_DATAGRAM))["payload"]) == 1460


GOOD_FMTP = "96 352 0 16 40 10 14 2 255 0 0 44100"
BAD_FMTP = ["", "96", "96 352 0 16 40 10 14 2 255 0 0", "96 352 0 16 40 10 14 2 255 0 0 x", "96 352 0 16 40 10 14 2 255 0 0 -1", "96 352 1 16 40 10 14 2 255 0 0 44100",
            "96 352 0 256 40 10 14 2 255 0 0 44100", "96 352 0 16 40 10 14 256 255 0 0 44100", "96 352 0 16 40 10 14 2 65536 0 0 44100",
            "96 4294967296 0 16 40 10 14 2 255 0 0 44100", "96 352 0 16 40 10 14 2 255 0 0 4294967296", "96 352 0 16 4O 10 14 2 255 0 0 44100",
            "96 352 0 16 40 10 14 2 255 0 0 99999999999", "96,352,0,16,40,10,14,2,255,0,0,44100"]


def test_fmtp_parse():
    cfg = R.parse_fmtp(GOOD_FMTP)
    assert cfg == dict(frame_length=352, bit_depth=16, pb=40, mb=10, kb=14, channels=2, max_run=255, max_frame_bytes=0, avg_bit_rate=0, sample_rate=44100)
    assert R.parse_fmtp(R.make_fmtp(cfg)) == cfg and R.parse_fmtp(GOOD_FMTP + " 7 8") == cfg and R.parse_fmtp("0  352 0 16 40 10 14 2 255 0 0 44100") == cfg
    for bad in BAD_FMTP:
        with pytest.raises(ValueError):
            R.parse_fmtp(bad)


def test_the_librarys_fmtp_parse_agrees_with_the_model():
    from ohpipeline_amd import capi
    for text in [GOOD_FMTP, GOOD_FMTP + " 7 8", "0  352 0 16 40 10 14 2 255 0 0 44100", "96 4096 0 24 40 10 14 1 65535 4294967295 1 48000"] + [s["fmtp"] for s in RC.sessions()]:
        got, want = capi.raop_fmtp_parse(text), R.parse_fmtp(text)
        assert {k: int(got[k]) for k in want} == want and int(got["compatible_version"]) == 0
    for bad in BAD_FMTP:
        with pytest.raises(capi.OhGpuError) as e:
            capi.raop_fmtp_parse(bad)
        assert e.value.code == capi.ERR_INVALID, bad
