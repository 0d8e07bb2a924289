"""A plain-Python model of what stands between a RAOP (AirPlay) datagram and the Apple Lossless decoder: the tests' independent model
of csrc/raop_aes_core.h and of the host element's parsing.

AES-128 here is FIPS-197 as the standard's pseudo code has it, on a 4 x 4 state of bytes: Cipher (SubBytes, ShiftRows, MixColumns,
AddRoundKey) to build cases, and the STRAIGHTFORWARD InvCipher (InvShiftRows, InvSubBytes, AddRoundKey, InvMixColumns, with the
encryption key schedule taken backwards) to check against -- not the equivalent inverse cipher, no T tables, no word arithmetic.  The
S-box is computed: the field inverse by exhaustive search, then the affine map bit by bit.  It imports nothing from the library.

RAOP's packet rule (RaopAudioDecryptor::Decrypt): every packet starts again from the session's IV; plaintext block j is
InvCipher(C_j) xor (IV if j == 0 else C_{j-1}); the len % 16 tail is copied as sent; a packet shorter than 16 bytes is all tail.

The fmtp parse refuses a value that does not fit its field, where the reference truncates it: the one deviation (include/ohgpu.h).
"""


def xtime(a):
    a <<= 1
    return (a ^ 0x11b) & 0xff if a & 0x100 else a


def gmul(a, b):
    p = 0
    while b:
        if b & 1:
            p ^= a
        a = xtime(a)
        b >>= 1
    return p


def _sbox():
    box = []
    for x in range(256):
        inv = 0 if x == 0 else next(y for y in range(1, 256) if gmul(x, y) == 1)
        bits = [(inv >> i) & 1 for i in range(8)]
        out = 0
        for i in range(8):
            bit = bits[i] ^ bits[(i + 4) % 8] ^ bits[(i + 5) % 8] ^ bits[(i + 6) % 8] ^ bits[(i + 7) % 8] ^ ((0x63 >> i) & 1)
            out |= bit << i
        box.append(out)
    return box


SBOX = _sbox()
INV_SBOX = [SBOX.index(x) for x in range(256)]


def key_expansion(key):
    """-> 11 round keys of 16 bytes each (FIPS-197 5.2, Nk = 4)"""
    assert len(key) == 16
    words = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(words[i - 1])
        if i % 4 == 0:
            t = t[1:] + t[:1]
            t = [SBOX[b] for b in t]
            t[0] ^= rcon
            rcon = xtime(rcon)
        words.append([a ^ b for a, b in zip(words[i - 4], t)])
    return [sum(words[4 * r:4 * r + 4], []) for r in range(11)]


# the state is state[row][column]; the block's byte 4 * c + r is row r of column c
def _to_state(block):
    return [[block[4 * c + r] for c in range(4)] for r in range(4)]


def _from_state(s):
    return bytes(s[r][c] for c in range(4) for r in range(4))


def _add_round_key(s, k):
    return [[s[r][c] ^ k[4 * c + r] for c in range(4)] for r in range(4)]


TIMES = {m: [gmul(m, x) for x in range(256)] for m in (1, 2, 3, 9, 11, 13, 14)}        # the field's products, looked up for speed


def _mix(s, m):
    return [[TIMES[m[r][0]][s[0][c]] ^ TIMES[m[r][1]][s[1][c]] ^ TIMES[m[r][2]][s[2][c]] ^ TIMES[m[r][3]][s[3][c]] for c in range(4)] for r in range(4)]


MIX = [[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]]
INV_MIX = [[14, 11, 13, 9], [9, 14, 11, 13], [13, 9, 14, 11], [11, 13, 9, 14]]


def encrypt_block(keys, block):
    s = _add_round_key(_to_state(block), keys[0])
    for r in range(1, 11):
        s = [[SBOX[v] for v in row] for row in s]
        s = [[s[row][(c + row) % 4] for c in range(4)] for row in range(4)]
        if r != 10:
            s = _mix(s, MIX)
        s = _add_round_key(s, keys[r])
    return _from_state(s)


def decrypt_block(keys, block):
    s = _add_round_key(_to_state(block), keys[10])
    for r in range(9, -1, -1):
        s = [[s[row][(c - row) % 4] for c in range(4)] for row in range(4)]
        s = [[INV_SBOX[v] for v in row] for row in s]
        s = _add_round_key(s, keys[r])
        if r != 0:
            s = _mix(s, INV_MIX)
    return _from_state(s)


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def encrypt_packet(key, iv, plain):
    """what a RAOP sender does: CBC over the whole blocks from the IV, the tail in the clear"""
    keys = key_expansion(key)
    out, prev = bytearray(), bytes(iv)
    whole = len(plain) // 16 * 16
    for at in range(0, whole, 16):
        prev = encrypt_block(keys, _xor(plain[at:at + 16], prev))
        out += prev
    return bytes(out) + bytes(plain[whole:])


_keys_cache = {}


def decrypt_packet(key, iv, data):
    """RAOP's packet rule"""
    key = bytes(key)
    if key not in _keys_cache:
        _keys_cache[key] = key_expansion(key)
    keys = _keys_cache[key]
    data = bytes(data)
    out, prev = bytearray(), bytes(iv)
    whole = len(data) // 16 * 16
    for at in range(0, whole, 16):
        out += _xor(decrypt_block(keys, data[at:at + 16]), prev)
        prev = data[at:at + 16]
    return bytes(out) + data[whole:]


# ---- the datagram (RtpPacketRaop::Set + RaopPacketAudio::Set) and the SDP fmtp string (CodecRaopApple::ParseFmtp) ----
MAX_DATAGRAM = 1472


class InvalidRaopPacket(Exception):
    pass


def parse_datagram(d):
    """-> dict(seq, timestamp, ssrc, payload): 4 bytes of RTP header (version and payload type ignored), 8 of timestamp and ssrc"""
    d = bytes(d)
    if len(d) > MAX_DATAGRAM or len(d) < 4 or len(d) - 4 < 8:
        raise InvalidRaopPacket("%d bytes" % len(d))
    return dict(seq=int.from_bytes(d[2:4], "big"), timestamp=int.from_bytes(d[4:8], "big"), ssrc=int.from_bytes(d[8:12], "big"), payload=d[12:])


def make_datagram(seq, timestamp, ssrc, payload, marker=False):
    return bytes([0x80, 0x60 | (0x80 if marker else 0)]) + (seq & 0xffff).to_bytes(2, "big") + (timestamp & 0xffffffff).to_bytes(4, "big") + \
        (ssrc & 0xffffffff).to_bytes(4, "big") + bytes(payload)


FMTP_FIELDS = ("frame_length", "compatible_version", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "max_frame_bytes", "avg_bit_rate", "sample_rate")
_FMTP_BITS = (32, 8, 8, 8, 8, 8, 8, 16, 32, 32, 32)


def parse_fmtp(text):
    """twelve decimal fields separated by blanks, the first ignored -> the configuration as tests/alac_textbook.parse_config gives it"""
    fields = [f for f in text.split(" ") if f]
    if len(fields) < 12:
        raise ValueError("%d fields" % len(fields))
    values = []
    for f in fields[:12]:
        if not (f.isascii() and f.isdigit()) or len(f) > 10:
            raise ValueError("not a number: %r" % f)
        values.append(int(f))
    if values[0] >= 1 << 32:
        raise ValueError("field 0 does not fit")
    cfg = {}
    for name, bits, v in zip(FMTP_FIELDS, _FMTP_BITS, values[1:]):
        if v >= 1 << bits:
            raise ValueError("%s: %d does not fit" % (name, v))
        cfg[name] = v
    if cfg.pop("compatible_version") != 0:
        raise ValueError("compatible version")
    return cfg


def make_fmtp(cfg, payload_type=96):
    return " ".join(str(v) for v in [payload_type] + [0 if name == "compatible_version" else cfg[name] for name in FMTP_FIELDS])
