"""An independent model of the second protected fragmented MPEG-4 layer (ohgpu_cbcs_*, include/ohgpu_cbcs.h) with the simplest means there
are.  The demultiplexer is tests/mp4f_textbook.py's reader with tests/cenc_textbook.py's walk of the sample entry on top, both imported
and not edited; what this file adds is its own reading of the scheme, of the tenc (version 1, the pattern, the constant IV) and of the
senc's subsample entries, its own inverse cipher -- InvShiftRows, InvSubBytes, AddRoundKey and InvMixColumns on a list of sixteen bytes,
straight from FIPS-197 5.3, with an S-box and a key expansion computed here from the field's arithmetic, no T tables, no equivalent inverse
cipher -- and a sample taken apart part by part in Python slices.  It shares no text with csrc/cbcs_core.h.  With the muxer
pieces of tests/cbcs_cases.py it shares no cipher and no box code; both take a sample apart by the same plain loop over (clear,
protected) pairs, and the pattern rule is one line in each.  The hooks into the sibling models are swaps of their module globals
(FX.Reader here; CC.tenc and FC.trun_node in the cases) and a re-read of the entry over a copy whose schm and tenc read as `cenc`: an
edit to those models is an edit to this one, which tests/test_cbcs_textbook.py holds to openssl and to the muxer's record.

demux(data, codecs, packet_capacity, run_capacity, gather_first_row, dst_capacity, head_only, kid, key, subsample_capacity) -> dict: the
model of tests/cenc_textbook.py's demux, and crypt_blocks, skip_blocks, constant_iv_size, constant_iv, subsamples.

Where this reading differs from the reference's (OpenHome/Media/Codec/Mpeg4.cpp; include/ohgpu_cbcs.h carries the same list), beyond
tests/cenc_textbook.py's list:
  - the reference serves scheme `cenc` only (Mpeg4.cpp:2266); here `cbcs` is served too, and tenc version 1;
  - the reference reads the subsample flag of a senc (Mpeg4.cpp:2478) and hands the entries to its provider; here they are applied."""
import cenc_textbook as CX
import mp4f_textbook as FX

OK, NOT_MP4, TRUNCATED, INVALID, NOT_CODEC, UNSUPPORTED, NOT_FRAGMENTED, NO_KEY = range(8)
RESULT_FIELDS, CONFIG_FIELDS, FLAC_FIELDS, EXTRA_FIELDS = CX.RESULT_FIELDS, CX.CONFIG_FIELDS, CX.FLAC_FIELDS, CX.EXTRA_FIELDS
MORE_FIELDS = ("crypt_blocks", "skip_blocks", "constant_iv_size", "subsamples", "constant_iv")
Refuse, u, code = FX.Refuse, FX.u, FX.code


# ---- the inverse cipher, FIPS-197
def times(a, b):
    """a b in GF(2^8) modulo x^8 + x^4 + x^3 + x + 1"""
    out = 0
    while b:
        if b & 1:
            out ^= a
        a = (a << 1) ^ (0x11b if a & 0x80 else 0)
        b >>= 1
    return out


def _boxes():
    inverse = [0] + [next(y for y in range(1, 256) if times(x, y) == 1) for x in range(1, 256)]
    sbox = []
    for x in range(256):
        b = inverse[x]
        sbox.append(b ^ rot(b, 1) ^ rot(b, 2) ^ rot(b, 3) ^ rot(b, 4) ^ 0x63)
    return sbox, [sbox.index(x) for x in range(256)]


def rot(b, n):
    return ((b << n) | (b >> (8 - n))) & 0xff


SBOX, INV_SBOX = _boxes()
BY = {m: [times(m, x) for x in range(256)] for m in (9, 11, 13, 14)}


def round_keys(key):
    """FIPS-197 5.2: eleven round keys of sixteen bytes"""
    words, rcon = [list(key[4 * i:4 * i + 4]) for i in range(4)], 1
    for i in range(4, 44):
        t = list(words[i - 1])
        if i % 4 == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = times(rcon, 2)
        words.append([a ^ b for a, b in zip(words[i - 4], t)])
    return [sum(words[4 * r:4 * r + 4], []) for r in range(11)]


_keys = {}


def inv_cipher(key, block):
    """FIPS-197 5.3: the state is sixteen bytes, byte r + 4 c is row r of column c"""
    key = bytes(key)
    if key not in _keys:
        _keys[key] = round_keys(key)
    w = _keys[key]
    s = [a ^ b for a, b in zip(block, w[10])]
    for rnd in range(9, -1, -1):
        s = [s[(r + 4 * ((c - r) % 4))] for c in range(4) for r in range(4)]            # InvShiftRows: row r moves r columns to the right
        s = [INV_SBOX[b] for b in s]
        s = [a ^ b for a, b in zip(s, w[rnd])]
        if rnd:
            out = []
            for c in range(4):
                col = s[4 * c:4 * c + 4]
                for r in range(4):
                    out.append(BY[14][col[r]] ^ BY[11][col[(r + 1) % 4]] ^ BY[13][col[(r + 2) % 4]] ^ BY[9][col[(r + 3) % 4]])
            s = out
    return bytes(s)


def cbc_iv(iv):
    """an IV of 8 bytes is the first half, the second half zero"""
    return bytes(iv) + bytes(16 - len(iv))


def encrypted_blocks(whole, crypt, skip):
    """the indices of the encrypted ones among a part's `whole` whole blocks"""
    return [b for b in range(whole) if crypt == 0 or skip == 0 or b % (crypt + skip) < crypt]


def cbcs_part(key, iv, part, crypt, skip):
    """one protected part -> (its clear bytes, the inverse-cipher blocks computed)"""
    out, prev = bytearray(part), cbc_iv(iv)
    mine = encrypted_blocks(len(part) // 16, crypt, skip)
    for b in mine:
        cipher = bytes(part[16 * b:16 * b + 16])
        out[16 * b:16 * b + 16] = bytes(x ^ y for x, y in zip(inv_cipher(key, cipher), prev))
        prev = cipher
    return bytes(out), len(mine)


def clear_sample(scheme, key, iv, sample, entries, crypt, skip):
    """entries: [(clear_bytes, protected_bytes)] or None for one protected part -> (the clear sample, the cipher blocks computed)"""
    entries = [(0, len(sample))] if not entries else entries
    assert sum(c + p for c, p in entries) == len(sample)
    out, at, blocks, used = [], 0, 0, 0
    stream = CX.keystream(key, iv, sum(p for _, p in entries)) if scheme == code(b"cenc") else b""
    for clear, prot in entries:
        out.append(sample[at:at + clear])
        part = sample[at + clear:at + clear + prot]
        if scheme == code(b"cenc"):
            out.append(bytes(a ^ b for a, b in zip(part, stream[used:used + prot])))
            blocks += (used % 16 + prot + 15) // 16 if prot else 0
            used += prot
        else:
            got, n = cbcs_part(key, iv, part, crypt, skip)
            out.append(got)
            blocks += n
        at += clear + prot
    return b"".join(out), blocks


# ---- the boxes
class Reader(CX.Reader):
    def __init__(self, data, codecs, head_only, kid, key):
        super().__init__(data, codecs, head_only, kid, key)
        self.judged_runs = 0
        self.parts = []                 # a (IV, entries or None) a sample of a protected track's runs, in order

    def protected_entry(self, t, entry, end):
        data = self.data
        found = self.first_boxes(entry, end)
        shaped = found is not None and all(k in found for k in (b"frma", b"schm", b"tenc")) and found[b"frma"][2] - found[b"frma"][1] >= 4 and found[b"schm"][2] - found[b"schm"][1] >= 12
        if not shaped:
            return super().protected_entry(t, entry, end)          # (the sibling's INVALIDs: the rules are the same up to here)
        more = self.entry_seen
        more.update(crypt_blocks=0, skip_blocks=0, constant_iv_size=0, constant_iv=bytes(16))
        scheme = u(data, found[b"schm"][1] + 4, 4)
        if scheme not in (code(b"cenc"), code(b"cbcs")):
            raise Refuse(UNSUPPORTED, found[b"schm"][0])
        tenc, pay, tenc_end = found[b"tenc"]
        if tenc_end - pay < 24:
            raise Refuse(INVALID, tenc)
        if data[pay] > 1:
            raise Refuse(UNSUPPORTED, tenc)
        pattern, prot, ivs = data[pay + 5] if data[pay] == 1 else 0, data[pay + 6], data[pay + 7]
        if prot > 1:
            raise Refuse(INVALID, tenc)
        constant = b""
        if prot == 1:
            if ivs == 0:
                if tenc_end - pay < 25 or tenc_end - pay - 25 < data[pay + 24]:
                    raise Refuse(INVALID, tenc)
                constant = data[pay + 25:pay + 25 + data[pay + 24]]
                if len(constant) not in (8, 16):
                    raise Refuse(UNSUPPORTED, tenc)
            if scheme == code(b"cenc") and (pattern or ivs not in (8, 16)):
                raise Refuse(UNSUPPORTED, tenc)
            if scheme == code(b"cbcs") and (ivs not in (0, 8, 16) or (pattern >> 4 == 0 and pattern & 15)):
                raise Refuse(UNSUPPORTED, tenc)
        # the codec's own children by the sibling's text, over a copy whose schm and tenc read as its own: same sizes, same places
        copy = bytearray(data)
        copy[found[b"schm"][1] + 4:found[b"schm"][1] + 8] = b"cenc"
        copy[pay] = 0
        if prot == 1:
            copy[pay + 7] = 8
        self.data = bytes(copy)
        try:
            super().protected_entry(t, entry, end)
        finally:
            self.data = data
        more.update(scheme=scheme, iv_size=ivs if prot else 0)
        if prot:
            more.update(crypt_blocks=pattern >> 4, skip_blocks=pattern & 15, constant_iv_size=len(constant), constant_iv=bytes(constant) + bytes(16 - len(constant)))
        more["constant"] = bytes(constant)

    def first_boxes(self, entry, end):
        """the first frma, schm and tenc of the entry's first sinf, where the sibling looks for them: {kind: (box, payload, end)}"""
        data = self.data
        inner = FX.Counter(FX.ENTRY_BOXES)
        _, _, body, entry_end = next(FX.boxes(data, entry, end, inner))
        if entry_end - body < 28:
            return None
        found = {}
        for kind, child, pay, child_end in FX.boxes(data, body + 28, entry_end, inner):
            if kind != b"sinf" or b"sinf" in found:
                continue
            found[b"sinf"] = child
            for kind2, child2, pay2, end2 in FX.boxes(data, pay, child_end, inner):
                if kind2 in (b"frma", b"schm") and kind2 not in found:
                    found[kind2] = (child2, pay2, end2)
                elif kind2 == b"schi" and b"schi" not in found:
                    found[b"schi"] = child2
                    for kind3, child3, pay3, end3 in FX.boxes(data, pay2, end2, inner):
                        if kind3 == b"tenc" and b"tenc" not in found:
                            found[b"tenc"] = (child3, pay3, end3)
        return found

    def judge(self, traf, senc, seig, samples):
        data, prot = self.data, self.track["prot"]
        runs = list(enumerate(self.runs))[self.judged_runs:]          # the traf's own, whatever the caller's capacities
        self.judged_runs = len(self.runs)
        if seig is not None:
            raise Refuse(UNSUPPORTED, seig)
        if not prot["is_protected"]:
            return
        size = prot["iv_size"]
        if senc is None:
            if samples and size:
                raise Refuse(UNSUPPORTED, traf)
            self.parts += [(prot["constant"], None)] * samples
            return
        box, pay, end = senc
        if end - pay < 8:
            raise Refuse(INVALID, box)
        if data[pay] != 0 or data[pay + 3] & 1:
            raise Refuse(UNSUPPORTED, box)
        if u(data, pay + 4, 4) != samples:
            raise Refuse(INVALID, box)
        listed = bool(data[pay + 3] & 2)
        sizes = [e[0] for _, run in runs for e in FX.run_entries(run)]
        at = pay + 8
        for s in range(samples):
            if end - at < size:
                raise Refuse(INVALID, box)
            iv = data[at:at + size] if size else prot["constant"]
            at += size
            entries = None
            if listed:
                if end - at < 2 or (end - at - 2) // 6 < u(data, at, 2):
                    raise Refuse(INVALID, box)
                entries = [(u(data, at + 2 + 6 * e, 2), u(data, at + 4 + 6 * e, 4)) for e in range(u(data, at, 2))]
                at += 2 + 6 * len(entries)
                if entries and sum(c + p for c, p in entries) != sizes[s]:
                    raise Refuse(INVALID, box)
            self.parts.append((bytes(iv), entries or None))


def _walk(data, codecs, packet_capacity, run_capacity, gather_first_row, dst_capacity, head_only, kid, key):
    r = Reader(data, codecs, head_only, kid, key)
    sibling = FX.Reader
    FX.Reader = lambda d, c, h: r                     # the sibling's demux() over this reader: its Reader is looked up when it runs
    try:
        out = FX.demux(data, codecs, packet_capacity, run_capacity, True, gather_first_row, dst_capacity, head_only)
    finally:
        FX.Reader = sibling
    return r, out


def demux(data, codecs=3, packet_capacity=1 << 20, run_capacity=1 << 20, gather_first_row=0, dst_capacity=0, head_only=False, kid=None, key=None,
          subsample_capacity=1 << 20):
    data = bytes(data)
    r, out = _walk(data, codecs, packet_capacity, run_capacity, gather_first_row, dst_capacity, head_only, kid, key)
    kept = 0
    if out["status"] == OK and r.track["prot"]["is_protected"]:
        # the first sample whose entries do not fit what is left of the share ends the rows served, as packet_capacity does
        for s in range(len(out["rows"])):
            count = len(r.parts[s][1] or ())
            if count > subsample_capacity - kept:
                r, out = _walk(data, codecs, s, run_capacity, gather_first_row, dst_capacity, head_only, kid, key)
                break
            kept += count
    out.update(entry=0, scheme=0, is_protected=0, iv_size=0, kid=bytes(16), blocks=0, clear_rows=[(0, 0)] * len(out["rows"]),
               crypt_blocks=0, skip_blocks=0, constant_iv_size=0, constant_iv=bytes(16), subsamples=0)
    if out["status"] == NO_KEY:                       # what moov gave is kept
        head = demux(data, codecs, head_only=True)
        out.update({k: head[k] for k in ("codec", "track_id", "timescale", "duration", "entry_rate", "entry_channels", "entry_bits", "moov_offset", "config", "flac")})
    if out["status"] not in (OK, NO_KEY):
        return out
    prot = r.track["prot"]
    out.update(entry=prot["entry"] or r.track["codec"], scheme=prot["scheme"], is_protected=prot["is_protected"], iv_size=prot["iv_size"], kid=bytes(prot["kid"]))
    out.update({k: prot[k] for k in MORE_FIELDS if k in prot and k != "subsamples"})
    out["subsamples"] = kept
    if not out["bytes_gathered"]:
        return out
    clear, at = [], 0
    for row in range(gather_first_row, out["samples_available"]):
        place, size = out["rows"][row]
        sample = data[place:place + size]
        if prot["is_protected"]:
            iv, entries = r.parts[row]
            sample, blocks = clear_sample(prot["scheme"], key, iv, sample, entries, prot["crypt_blocks"], prot["skip_blocks"])
            out["blocks"] += blocks
        out["clear_rows"][row] = (at, size)
        clear.append(sample)
        at += size
    out["gathered"] = b"".join(clear)
    assert len(out["gathered"]) == out["bytes_gathered"]
    return out
