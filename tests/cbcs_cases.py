"""What the tests of the second protected MPEG-4 family (ohgpu_cbcs_*) share: the muxer pieces of their own -- a tenc of either version
with its pattern and constant IV, a senc with subsample entries, the ENCRYPTION of a sample part by part under either scheme -- on top of
tests/cenc_cases.py's and tests/mp4f_cases.py's builders, which are imported and not edited; the muxer's own record of every clear sample;
the named good and malformed files; the fixed-seed damage; and the batches: the arenas, the descriptors with their shares of the
subsample table, and what the model (tests/cbcs_textbook.py) says every output must be.  The encryptor here uses the FORWARD cipher of
tests/raop_textbook.py (through cenc_textbook.keystream_block); the model decrypts with an inverse cipher of its own."""
import functools
import struct

import numpy as np

import cbcs_textbook as BX
import cenc_cases as CC
import cenc_textbook as CX
import mp4f_cases as FC

FILL, GUARD_ROWS, GUARD_BYTES = FC.FILL, FC.GUARD_ROWS, FC.GUARD_BYTES
Node, Lcg = FC.Node, FC.Lcg
ALAC, FLAC = FC.ALAC, FC.FLAC
KEY, KID, key_of, kid_of = CC.KEY, CC.KID, CC.key_of, CC.kid_of
CENC, CBCS = b"cenc", b"cbcs"
WRAP_IV = bytes.fromhex("0001020304050607fffffffffffffffe")
PATTERNS = ((0, 0), (1, 0), (1, 9), (1, 1), (5, 5), (15, 15))
EDGE_PARTS = (0, 1, 15, 16, 17, 31, 32, 33)
CLEAR_PARTS = (0, 1, 15, 16, 17)
PIECE_BLOCKS = (63, 64, 65, 128, 129)
CTR_PARTS = (5, 11, 16, 1, 40)               # the keystream is entered at offsets 0, 5, 16, 32 and 33


def tenc(kid=KID, iv_size=8, is_protected=1, version=0, short=0, pattern=(0, 0), constant_iv=None, pattern_byte=None):
    """a tenc of either version; constant_iv: bytes, written (with their length) behind the KID"""
    byte = (pattern[0] << 4 | pattern[1]) if pattern_byte is None else pattern_byte
    body = bytes([version, 0, 0, 0, 0, byte, is_protected, iv_size]) + kid
    if constant_iv is not None:
        body += bytes([len(constant_iv)]) + constant_iv
    return Node(b"tenc", body[:len(body) - short])


def protected_init(codec=FLAC, *, scheme=CBCS, **options):
    """CC.protected_init with this file's tenc: sinf_options takes version, pattern, constant_iv"""
    sibling = CC.tenc
    CC.tenc = tenc
    try:
        opts = dict(options.pop("sinf_options", None) or {}, scheme=scheme)
        return CC.protected_init(codec, sinf_options=opts, **options)
    finally:
        CC.tenc = sibling


# ---- the encryptor
def cbc_iv(iv):
    return bytes(iv) + bytes(16 - len(iv))


def encrypt_part(key, iv, part, crypt, skip):
    out, prev = bytearray(part), cbc_iv(iv)
    for b in range(len(part) // 16):
        if crypt and skip and b % (crypt + skip) >= crypt:
            continue
        prev = CX.keystream_block(key, bytes(x ^ y for x, y in zip(part[16 * b:16 * b + 16], prev)))       # (the forward cipher of one block)
        out[16 * b:16 * b + 16] = prev
    return bytes(out)


def protect(scheme, key, iv, sample, entries, pattern):
    entries = entries or [(0, len(sample))]
    assert sum(c + p for c, p in entries) == len(sample), (entries, len(sample))
    out, at, used = [], 0, 0
    stream = CX.keystream(key, iv, sum(p for _, p in entries)) if scheme == CENC else b""
    for clear, prot in entries:
        out.append(sample[at:at + clear])
        part = sample[at + clear:at + clear + prot]
        out.append(bytes(a ^ b for a, b in zip(part, stream[used:used + prot])) if scheme == CENC else encrypt_part(key, iv, part, *pattern))
        used += prot
        at += clear + prot
    return b"".join(out)


def senc_node(ivs, entries, listed, *, version=0, extra_flags=0, count=None):
    body = b""
    for iv, e in zip(ivs, entries):
        body += iv
        if listed:
            body += struct.pack(">H", len(e or ())) + b"".join(struct.pack(">HI", c, p) for c, p in (e or ()))
    flags = (2 if listed else 0) | extra_flags
    return Node(b"senc", bytes([version]) + flags.to_bytes(3, "big") + struct.pack(">I", len(ivs) if count is None else count) + body)


def mux(init, fragments, *, scheme=CBCS, key=KEY, kid=KID, iv_size=8, constant_iv=None, pattern=(0, 0), layout=None, listed=True, senc="behind", ivs=None,
        protect_samples=True, **record):
    """FC.mux over fragments whose samples are encrypted part by part first and whose trafs get a senc "behind" the truns, in "front" of
    them, or none (None: a constant IV).  layout(i, size) -> [(clear, protected)] or None for sample i of the file; listed: the senc
    has flag 0x2; protect_samples=False lays the samples out as they are (a benchmark's
    file, whose bytes the device decrypts to something).  The record keeps .clear, .entries, .ivs, .key, .kid, .scheme, .pattern."""
    clear, used, parts, made = [], [], [], []
    for f in fragments:
        f = dict(f, runs=[dict(r) for r in f["runs"]])
        filled = [r for r in f["runs"] if r["samples"]]
        traf_ivs, traf_entries = [], []
        for r in f["runs"]:
            secret = []
            for s in r["samples"]:
                i = len(clear)
                iv = constant_iv if constant_iv is not None else ivs[i] if ivs is not None else CC.ivs_for(1, iv_size, i)[0]
                e = layout(i, len(s)) if layout and listed else None
                secret.append(protect(scheme, key, iv, s, e, pattern) if protect_samples else s)
                clear.append(s)
                traf_ivs.append(b"" if constant_iv is not None else iv)
                traf_entries.append(e)
                used.append(iv)
            r["samples"] = secret
        parts += traf_entries
        if senc is not None and filled:
            (filled[0] if senc == "front" else filled[-1])["senc"] = (senc, senc_node(traf_ivs, traf_entries, listed))
        made.append(f)
    plain = FC.trun_node

    def trun_and_senc(r, offset):
        node = plain(r, offset)
        if "senc" not in r:
            return node
        return CC.Beside(r["senc"][1], node) if r["senc"][0] == "front" else CC.Beside(node, r["senc"][1])

    FC.trun_node = trun_and_senc
    try:
        m = FC.mux(init, made, **record)
    finally:
        FC.trun_node = plain
    m.clear, m.ivs, m.entries, m.key, m.kid, m.protected, m.scheme, m.pattern = clear, used, parts, key, kid, True, scheme, pattern
    m.subsamples = sum(len(e or ()) for e in parts)
    return m


def sample_bytes(i, size, seed):
    return bytes((7 * j + 3 * i + seed) & 0xff for j in range(size))


def build(sizes, *, counts=None, codec=FLAC, scheme=CBCS, seed=1, iv_size=8, constant_iv=None, version=None, pattern=(0, 0), key=KEY, kid=KID, runs_of=None,
          samples=None, durations=None, init=None, **options):
    """a file of samples of `sizes` (or the given samples), counts[k] of them in fragment k (one run a fragment, or runs_of[k] = the
    runs' counts), under a tenc made to match"""
    counts = counts or [len(sizes)]
    samples = samples or [sample_bytes(i, n, seed) for i, n in enumerate(sizes)]
    durations = durations or [1 + (5 * i) % 7 for i in range(len(samples))]
    fragments, at = [], 0
    for k, n in enumerate(counts):
        runs = []
        for j, m in enumerate(runs_of[k] if runs_of else [n]):
            runs.append(FC.run(samples[at:at + m], durations[at:at + m], gap=5 if j else 0))
            at += m
        fragments.append(FC.fragment(runs, sequence=k + 1))
    version = (1 if pattern != (0, 0) or constant_iv is not None else 0) if version is None else version
    opts = dict(kid=kid, iv_size=0 if constant_iv is not None else iv_size, version=version, pattern=pattern, constant_iv=constant_iv)
    big = max([len(s) for s in samples] + [1])
    init = dict(dict(info=FC.streaminfo(max_block=max(4096, big))) if codec == FLAC else {}, **(init or {}))
    return mux(protected_init(codec, scheme=scheme, sinf_options=opts, **init), fragments, codec=codec, scheme=scheme, key=key, kid=kid, iv_size=iv_size,
               constant_iv=constant_iv, pattern=pattern, **options)


def flac_file(name, per_fragment, k, **how):
    """-> (a committed FLAC fixture cut into fragments and protected as `how` says under key k, the same audio muxed clear)"""
    base = FC.flac_file(name, per_fragment)
    fx = base.fixture
    samples = [base.data[o:o + s] for o, s in zip(base.offsets, base.sizes)]
    counts = [min(per_fragment, len(samples) - at) for at in range(0, len(samples), per_fragment)]
    m = build(None, samples=samples, durations=base.frames, counts=counts, key=key_of(k), kid=kid_of(k),
                 init=dict(info=fx.data[8:42], timescale=fx.info["sample_rate"], entry_channels=fx.info["channels"], entry_bits=fx.info["bits"], mehd=(0, fx.info["total_samples"])), **how)
    m.fixture = fx
    return m, base


def alac_file(name, per_fragment, k, **how):
    """a committed Apple Lossless fixture cut into fragments and protected as `how` says under key k"""
    base = FC.alac_file(name, per_fragment)
    fx, cfg = base.fixture, base.cfg
    counts = [min(per_fragment, len(fx["packets"]) - at) for at in range(0, len(fx["packets"]), per_fragment)]
    m = build(None, samples=list(fx["packets"]), durations=base.frames, counts=counts, codec=ALAC, key=key_of(k), kid=kid_of(k),
                 init=dict(cookie=fx["cookie"], timescale=cfg["sample_rate"], entry_channels=cfg["channels"], entry_bits=cfg["bit_depth"]), **how)
    m.fixture = fx
    return m


def split_layout(parts):
    """a layout that gives sample i the entries parts[i] (None: no entries)"""
    return lambda i, size: parts[i]


def edge_samples():
    """-> (sizes, entries): a sample a protected part size of EDGE_PARTS with a clear part of every CLEAR_PARTS size in front of a copy of it"""
    entries = [[(c, p) for c in CLEAR_PARTS] for p in EDGE_PARTS]
    return [sum(c + p for c, p in e) for e in entries], entries


def pattern_samples(crypt, skip):
    """parts of crypt - 1, crypt, crypt + skip, crypt + skip + 1 and 2 (crypt + skip) + 1 whole blocks, with tails of 0 and 9 bytes, two parts a sample"""
    period = crypt + skip
    blocks = sorted({max(crypt - 1, 0), crypt, period, period + 1, 2 * period + 1})
    entries = [[(3, 16 * b), (0, 16 * b + 9)] for b in blocks]
    return [sum(c + p for c, p in e) for e in entries], entries


@functools.lru_cache(maxsize=None)
def named_good():
    """-> {name: Fragmented}: every way a good file of the family is written, and files of the sibling's that this family serves too"""
    out = {}
    out["cbcs_whole_samples_iv16"] = build([0, 1, 15, 16, 17, 33, 100], iv_size=16, listed=False, seed=2)
    out["cbcs_whole_samples_iv8_alac"] = build([40, 50, 64], codec=ALAC, iv_size=8, listed=False, seed=3)
    out["cbcs_1_9_constant_iv16_no_senc"] = build([16 * 25 + 3, 7, 16 * 11], constant_iv=bytes(range(0x30, 0x40)), pattern=(1, 9), senc=None, seed=4)
    out["cbcs_1_9_constant_iv8_no_senc_alac"] = build([200, 100, 16], codec=ALAC, constant_iv=bytes(range(0x50, 0x58)), pattern=(1, 9), senc=None, counts=[2, 1], seed=5)
    sizes, entries = edge_samples()
    out["cbcs_edge_parts"] = build(sizes, iv_size=16, layout=split_layout(entries), seed=6)
    out["cbcs_edge_parts_constant_iv8_senc_of_entries_alone"] = build(sizes, constant_iv=bytes(range(0x60, 0x68)), layout=split_layout(entries), seed=7)
    big = [[(1, 16 * b)] if b % 2 else [(0, 16 * b + 5), (16, 0)] for b in PIECE_BLOCKS]
    out["cbcs_parts_of_63_to_129_blocks"] = build([sum(c + p for c, p in e) for e in big], layout=split_layout(big), iv_size=8, seed=8, counts=[3, 2])
    for crypt, skip in PATTERNS:
        sizes, entries = pattern_samples(crypt, skip)
        out[f"cbcs_pattern_{crypt}_{skip}"] = build(sizes, pattern=(crypt, skip), version=1, iv_size=(8, 16)[crypt % 2], layout=split_layout(entries), seed=10 + crypt,
                                                    key=key_of(1 + crypt % 3), kid=kid_of(1 + crypt % 3))
    counts = (0, 1, 2, 3, 17)
    many = [[(0, 0), (4, 0), (0, 20)] if n == 3 else [(2 + (3 * k) % 5, 16 + k)] * n for k, n in enumerate(counts)]      # (three: an empty entry, a clear one, a protected one)
    sizes = [sum(c + p for c, p in e) if e else 37 for e in many]
    out["cbcs_counts_0_1_2_3_17"] = build(sizes, layout=split_layout([e or None for e in many]), iv_size=16, pattern=(1, 1), seed=20)
    out["cenc_counts_0_1_2_3_17"] = build(sizes, scheme=CENC, layout=split_layout([e or None for e in many]), iv_size=8, seed=21)
    ctr = [[(3, p) for p in CTR_PARTS], [(0, 48)], [(1, 15), (2, 2), (0, 31)]]
    out["cenc_keystream_offsets_and_the_wrap"] = build([sum(c + p for c, p in e) for e in ctr], scheme=CENC, iv_size=16, layout=split_layout(ctr), seed=22,
                                                       ivs=[WRAP_IV, bytes(8) + b"\xff" * 8, b"\x11" * 8 + b"\xff" * 7 + b"\xfe"])
    sizes, entries = edge_samples()
    out["cenc_edge_parts_alac"] = build(sizes, scheme=CENC, codec=ALAC, iv_size=8, layout=split_layout(entries), seed=23, init=dict(cookie=FC.PATTERN_COOKIE))
    out["cenc_whole_samples_listed_count_0"] = build([5, 16, 70], scheme=CENC, iv_size=16, layout=lambda i, size: None, seed=24)
    two = [[(1, 30), (0, 20)]] * 5 + [[(4, 16 * 3), (7, 0)]] * 66
    for where in ("front", "behind"):
        out[f"two_truns_under_one_subsample_senc_{where}"] = build([sum(c + p for c, p in e) for e in two], runs_of=[[5, 66]], layout=split_layout(two), iv_size=16,
                                                                   pattern=(1, 1), senc=where, seed=25)
    for name in ("flac_iv8", "alac_iv16", "wrap_inside_three_blocks", "enca_not_protected", "clear_plain_flac", "clear_with_a_senc_skipped", "init_segment_alone"):
        m = CC.named_good()[name]
        m.scheme, m.pattern, m.entries, m.subsamples = CENC, (0, 0), [None] * m.n, 0
        out[f"sibling_{name}"] = m
    return out


at_of, entry_at = CC.at_of, CC.entry_at


@functools.lru_cache(maxsize=None)
def named_malformed():
    """-> {name: (bytes, status, error_offset, codecs, have key, kid)}: one thing wrong each, for every rule of the section"""
    X = BX
    out = {}

    def add(name, data, status, at, codecs=3, have_key=True, kid=KID):
        out[name] = (bytes(data), status, at, codecs, have_key, kid)

    def entry(name, status, where, **kw):
        m = build([20, 30], **kw)
        add(name, m.data, status, at_of(m.data, where))

    for scheme in (b"cbc1", b"cens", b"piff"):
        entry(f"scheme_{scheme.decode()}", X.UNSUPPORTED, b"schm", scheme=scheme, listed=False)
    entry("tenc_version_2", X.UNSUPPORTED, b"tenc", version=2)
    m = mux(protected_init(sinf_options=dict(iv_size=0, version=1, constant_iv=bytes(16), short=1)), [])
    add("constant_iv_leaves_the_tenc", m.data, X.INVALID, at_of(m.data, b"tenc"))
    m = mux(protected_init(sinf_options=dict(iv_size=0, version=1)), [])
    add("constant_iv_size_missing", m.data, X.INVALID, at_of(m.data, b"tenc"))
    for size in (0, 4, 12):
        m = mux(protected_init(sinf_options=dict(iv_size=0, version=1, constant_iv=bytes(size))), [])
        add(f"constant_iv_of_{size}_bytes", m.data, X.UNSUPPORTED, at_of(m.data, b"tenc"))
    entry("cenc_with_a_pattern", X.UNSUPPORTED, b"tenc", scheme=CENC, pattern=(1, 9), listed=False)
    m = mux(protected_init(scheme=CENC, sinf_options=dict(iv_size=0, version=1, constant_iv=bytes(16))), [])
    add("cenc_with_a_constant_iv", m.data, X.UNSUPPORTED, at_of(m.data, b"tenc"))
    for size in (4, 12, 32):
        m = mux(protected_init(sinf_options=dict(iv_size=size)), [])
        add(f"cbcs_iv_size_{size}", m.data, X.UNSUPPORTED, at_of(m.data, b"tenc"))
    entry("cbcs_crypt_0_skip_3", X.UNSUPPORTED, b"tenc", pattern=(0, 3))
    m = mux(protected_init(sinf_options=dict(is_protected=2)), [])
    add("is_protected_2", m.data, X.INVALID, at_of(m.data, b"tenc"))
    m = mux(protected_init(sinf_options=dict(short=1)), [])
    add("tenc_of_23_bytes", m.data, X.INVALID, at_of(m.data, b"tenc"))
    good = build([40, 50, 60, 70], counts=[2, 2], iv_size=16, layout=lambda i, size: [(4, size - 4 - i), (i, 0)], seed=30)
    add("no_key", good.data, X.NO_KEY, at_of(good.data, b"tenc"), have_key=False)
    add("key_of_another_kid", good.data, X.NO_KEY, at_of(good.data, b"tenc"), kid=kid_of(3))
    senc, senc2, traf2 = good.find("senc"), good.find("senc", 1), good.find("traf", 1)
    add("senc_version_1", FC.patched(good, senc[1], 1, 1), X.UNSUPPORTED, senc[0])
    add("senc_overridden_parameters", FC.patched(good, senc2[1], 3, 4), X.UNSUPPORTED, senc2[0])
    add("senc_count_above_the_truns", FC.patched(good, senc[1] + 4, 3), X.INVALID, senc[0])
    add("senc_count_below_the_truns", FC.patched(good, senc2[1] + 4, 1), X.INVALID, senc2[0])
    first_entry = senc[1] + 8 + 16 + 2                   # (sample 0's first entry: u16 clear, u32 protected)
    add("parts_below_the_sample", FC.patched(good, first_entry + 2, 35), X.INVALID, senc[0])
    add("parts_above_the_sample", FC.patched(good, first_entry, 5, 2), X.INVALID, senc[0])
    add("entry_count_leaves_the_senc", FC.patched(good, senc[1] + 8 + 16, 200, 2), X.INVALID, senc[0])
    short = bytearray(good.data)           # the senc ends inside its last entry: the rest becomes a `free` box
    short[senc[0]:senc[0] + 4] = struct.pack(">I", senc[2] - senc[0] - 8)
    short[senc[2] - 8:senc[2]] = struct.pack(">I4s", 8, b"free")
    add("last_entry_leaves_the_senc", short, X.INVALID, senc[0])
    cut = bytearray(good.data)
    cut[senc2[0] + 4:senc2[0] + 8] = b"free"
    add("per_sample_iv_and_no_senc", cut, X.UNSUPPORTED, traf2[0])
    m = build([30, 40], constant_iv=bytes(range(16)), senc=None, seed=31)
    add("constant_iv_and_no_senc_is_served", m.data, X.OK, 0)
    return out


def damaged(count, seed=20270):
    """-> [(bytes, Fragmented)]: fixed-seed damage to good files of the family.  k % 3 == 0: a bit of the protection boxes (sinf and its
    children, senc) is flipped; 1: a bit anywhere in moov or a moof; 2: a bit of a sample (such a file stays OK and decrypts to other bytes)."""
    goods = [m for name, m in named_good().items() if m.protected and m.n and not name.startswith("sibling")]
    rng = Lcg(seed)
    out = []
    for k in range(count):
        m = goods[rng.next() % len(goods)]
        data = bytearray(m.data)
        sinf_at = at_of(m.data, b"sinf")
        spans = [(sinf_at, sinf_at + int.from_bytes(m.data[sinf_at:sinf_at + 4], "big"))] + [(x[1], x[3]) for x in m.marks if x[0].endswith("/senc")]
        if k % 3 == 1:
            spans = [(x[1], x[3]) for x in m.marks if x[0] in ("moov", "moof")]
        elif k % 3 == 2:
            spans = [(o, o + s) for o, s in zip(m.offsets, m.sizes) if s]
        a, b = spans[rng.next() % len(spans)]
        at = a + rng.next() % (b - a)
        data[at] ^= 1 << (rng.next() % 8)
        out.append((bytes(data), m))
    return out


# ---- batches
def stream(data, capacity=None, run_capacity=None, codecs=3, gather_first_row=0, dst_capacity=None, key=None, kid=None, have_key=True, sub_capacity=None):
    if isinstance(data, FC.Fragmented):
        m = data
        return dict(data=m.data, capacity=m.n if capacity is None else capacity, run_capacity=len(m.runs) if run_capacity is None else run_capacity, codecs=codecs,
                    gather_first_row=gather_first_row, dst_capacity=len(m.data) if dst_capacity is None else dst_capacity, key=m.key if key is None else key,
                    kid=m.kid if kid is None else kid, have_key=have_key, sub_capacity=m.subsamples if sub_capacity is None else sub_capacity)
    return dict(data=bytes(data), capacity=8 if capacity is None else capacity, run_capacity=4 if run_capacity is None else run_capacity, codecs=codecs,
                gather_first_row=gather_first_row, dst_capacity=len(data) if dst_capacity is None else dst_capacity, key=KEY if key is None else key,
                kid=KID if kid is None else kid, have_key=have_key, sub_capacity=40 if sub_capacity is None else sub_capacity)


class Job:
    """CC.Job for this family: the same arenas and guards; the descriptors carry the keys and the shares of the subsample table (with
    GUARD_ROWS rows between them); `want_packets` are places in the destination arena and `want_dst` holds the clear bytes."""

    def __init__(self, streams, align=lambda i: (5 * i + 1) % 16, dst_align=lambda i: (7 * i + 3) % 16, models=None):
        from ohpipeline_amd import capi
        self.streams = streams
        src = bytearray()
        self.descs = np.zeros(len(streams), dtype=capi.CBCS_STREAM_DESC)
        row = run_row = sub_row = GUARD_ROWS
        dst = GUARD_BYTES
        for i, s in enumerate(streams):
            while len(src) % 16 != align(i) % 16:
                src.append(0xee)
            while dst % 16 != dst_align(i) % 16:
                dst += 1
            d = self.descs[i]
            d["src_offset"], d["src_bytes"], d["codecs"], d["flags"] = len(src), len(s["data"]), s["codecs"], 1
            d["packet_first"], d["packet_capacity"], d["run_first"], d["run_capacity"] = row, s["capacity"], run_row, s["run_capacity"]
            d["gather_first_row"], d["dst_offset"], d["dst_capacity"] = s["gather_first_row"], dst, s["dst_capacity"]
            d["subsample_first"], d["subsample_capacity"] = sub_row, s["sub_capacity"]
            d["key_flags"] = 1 if s["have_key"] else 0
            d["kid"] = np.frombuffer(s["kid"], dtype=np.uint8)
            if s["have_key"]:
                d["key"] = np.frombuffer(s["key"], dtype=np.uint8)
            src += s["data"]
            row += s["capacity"] + GUARD_ROWS
            run_row += s["run_capacity"] + GUARD_ROWS
            sub_row += s["sub_capacity"] + GUARD_ROWS
            dst += s["dst_capacity"] + GUARD_BYTES
        while len(src) % 4:
            src.append(0xee)
        self.n_packets, self.n_runs, self.n_subsamples, self.dst_bytes = (row, run_row, sub_row, dst) if streams else (0, 0, 0, 0)
        self.src = np.frombuffer(bytes(src), dtype=np.uint8).copy()
        self.models = models or [BX.demux(s["data"], s["codecs"], s["capacity"], s["run_capacity"], s["gather_first_row"], s["dst_capacity"],
                                          kid=s["kid"], key=s["key"] if s["have_key"] else None, subsample_capacity=s["sub_capacity"]) for s in streams]
        self.want_results = np.zeros(len(streams), dtype=capi.CBCS_STREAM_RESULT)
        self.want_packets = np.frombuffer(bytes([FILL]) * (16 * self.n_packets), dtype=capi.ALAC_PACKET).copy()
        self.want_samples = np.frombuffer(bytes([FILL]) * (16 * self.n_packets), dtype=capi.MP4_SAMPLE).copy()
        self.want_runs = np.frombuffer(bytes([FILL]) * (32 * self.n_runs), dtype=capi.MP4F_RUN).copy()
        self.want_dst = np.full(self.dst_bytes, FILL, dtype=np.uint8)
        for i, (d, m) in enumerate(zip(self.descs, self.models)):
            fill_result(self.want_results[i], m)
            first, base, room = int(d["packet_first"]), int(d["src_offset"]), int(d["dst_offset"])
            for s, ((off, size), sm) in enumerate(zip(m["clear_rows"], m["samples_rows"])):
                self.want_packets[first + s] = (room + off, size, 0)
                self.want_samples[first + s] = sm
            for k, (place, frame, first_sample, samples, total) in enumerate(m["run_rows"]):
                self.want_runs[int(d["run_first"]) + k] = ((base + place) & FC.M64, frame, first_sample, samples, total)
            self.want_dst[room:room + len(m["gathered"])] = np.frombuffer(m["gathered"], dtype=np.uint8)

    def driver_blob(self):
        """the job file of tests/cpp/cbcs_core_driver.cpp"""
        return struct.pack("<QQQQQQ", len(self.streams), self.n_packets, self.n_runs, self.n_subsamples, self.src.size, self.dst_bytes) + self.descs.tobytes() + self.src.tobytes()


def fill_result(r, m):
    """a CBCS_STREAM_RESULT record from the model's dict"""
    CC.fill_result(r["cenc"], m)
    for k in BX.MORE_FIELDS:
        r[k] = np.frombuffer(m[k], dtype=np.uint8) if k == "constant_iv" else m[k]


assert_same = FC.assert_same


def check_against_record(model, m, gather_first_row=0):
    """the model's clear bytes are the muxer's own record of the samples"""
    assert model["status"] == BX.OK and model["samples_available"] == m.n, (model["status"], model["error_offset"])
    assert model["gathered"] == b"".join(m.clear[gather_first_row:])
