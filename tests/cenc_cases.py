"""What the protected MPEG-4 tests share: the muxer pieces of their own (sinf, senc, the encryption of a fragment's samples) on top of
tests/mp4f_cases.py's builders, which are imported and not edited; the muxer's OWN RECORD of every clear sample, IV and key -- the truth
the model (tests/cenc_textbook.py) and the product are held to --; the named good and malformed files; the fixed-seed damage; and the
batches: the arenas, the descriptors, and what the model says every output must be."""
import functools
import struct

import numpy as np

import cenc_textbook as CX
import mp4_cases as MC
import mp4f_cases as FC

FILL, GUARD_ROWS, GUARD_BYTES = FC.FILL, FC.GUARD_ROWS, FC.GUARD_BYTES
Node, full, Lcg = FC.Node, FC.full, FC.Lcg
ALAC, FLAC = FC.ALAC, FC.FLAC
KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
KID = bytes(range(0xa0, 0xb0))
WRAP_IV = bytes.fromhex("0001020304050607fffffffffffffffe")


def key_of(k):
    """key k of the tests: KEY for 0, else made from a fixed-seed generator"""
    rng = Lcg(7000 + k)
    return KEY if k == 0 else bytes(rng.next() & 0xff for _ in range(16))


def kid_of(k):
    return bytes((0xa0 + 17 * k + j) & 0xff for j in range(16))


class Beside(Node):
    """two boxes where the sibling's muxer puts one"""

    def __init__(self, first, second):
        self.first, self.second = first, second

    def emit(self, at, marks, path=""):
        a = self.first.emit(at, marks, path)
        return a + self.second.emit(at + len(a), marks, path)


def tenc(kid=KID, iv_size=8, is_protected=1, version=0, short=0):
    body = bytes([version, 0, 0, 0, 0, 0, is_protected, iv_size]) + kid
    return Node(b"tenc", body[:len(body) - short])


def sinf(codec, *, scheme=b"cenc", drop=(), frma_bytes=4, schm_bytes=12, extra=True, **tenc_options):
    """drop: of "frma", "schm", "schi", "tenc" """
    kids = [Node(b"free", b"x")] if extra else []
    if "frma" not in drop:
        kids.append(Node(b"frma", codec[:frma_bytes]))
    if "schm" not in drop:
        kids.append(Node(b"schm", (bytes(4) + scheme + struct.pack(">I", 0x10000))[:schm_bytes]))
    if "schi" not in drop:
        kids.append(Node(b"schi", ([Node(b"free", b"")] if extra else []) + ([] if "tenc" in drop else [tenc(**tenc_options)])))
    return Node(b"sinf", kids)


def protected_init(codec=FLAC, *, info=FC.PATTERN_INFO, cookie=FC.PATTERN_COOKIE, inner=True, protection=True, sinf_first=True, entry_extra=(), entry_kind=b"enca",
                   sinf_options=None, **init):
    """FC.init_segment with an `enca` entry: the 28-byte head, sinf and the codec's own child, in either order"""
    own = [] if not inner else [Node(b"alac", bytes(4) + cookie)] if codec == ALAC else [FC.dfla(info)]
    guard = [sinf(codec, **(sinf_options or {}))] if protection else []
    kids = [Node(b"free", b"pad")] + list(entry_extra) + (guard + own if sinf_first else own + guard)
    entry = MC.sample_entry(entry_kind, init.pop("entry_channels", 2), init.pop("entry_bits", 16), init.get("timescale", 44100), kids)
    return FC.init_segment(codec, entry=entry, **init)


def senc_node(ivs, *, version=0, flags=0, count=None):
    return Node(b"senc", bytes([version]) + flags.to_bytes(3, "big") + struct.pack(">I", len(ivs) if count is None else count) + b"".join(ivs))


def ivs_for(n, iv_size, seed):
    rng = Lcg(900 + seed)
    return [bytes(rng.next() & 0xff for _ in range(iv_size)) for _ in range(n)]


def mux(init, fragments, *, key=KEY, kid=KID, iv_size=8, senc="behind", ivs=None, protect=True, extra_senc=False, aux=False, **record):
    """FC.mux over fragments whose samples are encrypted first (protect) and whose trafs get a senc: "behind" the truns, in "front" of them,
    or None.  ivs: None (from a fixed seed) or a list a sample, in order.  extra_senc: a second senc of other content behind the first;
    aux: saiz and saio boxes in front of the senc.  The record keeps .clear, the samples as they were, .ivs, .key, .kid."""
    clear, used, made = [], [], []
    for n, f in enumerate(fragments):
        f = dict(f, runs=[dict(r) for r in f["runs"]])
        filled = [r for r in f["runs"] if r["samples"]]
        traf_ivs = []
        for r in f["runs"]:
            mine = [ivs[len(clear) + k] for k in range(len(r["samples"]))] if ivs is not None else ivs_for(len(r["samples"]), iv_size, len(clear))
            clear += r["samples"]
            if protect:
                r["samples"] = [CX.crypt(key, iv, s) for iv, s in zip(mine, r["samples"])]
            traf_ivs += mine
        used += traf_ivs
        if senc is not None and filled:
            node = senc_node(traf_ivs)
            if extra_senc:
                node = Beside(node, senc_node([bytes(len(iv)) for iv in traf_ivs]))
            if aux:
                node = Beside(Beside(full(b"saiz", bytes([iv_size]) + struct.pack(">I", len(traf_ivs))), full(b"saio", struct.pack(">II", 1, 0))), node)
            (filled[0] if senc == "front" else filled[-1])["senc"] = (senc, node)
        made.append(f)
    plain = FC.trun_node

    def trun_and_senc(r, offset):
        node = plain(r, offset)
        if "senc" not in r:
            return node
        return Beside(r["senc"][1], node) if r["senc"][0] == "front" else Beside(node, r["senc"][1])

    FC.trun_node = trun_and_senc
    try:
        m = FC.mux(init, made, **record)
    finally:
        FC.trun_node = plain
    m.clear, m.ivs, m.key, m.kid, m.protected = clear, used, key, kid, protect
    return m


def simple(counts, *, codec=FLAC, seed=1, sizes=None, iv_size=8, init=None, sinf_options=None, **options):
    """a pattern file: one fragment a count, one run a fragment; sizes: the samples' sizes, in order, or None for the sibling's patterns"""
    fragments, at = [], 0
    for k, n in enumerate(counts):
        samples = FC.pattern_samples(n, seed + k) if sizes is None else [bytes((7 * j + 3 * (at + i) + seed) & 0xff for j in range(sizes[at + i])) for i in range(n)]
        at += n
        fragments.append(FC.fragment([FC.run(samples, [1 + (j * 5 + k) % 7 for j in range(n)])], sequence=k + 1))
    opts = dict(dict(iv_size=iv_size, kid=options.get("kid", KID)), **(sinf_options or {}))
    return mux(protected_init(codec, sinf_options=opts, **(init or {})), fragments, codec=codec, iv_size=iv_size, **options)


def flac_file(name, per_fragment=3, key=KEY, kid=KID, iv_size=8, **options):
    """FC.flac_file, protected"""
    base = FC.flac_file(name, per_fragment)
    fx = base.fixture
    samples, durations = [base.data[o:o + s] for o, s in zip(base.offsets, base.sizes)], base.frames
    fragments = [FC.fragment([FC.run(samples[k:k + per_fragment], durations[k:k + per_fragment])], tfdt=(1, sum(durations[:k])), sequence=k // per_fragment + 1)
                 for k in range(0, len(samples), per_fragment)]
    init = protected_init(FLAC, info=fx.data[8:42], timescale=fx.info["sample_rate"], entry_channels=fx.info["channels"], entry_bits=fx.info["bits"],
                          mehd=(0, fx.info["total_samples"]), sinf_options=dict(kid=kid, iv_size=iv_size))
    m = mux(init, fragments, codec=FLAC, key=key, kid=kid, iv_size=iv_size, **options)
    m.fixture, m.info = fx, fx.info
    return m


def alac_file(name, per_fragment=4, key=KEY, kid=KID, iv_size=16, **options):
    base = FC.alac_file(name, per_fragment)
    fx, cfg = base.fixture, base.cfg
    fragments = [FC.fragment([FC.run(fx["packets"][k:k + per_fragment], base.frames[k:k + per_fragment])], sequence=k // per_fragment + 1)
                 for k in range(0, len(fx["packets"]), per_fragment)]
    init = protected_init(ALAC, cookie=fx["cookie"], timescale=cfg["sample_rate"], entry_channels=cfg["channels"], entry_bits=cfg["bit_depth"],
                          sinf_options=dict(kid=kid, iv_size=iv_size))
    m = mux(init, fragments, codec=ALAC, key=key, kid=kid, iv_size=iv_size, **options)
    m.fixture, m.cfg = fx, cfg
    return m


EDGE_SIZES = [0, 1, 15, 16, 17, 33]
PIECE_SIZES = [63 * 16, 64 * 16, 65 * 16, 128 * 16, 128 * 16 + 1]           # 63, 64, 65, 128 and 129 keystream blocks


def named_good():
    """-> {name: Fragmented}: every way a good protected file is written, and the clear ones the family serves"""
    out = {}
    for codec, name in ((FLAC, "flac"), (ALAC, "alac")):
        for iv_size in (8, 16):
            out[f"{name}_iv{iv_size}"] = simple([5, 6], codec=codec, iv_size=iv_size, seed=iv_size)
    out["senc_in_front_of_the_truns"] = simple([4, 70], senc="front", seed=3)
    out["senc_behind_the_truns"] = simple([4, 70], senc="behind", seed=4)
    two = [FC.run(FC.pattern_samples(5, 5), [100] * 5), FC.run(FC.pattern_samples(66, 6), [200] * 66, gap=7)]
    for where in ("front", "behind"):
        out[f"two_truns_under_one_senc_{where}"] = mux(protected_init(sinf_options=dict(iv_size=16)), [FC.fragment(two), FC.fragment(two, sequence=2)], iv_size=16, senc=where)
    out["sizes_0_1_15_16_17_33"] = simple([len(EDGE_SIZES)], sizes=EDGE_SIZES, iv_size=16)
    out["piece_edges"] = simple([3, 2], sizes=PIECE_SIZES)
    wrap = [bytes(range(40, 88)), bytes(range(7)), bytes(range(100, 133))]
    out["wrap_inside_three_blocks"] = mux(protected_init(sinf_options=dict(iv_size=16)), [FC.fragment([FC.run(wrap, [10] * 3)])], iv_size=16,
                                          ivs=[WRAP_IV, bytes(8) + b"\xff" * 8, b"\x11" * 8 + b"\xff" * 7 + b"\xfe"])
    out["second_senc_skipped"] = simple([6], extra_senc=True, seed=8)
    out["saiz_and_saio_skipped"] = simple([6], aux=True, seed=9)
    out["sinf_behind_the_codec_box"] = simple([6], init=dict(sinf_first=False), seed=10)
    out["unknown_boxes_in_the_entry"] = simple([6], init=dict(entry_extra=[Node(b"btrt", bytes(12)), Node(b"chnl", bytes(5))]), seed=11)
    out["enca_not_protected"] = simple([6, 3], sinf_options=dict(is_protected=0, iv_size=0), protect=False, seed=12)
    out["enca_not_protected_iv_size_ignored"] = simple([6], sinf_options=dict(is_protected=0, iv_size=5), protect=False, senc=None, seed=13)
    out["clear_plain_flac"] = FC.simple([5, 6], seed=14)
    out["clear_plain_alac"] = FC.simple([5, 6], codec=ALAC, seed=15)
    out["clear_with_a_senc_skipped"] = mux(FC.init_segment(), [FC.fragment([FC.run(FC.pattern_samples(6, 16), [10] * 6)])], protect=False)
    out["protected_traf_without_samples"] = mux(protected_init(), [FC.fragment([FC.run(FC.pattern_samples(3, 17), [10] * 3)]), FC.fragment([FC.run([], [])], sequence=2),
                                                                   FC.fragment([FC.run(FC.pattern_samples(2, 18), [10] * 2)], sequence=3)])
    out["init_segment_alone"] = mux(protected_init(), [])
    for m in out.values():
        if not hasattr(m, "clear"):
            m.clear, m.ivs, m.key, m.kid, m.protected = [m.data[o:o + s] for o, s in zip(m.offsets, m.sizes)], [], KEY, KID, False
    return out


def at_of(data, kind, nth=0):
    """where the nth box called `kind` begins (by its fourcc: the sample entry's children are in no marks)"""
    at = -1
    for _ in range(nth + 1):
        at = bytes(data).index(kind, at + 1)
    return at - 4


def entry_at(m):
    return m.find("stsd")[1] + 8


def named_malformed():
    """-> {name: (bytes, status, error_offset, codecs, have key, kid)}: one thing wrong each, for every rule of the section"""
    X = CX
    out = {}

    def add(name, data, status, at, codecs=3, have_key=True, kid=KID):
        out[name] = (bytes(data), status, at, codecs, have_key, kid)

    def entry(name, status, where, **kw):
        m = simple([4], **kw)
        add(name, m.data, status, entry_at(m) if where == "entry" else at_of(m.data, where))

    for what in ("frma", "schm", "schi", "tenc"):
        entry(f"sinf_without_{what}", X.INVALID, "entry", sinf_options=dict(drop=(what,)))
    entry("enca_without_sinf", X.INVALID, "entry", init=dict(protection=False))
    entry("frma_of_3_bytes", X.INVALID, b"frma", sinf_options=dict(frma_bytes=3))
    entry("schm_of_11_bytes", X.INVALID, b"schm", sinf_options=dict(schm_bytes=11))
    for scheme in (b"cbcs", b"cbc1", b"cens", b"piff"):
        entry(f"scheme_{scheme.decode()}", X.UNSUPPORTED, b"schm", sinf_options=dict(scheme=scheme))
    entry("tenc_of_23_bytes", X.INVALID, b"tenc", sinf_options=dict(short=1))
    entry("tenc_version_1", X.UNSUPPORTED, b"tenc", sinf_options=dict(version=1))
    entry("is_protected_2", X.INVALID, b"tenc", sinf_options=dict(is_protected=2))
    for size in (0, 4, 12, 32):
        m = mux(protected_init(sinf_options=dict(iv_size=size)), [])
        add(f"iv_size_{size}", m.data, X.UNSUPPORTED, at_of(m.data, b"tenc"))
    short = Node(b"enca", bytes(27))
    m = mux(FC.init_segment(entry=short), [])
    add("enca_entry_of_27_bytes", m.data, X.INVALID, entry_at(m))
    entry("enca_flac_without_dfla", X.UNSUPPORTED, "entry", init=dict(inner=False))
    entry("enca_alac_without_the_inner_box", X.UNSUPPORTED, "entry", codec=ALAC, init=dict(inner=False))
    m = simple([4], codec=b"mp4a", init=dict(inner=False))
    add("enca_mp4a", m.data, X.NOT_CODEC, m.find("moov")[0])
    m = simple([4], codec=ALAC)
    add("enca_alac_asked_flac", m.data, X.NOT_CODEC, m.find("moov")[0], codecs=2)
    # the entry and its children are 4096 boxes: the 4097th is one too many (the entry, `free`, 4093 more, sinf; then sinf's first child)
    m = simple([4], init=dict(entry_extra=[Node(b"free", b"")] * 4093))
    add("entry_of_too_many_boxes", m.data, X.INVALID, at_of(m.data, b"sinf") + 8)
    m = simple([4], init=dict(entry_extra=[Node(b"free", b"")] * 4080))
    add("entry_of_many_boxes", m.data, X.OK, 0)
    m = simple([4])
    add("child_of_sinf_past_its_parent", FC.patched(m, at_of(m.data, b"schm"), 200), X.INVALID, at_of(m.data, b"schm"))
    add("no_key", m.data, X.NO_KEY, at_of(m.data, b"tenc"), have_key=False)
    add("key_of_another_kid", m.data, X.NO_KEY, at_of(m.data, b"tenc"), kid=kid_of(3))
    # the traf
    good = simple([5, 6], iv_size=16)
    senc, senc2, traf2 = good.find("senc"), good.find("senc", 1), good.find("traf", 1)
    add("senc_version_1", FC.patched(good, senc[1], 1, 1), X.UNSUPPORTED, senc[0])
    add("senc_overridden_parameters", FC.patched(good, senc2[1], 1, 4), X.UNSUPPORTED, senc2[0])
    add("senc_subsamples", FC.patched(good, senc[1], 2, 4), X.UNSUPPORTED, senc[0])
    add("senc_count_leaves_the_box", FC.patched(good, senc[1] + 4, 6), X.INVALID, senc[0])
    add("senc_count_below_the_truns", FC.patched(good, senc2[1] + 4, 5), X.INVALID, senc2[0])
    cut = bytearray(good.data)
    cut[senc2[0] + 4:senc2[0] + 8] = b"free"
    add("protected_traf_without_senc", cut, X.UNSUPPORTED, traf2[0])
    m = mux(protected_init(), [FC.fragment([FC.run(FC.pattern_samples(3, 1), [10] * 3)])], ivs=[bytes(8)] * 3)
    s = m.find("senc")
    short = bytearray(m.data)          # the senc becomes a senc of 4 payload bytes and a `free` box of the rest
    short[s[0]:s[0] + 12] = struct.pack(">I4sI", 12, b"senc", 0)
    short[s[0] + 12:s[0] + 20] = struct.pack(">I4s", s[2] - s[0] - 12, b"free")
    add("senc_of_4_bytes", short, X.INVALID, s[0])
    big = bytearray(m.data)            # sample_count is right and the entries leave the box: the last IV becomes a `free` box
    big[s[0]:s[0] + 4] = struct.pack(">I", s[2] - s[0] - 8)
    big[s[2] - 8:s[2]] = struct.pack(">I4s", 8, b"free")
    add("senc_entries_leave_the_box", big, X.INVALID, s[0])
    for kind in (b"sbgp", b"sgpd"):
        m = mux(protected_init(), [FC.fragment([FC.run(FC.pattern_samples(3, 1), [10] * 3)])], aux=True)
        grouped = bytearray(m.data)
        z = m.find("saiz")
        grouped[z[0] + 4:z[0] + 8] = kind
        grouped[z[1] + 4:z[1] + 8] = b"seig"
        add(f"{kind.decode()}_seig", grouped, X.UNSUPPORTED, z[0])
    return out


def damaged(count, seed=20263):
    """-> [(bytes, Fragmented)]: fixed-seed damage to good protected files.  k % 3 == 0: a bit of the protection boxes (sinf and its children,
    senc) is flipped; 1: a bit anywhere in moov or a moof; 2: a bit of a sample (such a file stays OK and decrypts to other bytes)."""
    goods = [m for name, m in named_good().items() if m.protected and m.n]
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


def protection_cuts(m):
    """a cut at every byte of the protection boxes: the sinf of the entry and every senc"""
    sinf_at = at_of(m.data, b"sinf")
    spans = [(sinf_at, sinf_at + int.from_bytes(m.data[sinf_at:sinf_at + 4], "big"))] + [(x[1], x[3]) for x in m.marks if x[0].endswith("/senc")]
    return [m.data[:e] for a, b in spans for e in range(a, b + 1)]


# ---- batches
def stream(data, capacity=None, run_capacity=None, codecs=3, gather_first_row=0, dst_capacity=None, key=None, kid=None, have_key=True):
    if isinstance(data, FC.Fragmented):
        m = data
        return dict(data=m.data, capacity=m.n if capacity is None else capacity, run_capacity=len(m.runs) if run_capacity is None else run_capacity, codecs=codecs,
                    gather_first_row=gather_first_row, dst_capacity=len(m.data) if dst_capacity is None else dst_capacity, key=m.key if key is None else key,
                    kid=m.kid if kid is None else kid, have_key=have_key)
    return dict(data=bytes(data), capacity=8 if capacity is None else capacity, run_capacity=4 if run_capacity is None else run_capacity, codecs=codecs,
                gather_first_row=gather_first_row, dst_capacity=len(data) if dst_capacity is None else dst_capacity, key=KEY if key is None else key,
                kid=KID if kid is None else kid, have_key=have_key)


class Job:
    """FC.Job for the protected family: the same arenas and guards; the descriptors carry the keys; `want_packets` are places in the
    destination arena and `want_dst` holds the clear bytes."""

    def __init__(self, streams, align=lambda i: (5 * i + 1) % 16, dst_align=lambda i: (7 * i + 3) % 16, models=None):
        from ohpipeline_amd import capi
        self.streams = streams
        src = bytearray()
        self.descs = np.zeros(len(streams), dtype=capi.CENC_STREAM_DESC)
        row = run_row = GUARD_ROWS
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
            d["key_flags"] = 1 if s["have_key"] else 0
            d["kid"] = np.frombuffer(s["kid"], dtype=np.uint8)
            if s["have_key"]:
                d["key"] = np.frombuffer(s["key"], dtype=np.uint8)
            src += s["data"]
            row += s["capacity"] + GUARD_ROWS
            run_row += s["run_capacity"] + GUARD_ROWS
            dst += s["dst_capacity"] + GUARD_BYTES
        while len(src) % 4:
            src.append(0xee)
        self.n_packets, self.n_runs, self.dst_bytes = (row, run_row, dst) if streams else (0, 0, 0)
        self.src = np.frombuffer(bytes(src), dtype=np.uint8).copy()
        self.models = models or [CX.demux(s["data"], s["codecs"], s["capacity"], s["run_capacity"], s["gather_first_row"], s["dst_capacity"],
                                          kid=s["kid"], key=s["key"] if s["have_key"] else None) for s in streams]
        self.want_results = np.zeros(len(streams), dtype=capi.CENC_STREAM_RESULT)
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
        """the job file of tests/cpp/cenc_core_driver.cpp"""
        return struct.pack("<QQQQQ", len(self.streams), self.n_packets, self.n_runs, self.src.size, self.dst_bytes) + self.descs.tobytes() + self.src.tobytes()


def fill_result(r, m):
    """a CENC_STREAM_RESULT record from the model's dict"""
    for k in CX.RESULT_FIELDS:
        r["mp4f"][k] = m[k]
    for k in CX.CONFIG_FIELDS:
        r["mp4f"]["config"][k] = m["config"][k]
    for k in CX.FLAC_FIELDS:
        r["mp4f"]["flac"][k] = np.frombuffer(m["flac"][k], dtype=np.uint8) if k == "md5" else m["flac"][k]
    for k in CX.EXTRA_FIELDS:
        r[k] = np.frombuffer(m[k], dtype=np.uint8) if k == "kid" else m[k]


assert_same = FC.assert_same


@functools.lru_cache(maxsize=None)
def damage_job():
    """-> Job, made once: a cut at every byte of the protection boxes of the small 16-byte-IV file (308 streams) and 300 files of
    fixed-seed damage, a stream each.  tests/test_cenc_core_cpu.py takes it through the sanitised driver in both builds before
    tests/test_gpu_cenc_textbook.py takes it to the device."""
    m = named_good()["two_truns_under_one_senc_front"]
    small = named_good()["flac_iv16"]
    streams = [stream(data, capacity=m.n, run_capacity=len(m.runs), dst_capacity=len(m.data), key=m.key, kid=m.kid) for data in protection_cuts(small)]
    streams += [stream(data, capacity=150, run_capacity=4, dst_capacity=len(data), key=f.key, kid=f.kid) for data, f in damaged(300)]
    return Job(streams)


# ---- streams of more than one tile (cenc_rows_kernel's wave prefix, cenc_tiles_kernel's loop, cenc_crypt_kernel's two searches)
TILE = 1024                 # mp4box::kTile: the samples a workgroup of cenc_rows_kernel takes, four a thread, 256 a wave
WAVE_ROWS = 256
RARE_SIZES = (63 * 16, 65 * 16)
TILE_COUNTS = (255, 256, 257, 1023, 1024, 1025, 2049, 3 * TILE + 5)


def tile_sizes(n, seed, hollow=False):
    """the sizes of n samples: by a fixed-seed generator from EDGE_SIZES; a few of 63 and 65 keystream blocks, of which one each
    lies behind row 1024 where there is one; nothing at rows 1023 and 1024; hollow: nothing in the whole of tile 1"""
    rng = Lcg(4100 + seed)
    sizes = [EDGE_SIZES[rng.next() % len(EDGE_SIZES)] for _ in range(n)]
    for _ in range(2 + n // 600):
        sizes[rng.next() % n] = RARE_SIZES[rng.next() % 2]
    if n > TILE + 2:
        a, b = (TILE + 1 + rng.next() % (n - TILE - 1) for _ in range(2))
        sizes[a], sizes[b if b != a else TILE + 1 + (a - TILE) % (n - TILE - 1)] = RARE_SIZES
    for row in (TILE - 1, TILE):
        if row < n:
            sizes[row] = 0
    if hollow:
        sizes[TILE:2 * TILE] = [0] * len(sizes[TILE:2 * TILE])
    return sizes


def tiled(n, *, seed, fragments=None, iv_size=8, k=0, codec=FLAC, hollow=False, protection="cenc", senc="behind"):
    """a file of n samples of tile_sizes(); fragments: [[samples of a run, ...] a fragment], one senc a fragment; protection: "cenc"
    under key k, "enca_clear" (an enca entry whose tenc says isProtected 0) or "plain" (the sibling's own fLaC / alac entry)"""
    sizes = tile_sizes(n, seed, hollow)
    fragments = fragments or [[n]]
    assert sum(sum(f) for f in fragments) == n
    made, at = [], 0
    for q, counts in enumerate(fragments):
        runs = []
        for j, count in enumerate(counts):
            samples = [bytes((7 * b + 3 * i + seed) & 0xff for b in range(sizes[i])) for i in range(at, at + count)]
            runs.append(FC.run(samples, [1 + (5 * i + q) % 7 for i in range(at, at + count)], gap=5 if j else 0))
            at += count
        made.append(FC.fragment(runs, sequence=q + 1))
    if protection == "plain":
        m = FC.mux(FC.init_segment(codec), made, codec=codec)
        m.clear, m.ivs, m.key, m.kid, m.protected = [m.data[o:o + s] for o, s in zip(m.offsets, m.sizes)], [], KEY, KID, False
    elif protection == "enca_clear":
        m = mux(protected_init(codec, sinf_options=dict(is_protected=0, iv_size=0, kid=kid_of(k))), made, codec=codec, protect=False, key=key_of(k), kid=kid_of(k), senc=senc)
    else:
        m = mux(protected_init(codec, sinf_options=dict(iv_size=iv_size, kid=kid_of(k))), made, codec=codec, iv_size=iv_size, key=key_of(k), kid=kid_of(k), senc=senc)
    assert m.sizes == sizes
    return m


@functools.lru_cache(maxsize=None)
def multi_tile_files():
    """-> {name: Fragmented}, made once: a file a count of TILE_COUNTS (255 to 257 cross a wave's edge inside a tile, the larger ones
    a tile's), under three keys and both IV sizes; 2049 samples in two truns under one senc, the second from row 1019 on, so that the
    senc's IVs and the second run cross row 1024; 3077 samples in fragments of about 700, so that tiles 1 and 2 hold the end of one
    run and the start of the next; 3077 samples of which tile 1 holds no byte; and two clear files of 2049 samples."""
    out = {}
    for q, n in enumerate(TILE_COUNTS[:6]):
        out[f"samples_{n}"] = tiled(n, seed=n, iv_size=(8, 16)[q % 2], k=1 + q % 3, codec=(FLAC, ALAC)[q // 2 % 2])
    out["samples_2049_two_truns_under_one_senc"] = tiled(2049, seed=31, fragments=[[1019, 1030]], iv_size=16, k=1, senc="front")
    out["samples_3077_fragments_of_700"] = tiled(3077, seed=32, fragments=[[703], [689], [711], [697], [277]], iv_size=8, k=2)
    out["samples_3077_tile_1_empty"] = tiled(3077, seed=33, fragments=[[1500], [1577]], iv_size=16, k=3, hollow=True)
    out["samples_2049_plain_flac"] = tiled(2049, seed=34, fragments=[[700], [700, 649]], protection="plain")
    out["samples_2049_enca_not_protected"] = tiled(2049, seed=35, fragments=[[1030], [1019]], k=2, protection="enca_clear")
    return out


def tile_blocks_of(model):
    """the keystream blocks (for a clear stream: the 16-byte pieces) of every tile of the stream's rows, from the model's clear_rows"""
    rows = model["clear_rows"]
    return [sum((size + 15) // 16 for _, size in rows[t:t + TILE]) for t in range(0, len(rows), TILE)]


def tile_claims(models):
    """what a multi-tile job is for, counted from the models: the streams in which
      waves      a tile with s0 >= 1024 has rows with blocks in each of waves 1, 2 and 3 of cenc_rows_kernel (256 rows a wave);
      three      three or more tiles hold blocks;
      hole       a tile without blocks lies between two that hold some;
      late_run   a gathered row of some bytes lies in a run behind the first and in a tile behind the first."""
    out = dict(waves=0, three=0, hole=0, late_run=0)
    for m in models:
        rows, per_tile = m["clear_rows"], tile_blocks_of(m)
        out["waves"] += any(all(any(size for _, size in rows[t + w * WAVE_ROWS:t + (w + 1) * WAVE_ROWS]) for w in (1, 2, 3)) for t in range(TILE, len(rows), TILE))
        out["three"] += sum(1 for b in per_tile if b) >= 3
        filled = [t for t, b in enumerate(per_tile) if b]
        out["hole"] += bool(filled) and any(not per_tile[t] for t in range(filled[0], filled[-1]))
        out["late_run"] += any(size and m["samples_rows"][row][2] > 0 for row, (_, size) in enumerate(rows) if row >= TILE)
    return out


def _between_short(big, align=(0, 1, 7, 14), dst_align=(0, 3, 8, 15)):
    """a job of the big streams with a short named stream in front of, between and behind them; big stream j lies at source
    alignment align[j % 4] and destination alignment dst_align[(j + j // 4) % 4]"""
    good = named_good()
    short = [good[name] for name in ("flac_iv8", "sizes_0_1_15_16_17_33", "clear_plain_alac", "alac_iv16", "enca_not_protected")]
    rng = Lcg(4200 + len(big))
    streams = [stream(short[rng.next() % len(short)])]
    for s in big:
        streams += [s, stream(short[rng.next() % len(short)])]
    job = Job(streams, align=lambda i: align[i // 2 % 4] if i % 2 else (5 * i + 1) % 16, dst_align=lambda i: dst_align[(i // 2 + i // 8) % 4] if i % 2 else (7 * i + 3) % 16)
    job.big = list(range(1, len(streams), 2))
    return job


@functools.lru_cache(maxsize=None)
def multi_tile_jobs():
    """-> {name: Job}, made once.  "every_count": every file of multi_tile_files(), whole.  "descriptors": the 2049- and 3077-sample
    files under gather_first_row 0, 255, 256, 1023, 1024, 1025 and 2048 (from 1024 on tile 0 has rows and no blocks); packet_capacity
    TILE + 1 with room for exactly those rows' bytes; the same capacity over a prefix of the file that ends inside row 1000, whose
    later rows are refused; dst_capacity ending in the middle of tile 1 and exactly where tile 1's first byte would go (the gather is
    all or nothing: such a stream gathers nothing and has no blocks); and dst_capacity 0."""
    files = multi_tile_files()
    jobs = {"every_count": _between_short([stream(m) for m in files.values()])}
    big = []
    for name in ("samples_2049_two_truns_under_one_senc", "samples_3077_fragments_of_700", "samples_3077_tile_1_empty", "samples_2049_plain_flac"):
        m = files[name]
        rows = (0, 255, 256, 1023, 1024, 1025, 2048) if "plain" not in name and "empty" not in name else (1024, 2048)
        big += [stream(m, gather_first_row=row) for row in rows if row]
        if "plain" in name or "empty" in name:
            continue
        upto = [sum(m.sizes[:row]) for row in range(m.n + 1)]
        big += [stream(m, capacity=TILE + 1, dst_capacity=upto[TILE + 1]), stream(m, dst_capacity=(upto[TILE] + upto[2 * TILE]) // 2), stream(m, dst_capacity=upto[TILE]),
                stream(m, dst_capacity=0)]
        cut = next(row for row in range(1000, m.n) if m.sizes[row])
        big.append(stream(m.data[:m.offsets[cut] + 1], capacity=TILE + 1, run_capacity=len(m.runs), dst_capacity=upto[TILE], key=m.key, kid=m.kid))
    jobs["descriptors"] = _between_short(big)
    return jobs


def assert_reaches(name, job):
    """a job of multi_tile_jobs() reaches what it is for, by its models -- asserted before the job goes anywhere, so that a fixture
    that shrinks fails here and does not quietly stop testing the paths"""
    models = [job.models[i] for i in job.big]
    claims = tile_claims(models)
    assert all(m["status"] == CX.OK for m in job.models)
    assert len({int(job.descs[i]["src_offset"]) % 16 for i in job.big}) == 4 == len({int(job.descs[i]["dst_offset"]) % 16 for i in job.big})
    assert claims["waves"] >= 1 and claims["three"] >= 1 and claims["late_run"] >= 1, claims
    assert {m["iv_size"] for m in models} == {0, 8, 16} and len({m["kid"] for m in models if m["is_protected"]}) >= 2
    per_tile = [tile_blocks_of(m) for m in models]
    if name == "every_count":
        assert claims["hole"] >= 1 and [m["samples"] for m in models[:len(TILE_COUNTS)]] == list(TILE_COUNTS)
        assert all(m["samples_available"] == m["samples"] == len(m["clear_rows"]) and m["bytes_gathered"] for m in models)
        assert sum(1 for m in models if not m["is_protected"] and len(tile_blocks_of(m)) >= 3) >= 2            # the clear streams of several tiles
        assert all(m["clear_rows"][row][1] == 0 for m in models for row in (TILE - 1, TILE) if row < m["samples"])
        # a sample of 63 or 65 blocks behind row 1024 in front of further rows of the tile: a prefix that crosses a slot's edge there
        assert sum(1 for m in models if any(size in RARE_SIZES for _, size in m["clear_rows"][TILE:])) >= 4
    else:
        firsts = {int(job.descs[i]["gather_first_row"]) for i in job.big}
        assert firsts == {0, 255, 256, 1023, 1024, 1025, 2048}
        assert sum(1 for t in per_tile if len(t) >= 2 and t[0] == 0 and any(t[1:])) >= 6                       # tile 0: rows and no blocks
        assert sum(1 for t in per_tile if len(t) >= 3 and t[0] == t[1] == 0 and t[2]) >= 2                     # ... and tile 1 as well
        cut = [m for m in models if len(m["clear_rows"]) == TILE + 1]
        assert len(cut) == 4 and sum(1 for m in cut if m["samples_refused"] and m["samples_available"] < TILE and m["bytes_gathered"]) == 2
        assert sum(1 for m in cut if m["samples"] > TILE + 1 and m["samples_available"] == TILE + 1 and m["bytes_gathered"]) == 2
        nothing = [i for i in job.big if not job.models[i]["bytes_gathered"]]
        assert len(nothing) == 6 and sorted(int(job.descs[i]["dst_capacity"]) > 0 for i in nothing) == [False] * 2 + [True] * 4
    return claims


# ---- more chunk slots than the persistent decrypt-gather launch has waves (cenc_crypt_kernel's loop over `g`)
SLOT_BLOCKS = 64            # cenc::kLaneBlocks: the keystream blocks of a chunk slot, a lane each
CRYPT_WAVES, CRYPT_GROUPS_PER_CU = 4, 8          # kProtWaves, kProtGroupsPerCu (csrc/protected_shell.h): the launch's cap today
TRIP_SEED = 20264
TRIPS = 5                   # the builder's target: 5 W + 67 slots (the condition is 3 W + 67; see trip_claims on why more)


def trip_waves(cus):
    """W: the waves a launch holds -- the larger of today's cap (8 workgroups of 4 waves a CU) and what the CUs keep resident"""
    from device_shape import MAX_WAVES_PER_CU
    return max(CRYPT_GROUPS_PER_CU * CRYPT_WAVES, MAX_WAVES_PER_CU) * cus


def slots_of(dst_capacity, packet_capacity):
    """the documented rule: a stream has room for dst_capacity / 16 + packet_capacity blocks, and none if either is 0"""
    return (dst_capacity // 16 + packet_capacity + SLOT_BLOCKS - 1) // SLOT_BLOCKS if dst_capacity and packet_capacity else 0


@functools.lru_cache(maxsize=None)
def trip_pool():
    """-> (small, medium, big): sixteen files of one to four short samples -- twelve protected, each under a key and kid of its own,
    both IV sizes and both codecs, and four clear ones --; two of 70 to 100 blocks (two working slots); three of 130 to 200 blocks, of
    which the last fills four slots; a clear one in each of the two"""
    rng = Lcg(4300)
    small = []
    for k in range(16):
        n = 1 + rng.next() % 4
        sizes = [(1, 15, 16, 17, 33, 48, 100)[rng.next() % 7] for _ in range(n)]
        codec = (FLAC, ALAC)[rng.next() % 2]
        if k % 4 != 3:
            small.append(simple([n], sizes=sizes, codec=codec, seed=40 + k, iv_size=(8, 16)[k % 2], key=key_of(20 + k), kid=kid_of(20 + k)))
        elif k % 8 == 3:
            small.append(simple([n], sizes=sizes, codec=codec, seed=40 + k, sinf_options=dict(is_protected=0, iv_size=0), protect=False))
        else:
            m = FC.simple([n], codec=codec, seed=40 + k)
            m.clear, m.ivs, m.key, m.kid, m.protected = [m.data[o:o + s] for o, s in zip(m.offsets, m.sizes)], [], KEY, KID, False
            small.append(m)

    def filled(k, blocks, n, protect=True):
        sizes = [16 * (blocks // n) - rng.next() % 16 for _ in range(n - 1)]
        sizes.append(16 * (blocks - sum((s + 15) // 16 for s in sizes)) - 3)
        m = simple([n], sizes=sizes, seed=60 + k, iv_size=(8, 16)[k % 2], key=key_of(40 + k), kid=kid_of(40 + k),
                   **({} if protect else dict(sinf_options=dict(is_protected=0, iv_size=0), protect=False)))
        assert sum((s + 15) // 16 for s in m.sizes) == blocks
        return m

    return small, [filled(0, 71, 5), filled(1, 97, 4, protect=False)], [filled(2, 131, 6), filled(3, 170, 5, protect=False), filled(4, 199, 7)]


@functools.lru_cache(maxsize=None)
def many_trip_job(cus, seed=TRIP_SEED):
    """-> (Job, slots, [(stream, working, key) a slot]): a work list of TRIPS x W + 67 chunk slots and more for a device of `cus`
    CUs, W = trip_waves(cus).  key: the index of the stream's file in the pool's files, which all have keys of their own, or -1 for
    a clear stream.  Slot k of a stream is working when 64 k < B, B the stream's blocks by the model's clear_rows.  By one seeded
    generator: mostly one-slot streams over the sixteen small files, under one of three pairs of capacities; one stream in thirty has
    capacities for 3 to 39 slots (never a count that divides W or that W divides) of which one works, or two with a medium file: the
    waves that come to its other slots jump; one in sixty is a big file that fills three or four slots in a row.  (One-slot streams
    are the list's stuff, and 1 divides everything: what keeps the list from lining up with the grid is that the others fall among
    them at seeded places.)  One rule binds the generator: a wave -- a residue of the slot index mod W -- that has not yet had
    working slots of protected streams under two keys, and has only as many slots to come as it lacks, gets a one-slot protected
    stream under a key it has not had.  Chance alone would leave some of W waves short after any affordable number of trips.
    The model runs once per distinct (file, capacities)."""
    small, medium, big = trip_pool()
    files = small + medium + big
    W = trip_waves(cus)
    need = TRIPS * W + 67
    counts = [c for c in range(3, 40) if W % c and c % W]
    few = len([c for c in counts if c < 10])
    protected_small = [f for f, m in enumerate(small) if m.protected]
    rng = np.random.default_rng(seed)
    streams, models, per_slot, cache, slots = [], [], [], {}, 0
    had = [set() for _ in range(W)]                                # the keys of the protected working slots a residue has had

    def short(g):
        """residue g % W lacks as many keys as it has slots to come, slot g included"""
        return g < need and 0 < 2 - len(had[g % W]) >= (need - g + W - 1) // W

    def one_slot(f):
        extra_rows, extra_bytes = ((0, 0), (1, 5), (0, 48))[int(rng.integers(3))]
        return f, files[f].n + extra_rows, max(sum(files[f].sizes), 1) + extra_bytes, 1

    while slots < need:
        u = rng.random()
        if short(slots):
            f, capacity, dst_capacity, want = one_slot([f for f in protected_small if f not in had[slots % W]][int(rng.integers(len(protected_small) - 1))])
        elif u < 1 / 30:
            f = len(small) + int(rng.integers(len(medium))) if rng.random() < 0.3 else int(rng.integers(len(small)))
            want = counts[int(rng.integers(few))] if rng.random() < 0.85 else counts[int(rng.integers(len(counts)))]
            capacity = files[f].n
            dst_capacity = 16 * (SLOT_BLOCKS * (want - 1) + 1 - capacity) + 7
        elif u < 1 / 30 + 1 / 60:
            f = len(small) + len(medium) + int(rng.integers(len(big)))
            capacity, dst_capacity = files[f].n, sum(files[f].sizes)
            want = slots_of(dst_capacity, capacity)
            if W % want == 0:                                      # (four slots: room for a fifth, which does not work)
                dst_capacity, want = 16 * (SLOT_BLOCKS * want + 1 - capacity), want + 1
        else:
            f, capacity, dst_capacity, want = one_slot(int(rng.integers(len(small))))
        if any(short(slots + k) for k in range(1, want)):          # (a stream of several slots does not lie over a residue that is short)
            f, capacity, dst_capacity, want = one_slot(int(rng.integers(len(small))))
        assert slots_of(dst_capacity, capacity) == want, (f, capacity, dst_capacity, want)
        m = files[f]
        if (f, capacity, dst_capacity) not in cache:
            cache[(f, capacity, dst_capacity)] = CX.demux(m.data, 3, capacity, len(m.runs), 0, dst_capacity, kid=m.kid, key=m.key)
        model = cache[(f, capacity, dst_capacity)]
        blocks = sum((size + 15) // 16 for _, size in model["clear_rows"])
        for k in range(want):
            per_slot.append((len(streams), SLOT_BLOCKS * k < blocks, f if m.protected else -1))
            if m.protected and SLOT_BLOCKS * k < blocks:
                had[(slots + k) % W].add(f)
        streams.append(stream(m, capacity=capacity, dst_capacity=dst_capacity))
        models.append(model)
        slots += want
    return Job(streams, models=models), slots, per_slot


def trip_claims(cus, job, slots, per_slot):
    """What the work list of many_trip_job holds, for the tests to assert.  A wave of residue r takes slots r, r + W, r + 2 W, ...
    (W is a whole number of workgroups, so slots 4 m .. 4 m + 3 are one workgroup's four waves in one trip).
      slots_by_rule     the slot count by the documented rule over the job's descriptors
      launch_groups     min(ceil(slots / 4), 8 cus): the launch's workgroups by the cap as csrc/cenc_kernel.hip states it
      chunk_first       the running sums
      two_working       the residues with two working slots or more
      two_keys          ... of which two belong to protected streams under different keys
      clear_between     the residues where a clear working slot lies between two protected working ones.  Three trips cannot give a
                        quarter of the residues that: with p protected and c clear the best of p p c is 4 / 27, which is why the
                        list is TRIPS = 5 trips long
      jumps             the residues that meet a slot that does not work and a working one later on
      mixed_groups      the workgroup trips (four consecutive slots from a multiple of 4) whose working slots lie in two streams or
                        more under different keys, and those of them where a clear stream is among them"""
    W = trip_waves(cus)
    d = job.descs
    by_rule = [slots_of(int(x["dst_capacity"]), int(x["packet_capacity"])) for x in d]
    out = dict(W=W, slots_by_rule=sum(by_rule), launch_groups=min((slots + CRYPT_WAVES - 1) // CRYPT_WAVES, CRYPT_GROUPS_PER_CU * cus),
               chunk_first=np.concatenate([[0], np.cumsum(by_rule)]), two_working=0, two_keys=0, clear_between=0, jumps=0, mixed_groups=0, mixed_with_clear=0)
    for r in range(W):
        mine = per_slot[r::W]
        working = [key for _, works, key in mine if works]
        protected = [n for n, key in enumerate(working) if key >= 0]
        out["two_working"] += len(working) >= 2
        out["two_keys"] += len({working[n] for n in protected}) >= 2
        out["clear_between"] += len(protected) >= 2 and any(key < 0 for key in working[protected[0]:protected[-1]])
        idle = [n for n, (_, works, _) in enumerate(mine) if not works]
        out["jumps"] += bool(idle) and any(works for _, works, _ in mine[idle[0]:])
    for g in range(0, len(per_slot), CRYPT_WAVES):
        working = {(i, key) for i, works, key in per_slot[g:g + CRYPT_WAVES] if works}
        if len({key for _, key in working}) >= 2:
            out["mixed_groups"] += 1
            out["mixed_with_clear"] += any(key < 0 for _, key in working)
    return out


def assert_trips(cus, job, slots, per_slot):
    """items 1 and 2 of the conditions (tests/test_cenc_cases.py holds all of them at four CU counts) -> trip_claims()"""
    c = trip_claims(cus, job, slots, per_slot)
    W = c["W"]
    assert c["slots_by_rule"] == slots == len(per_slot) >= 3 * W + 67 and 4 * c["launch_groups"] < slots and c["launch_groups"] == CRYPT_GROUPS_PER_CU * cus, c
    assert c["two_working"] == W and c["two_keys"] == W and 4 * c["clear_between"] >= W, c
    return c
