"""What the protected MPEG-4 tests share: the muxer pieces of their own (sinf, senc, the encryption of a fragment's samples) on top of
tests/mp4f_cases.py's builders, which are imported and not edited; the muxer's OWN RECORD of every clear sample, IV and key -- the truth
the model (tests/cenc_textbook.py) and the product are held to --; the named good and malformed files; the fixed-seed damage; and the
batches: the arenas, the descriptors, and what the model says every output must be."""
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
