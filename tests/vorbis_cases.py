"""The Vorbis streams the CPU and the GPU tests share (tests/vorbis_frames.py writes them, tests/vorbis_textbook.py decodes them), each
made once a session: the shapes at which the decoder can go wrong -- the smallest blocks and the largest, both sizes in one stream with
all four neighbour pairs, 1 / 2 / 6 / 8 channels, coupling and submaps, 70 and more packets so that a wave of packets is crossed, and one
stream whose PCM clips."""
import collections
import functools
import random
import time

import numpy as np

import vorbis_frames as VF
import vorbis_textbook as TB

#        name            seed channels e0 e1 packets coupling submaps peak
SHAPES = {
    "mono_64_128":      (11, 1, 6, 7, 72, 0, 1, 0.45),
    "stereo_256_2048":  (12, 2, 8, 11, 70, 1, 1, 0.45),
    "mono_8192":        (13, 1, 11, 13, 6, 0, 1, 0.45),
    "six_128_512":      (14, 6, 7, 9, 16, 2, 2, 0.45),
    "eight_64_256":     (15, 8, 6, 8, 12, 3, 3, 0.45),
    "stereo_clips":     (16, 2, 6, 7, 20, 1, 1, 3.0),
    "encoder_256":      None,          # (not random: see ENCODER)
}
# The streams held against Tremor (tests/test_vorbis_tremor.py).  They keep to what an encoder writes where Tremor and the specification
# part: (1) the floors' end amplitudes are drawn from the lower 45 % of their range, so that the floor carries the
# level and the residue's value vectors are of the size of whole numbers -- Tremor keeps the residue in fixed point, eight bits behind the
# point; (2) a residue has as many classes as its class book's entries decompose into -- Tremor ends the residue at a class word out of
# range, the specification takes it modulo; (3) the long block is twice the short one, so that every floor's last post stands at or
# beyond the block's half -- behind the last post Tremor multiplies by the curve's level itself, not by the table's value of it; (4) a
# type 2 residue's partition size is a multiple of its submap's channel count -- Tremor begins the round of the channels anew at every
# partition, the specification deinterleaves the vector as a whole (the six-channel stream's seed is chosen for bundles of 2 and 4).
TREMOR_SHAPES = {
    "tremor_mono_64_128":      (21, 1, 6, 7, 40, 0, 1, 0.45),
    "tremor_stereo_1024_2048": (22, 2, 10, 11, 12, 1, 1, 0.45),
    "tremor_six_128_256":      (24, 6, 7, 8, 16, 2, 2, 0.45),
}


ENCODER = "encoder_256"            # the minimal encoder's stream (tests/vorbis_frames.encode of a sine sweep), a shape like the others


def sweep():
    t = np.arange(256 * 24)
    return 0.5 * np.sin(2 * np.pi * (0.01 + 0.00002 * t) * t)


@functools.lru_cache(maxsize=None)
def stream(name):
    if name == ENCODER:
        return VF.encode(sweep())
    if name in TREMOR_SHAPES:
        seed, ch, e0, e1, n, coupling, submaps, peak = TREMOR_SHAPES[name]
        return VF.random_stream(seed, ch, e0, e1, n, coupling, submaps, peak, floor_cap=0.45, one_entry=1, strict=True)
    seed, ch, e0, e1, n, coupling, submaps, peak = SHAPES[name]
    return VF.random_stream(seed, ch, e0, e1, n, coupling, submaps, peak)


@functools.lru_cache(maxsize=None)
def expected(name, max_samples=None):
    """(records, spectra, pcm) of the whole stream by the model; the arrays are shared: do not write to them."""
    st = stream(name)
    return TB.decode_stream(st.model, st.packets, max_samples)


def pcm_s16be(pcm):
    """int32 [channels][samples] -> the interleaved big-endian bytes"""
    return pcm.T.astype(">i2").tobytes()


BAD_MODE = bytes([0b110])          # an audio packet whose mode number is 3 where the streams have three modes


def damaged(name):
    """The stream's packets with every fifth cut short (at a third of its bytes) and two replaced by a bad mode and an empty packet."""
    st = stream(name)
    packets = list(st.packets)
    for k in range(2, len(packets), 5):
        packets[k] = packets[k][:max(1, len(packets[k]) // 3)]
    packets[4] = BAD_MODE
    packets[7] = b""
    packets[9] = b"\x05vorbis"
    return packets


# ---------------------------------------------------------------- the fixed-seed damage set
# A case is a stream of four packets, [p[k-1], mutated p[k], p[k+1], p[k+2]] of a shape (indices modulo the stream's length): the
# packet in front primes the overlap, the two behind show what the damage does to its neighbours.  Nothing is random at run time.
Case = collections.namedtuple("Case", "label shape k kind packets")
# (shape, k): a short and a long block of each shape; a short block follows the mutated packet in mono_64_128 (k = 1, 4) and
# eight_64_256 (k = 1), a long one in the others
MUTATED = (("mono_64_128", 1), ("mono_64_128", 4), ("six_128_512", 2), ("six_128_512", 3),
           ("eight_64_256", 1), ("eight_64_256", 3), ("stereo_256_2048", 2), ("stereo_256_2048", 3))
LARGEST = ("mono_8192", 4)         # one block of 8192: cuts only, at 16 lengths
DAMAGE_SEED = 20261021
FIRST_BITS, SEEDED_BITS = 48, 40


def _neighbours(shape, k):
    p = stream(shape).packets
    return p[(k - 1) % len(p)], p[k % len(p)], p[(k + 1) % len(p)], p[(k + 2) % len(p)]


def mutations(seed=DAMAGE_SEED):
    """Per mutated packet: a cut at every byte length below its own, a flip of each of its first 48 bits (type, mode, window flags, the
    first floor words), flips of 40 seeded bits behind those, and its first half spliced to the second half of another packet."""
    out = []
    for at, (shape, k) in enumerate(MUTATED):
        rnd = random.Random(seed + at)
        before, p, after, last = _neighbours(shape, k)

        def case(kind, what, data):
            out.append(Case("%s:%d:%s:%s" % (shape, k, kind, what), shape, k, kind, (before, bytes(data), after, last)))
        for n in range(len(p)):
            case("cut", n, p[:n])
        bits = list(range(min(FIRST_BITS, 8 * len(p)))) + sorted(rnd.sample(range(FIRST_BITS, 8 * len(p)), SEEDED_BITS))
        for bit in bits:
            b = bytearray(p)
            b[bit >> 3] ^= 1 << (bit & 7)                            # (bit 0 is the first the decoder reads)
            case("flip", bit, b)
        other = stream(shape).packets[(k + 3) % len(stream(shape).packets)]
        case("splice", k + 3, p[:len(p) // 2] + other[len(other) // 2:])
    shape, k = LARGEST
    before, p, after, last = _neighbours(shape, k)
    for j in range(16):
        out.append(Case("%s:%d:cut:%d" % (shape, k, len(p) * j // 16), shape, k, "cut", (before, p[:len(p) * j // 16], after, last)))
    return out


@functools.lru_cache(maxsize=None)
def device_mutations():
    """The damaged streams that also run on the device: all of mutations().  tests/test_vorbis_core_cpu.py takes every one of them
    through the sanitised CPU build of the core first."""
    return tuple(mutations())


class CaseStream:
    """A case as vorbis_frames.batch_tables takes a stream: the shape's headers and model, the case's four packets."""
    def __init__(self, case):
        st = stream(case.shape)
        self.ident, self.setup, self.model, self.packets = st.ident, st.setup, st.model, list(case.packets)


_PACKETS = collections.defaultdict(dict)       # per shape: vorbis_textbook.decode_packet's results by the packet's bytes


def mutation_model(case):
    """(records, spectra, pcm) of a case by the model; the arrays are shared among the cases: do not write to them."""
    return TB.decode_stream(stream(case.shape).model, case.packets, cache=_PACKETS[case.shape])


@functools.lru_cache(maxsize=None)
def mutation_models():
    """mutation_model of every case of device_mutations(), in order, made once; and the seconds the model took."""
    for shape in {c.shape for c in device_mutations()}:
        stream(shape)
    t0 = time.perf_counter()
    out = tuple(mutation_model(c) for c in device_mutations())
    return out, time.perf_counter() - t0


def _floors(model, data):
    """(status, mode, prev flag, next flag, per channel: is the floor used) of one packet, by the model's own walk"""
    b = TB.Bits(data)
    status, mode, n, pf, nf = TB.packet_head(model, b)
    if status != TB.OK:
        return status, 0, 0, 0, ()
    m = model.mappings[model.modes[mode][1]]
    return status, mode, pf, nf, tuple(TB.floor_decode(model, model.floors[m.sub[m.mux[c]][0]], b) is not None for c in range(model.channels))


def mutation_reach():
    """What the set reaches, counted from the model alone: a Counter of "status:N", of flips that changed the mode or a long block's
    window flags, of mutated packets with a floor unused that the intact packet used, of cut packets whose floors stand as in the
    intact one and whose spectrum differs (the residue ended early), and of cases whose packet behind the damage delivers samples."""
    reach = collections.Counter()
    for case, (recs, spectra, _) in zip(device_mutations(), mutation_models()[0]):
        model = stream(case.shape).model
        intact = stream(case.shape).packets[case.k]
        status, mode, pf, nf, used = _floors(model, case.packets[1])
        _, mode0, pf0, nf0, used0 = _floors(model, intact)
        reach["status:%d" % status] += 1
        assert recs[1][0] == status
        if recs[2][3] > 0:
            reach["delivers behind"] += 1
        if status != TB.OK:
            continue
        if case.kind == "flip" and mode != mode0:
            reach["mode changed"] += 1
        if case.kind == "flip" and mode == mode0 and model.modes[mode][0] and (pf, nf) != (pf0, nf0):
            reach["window flags changed"] += 1
        if mode == mode0 and any(a and not b for a, b in zip(used0, used)):
            reach["floor unused"] += 1
        if case.kind == "cut" and mode == mode0 and used == used0 and any(used):
            cache = _PACKETS[case.shape]
            if intact not in cache:
                cache[intact] = TB.decode_packet(model, intact)
            if spectra[1].tobytes() != cache[intact][3].tobytes():
                reach["residue ended early"] += 1
    return reach


N_MUTATIONS = 2306


def assert_mutations_reach():
    """The conditions the set is there for, from the models alone, before anything of the product runs."""
    cases, reach = device_mutations(), mutation_reach()
    assert len(cases) == N_MUTATIONS and len({c.label for c in cases}) == len(cases)
    assert {c.shape for c in cases} == {s for s, _ in MUTATED} | {LARGEST[0]}
    for shape in {s for s, _ in MUTATED}:
        blocks = {expected(shape)[0][k][2] for s, k in MUTATED if s == shape}
        assert blocks == set(stream(shape).model.bs), shape                  # both sizes are mutated
    behind = {expected(s)[0][k + 1][2] > stream(s).model.bs[0] for s, k in MUTATED}
    assert behind == {False, True}                                           # ... and both follow a mutated packet
    assert expected(LARGEST[0])[0][LARGEST[1]][2] == 8192
    assert reach["status:%d" % TB.OK] and reach["status:%d" % TB.CORRUPT] and reach["status:%d" % TB.HEADER], reach
    assert reach["mode changed"] and reach["window flags changed"] and reach["floor unused"] and reach["residue ended early"], reach
    assert 3 * reach["delivers behind"] > len(cases), reach
    return reach


# ---------------------------------------------------------------- setup header damage (host only: the setup parse never runs on the device)
SETUP_SEED, SETUP_FLIPS, SETUP_MAX_ENTRIES = 31, 400, 4096
SetupCase = collections.namedtuple("SetupCase", "label ident setup packets")


@functools.lru_cache(maxsize=None)
def setup_stream():
    """One channel, blocks of 64 and 128, the headers as vorbis_frames.write_headers(cfg, -12) writes them."""
    return VF.random_stream(SETUP_SEED, 1, 6, 7, 8, exponent=-12)


def setup_cfg():
    return VF.random_setup(np.random.default_rng(SETUP_SEED), 1, 6, 7)


def handmade_setups():
    """[(name, cfg, the model accepts it)]: an index one past each count, and the configurations a random setup never is."""
    out = []

    def make(name, accepted=False):
        cfg = setup_cfg()
        out.append((name, cfg, accepted))
        return cfg
    n_books = len(setup_cfg()["books"])
    cfg = make("book_past_count")
    row = next(row for row in cfg["residues"][0]["books"] if any(k is not None for k in row))
    row[next(j for j, k in enumerate(row) if k is not None)] = n_books
    make("floor_past_count")["mappings"][0]["sub"][0] = (2, 0)
    make("residue_past_count")["mappings"][0]["sub"][0] = (0, 3)
    make("mapping_past_count")["modes"][1] = (1, 2)
    make("class_book_past_count")["residues"][1]["classbook"] = n_books
    for name, field in (("master_book_past_count", "master"), ("sub_book_past_count", "books")):
        cfg = make(name)
        cls = cfg["floors"][0]["classes"][cfg["floors"][0]["part"][0]]      # (the highest class: it is written)
        cls["sub"] = max(cls["sub"], 1)
        cls["books"] = (cls["books"] * 2)[:1 << cls["sub"]]
        if field == "master":
            cls["master"] = n_books
        else:
            cls["books"][0] = n_books                                       # (written as k + 1)
    cfg = make("floor_x_repeats")
    cfg["floors"][1]["x"][1] = cfg["floors"][1]["x"][0]
    make("coupling_magnitude_is_angle")["mappings"][0]["coupling"] = [(0, 0)]
    cfg = make("mux_beyond_submaps")
    cfg["mappings"][0].update(submaps=2, mux=[2], sub=[(0, 0), (1, 1)])
    cfg = make("residue_begin_behind_end", accepted=True)
    for r in cfg["residues"]:
        r["begin"], r["end"] = 32, 16
    cfg = make("class_book_of_dimension_0")
    cfg["books"][3]["dim"] = 0
    for r in cfg["residues"]:
        r["classbook"] = 3
    cfg = make("residue_book_without_values")
    row = next(row for row in cfg["residues"][2]["books"] if any(k is not None for k in row))
    row[next(j for j, k in enumerate(row) if k is not None)] = 0
    make("lookup_type_3")["books"][5]["lookup"] = 3
    make("ordered_counts_overrun")["books"][1]["overrun"] = True
    make("framing_bit_0")["framing"] = 0
    return out


@functools.lru_cache(maxsize=None)
def setup_mutations():
    """SetupCase by SetupCase: the setup packet cut at every byte length, 400 seeded bits of it flipped -- without the flips behind
    which the header, as the model reads it, declares a codebook of more than 4096 entries: the model is plain Python --, the
    hand-made configurations, and the intact headers in front of a packet that names a mode one past the count.  The packets are the
    intact stream's first five."""
    st = setup_stream()
    packets = tuple(st.packets[:5])
    out = [SetupCase("cut:%d" % n, st.ident, st.setup[:n], packets) for n in range(len(st.setup))]
    rnd = random.Random(SETUP_SEED)
    for bit in sorted(rnd.sample(range(8 * len(st.setup)), SETUP_FLIPS)):
        b = bytearray(st.setup)
        b[bit >> 3] ^= 1 << (bit & 7)
        try:
            TB.parse_headers(st.ident, bytes(b), max_entries=SETUP_MAX_ENTRIES)
        except TB.TooLarge:
            continue
        except ValueError:
            pass
        out.append(SetupCase("flip:%d" % bit, st.ident, bytes(b), packets))
    for name, cfg, _ in handmade_setups():
        out.append(SetupCase("made:" + name, *VF.write_headers(cfg, -12), packets))
    out.append(SetupCase("made:mode_past_count", st.ident, st.setup, (BAD_MODE,) + packets[:4]))
    return tuple(out)


# ---------------------------------------------------------------- V6: value vectors finite and huge
V6_DOMAIN = 2.0 ** 100             # the 1 LSB bound is asserted where max|X| * N stays below this
V6_SEED = 18                       # (chosen: the model's spectra hold infinities and NaNs)


def v6_cfg():
    """The configuration of v6_stream() (vorbis_frames.random_stream draws it first from the same seed)."""
    return VF.random_setup(np.random.default_rng(V6_SEED), 2, 6, 8, 1, 1, 1, False)


@functools.lru_cache(maxsize=None)
def v6_stream():
    """Two coupled channels, blocks of 64 and 256, under the greatest common exponent at which every value vector entry is still
    finite (the model accepts the headers; one more and it refuses them): the largest entry lies in [2^127, 2^128), so the
    residue's sums leave float32 -- infinities, and inf - inf in the coupling -- where the headers are valid by V6."""
    packets = VF.random_stream(V6_SEED, 2, 6, 8, 24, coupling=1, exponent=0).packets
    for exponent in range(127, 0, -1):
        try:
            return VF.Stream(*VF.write_headers(v6_cfg(), exponent), packets)
        except ValueError:
            pass


@functools.lru_cache(maxsize=None)
def v6_expected(max_samples=None):
    st = v6_stream()
    return TB.decode_stream(st.model, st.packets, max_samples)


def in_v6_domain(spectra):
    """Is every spectrum of a stream finite with max|X| * N below V6_DOMAIN?"""
    return all(rows is None or (np.isfinite(rows).all() and float(np.abs(rows).max()) * rows.shape[1] < V6_DOMAIN) for rows in spectra)


def granules(name):
    """Per audio packet, the samples delivered up to and with it: the granule positions of the stream's Ogg pages."""
    return [r[4] + r[3] for r in expected(name)[0]]


@functools.lru_cache(maxsize=None)
def ogg(name):
    return VF.ogg_file(stream(name), granules(name))
