"""The Vorbis decoder without a device: the codeword assignment on the specification's own example, the setup parse's return codes, the ABI's
sizes, the batch check's codes, csrc/vorbis_core.h stand-alone under ASan and UBSan against the model (records and spectrum exact, PCM
within 1 LSB through the core's serial synthesis) -- whole streams, the fixed-seed packet damage set, the setup header damage set and
V6's huge finite values, the sets in one process each --, the
model against the minimal encoder, and the premise of the GPU tests' 1 LSB: a float32 FFT transform of a full-scale block of 8192."""
import collections
import os
import struct
import subprocess

import numpy as np
import pytest

import vorbis_cases as VC
import vorbis_frames as VF
import vorbis_textbook as TB
from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_codewords_of_the_specifications_example():
    """Section 3.2.1: lengths 2,4,4,4,4,2,3,3 give 00, 0100, 0101, 0110, 0111, 10, 110, 111 -- by the library and by the model."""
    lengths = [2, 4, 4, 4, 4, 2, 3, 3]
    want = [0b00, 0b0100, 0b0101, 0b0110, 0b0111, 0b10, 0b110, 0b111]
    assert list(capi.vorbis_codewords(lengths)) == want
    assert [TB.assign_codewords(lengths)[e] for e in range(8)] == want


def test_codewords_agree_on_random_trees_and_refuse_over_specified_ones():
    rng = np.random.default_rng(5)
    for _ in range(200):
        l = VF.tree_lengths(rng, int(rng.integers(2, 60))) + [0] * int(rng.integers(0, 5))
        l = [int(v) for v in rng.permutation(l)]
        drop = int(rng.integers(0, len(l)))
        if rng.random() < 0.5:
            l[drop] = 0                                              # (an under-specified tree is legal)
        model = TB.assign_codewords(l)
        assert [model.get(e, 0) for e in range(len(l))] == list(capi.vorbis_codewords(l))
    for over in ([1, 1, 1], [1, 2, 2, 3], [2, 2, 2, 2, 5]):
        with pytest.raises(ValueError):
            TB.assign_codewords(over)
        with pytest.raises(capi.OhGpuError) as e:
            capi.vorbis_codewords(over)
        assert e.value.code == capi.ERR_INVALID
    assert list(capi.vorbis_codewords([1])) == [0] and list(capi.vorbis_codewords([0, 0])) == [0, 0]


def test_abi_sizes_and_info():
    src = '#include "ohgpu.h"\n_Static_assert(sizeof(ohgpu_vorbis_info) == 32 && sizeof(ohgpu_vorbis_stream_desc) == 64 && sizeof(ohgpu_vorbis_packet_result) == 24 && sizeof(ohgpu_vorbis_stream_result) == 24, "sizes");\nint main(void){ return 0; }\n'
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src.encode(), check=True)
    assert capi.lib().ohgpu_abi_version() == 1
    st = VC.stream("six_128_512")
    image, info = capi.vorbis_setup_parse(st.ident, st.setup)
    assert (int(info["channels"]), int(info["blocksize_short"]), int(info["blocksize_long"]), int(info["codebooks"]), int(info["modes"])) == (6, 128, 512, 10, 3)
    assert image.size == int(info["image_bytes"]) and image.size % 4 == 0


def _setup_error(ident, setup):
    with pytest.raises(capi.OhGpuError) as e:
        capi.vorbis_setup_parse(ident, setup)
    return e.value.code


def test_setup_parse_return_codes():
    st = VC.stream("mono_64_128")
    assert _setup_error(st.ident, st.setup[:len(st.setup) // 2]) == capi.ERR_INVALID          # the header ends
    assert _setup_error(st.ident[:10], st.setup) == capi.ERR_INVALID
    assert _setup_error(st.setup, st.setup) == capi.ERR_INVALID
    rng = np.random.default_rng(3)
    cfg = VF.random_setup(rng, 1, 6, 7)
    cfg["books"][0]["lengths"] = [1, 1, 1] + [0] * 21                                           # an over-specified tree
    assert _setup_error(*VF.write_headers(cfg, -12)) == capi.ERR_INVALID
    cfg = VF.random_setup(np.random.default_rng(3), 1, 6, 7)
    ident, setup = VF.write_headers(cfg, -12)
    assert _setup_error(*VF.write_headers(dict(cfg, floor_type=0), -12)) == capi.ERR_UNSUPPORTED
    assert _setup_error(*VF.write_headers(dict(cfg, floor_type=2), -12)) == capi.ERR_INVALID
    # nine channels
    w = VF.Writer()
    for c in b"\x01vorbis":
        w.write(c, 8)
    w.write(0, 32), w.write(9, 8), w.write(44100, 32), w.write(0, 32), w.write(0, 32), w.write(0, 32), w.write(6, 4), w.write(7, 4), w.write(1, 1)
    assert _setup_error(w.bytes(), setup) == capi.ERR_UNSUPPORTED


def test_batch_check_codes():
    st = VC.stream("mono_64_128")
    blob, descs, packets, src, dst_bytes, _ = VF.batch_tables(capi, [st, st])
    assert capi.vorbis_batch_check(descs, packets, blob, src.size, dst_bytes) is None
    assert capi.vorbis_batch_check(descs[:0], packets[:0], blob[:0], 0, 0) is None

    def code(d=descs, p=packets, b=blob, s=src.size, t=dst_bytes):
        with pytest.raises(capi.OhGpuError) as e:
            capi.vorbis_batch_check(d, p, b, s, t)
        return e.value.code
    for field, value in (("flags", 2), ("first_packet", 1), ("image_offset", 2), ("image_bytes", 64), ("dst_offset", 2)):
        d = descs.copy()
        d[field][1] = value
        assert code(d=d) == capi.ERR_INVALID, field
    d = descs.copy()
    d["reserved"][0][2] = 1
    assert code(d=d) == capi.ERR_INVALID
    bad = blob.copy()
    bad[0] ^= 1                                                      # not an image
    assert code(b=bad) == capi.ERR_INVALID
    assert code(p=packets[:-1]) == capi.ERR_INVALID
    # an image is walked, not only its head: a tree that points outside itself, value vectors beyond the image, a book index out of range
    words = blob.view("<u4").copy()
    head = dict(zip(("magic", "words", "channels", "rate", "bs0", "bs1", "n_books", "n_floors", "n_residues", "n_mappings", "n_modes", "mode_bits",
                     "off_books", "off_floors", "off_residues", "off_mappings", "off_modes"), (int(v) for v in words[:17])))
    book0 = head["off_books"]                                        # entries, dim, lookup, off_tree, n_nodes, off_values, used, reserved
    value_book = next(k for k in range(head["n_books"]) if words[book0 + 8 * k + 2])
    for at, value in ((int(words[book0 + 3]), 1 << 20), (book0 + 8 * value_book + 5, head["words"] - 1), (book0 + 4, 0),
                      (head["off_residues"] + 5, 200), (head["off_modes"] + 1, 9)):
        hurt = words.copy()
        hurt[at] = value
        assert code(b=hurt.view(np.uint8)) == capi.ERR_INVALID, at
    assert code(s=src.size - 5) == capi.ERR_BOUNDS
    assert code(t=dst_bytes - 1) == capi.ERR_BOUNDS


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = tmp_path_factory.mktemp("vorbis_core") / "driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpp", "vorbis_core_driver.cpp"), "-o", str(out)], check=True)
    return out


def _case_bytes(st, packets, model=None):
    """(case, expect, pcm) as tests/cpp/vorbis_core_driver.cpp reads them; model: (records, spectra, pcm), None for headers the model refuses"""
    case = struct.pack("<I", len(st.ident)) + st.ident + struct.pack("<I", len(st.setup)) + st.setup + struct.pack("<I", len(packets))
    for p in packets:
        case += struct.pack("<I", len(p)) + p
    if model is None:
        return case, b"", b""
    recs, spectra, pcm = model
    want = b""
    for (status, mode, block, samples, position), rows in zip(recs, spectra):
        want += struct.pack("<IIIIQ", status, mode, block, samples, position)
        if rows is not None:
            want += rows.astype("<f4").tobytes()
    return case, want, pcm.T.astype("<i4").tobytes()


def _case_files(tmp_path, st, packets, max_samples):
    case, want, pcm = _case_bytes(st, packets, TB.decode_stream(st.model, packets, max_samples))
    (tmp_path / "case").write_bytes(case)
    (tmp_path / "expect").write_bytes(want)
    (tmp_path / "pcm").write_bytes(pcm)
    return str(tmp_path / "case"), str(tmp_path / "expect"), str(tmp_path / "pcm")


PCM_MODEL, PCM_V6 = 1, 2


def _run_many(driver, path, entries):
    """The driver's --many mode over entries of (label, (case, expect, pcm), refused by the model, PCM_MODEL or PCM_V6), all with no
    bound on the samples: the finished process, and {label: the core's parse code} of the cases whose headers it refused."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(entries)))
        for label, (case, want, pcm), refused, pcm_mode in entries:
            name = label.encode()
            f.write(struct.pack("<I", len(name)) + name + struct.pack("<IIQ", int(refused), pcm_mode, 1 << 40))
            for blob in (case, want, pcm):
                f.write(struct.pack("<I", len(blob)) + blob)
    r = subprocess.run([str(driver), "--many", str(path)], capture_output=True, text=True)
    codes = {line.split()[1]: int(line.split()[2]) for line in r.stdout.splitlines() if line.startswith("PARSE ")}
    return r, codes


@pytest.mark.parametrize("name", sorted(VC.SHAPES))
def test_core_under_the_sanitizers_matches_the_model(driver, tmp_path, name):
    st = VC.stream(name)
    total = sum(r[3] for r in VC.expected(name)[0])
    case, want, pcm = _case_files(tmp_path, st, st.packets, total - 7)
    r = subprocess.run([str(driver), case, want, str(total - 7), pcm], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stderr[-2000:]


def test_core_under_the_sanitizers_takes_damage(driver, tmp_path):
    name = "six_128_512"
    packets = VC.damaged(name)
    case, want, pcm = _case_files(tmp_path, VC.stream(name), packets, 1 << 30)
    r = subprocess.run([str(driver), case, want, str(1 << 30), pcm], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stderr[-2000:]
    recs = TB.decode_stream(VC.stream(name).model, packets)[0]
    assert [recs[k][0] for k in (4, 7, 9)] == [TB.CORRUPT, TB.CORRUPT, TB.HEADER] and recs[2][0] == TB.OK


def test_core_under_the_sanitizers_takes_every_mutation(driver, tmp_path):
    """All 2 306 cases of tests/vorbis_cases.device_mutations -- a cut at every byte, the first 48 bits and 40 seeded ones flipped, a
    splice, per mutated packet -- through the core's serial text in one process: records and spectrum exact, PCM within 1 LSB, the
    sanitizers silent.  This is what lets the set onto the device (tests/test_gpu_vorbis_damage.py).  What the set is there for is
    asserted from the model alone first."""
    reach = VC.assert_mutations_reach()
    cases, (models, seconds) = VC.device_mutations(), VC.mutation_models()
    print("Vorbis damage set: %d cases, the model took %.1f s; %s" % (len(cases), seconds, dict(reach)))
    entries = [(c.label, _case_bytes(VC.stream(c.shape), c.packets, m), False, PCM_MODEL) for c, m in zip(cases, models)]
    r, codes = _run_many(driver, tmp_path / "mutations", entries)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK %d" % VC.N_MUTATIONS) and not codes, r.stderr[-4000:]


UNSUPPORTED_BY_DESIGN = ("unsupported floor 0", "unsupported: more than 32 coupling steps", "unsupported: value vectors beyond the image's cap")


def test_core_under_the_sanitizers_takes_setup_header_damage(driver, tmp_path):
    """tests/vorbis_cases.setup_mutations -- every cut of a setup packet, 400 seeded flips of it, the hand-made configurations -- through
    vorbiscore::parse_setup under the sanitizers, held to the model's parse: both accept or both refuse (ValueError is the model's
    refusal; any other exception of the model's is the model's bug and fails here).  Accepted by both: the image passes
    vorbiscore::image_valid, the intact stream's first five packets decode with records and spectrum exact, and the PCM within 1 LSB
    where the model's spectra stay in V6's domain (finite, max|X| * N < 2^100; outside it the stored samples are held to V6 alone).
    Refused by both: the core's code is INVALID, UNSUPPORTED only for what DESIGN.md 5.23 lists under that name."""
    cases = VC.setup_mutations()
    kinds = collections.Counter(c.label.split(":")[0] for c in cases)
    assert kinds["cut"] == len(VC.setup_stream().setup) and 300 < kinds["flip"] <= VC.SETUP_FLIPS and kinds["made"] == len(VC.handmade_setups()) + 1 == 17, kinds
    expected_made = {"made:" + name: accepted for name, _, accepted in VC.handmade_setups()}
    expected_made["made:mode_past_count"] = True
    entries, refusals = [], {}
    for c in cases:
        try:
            model = TB.parse_headers(c.ident, c.setup)
        except ValueError as e:
            refusals[c.label] = str(e)
            entries.append((c.label, _case_bytes(c, c.packets), True, PCM_MODEL))
            continue
        want = TB.decode_stream(model, c.packets)
        entries.append((c.label, _case_bytes(c, c.packets, want), False, PCM_MODEL if VC.in_v6_domain(want[1]) else PCM_V6))
    for label, accepted in expected_made.items():
        assert (label not in refusals) == accepted, (label, refusals.get(label))
    accepted = len(cases) - len(refusals)
    print("Vorbis setup damage: %d cases (%s), the model accepts %d; outside V6's domain %d" % (len(cases), dict(kinds), accepted, sum(1 for e in entries if e[3] == PCM_V6)))
    assert accepted > 100 and len(refusals) > 100                     # (the set reaches both answers many times over)
    r, codes = _run_many(driver, tmp_path / "setups", entries)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK %d" % len(cases)), r.stderr[-4000:]
    assert set(codes) == set(refusals)
    for label, code in codes.items():
        assert code == (capi.ERR_UNSUPPORTED if refusals[label] in UNSUPPORTED_BY_DESIGN else capi.ERR_INVALID), (label, code, refusals[label])


def _headers_code(ident, setup):
    """(the library's answer to the headers: 0 or its error code, the model's refusal or None)"""
    try:
        TB.parse_headers(ident, setup)
        refusal = None
    except ValueError as e:
        refusal = str(e)
    try:
        capi.vorbis_setup_parse(ident, setup)
        return 0, refusal
    except capi.OhGpuError as e:
        return e.code, refusal


def test_setup_parse_refuses_values_that_are_not_finite():
    """V6's first half, in three shapes.  The exponent field of min and delta at its top (2^235: every entry infinite): INVALID.  Every
    entry finite and above 2^100: accepted.  A book of sequence_p whose entries are finite each and whose running sum is not: INVALID,
    and accepted without sequence_p."""
    cfg = VC.v6_cfg()
    assert _headers_code(*VF.write_headers(cfg, 1023 - 788)) == (capi.ERR_INVALID, "invalid: a value vector entry is not finite (V6)")
    st = VC.v6_stream()
    assert _headers_code(st.ident, st.setup) == (0, None)
    values = np.concatenate([np.abs(b.values).ravel() for b in st.model.books if b.values is not None])
    assert np.isfinite(values).all() and values.max() >= 2.0 ** 127 and 2 * (values > 2.0 ** 100).sum() > values.size
    for seq, want in ((1, (capi.ERR_INVALID, "invalid: a value vector entry is not finite (V6)")), (0, (0, None))):
        cfg = VC.v6_cfg()
        for b in cfg["books"]:
            if b["lookup"]:                                           # every entry (1 * 1 - 1) * 2^123 = 0 ...
                b.update(min_mant=1, delta_mant=1, vbits=4, seq=0, mult=[1] * len(b["mult"]))
        b = cfg["books"][8]                                          # ... but this book's: 64 entries of dimension 8, each (15 * 2 - 1) * 2^123
        assert b["dim"] == 8 and b["lookup"] == 1                    # = 2^127.86, finite; the second running sum is not
        b.update(delta_mant=2, seq=seq, mult=[15] * len(b["mult"]))
        assert _headers_code(*VF.write_headers(cfg, 123)) == want, seq


def test_core_under_the_sanitizers_on_huge_finite_values(driver, tmp_path):
    """V6's second half on the CPU.  tests/vorbis_cases.v6_stream: value vectors finite and up to 2^127, so that the residue's float32
    sums reach infinity and the coupling inf - inf.  Records exact, spectrum bit-identical (two NaNs count as equal), and every stored
    sample by V6: 0 where the overlap's sum is not a number, clamped where it is beyond 16 bits.

    THE 1 LSB DOMAIN.  The model's PCM is the judge only where its spectrum satisfies max|X| * N < 2^100 (N = block / 2 values, all
    finite): there a float32 transform cannot overflow (N terms of at most max|X|, far below 2^128) and its error is the relative one
    the 1 LSB bound is derived from.  Outside it -- this stream -- the float32 transforms may overflow where the model's float64 direct
    form does not; no route is wrong by a written rule, and only the properties above hold.  Every other stream of the tests lies
    inside the domain, which is asserted here."""
    for name in VC.SHAPES:
        assert VC.in_v6_domain(VC.expected(name)[1]), name
    st = VC.v6_stream()
    want = VC.v6_expected()
    assert not VC.in_v6_domain(want[1])
    assert any(np.isnan(rows).any() for rows in want[1] if rows is not None) and any(np.isinf(rows).any() for rows in want[1] if rows is not None)
    r, codes = _run_many(driver, tmp_path / "v6", [("v6", _case_bytes(st, st.packets, want), False, PCM_V6)])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK 1") and not codes, r.stderr[-4000:]


def test_every_shape_covers_what_it_is_there_for():
    pairs = set()
    for name in ("mono_64_128", "stereo_256_2048"):
        st = VC.stream(name)
        blocks = [r[2] for r in VC.expected(name)[0]]
        pairs |= {(a > min(blocks), b > min(blocks)) for a, b in zip(blocks, blocks[1:])}
        assert len(st.packets) >= 70
    assert len(pairs) == 4
    pcm = VC.expected("stereo_clips")[2]
    assert (pcm == 32767).any() and (pcm == -32768).any()
    for name in VC.SHAPES:
        if name != "stereo_clips":
            assert 8000 < np.abs(VC.expected(name)[2]).max() < 32767, name
    m = VC.stream("six_128_512").model
    assert all(len(mp.coupling) == 2 and mp.submaps == 2 for mp in m.mappings)
    assert {r.type for r in m.residues} == {0, 1, 2} and any(bin(c).count("1") > 1 for r in m.residues for c in r.cascade)
    assert {b.lookup for b in m.books} == {0, 1, 2} and any(b.entries == 1 for b in m.books) and any(0 in b.lengths for b in m.books)


def test_minimal_encoder_round_trip():
    """A sine sweep through the textbook forward MDCT, a flat floor and a scalar book of whole numbers -- a quantiser of step q = the floor's 9.82e-4 --, decoded by the model.
    Each of the N = n / 2 coefficients of a block errs by at most q / 2, uniformly for a coefficient that is busy: variance q^2 / 12.  The
    IMDCT sums N of them through cosines (mean square 1 / 2): N q^2 / 24 a block sample; the two overlapping blocks' windows square-sum to
    1, so that is the output's noise power: with N = 128, 5.1e-6.  The sweep's power is 0.5^2 / 2: SNR 43.8 dB.  Quiet coefficients err by
    less, so the figure is a floor; 3 dB are left for the blocks in which the few busy coefficients all round one way.  A wrong window,
    scale or overlap leaves an error the size of the signal: SNR below 10 dB."""
    n, N = 256, 128
    t = np.arange(n * 24)
    signal = 0.5 * np.sin(2 * np.pi * (0.01 + 0.00002 * t) * t)
    st = VF.encode(signal)
    _, _, x = TB.decode_stream(st.model, st.packets, want_float=True)
    ref = signal[N:N + x.shape[1]]
    q = float(TB.DB[VF.ENC_FLOOR])
    want_db = 10 * np.log10((0.5 ** 2 / 2) / (N * q * q / 24)) - 3.0
    got_db = 10 * np.log10((ref ** 2).mean() / ((x[0] - ref) ** 2).mean())
    print("minimal encoder: SNR %.1f dB, asked %.1f dB" % (got_db, want_db))
    assert x.shape[1] == len(signal) - n and got_db >= want_db


def test_float32_fft_transform_of_a_full_scale_block_is_far_inside_a_quarter_lsb():
    """The GPU tests' premise: the product's transform -- the DCT-IV through an N / 2-point radix-2 FFT, float32 throughout, tables rounded
    from double -- against the model's float64 direct form, at n = 8192 on a block whose output peaks at full scale."""
    N = 4096
    M = N // 2
    rng = np.random.default_rng(8)
    x = rng.standard_normal(N)
    x = (x / np.abs(TB.imdct(x)).max()).astype(np.float32)
    m = np.arange(M)
    A = np.exp(-1j * np.pi * (4 * m + 1) / (4 * N)).astype(np.complex64)
    B = np.exp(-1j * np.pi * m / N).astype(np.complex64)
    a = ((x[0::2] + 1j * x[::-1][0::2]).astype(np.complex64) * A)[[int(format(j, "011b")[::-1], 2) for j in range(M)]]
    h = 1
    while h < M:
        W = np.exp(-2j * np.pi * np.arange(h) / (2 * h)).astype(np.complex64)
        a = a.reshape(-1, 2, h)
        hi = (a[:, 1, :] * W[None, :]).astype(np.complex64)
        a = np.stack([a[:, 0, :] + hi, a[:, 0, :] - hi], axis=1).reshape(-1).astype(np.complex64)
        h *= 2
    c = (a * B).astype(np.complex64)
    u = np.empty(N, dtype=np.float32)
    u[0::2], u[::-1][0::2] = c.real, -c.imag
    err = np.abs(u.astype(np.float64) - TB.dct4(x)).max()
    print("float32 FFT transform at n = 8192: largest difference %.3g, a quarter LSB is %.3g" % (err, 0.25 / 32768))
    assert err < 0.25 / 32768
