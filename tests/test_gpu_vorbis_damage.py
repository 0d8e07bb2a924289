"""The Vorbis decoder's fixed-seed damage on the device: all 2 306 cases of tests/vorbis_cases.device_mutations -- per mutated packet a
cut at every byte length, its first 48 bits and 40 seeded ones flipped, a splice; each case the four packets [p[k-1], mutated p[k],
p[k+1], p[k+2]] -- as ONE batch, a descriptor each, against the independent model (tests/vorbis_textbook.py) on both routes: every
packet record equal, the PCM of every case within 1 LSB (derived in tests/test_gpu_vorbis_textbook.py, not measured), every spectrum of
a seeded tenth bit-identical, the destination arena outside what each case wrote untouched, a second run that allocates nothing.

What this reaches that the one hand-made pattern of tests/test_gpu_vorbis_textbook.py does not is the text that exists only on the
device (csrc/vorbis_kernel.hip) and the device compile of the core: the entropy kernel's own reads of the source arena where a
packet ends at every bit of its floors and its residue -- with the packets laid at every byte alignment, a cut packet's last byte
followed at once by another packet's first, so that a reader one byte too far reads other bits --, the scan over 36 waves of
streams, a synthesis over rows the residue left half filled and floors that went unused, and the FFT route behind them.  Then V6:
value vectors finite and huge, whose sums leave float32.

Every one of these streams has passed the core's serial text under AddressSanitizer and UBSan in tests/test_vorbis_core_cpu.py first
(records and spectrum exact, PCM within 1 LSB); the conditions the set is there for are asserted from the model before anything
runs.  Nothing here is random, and nothing aims at a fault."""
import random

import numpy as np
import pytest

import vorbis_cases as VC
import vorbis_frames as VF
from ohpipeline_amd import capi
from vorbis_device import FILL, check_records, stream_pcm

pytestmark = pytest.mark.gpu

ROUTES = [pytest.param(0, id="fft"), pytest.param(1, id="plain")]
HOST_FILL = 0x5A


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.set_kernel_variant(0)
    c.close()


@pytest.fixture(scope="module")
def models():
    """by the model alone, before anything runs: what the set is there for; then every case's records, spectra and PCM"""
    VC.assert_mutations_reach()
    assert len(VC.device_mutations()) == 2306
    return VC.mutation_models()[0]


def tenth():
    """A seeded tenth of the cases, and every case of the block of 8192."""
    cases = VC.device_mutations()
    pick = set(random.Random(5).sample(range(len(cases)), len(cases) // 10))
    return sorted(pick | {i for i, c in enumerate(cases) if c.shape == VC.LARGEST[0]})


def tables(picked, pad=0):
    streams = [VC.CaseStream(VC.device_mutations()[i]) for i in picked]
    return streams, VF.batch_tables(capi, streams, pad=pad, fill=0xFF, share_images=True)


def check_arena(got, descs, pres, picked, models, fill):
    """Every case's records and PCM against the model; every byte of the arena that no case wrote still `fill`.  Returns the largest
    PCM difference."""
    untouched = np.ones(got.size, dtype=bool)
    worst = 0
    for d, i in zip(descs, picked):
        recs, _, pcm = models[i]
        case = VC.device_mutations()[i]
        check_records(pres[int(d["first_packet"]):][:int(d["n_packets"])], recs)
        mine, _ = stream_pcm(got, d, pcm.shape[0], pcm.shape[1])
        if pcm.size:
            diff = int(np.abs(mine - pcm).max())
            assert diff <= 1, (case.label, diff)
            worst = max(worst, diff)
        at = int(d["dst_offset"])
        untouched[at:at + pcm.size * 2] = False
    assert (got[untouched] == fill).all()
    return worst


def run(ctx, variant, picked, models, pad=0, spectra_of=(), times=1):
    """One batch of the picked cases on device arenas, `times` runs of it."""
    streams, (blob, descs, packets, src, dst_bytes, infos) = tables(picked, pad)
    at = packets["src_offset"]
    assert int(at[0]) == pad and (at[1:] == at[:-1] + packets["bytes"][:-1]).all()        # back to back, from the pad on
    ctx.set_kernel_variant(variant)
    b = ctx.vorbis_batch(descs, packets, blob, src.size, dst_bytes)
    ctx.set_kernel_variant(0)
    assert ctx.batch_paths(b)["vorbis_route"] == (2 if variant == 1 else 1) and ctx.vorbis_paths(b)["route"] == ctx.batch_paths(b)["vorbis_route"]
    d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
    first, allocations, worst = None, None, 0
    for _ in range(times):
        ctx.memset(d_dst, FILL, dst_bytes)
        ctx.vorbis_run(b, d_src, d_dst)
        res, pres = ctx.vorbis_results(b, descs.size, packets.size)
        got = ctx.download(d_dst, dst_bytes)
        if first is None:
            worst = check_arena(got, descs, pres, picked, models, FILL)
            for d, i, r in zip(descs, picked, res):
                assert int(r["samples"]) == models[i][2].shape[1] and int(r["reserved"]) == 0
            first, allocations = got, ctx.device_allocations()
        else:
            assert ctx.device_allocations() == allocations
            assert np.array_equal(got, first)
    for at in spectra_of:
        d, (_, spectra, _) = descs[at], models[picked[at]]
        for k, rows in enumerate(spectra):
            for c in range(0 if rows is None else rows.shape[0]):
                mine = ctx.vorbis_spectrum(b, int(d["first_packet"]) + k, c, rows.shape[1])
                assert mine.tobytes() == rows[c].tobytes(), (VC.device_mutations()[picked[at]].label, k, c)
    ctx.batch_destroy(b)
    ctx.free(d_src)
    ctx.free(d_dst)
    return worst


@pytest.mark.parametrize("variant", ROUTES)
def test_every_mutation_in_one_batch_twice_without_allocating(ctx, models, variant):
    everything = list(range(len(VC.device_mutations())))
    where = {i: at for at, i in enumerate(everything)}
    worst = run(ctx, variant, everything, models, spectra_of=[where[i] for i in tenth()], times=2)
    print("Vorbis damage set, route %d: %d cases in one batch, largest PCM difference %d LSB" % (2 if variant else 1, len(everything), worst))


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_sources_at_every_byte_alignment(ctx, models, pad):
    """The tenth's packets back to back behind 1, 2 and 3 bytes: every spectrum bit-identical, whatever follows a cut packet's last byte."""
    picked = tenth()
    run(ctx, 0, picked, models, pad=pad, spectra_of=range(len(picked)))


def test_process_host_writes_only_what_was_decoded(ctx, models):
    picked = list(range(0, len(VC.device_mutations()), 10))
    _, (blob, descs, packets, src, dst_bytes, _) = tables(picked)
    dst = np.full(dst_bytes, HOST_FILL, dtype=np.uint8)
    res, pres = ctx.vorbis_process_host(descs, packets, blob, src, dst)
    check_arena(dst, descs, pres, picked, models, HOST_FILL)
    for i, r in zip(picked, res):
        assert int(r["samples"]) == models[i][2].shape[1]


@pytest.mark.parametrize("variant", ROUTES)
def test_huge_finite_values_follow_v6(ctx, variant):
    """V6 on the device, on tests/vorbis_cases.v6_stream (value vectors finite and up to 2^127; the model's spectra hold infinities and
    NaNs): records equal, spectrum bit-identical with any NaN equal to any NaN, no byte behind max_samples written, a second run
    writes the same bytes, and every sample whose overlap's sum takes in a block transformed from a spectrum with a NaN in it -- the
    transform spreads it over the whole block -- is stored as 0.  The stream lies outside the domain of the 1 LSB bound
    (max|X| * N < 2^100, tests/test_vorbis_core_cpu.py), so the model's PCM is not the judge of the other samples."""
    st = VC.v6_stream()
    ch = st.model.channels
    total = VC.v6_expected()[2].shape[1]
    cut = total - 5
    recs, spectra, _ = VC.v6_expected(cut)
    assert not VC.in_v6_domain(spectra)
    blob, descs, packets, src, dst_bytes, _ = VF.batch_tables(capi, [st], max_samples=[cut])
    ctx.set_kernel_variant(variant)
    b = ctx.vorbis_batch(descs, packets, blob, src.size, dst_bytes)
    ctx.set_kernel_variant(0)
    assert ctx.batch_paths(b)["vorbis_route"] == (2 if variant == 1 else 1)
    d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
    runs = []
    for _ in range(2):
        ctx.memset(d_dst, FILL, dst_bytes)
        ctx.vorbis_run(b, d_src, d_dst)
        res, pres = ctx.vorbis_results(b, 1, packets.size)
        runs.append(ctx.download(d_dst, dst_bytes))
    check_records(pres, recs)
    assert np.array_equal(runs[0], runs[1])
    assert (runs[0][cut * ch * 2:] == FILL).all() and int(res["samples"][0]) == cut
    nan_block = {}
    for k, rows in enumerate(spectra):
        for c in range(ch):
            mine = ctx.vorbis_spectrum(b, k, c, rows.shape[1])
            same = (mine.view("<u4") == rows[c].view("<u4")) | (np.isnan(mine) & np.isnan(rows[c]))
            assert same.all(), (k, c)
            nan_block[(k, c)] = bool(np.isnan(mine).any())
    mine, _ = stream_pcm(runs[0], descs[0], ch, cut)
    checked, prev = 0, None
    for k, (status, mode, n, samples, position) in enumerate(recs):
        assert status == capi.VORBIS_OK
        if prev is not None:
            pk, pn = prev
            for c in range(ch):
                j = np.arange(samples)
                ci = j + n // 4 - pn // 4
                nan = (nan_block[(pk, c)] & (j < pn // 2)) | (nan_block[(k, c)] & (ci >= 0) & (ci < n // 2))
                assert (mine[c, position:position + samples][nan] == 0).all(), (k, c)
                checked += int(nan.sum())
        prev = (k, n)
    print("V6, route %d: %d of %d samples are not numbers and stored as 0" % (2 if variant else 1, checked, mine.size))
    assert checked > 100
    ctx.batch_destroy(b)
    ctx.free(d_src)
    ctx.free(d_dst)
