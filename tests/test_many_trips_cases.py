"""The batches of tests/test_gpu_many_trips.py without a device: built for assumed CU counts of 256 and 304, each holds its
list-length condition by the builders' own counts, the oracle accepts every descriptor, and on sampled items the Python model
and the oracle agree -- so that the references alone are shown to meet the conditions before anything reaches a GPU.

A decision: the expected arenas (the oracle or the model over every descriptor) and the sampled comparisons are computed at 256
CUs only; at 304 the same builders run with a longer list, and only the counts and the mix are checked.  The arenas are what this
file's time goes to (at 256 CUs: Songcast 12 s, the line kernel 3 s, DSD -> PCM 6 s, the pulled resampler 5 s, the block resamplers
10 s), the GPU tests compute them again for the device's own CU count, and a second CU count would double that for code paths
already taken."""
import numpy as np
import pytest

import dsd_pcm_textbook as DP
import many_trips_cases as MT
import ohm_textbook as OT
import pcm_textbook as PT
import src_pull_model as PM
import src_textbook as TB
from ohpipeline_amd import capi

CUS = [256, 304]


def _pcm_model_agrees(case):
    want = case.want()
    for k in case.sampled():
        d = case.descs[k]
        out = np.frombuffer(PT.process_message(d, case.src), dtype=np.uint8)
        assert np.array_equal(out, want[int(d["dst_offset"]):int(d["dst_offset"]) + out.size]), (case.label, k)


@pytest.mark.parametrize("cus", CUS)
def test_line_kernel_lists(cus):
    case = MT.pcm_staged(cus)
    assert case.counts["chunks"] > 3 * 32 * cus + 131 and case.counts["loads"] == {0, 1, 2, 3} and case.counts["residues"] == set(range(16))
    d = case.descs
    sub = d["n_frames"].astype(np.int64) * d["channels"]
    assert case.counts["chunks"] == int(((sub + 511) // 512).sum())
    assert ((d["src_bits"] == 8) | (d["dst_bits"] == 8)).all()                      # list 0, every one
    assert {int(c) for c in d["channels"]} == set(range(1, 9)) and int(sub.max()) == 512
    kinds = d["flags"] & (MT.O.FLAG_RAMP | MT.O.FLAG_SILENCE)
    assert {0, MT.O.FLAG_RAMP, MT.O.FLAG_SILENCE} <= {int(v) for v in kinds} and (d["attenuation"] != 256).any()
    assert case.dst_bytes < 4 << 20
    for which in MT.REGISTER_LISTS:
        reg = MT.pcm_register(cus, which)
        n = reg.counts["group"] + reg.counts["heavy"]
        assert n == reg.descs.size > 2 * 64 * cus + 131 and n % 2 == 1
        assert (reg.descs["src_bits"] == MT.REGISTER_LISTS[which][0]).all() and (reg.descs["dst_bits"] == 24).all()
        gaps = reg.descs["dst_offset"][1:].astype(np.int64) - (reg.descs["dst_offset"][:-1] + reg.descs["n_frames"][:-1].astype(np.int64) * reg.descs["channels"][:-1] * 3)
        assert (gaps >= 1).all()                                                     # no message continues its neighbour
        assert reg.dst_bytes < 8 << 20
        if cus == CUS[0]:
            _pcm_model_agrees(reg)
    if cus == CUS[0]:
        _pcm_model_agrees(case)


@pytest.mark.parametrize("cus", CUS)
def test_songcast_frames(cus):
    narrow = [(MT.ohm_narrow(cus, bits), 2 * 64 * cus + 67, {1, 2}) for bits in MT.OHM_NARROW_BITS]      # one depth, one list, one launch
    assert [{m["bits"] for m in case.meta} for case, _, _ in narrow] == [{16}, {24}, {32}]
    for case, need, channels in narrow + [(MT.ohm_wide(cus), 2 * 32 * cus + 67, {6, 8})]:
        # (narrow: every frame is a prefixed chunk, silent or not; wide: a record per fragment with audio)
        assert (case.n if channels == {1, 2} else case.records) > need and {m["ch"] for m in case.meta} == channels
        assert (case.frames["n_fragments"] == 1).all() and int(case.fragments["n_frames"].max()) <= 3
        assert (case.fragments["flags"] & MT.O.FLAG_RAMP).any()
        assert (case.fragments["attenuation"] != 256).any() == any(m["bits"] == 16 for m in case.meta)   # (Songcast attenuates 16 bits only)
        if cus != CUS[0]:
            continue
        frames, want, dst_bytes, grams = case.want()                                 # (the oracle took every fragment and every frame)
        assert len(grams) == case.n and dst_bytes < 8 << 20
        for k in range(0, case.n, MT.SAMPLE_EVERY):
            fr, d, m = frames[k], case.msgs[k], case.meta[int(frames[k]["stream"])]
            s = case.streams[int(fr["stream"])]
            wire_ch, wire_bits = OT.wire_format(m["ch"], m["bits"])
            header = OT.stream_header(int(s["samples_total"]), m["rate"], int(s["bit_rate"]), int(s["volume_offset"]), wire_bits, wire_ch, m["codec"])
            audio = OT.sender_audio(PT.process_message(d, case.src), m["ch"], m["bits"])
            gram = OT.audio_frame(int(fr["flags"]), int(d["n_frames"]), int(fr["frame"]), int(fr["network_timestamp"]), int(fr["media_latency"]),
                                  int(fr["sample_start"]), header, audio)
            assert grams[k][1].tobytes() == gram, (case.label, k)


@pytest.mark.parametrize("cus", CUS)
def test_dsd_pcm_tiles(cus):
    case, tiles = MT.dsd_pcm(cus)
    d = case.descs
    assert tiles == int(((d["n_frames"].astype(np.int64) + 511) // 512).sum()) > max(3 * 2 * cus + 37, 2 * 8 * cus + 37)
    assert {int(v) for v in d["out_frame0"]} == {0, 7, 1001} and int(d["n_frames"].max()) == 512 and int((d["n_frames"] == 512).sum()) > 50
    assert {(int(w), int(p)) for w, p in zip(d["sample_block_words"], d["pad_bytes_per_chunk"])} == set(MT.DC.FORMATS)
    assert {int(e) for e in d["dst_endian"]} == {capi.ENDIAN_LITTLE, capi.ENDIAN_BIG} and (d["flags"] & capi.FLAG_RAMP).any()
    assert case.dst_bytes < 4 << 20
    # a full tile is followed by a short message with out_frame0 == 0 somewhere: the lead-in goes into a stage that held real bytes
    full = np.nonzero(d["n_frames"] == 512)[0]
    assert any(int(d["out_frame0"][k + 1]) == 0 and int(d["n_frames"][k + 1]) < 6 for k in full if k + 1 < d.size)
    assert DP.totals(d, *case.key)["n_msgs"] == d.size                               # (the model takes every descriptor's fields)
    if cus == CUS[0]:
        want = case.want()                                                           # (tests/dsd_pcm_textbook.py over the whole batch: 6 s)
        assert want.size == case.dst_bytes and (want[:3] == MT.FILL).all() and (want[-5:] == MT.FILL).all()


@pytest.mark.parametrize("cus", CUS)
def test_pulled_messages(cus):
    ramp_table = capi.ramp_table()
    for stereo_only, T in ((False, 32), (False, 64), (True, 32)):
        case = MT.pull(cus, stereo_only, T)
        d = case.descs
        assert int((d["n_frames"] > 0).sum()) > 3 * 8 * cus + 37 and int(d["n_frames"].max()) == 256
        assert {int(c) for c in d["channels"]} == ({2} if stereo_only else set(range(1, 9)))
        assert {int(v) for v in d["src_bits"]} == {8, 16, 24, 32} and {int(v) for v in d["dst_bits"]} == {16, 24, 32}
        assert (d["pos_frame"] == 0).any() and (d["flags"] & capi.FLAG_RAMP).any()
        assert case.dst_bytes < 8 << 20
        for k in range(0, d.size, 997):                                              # every window holds what its message reads
            first, frames = PM.window(int(d["pos_frame"][k]), int(d["pos_frac"][k]), int(d["step"][k]), int(d["n_frames"][k]), T)
            assert (first, frames) == (int(d["src_frame0"][k]), int(d["src_frames"][k]))
            out = PM.message_bytes(case.table(), MT.PULL_S, d[k], case.src, ramp_table)
            assert out.size == int(d["n_frames"][k]) * int(d["channels"][k]) * int(d["dst_bits"][k]) // 8
            if cus == CUS[0]:                                                        # (the whole arena by the model: 2 s a case)
                assert np.array_equal(out, case.want(ramp_table)[int(d["dst_offset"][k]):int(d["dst_offset"][k]) + out.size])
        assert int(d["dst_offset"][-1]) + int(d["n_frames"][-1]) * int(d["channels"][-1]) * int(d["dst_bits"][-1]) // 8 + 3 == case.dst_bytes


@pytest.mark.parametrize("name", list(MT.SRC_CASES))
@pytest.mark.parametrize("cus", CUS)
def test_block_resampler_units(cus, name):
    """The units by ohgpu_src_plan_digest (the plan ohgpu_src_batch_create would make, on the host) under every variant the GPU
    test runs; the oracle's arena; tests/src_textbook.py on a handful of messages."""
    case = MT.src_streams(cus, name)
    flt, lay, runs = MT.SRC_CASES[name]
    L, M, coef = MT.src_filter(flt)
    for variant, kernel in runs:
        plan = capi.src_plan_digest(L, M, flt[2], case.descs, case.src.size, case.dst_bytes, variant, coef, cus)
        assert plan["units"] > 2 * 32 * cus and plan["generic_pieces"] > 0, (name, variant, plan, case.n_streams)
        assert plan["kernel"] == {MT.WG: 3, MT.LEAN: 1, MT.BLOCK: 0}[kernel], (name, variant, plan)
    d = case.descs
    assert (d["out_frame0"][np.unique(d["src_offset"], return_index=True)[1]] > 0).any() and (d["flags"] & capi.FLAG_RAMP).any()
    assert case.dst_bytes < 128 << 20                                                # (six channels at 304 CUs: 93 MB)
    if cus != CUS[0]:
        return
    want = case.want()                                                               # (the oracle accepts every descriptor)
    ramp_table = capi.ramp_table()
    for k in range(0, d.size, 2003):
        out = TB.message_bytes(coef, L, M, flt[2], d[k], case.src, ramp_table)
        assert np.array_equal(out, want[int(d["dst_offset"][k]):int(d["dst_offset"][k]) + out.size]), (name, k)


def test_flac_candidates_outgrow_the_first_list():
    import flac_cases as FC
    from test_gpu_flac_textbook import Layout
    cases = list(MT.flac_cases())
    assert len(cases) == 256 and sum(c.label.startswith("forms") for c in cases) == 16
    lay = Layout(cases, seed=11)
    candidates = sum(FC.model(c)[0].candidates for c in cases)
    assert candidates >= 2 * MT.flac_first_list(lay.src.size), (candidates, lay.src.size)
    assert all(FC.model(c)[0].status == capi.FLAC_OK for c in cases)
