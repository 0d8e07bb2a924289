"""tests/flac_textbook.py -- the plain-Python FLAC decoder the device is held against -- pinned without any reference code: for
every fixture, encoder-made and handmade, the MD5 of what it decodes is the MD5 in the stream's own STREAMINFO.  Where oracle/_ref
exists it also equals the reference's libFLAC frame by frame.  And the fixture set as a whole must contain every form on the list
below (the census): a condition on the committed fixtures."""
import pytest

import flac_cases as FC
import flac_ref
import flac_textbook as T


@pytest.mark.parametrize("name", FC.fixture_names())
def test_model_md5_is_streaminfos(name):
    fx = FC.fixture(name)
    res, _ = FC.model(FC.whole(fx))
    assert res.status == T.OK and res.samples == fx.samples and res.bytes_consumed == len(fx.data) - fx.audio
    assert res.candidates_rejected == res.candidates - len(res.frames)
    assert T.md5_of(res.frames, fx.info["bits"]) == fx.info["md5"]


def test_the_five_encoder_made_fixtures_hold_no_false_candidate():
    got = [FC.model(FC.whole(FC.fixture(n)))[0].candidates for n in
           ("s16_stereo_44k1_b1152_l5", "s24_6ch_48k_b4608_l3", "s24_stereo_44k1_b4096_l8", "s24_stereo_44k1_b576_l0", "s8_mono_8k_b256_l2")]
    assert got == [10, 2, 3, 11, 12]
    assert FC.model(FC.whole(FC.fixture("false_candidate_s16_stereo_44k1_b576")))[0].candidates_rejected == 1


@pytest.mark.skipif(not flac_ref.available(), reason="oracle/_ref/libflac_ref.so is not built")
@pytest.mark.parametrize("name", FC.fixture_names())
def test_model_equals_the_reference_decoder_frame_by_frame(name):
    fx = FC.fixture(name)
    res, _ = FC.model(FC.whole(fx))
    frames, md5_ok = flac_ref.decode(fx.data)
    assert md5_ok and len(frames) == len(res.frames)
    for (n, ch, bits, rate, planes), f in zip(frames, res.frames):
        assert (n, ch, bits, rate) == (f.header.blocksize, f.header.channels, f.header.bits, f.header.rate)
        assert planes.tolist() == f.planes


CENSUS = [
    "sub:CONSTANT", "sub:VERBATIM", "sub:FIXED:0", "sub:FIXED:1", "sub:FIXED:2", "sub:FIXED:3", "sub:FIXED:4",
    "sub:LPC:1", "sub:LPC:8", "sub:LPC:12", "sub:LPC:32:precision:15",
    "method:RICE", "method:RICE2", "partition_order:0", "escape:0", "escape:>0", "wasted:one_of_a_pair",
    "assignment:independent", "assignment:left_side", "assignment:right_side", "assignment:mid_side",
    "channels:1", "channels:2", "channels:6", "channels:8", "bits:8", "bits:16", "bits:24",
    "blocksize:16", "blocksize:192", "blocksize:576", "blocksize:4096", "blocksize:4608",
    "blocksize_code:6", "blocksize_code:7",            # the 8- and the 16-bit trailer
    "rate_code:0", "rate_code:12", "rate_code:13", "rate_code:14",   # STREAMINFO's, kHz, Hz, tens of Hz
    "blocking:fixed", "blocking:variable",
    "number_bytes:1", "number_bytes:2", "number_bytes:3", "number_bytes:4", "number_bytes:5", "number_bytes:6", "number_bytes:7",
]


FAR = {   # fixture -> (the first frame's coded number, the coded numbers' lengths); three frames of 16 samples each
    "variable_from_2p31m32_s16_stereo_48k_b16": ((1 << 31) - 32, [6, 6, 7]),
    "variable_from_2p36m48_s16_stereo_48k_b16": ((1 << 36) - 48, [7, 7, 7]),
    "fixed_from_frame_127_s16_stereo_44k1_b16": (127, [1, 2, 2]),
    "fixed_from_frame_2047_s16_stereo_44k1_b16": (2047, [2, 3, 3]),
    "fixed_from_frame_65535_s16_stereo_44k1_b16": (65535, [3, 4, 4]),
    "fixed_from_frame_2p21m1_s16_stereo_44k1_b16": ((1 << 21) - 1, [4, 5, 5]),
    "fixed_from_frame_2p26m1_s16_stereo_44k1_b16": ((1 << 26) - 1, [5, 6, 6]),
    "fixed_from_frame_2p31m3_s16_stereo_44k1_b16": ((1 << 31) - 3, [6, 6, 6]),
}


@pytest.mark.parametrize("name", sorted(FAR))
def test_far_fixtures_sit_where_their_names_say(name):
    """The streams of far positions: every length of coded number at its transition, first samples past 2^31, 2^32 and up to 2^36."""
    number, lengths = FAR[name]
    fx = FC.fixture(name)
    res, _ = FC.model(FC.whole(fx))
    variable = name.startswith("variable")
    assert fx.first_sample == (number if variable else number * 16) and fx.info["total_samples"] == 0 and fx.samples == 48
    assert [f.header.number for f in res.frames] == [number + (16 * j if variable else j) for j in range(3)]
    assert [f.header.number_bytes for f in res.frames] == lengths
    assert res.first_sample_decoded == fx.first_sample and res.places == [0, 16, 32]
    assert max(FC.fixture(n).first_sample for n in FAR) == (1 << 36) - 48 and sum(FC.fixture(n).first_sample >= 1 << 32 for n in FAR) >= 2


def test_census_of_the_committed_fixtures():
    seen = {}
    short_last = False
    for fx in FC.fixtures():
        res, _ = FC.model(FC.whole(fx))
        for k, v in res.census.items():
            seen[k] = seen.get(k, 0) + v
        sizes = [f.header.blocksize for f in res.frames]
        short_last = short_last or (len(sizes) > 1 and sizes[-1] < sizes[-2])
        if fx.name.startswith("variable"):
            assert res.frames[0].header.variable and res.frames[0].header.number >= 1 << 21       # five bytes of coded number
    missing = [k for k in CENSUS if not seen.get(k)]
    assert not missing, missing
    assert any(int(k.split(":")[1]) >= 6 for k in seen if k.startswith("partition_order:"))
    assert short_last
    # the stream whose LPC sums pass 2^32: 24-bit samples at full scale against a 15-bit coefficient
    fx = FC.fixture("fullscale_lpc_s24_stereo_48k_b192")
    res, _ = FC.model(FC.whole(fx))
    assert max(abs(v) for f in res.frames for v in f.planes[0]) * 16383 > 1 << 32
