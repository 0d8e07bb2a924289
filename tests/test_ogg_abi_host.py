"""The host-only calls of the Ogg section of include/ohgpu.h, without a device: the head of an Ogg FLAC stream (ohgpu_ogg_flac_head)
over every committed FLAC fixture wrapped in pages by the tests' own muxer, and what it refuses.  The wrapped streams are also what
tests/test_gpu_ogg_flac_to_driver.py decodes, so the muxer is held here to the model: from the audio page on, the packets' bytes are
the native stream's audio bytes."""
import pytest

import flac_cases as FC
import flac_textbook as FT
import ogg_cases as GC
import ogg_textbook as OX
from ohpipeline_amd import capi


@pytest.mark.parametrize("name", FC.fixture_names())
def test_the_head_of_every_fixture_as_ogg_flac(name):
    fx = FC.fixture(name)
    data, audio_page, audio_seq = GC.ogg_flac(fx, max_segments=7)
    assert data[:4] == b"OggS" and data[37:41] == b"fLaC"                      # what CodecFlac::Recognise asks of the second kind
    info, serial, off, seg, seq = capi.ogg_flac_head(data)
    want, _ = FT.streaminfo(fx.data)
    assert {k: int(info[k]) for k in ("min_blocksize", "max_blocksize", "sample_rate", "channels", "bits", "total_samples")} == \
        {k: want[k] for k in ("min_blocksize", "max_blocksize", "sample_rate", "channels", "bits", "total_samples")}
    assert bytes(info["md5"]) == bytes(want["md5"])
    assert (serial, off, seg, seq) == (0x464C, audio_page, 0, audio_seq)
    assert capi.ogg_flac_head(data[:audio_page])[1:] == (serial, off, seg, seq)     # (the metadata pages alone say where the audio will begin)
    out = OX.demux(data[off:], serial=serial, expect_seq=seq, first_page_segment=seg, flags=OX.FLAC_MAPPING)
    assert out["status"] == OX.OK and out["run"] == fx.data[fx.audio:] and out["eos_seen"] == 1
    spans = FC.frame_spans(name)
    assert [(k["run_pos"], k["run_pos"] + k["bytes"]) for k in out["packets"]] == [(a - fx.audio, b - fx.audio) for a, b in spans]


def code_of(data):
    with pytest.raises(capi.OhGpuError) as e:
        capi.ogg_flac_head(data)
    return e.value.code


def test_what_the_head_refuses():
    fx = FC.fixture("s8_mono_8k_b256_l2")
    data, audio_page, _ = GC.ogg_flac(fx)
    assert code_of(fx.data) == capi.ERR_INVALID                                   # a native stream
    assert code_of(data[:60]) == capi.ERR_INVALID                                 # the bytes end inside the first page
    assert code_of(b"") == capi.ERR_INVALID
    packets, granules, n_meta = GC.flac_packets(fx)
    plain = b"".join(GC.mux([b"fLaC" + packets[0][13:]] + packets[1:], 5, granules=granules))
    assert code_of(plain) == capi.ERR_INVALID                                     # pages, but no mapping header
    if n_meta > 1:
        assert code_of(data[:audio_page - 9]) == capi.ERR_INVALID                 # the bytes end inside the metadata
    joined = packets[:n_meta - 1] + [packets[n_meta - 1] + packets[n_meta]] + packets[n_meta + 1:]
    glued = b"".join(GC.mux(joined, 5, granules=granules[:n_meta - 1] + granules[n_meta:]))
    assert code_of(glued) == capi.ERR_UNSUPPORTED                                 # the last metadata block shares its packet with a frame
