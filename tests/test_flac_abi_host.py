"""The host-only half of the FLAC ABI: ohgpu_flac_streaminfo and the descriptor validation of ohgpu_flac_batch_create
(ohgpu_flac_batch_check) -- each refusal with its code and text, without a device."""
import numpy as np
import pytest

import flac_cases as FC
from ohpipeline_amd import capi


def desc(**over):
    d = np.zeros(1, dtype=capi.FLAC_STREAM_DESC)
    base = dict(src_offset=0, src_bytes=1000, dst_offset=0, dst_plane_stride=4000, first_sample=0, max_samples=1000, sample_rate=44100,
                blocksize=0, max_blocksize=4096, channels=2, bits=16, flags=0)
    base.update(over)
    for k, v in base.items():
        d[k] = v
    return d


@pytest.mark.parametrize("name", FC.fixture_names())
def test_streaminfo_of_every_fixture(name):
    fx = FC.fixture(name)
    info, audio = capi.flac_streaminfo(fx.data)
    assert audio == fx.audio
    assert {k: info[k] for k in fx.info} == fx.info
    assert capi.flac_streaminfo(fx.data[:fx.audio])[1] == fx.audio          # the metadata alone is enough


def test_streaminfo_refusals():
    fx = FC.fixture("tiny_s16_stereo_44k1_b16")
    for bad, text in ((b"fLaX" + fx.data[4:], "fLaC"), (fx.data[:20], "end inside the metadata"), (fx.data[:3], "fLaC"),
                      (fx.data[:4] + bytes([0x84]) + fx.data[5:], "not STREAMINFO")):
        with pytest.raises(capi.OhGpuError) as e:
            capi.flac_streaminfo(bad)
        assert e.value.code == capi.ERR_INVALID and text in str(e.value)
    # a padding block in front of the audio: skipped
    padded = fx.data[:4] + bytes([0x00]) + fx.data[5:fx.audio] + bytes([0x81, 0, 0, 5]) + bytes(5) + fx.data[fx.audio:]
    assert capi.flac_streaminfo(padded)[1] == fx.audio + 9


def test_descriptor_validation_without_a_device():
    capi.flac_batch_check(desc(), 1000, 8000)
    capi.flac_batch_check(desc(flags=capi.FLAC_OUT_PACKED_BE, dst_plane_stride=0), 1000, 4000)
    for d, sa, da, code, text in (
        (desc(), 999, 8000, capi.ERR_BOUNDS, "source arena"),
        (desc(src_offset=2 ** 40), 1000, 8000, capi.ERR_BOUNDS, "source arena"),
        (desc(), 1000, 7999, capi.ERR_BOUNDS, "destination arena"),
        (desc(dst_plane_stride=4002), 1000, 9000, capi.ERR_INVALID, "multiples of 4"),
        (desc(dst_offset=2), 1000, 9000, capi.ERR_INVALID, "multiples of 4"),
        (desc(dst_plane_stride=3996), 1000, 9000, capi.ERR_INVALID, "planes overlap"),
        (desc(bits=20), 1000, 8000, capi.ERR_UNSUPPORTED, "bit depth 20"),
        (desc(bits=32), 1000, 8000, capi.ERR_UNSUPPORTED, "bit depth 32"),
        (desc(channels=0), 1000, 8000, capi.ERR_INVALID, "channels"),
        (desc(channels=9), 1000, 80000, capi.ERR_INVALID, "channels"),
        (desc(flags=4), 1000, 8000, capi.ERR_INVALID, "flags"),
        (desc(max_blocksize=8), 1000, 8000, capi.ERR_INVALID, "block size"),
        (desc(flags=capi.FLAC_OUT_PACKED_BE), 1000, 8000, capi.ERR_INVALID, "packed"),
    ):
        with pytest.raises(capi.OhGpuError) as e:
            capi.flac_batch_check(d, sa, da)
        assert e.value.code == code and text in str(e.value), str(e.value)
