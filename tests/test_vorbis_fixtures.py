"""tests/golden/vorbis (written by tests/golden/make_vorbis_fixtures.py) pins what every Vorbis test decodes: each stream of
tests/vorbis_cases.py, made from its seed again, must be the fixture's packets byte for byte -- a change of numpy's generator or of the
stream writer shows here --, the model's PCM of the fixture's packets must have the recorded MD5 -- a change of the model shows here --,
and ohgpu_vorbis_head must find the headers and the first audio packet of every file."""
import gzip
import hashlib
import json
import os

import pytest

import vorbis_cases as VC
import vorbis_frames as VF
import vorbis_textbook as TB
from ohpipeline_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vorbis")
TABLE = json.load(open(os.path.join(GOLDEN, "streams.json")))


def test_every_stream_has_its_fixture():
    assert sorted(TABLE) == sorted(list(VC.SHAPES) + list(VC.TREMOR_SHAPES))
    for name in TABLE:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".ogg.gz")) < 1 << 20


@pytest.mark.parametrize("name", sorted(TABLE))
def test_stream_and_model_are_the_fixtures(name):
    data = gzip.decompress(open(os.path.join(GOLDEN, name + ".ogg.gz"), "rb").read())
    packets = VF.ogg_packets(data)
    st = VC.stream(name)
    assert packets[0] == st.ident and packets[1] == VF.COMMENT and packets[2] == st.setup and packets[3:] == list(st.packets)
    assert data == VC.ogg(name)
    model = TB.parse_headers(packets[0], packets[2])
    recs, _, pcm = TB.decode_stream(model, packets[3:])
    want = TABLE[name]
    assert (model.channels, len(packets) - 3, pcm.shape[1]) == (want["channels"], want["packets"], want["samples"])
    assert hashlib.md5(VC.pcm_s16be(pcm)).hexdigest() == want["pcm_md5"]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_head_finds_the_headers_and_the_first_audio_packet(name):
    data = VC.ogg(name)
    st = VC.stream(name)
    head = capi.vorbis_head(data)
    image, info = capi.vorbis_setup_parse(st.ident, st.setup)
    assert head["image"].tobytes() == image.tobytes() and head["info"].tobytes() == info.tobytes() and head["serial"] == 0x5642
    # the audio begins on the third page, at its first segment
    third = len(data) - len(data.split(b"OggS", 3)[3]) - 4
    assert (head["page_offset"], head["segment"], head["seq"]) == (third, 0, 2)
    # ... and the head asks for no more than the header pages: cut behind them it answers where the walk would go on, the same place
    cut = capi.vorbis_head(data[:third])
    assert (cut["page_offset"], cut["segment"], cut["seq"]) == (third, 0, 2)


def test_head_refuses_what_is_not_ogg_vorbis():
    data = VC.ogg("mono_64_128")
    for bad in (data[:100], b"OggS" + bytes(200), data.replace(b"\x05vorbis", b"\x05vorbiz", 1)):
        with pytest.raises(capi.OhGpuError) as e:
            capi.vorbis_head(bad)
        assert e.value.code == capi.ERR_INVALID
