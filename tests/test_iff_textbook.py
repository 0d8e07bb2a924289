"""The independent model of the PCM file layer (tests/iff_textbook.py) held to the record of the tests' own writer
(tests/iff_cases.py) on every named file, to the status every named malformed file must get, and -- where Python's own `wave` and
`aifc` modules can read a fixture -- to what those modules say of it: the format fields, and the audio after the byte-order change."""
import io

import numpy as np
import pytest

import iff_cases as IC
import iff_textbook as IX


@pytest.mark.parametrize("name", list(IC.named_good()))
def test_the_model_reads_what_the_writer_wrote(name):
    w = IC.named_good()[name]
    IC.check_against_record(IX.read(w.data, max_bit_depth=32), w)
    m = IX.read(w.data, max_bit_depth=24)
    IC.check_against_record(m, w, out_bytes=min(3, w.sample_bytes))
    assert m["out_bit_depth"] == min(w.depth, 24) and m["data_bytes"] == (w.frames_stated or w.frames) * w.channels * w.sample_bytes + \
        (1000 % 4 if name == "wav_data_longer_than_file" else 0)


@pytest.mark.parametrize("name", list(IC.named_malformed()))
def test_every_malformed_file_gets_its_status(name):
    data, status, at = IC.named_malformed()[name]
    m = IX.read(data)
    assert (m["status"], m["error_offset"]) == (status, at)
    assert all(m[k] == 0 for k in IC.FIELDS if k not in ("status", "error_offset")) and m["pcm"] == b""


def test_the_deviations_from_the_reference_show():
    good = IC.named_good()
    odd = IX.read(good["wav24_odd_data"].data)
    assert odd["data_bytes"] == 21 and odd["frames_total"] == 7                         # the stated size, not the padded one
    assert IX.read(good["aiff20"].data)["src_bit_depth"] == 24 and len(IX.read(good["aiff20"].data)["pcm"]) == 11 * 2 * 3
    assert IX.read(good["aiff32"].data)["status"] == IX.OK
    assert IX.read(good["aiff24_offset"].data)["data_offset"] == good["aiff24_offset"].marks[1][1] + 8 + 5
    assert IX.extended_rate(IC.ext80(96000)) == 96000 and IX.extended_rate(IC.ext80(0x100000)) == 0x100000     # exponents from 0x4013 up


def test_a_seek_a_short_room_and_the_unsigned_flag():
    w = IC.named_good()["wav32"]
    m = IX.read(w.data, frame_first=3, dst_frame_capacity=5, max_bit_depth=24)
    assert m["frames_written"] == 5 and m["pcm"] == w.pcm(3, first=3, frames=5)
    assert IX.read(w.data, frame_first=19)["frames_written"] == 0 and IX.read(w.data, frame_first=1 << 40)["pcm"] == b""
    assert IX.read(w.data, dst_bytes_capacity=6 * 4 + 5, max_bit_depth=24)["frames_written"] == 4
    w8 = IC.named_good()["wav8_mono"]
    plain, flipped = IX.read(w8.data)["pcm"], IX.read(w8.data, flags=IX.FLAG_WAV8_UNSIGNED)["pcm"]
    assert plain == w8.pcm() and flipped == bytes(b ^ 0x80 for b in plain)
    assert IX.read(IC.named_good()["aiff8"].data, flags=IX.FLAG_WAV8_UNSIGNED)["pcm"] == IC.named_good()["aiff8"].pcm()


def test_cuts_and_damage_cover_every_outcome():
    w = IC.named_good()["wav_junk_everywhere"]
    models = [IX.read(data, dst_frame_capacity=w.frames) for data in IC.cuts(w)]
    assert {m["status"] for m in models} == {IX.OK, IX.TRUNCATED, IX.NOT_IFF}
    assert any(m["status"] == IX.OK and 0 < m["frames_available"] < w.frames for m in models)
    assert {IX.read(data)["status"] for data in IC.damaged(2000)} == set(range(5))


def test_the_standard_librarys_wave_module_agrees():
    wave = pytest.importorskip("wave")
    for name in ("wav16", "wav8_mono", "wav24_odd_data", "wav32", "wav_fmt18", "wav_junk_everywhere", "wav_10ch"):        # (`wave` takes a file's last `fmt `: the file with two is left out)
        w = IC.named_good()[name]
        with wave.open(io.BytesIO(w.data), "rb") as f:
            m = IX.read(w.data, max_bit_depth=32)
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (m["channels"], m["src_bit_depth"] // 8, m["sample_rate"], m["frames_total"]), name
            little = np.frombuffer(f.readframes(f.getnframes()), dtype=np.uint8).reshape(-1, f.getsampwidth())
            assert little[:, ::-1].tobytes() == m["pcm"], name


def test_the_standard_librarys_aifc_module_agrees():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        aifc = pytest.importorskip("aifc")
    for name in ("aiff16", "aiff8", "aiff32",      # (`aifc` passes over SSND's offset field as the reference does: those files are left out)
                 "aiff_junk", "aifc_none", "aiff_ssnd_first"):
        w = IC.named_good()[name]
        f = aifc.open(io.BytesIO(w.data), "rb")
        m = IX.read(w.data, max_bit_depth=32)
        rate = {22255: 22050, 11127: 11025}.get(int(f.getframerate()), int(f.getframerate()))
        assert (f.getnchannels(), f.getsampwidth(), rate, f.getnframes()) == (m["channels"], m["src_bit_depth"] // 8, m["sample_rate"], m["frames_total"]), name
        assert f.readframes(f.getnframes()) == m["pcm"], name                           # (both big-endian: no change of byte order)
