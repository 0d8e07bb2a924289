"""The plain-Python Apple Lossless model (tests/alac_textbook.py) against what does not depend on it: the PCM the reference's own
encoder was given (losslessness: the model's output is that PCM, byte for byte and by SHA-256), hand-written answers for two packets
of eight samples, and a census -- every feature the format text names occurs in the committed fixtures, encoder-made or handmade.
tests/golden/alac_textbook.json pins the model's output on the handmade packets, so that the model cannot drift unnoticed."""
import json
import os

import pytest

import alac_cases as AC
import alac_textbook as T

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alac_textbook.json")


@pytest.mark.parametrize("name", list(AC.FIXTURES))
def test_model_reproduces_the_encoded_pcm(name):
    fx = AC.load_fixture(name)
    meta, cfg = fx["meta"], fx["cfg"]
    assert (cfg["frame_length"], cfg["bit_depth"], cfg["channels"], cfg["sample_rate"]) == (meta["frame_length"], meta["bits"], meta["channels"], meta["rate"])
    assert AC.sha256(fx["pcm"]) == meta["pcm_sha256"]                  # the regenerated PCM is the PCM that was encoded
    assert len(fx["packets"]) == -(-meta["frames"] // meta["frame_length"])
    out = bytearray()
    for k, packet in enumerate(fx["packets"]):
        status, n, chans = AC.decode_cached(cfg, packet)
        assert status == T.OK
        assert n == min(meta["frame_length"], meta["frames"] - k * meta["frame_length"])
        out += T.pack(cfg, chans, n, T.PACKED_LE)
    assert bytes(out) == fx["pcm"] and AC.sha256(bytes(out)) == meta["pcm_sha256"]
    assert len(fx["packets"][0]) + len(fx["packets"][1]) > 0 and os.path.getsize(os.path.join(AC.GOLDEN, name + ".bin")) <= 64 * 1024


def test_hand_written_answers():
    hand = AC.handmade()
    cookie, (packet,) = hand["hand_mono8"]
    assert T.decode_packet(T.parse_config(cookie), packet) == (T.OK, 8, AC.HAND_MONO8["expect"])
    cookie, (packet,) = hand["hand_stereo8"]
    assert T.decode_packet(T.parse_config(cookie), packet) == (T.OK, 8, AC.HAND_STEREO8["expect"])


CENSUS = ("SCE", "CPE", "LFE", "escape", "partial", "shift_0", "shift_1", "shift_2", "mix_0", "mix", "zero_run", "run_escape", "long_escape",
          "order_0", "order_4", "order_8", "order_31", "order_other", "mode", "factor_not_4", "FIL", "DSE", "DSE_aligned", "early_END",
          "CPE_beyond_channels", "escape_with_shift")
ENCODER_MADE = ("SCE", "CPE", "escape", "partial", "shift_0", "shift_1", "shift_2", "mix_0", "mix", "zero_run", "long_escape", "order_4", "order_8")


def test_census_of_the_committed_fixtures():
    made, hand = set(), set()
    for fx in AC.fixtures():
        for packet in fx["packets"]:
            T.decode_packet(fx["cfg"], packet, made)
    for cookie, packets in AC.handmade().values():
        for packet in packets:
            assert T.decode_packet(T.parse_config(cookie), packet, hand)[0] == T.OK
    missing = [item for item in CENSUS if item not in made | hand]
    assert not missing, missing
    assert not [item for item in ENCODER_MADE if item not in made]          # what the reference's own encoder showed
    total = sum(os.path.getsize(os.path.join(AC.GOLDEN, f)) for f in os.listdir(AC.GOLDEN))
    assert total <= 400 * 1024


def test_malformed_packets_have_the_statuses_they_are_named_for():
    for name, (cookie, packet, status) in AC.malformed().items():
        assert T.decode_packet(T.parse_config(cookie), packet) == (status, 0, []), name


def test_config_parse_with_and_without_the_atoms():
    import alac_frames as F
    plain = F.cookie(4096, 24, 2, sample_rate=96000, pb=40, mb=10, kb=14)
    want = dict(frame_length=4096, bit_depth=24, pb=40, mb=10, kb=14, channels=2, max_run=255, max_frame_bytes=0, avg_bit_rate=0, sample_rate=96000)
    for frma in (False, True):
        for alac in (False, True):
            assert T.parse_config(F.wrapped(plain, frma, alac)) == want
    with pytest.raises(ValueError):
        T.parse_config(plain[:23])
    with pytest.raises(ValueError):
        T.parse_config(F.cookie(4096, 16, 2, version=1))


def pins_now():
    out = {}
    for name, (cookie, packets) in AC.handmade().items():
        cfg = T.parse_config(cookie)
        rows = []
        for packet in packets:
            status, n, chans = T.decode_packet(cfg, packet)
            rows.append(dict(packet=packet.hex(), status=status, samples=n, sha256=AC.sha256(T.pack(cfg, chans, n, T.PACKED_LE)), first=[c[:4] for c in chans]))
        out[name] = dict(cookie=cookie.hex(), packets=rows)
    return out


def test_pinned_output_on_the_handmade_packets():
    with open(PINS) as f:
        assert json.load(f) == pins_now()
