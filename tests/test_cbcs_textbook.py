"""The model of the second protected MPEG-4 family (tests/cbcs_textbook.py) held to two things it shares no text with: openssl's CBC
(tests/golden/cbcs/*.json, made by tests/golden/make_cbcs_fixtures.py with `openssl enc -aes-128-cbc -nopad`) for its inverse cipher, its
8-byte IV and its pattern rule; and the muxer's own record of the clear samples (tests/cbcs_cases.py, whose encryptor uses another
file's forward cipher) for everything it reads from the boxes.  And the named malformed files: the model's status and error_offset."""
import json
import os

import pytest

import cbcs_cases as BC
import cbcs_textbook as BX

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cbcs")


def fixture(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_sp800_38a_f2():
    f = fixture("sp800_38a_f2.json")
    assert f["cipher"].startswith("7649abac8119b246cee98e9b12e9197d")       # (F.2.1's first cipher block, as openssl gave it)
    clear, blocks = BX.cbcs_part(bytes.fromhex(f["key"]), bytes.fromhex(f["iv"]), bytes.fromhex(f["cipher"]), 0, 0)
    assert clear.hex() == f["plain"] and blocks == 4


def test_chains_of_1_to_65_blocks_under_three_keys_and_the_8_byte_iv():
    chains = fixture("chains.json")
    assert sorted({len(c["plain"]) // 32 for c in chains}) == [1, 2, 5, 63, 64, 65] and len({c["key"] for c in chains}) == 3 and {len(c["iv"]) for c in chains} == {16, 32}
    for c in chains:
        clear, blocks = BX.cbcs_part(bytes.fromhex(c["key"]), bytes.fromhex(c["iv"]), bytes.fromhex(c["cipher"]), 0, 0)
        assert clear.hex() == c["plain"] and blocks == len(c["plain"]) // 32


def test_the_pattern_rule():
    patterns = fixture("patterns.json")
    assert {(p["crypt"], p["skip"]) for p in patterns} == set(BC.PATTERNS)
    for p in patterns:
        cipher = bytes.fromhex(p["cipher"])
        clear, blocks = BX.cbcs_part(bytes.fromhex(p["key"]), bytes.fromhex(p["iv"]), cipher, p["crypt"], p["skip"])
        assert clear.hex() == p["plain"], p
        assert blocks == len(BX.encrypted_blocks(len(cipher) // 16, p["crypt"], p["skip"]))
        assert clear[len(cipher) // 16 * 16:] == cipher[len(cipher) // 16 * 16:]                          # the tail is copied
    assert any(p["crypt"] == 1 and p["skip"] == 9 and len(p["cipher"]) // 32 == 21 for p in patterns)     # 2 (crypt + skip) + 1: three encrypted blocks, two gaps


def test_the_clear_bytes_of_every_named_good_file_are_the_muxers_record():
    for name, m in BC.named_good().items():
        for first in (0, 1):
            if first < m.n:
                model = BX.demux(m.data, 3, m.n, len(m.runs), first, len(m.data), kid=m.kid, key=m.key, subsample_capacity=m.subsamples)
                BC.check_against_record(model, m, first)
                assert model["subsamples"] == m.subsamples and model["scheme"] == (BX.code(m.scheme) if model["entry"] == BX.code(b"enca") else 0), name


def test_the_cenc_block_count_is_the_siblings_for_whole_samples():
    import cenc_textbook as CX
    for name in ("sibling_flac_iv8", "sibling_alac_iv16", "sibling_wrap_inside_three_blocks"):
        m = BC.named_good()[name]
        mine = BX.demux(m.data, 3, m.n, len(m.runs), 0, len(m.data), kid=m.kid, key=m.key)
        theirs = CX.demux(m.data, 3, m.n, len(m.runs), 0, len(m.data), kid=m.kid, key=m.key)
        assert mine["blocks"] == theirs["blocks"] and mine["gathered"] == theirs["gathered"] and mine["clear_rows"] == theirs["clear_rows"]


def test_every_named_malformed_file():
    for name, (data, status, at, codecs, have_key, kid) in BC.named_malformed().items():
        model = BX.demux(data, codecs, 8, 4, 0, len(data), kid=kid, key=BC.KEY if have_key else None, subsample_capacity=40)
        assert (model["status"], model["error_offset"]) == (status, at), name


@pytest.mark.parametrize("capacity,rows,kept", [(23, 5, 23), (22, 4, 6), (6, 4, 6), (5, 3, 3), (0, 1, 0)])
def test_the_subsample_capacity_ends_the_rows_served(capacity, rows, kept):
    m = BC.named_good()["cbcs_counts_0_1_2_3_17"]
    model = BX.demux(m.data, 3, m.n, len(m.runs), 0, len(m.data), kid=m.kid, key=m.key, subsample_capacity=capacity)
    assert (model["samples_available"], model["subsamples"], model["samples"], len(model["clear_rows"])) == (rows, kept, 5, rows)
    assert model["gathered"] == b"".join(m.clear[:rows])
