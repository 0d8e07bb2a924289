"""The model of the protected MPEG-4 layer (tests/cenc_textbook.py) held to what is not the model: its keystream to the golden files
(tests/golden/cenc: openssl's counter mode where the counter does not wrap, single-block ECB calls for the three blocks of the wrapping
case, SP 800-38A F.5.1), its reading of every good file to the muxer's own record of the clear samples, its reading of a clear stream to
tests/mp4f_textbook.py's gather; and a census: the committed cases hold every rule of include/ohgpu_cenc.h."""
import json
import os

import cenc_cases as CC
import cenc_textbook as CX
import mp4f_cases as FC
import mp4f_textbook as FX

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cenc")


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_keystreams_that_do_not_wrap_are_the_librarys():
    triples = golden("keystreams.json")["triples"]
    assert len(triples) >= 20 and {len(t["iv"]) // 2 for t in triples} == {8, 16} and {0, 1, 15, 16, 17, 2049} <= {t["length"] for t in triples}
    for t in triples:
        assert CX.keystream(bytes.fromhex(t["key"]), bytes.fromhex(t["iv"]), t["length"]).hex() == t["keystream"], t


def test_the_low_half_wraps_and_carries_nowhere():
    g = golden("wrap.json")
    key, iv = bytes.fromhex(g["key"]), bytes.fromhex(g["iv"])
    assert [CX.counter_block(iv, j).hex() for j in range(3)] == [b["counter"] for b in g["blocks"]]
    assert CX.keystream(key, iv, 48).hex() == "".join(b["block"] for b in g["blocks"])
    assert g["blocks"][2]["block"] == "720f9ee37b13a7c8b98e955d56b0f313"          # (a 128-bit increment gives 2a8891d2...)
    assert CX.crypt(key, iv, CX.crypt(key, iv, bytes(range(41)))) == bytes(range(41))


def test_sp800_38a_f51():
    g = golden("sp800_38a_f51.json")
    assert g["ciphertext"].startswith("874d6191b620e3261bef6864990db6ce")
    assert CX.crypt(bytes.fromhex(g["key"]), bytes.fromhex(g["iv"]), bytes.fromhex(g["plaintext"])).hex() == g["ciphertext"]


def test_every_good_file_reads_as_the_muxer_wrote_it():
    for name, m in CC.named_good().items():
        model = CX.demux(m.data, kid=m.kid, key=m.key, dst_capacity=len(m.data))
        FC.check_against_record(model, m)
        assert model["gathered"] == b"".join(m.clear), name
        assert model["clear_rows"] == [(sum(m.sizes[:k]), m.sizes[k]) for k in range(m.n)] or not m.n, name
        assert model["is_protected"] == (1 if m.protected else 0) and model["blocks"] == (sum((s + 15) // 16 for s in m.sizes) if m.protected else 0), name
        if m.protected:
            assert model["kid"] == m.kid and model["scheme"] == CX.code(b"cenc") and model["entry"] == CX.code(b"enca") and model["iv_size"] == len(m.ivs[0]) if m.ivs else True
            assert model["gathered"] != b"".join(m.data[o:o + s] for o, s in zip(m.offsets, m.sizes)) or not sum(m.sizes), name


def test_a_clear_stream_reads_as_the_sibling_reads_it():
    for name, m in FC.named_good().items():
        for first in (0, 2):
            mine = CX.demux(m.data, gather_first_row=first, dst_capacity=len(m.data))
            theirs = FX.demux(m.data, gather=True, gather_first_row=first, dst_capacity=len(m.data))
            for k in theirs:
                assert mine[k] == theirs[k], (name, k)
            assert (mine["entry"], mine["scheme"], mine["is_protected"], mine["blocks"]) == (theirs["codec"], 0, 0, 0)
    for name, (data, status, at, codecs) in FC.named_malformed().items():
        if name == "enca":                                                      # (an entry with no sinf: the sibling's UNSUPPORTED is INVALID here)
            assert (CX.demux(data, codecs)["status"], CX.demux(data, codecs)["error_offset"]) == (CX.INVALID, at)
            continue
        mine, theirs = CX.demux(data, codecs), FX.demux(data, codecs, gather=True)
        assert all(mine[k] == theirs[k] for k in theirs), name


def test_every_named_malformed_file():
    for name, (data, status, at, codecs, have_key, kid) in CC.named_malformed().items():
        model = CX.demux(data, codecs, kid=kid, key=CC.KEY if have_key else None, dst_capacity=len(data))
        assert (model["status"], model["error_offset"]) == (status, at), name
        if status == CX.NO_KEY:
            assert model["codec"] == CX.code(b"fLaC") and model["kid"] == CC.KID and model["iv_size"] == 8 and model["scheme"] == CX.code(b"cenc")
            assert model["samples"] == model["runs"] == model["frames"] == model["bytes_gathered"] == 0 and model["rows"] == [] and model["flac"]["sample_rate"] == 44100


def test_census_the_cases_hold_every_rule():
    good, bad = CC.named_good(), CC.named_malformed()
    status = {name: (s, at) for name, (_, s, at, _, _, _) in bad.items()}
    X = CX
    # the sample entry
    assert all(status[f"sinf_without_{k}"][0] == X.INVALID for k in ("frma", "schm", "schi", "tenc")) and status["enca_without_sinf"][0] == X.INVALID
    assert all(status[f"scheme_{k}"][0] == X.UNSUPPORTED for k in ("cbcs", "cbc1", "cens"))
    assert status["frma_of_3_bytes"][0] == status["schm_of_11_bytes"][0] == status["enca_entry_of_27_bytes"][0] == X.INVALID
    assert status["entry_of_too_many_boxes"][0] == X.INVALID and status["entry_of_many_boxes"][0] == X.OK and status["child_of_sinf_past_its_parent"][0] == X.INVALID
    assert {"sinf_behind_the_codec_box", "unknown_boxes_in_the_entry", "clear_plain_flac", "clear_plain_alac"} <= set(good)
    assert status["enca_mp4a"][0] == status["enca_alac_asked_flac"][0] == X.NOT_CODEC
    assert status["enca_flac_without_dfla"][0] == status["enca_alac_without_the_inner_box"][0] == X.UNSUPPORTED
    # tenc
    assert status["tenc_of_23_bytes"][0] == X.INVALID and status["tenc_version_1"][0] == X.UNSUPPORTED and status["is_protected_2"][0] == X.INVALID
    assert all(status[f"iv_size_{k}"][0] == X.UNSUPPORTED for k in (0, 4, 12, 32))
    assert {"enca_not_protected", "enca_not_protected_iv_size_ignored"} <= set(good)
    assert {len(m.ivs[0]) for m in good.values() if m.protected and m.ivs} == {8, 16}
    assert {m.codec for m in good.values() if m.protected} == {CC.FLAC, CC.ALAC}
    # senc
    for name in ("senc_in_front_of_the_truns", "senc_behind_the_truns", "two_truns_under_one_senc_front", "two_truns_under_one_senc_behind", "second_senc_skipped",
                 "saiz_and_saio_skipped", "clear_with_a_senc_skipped", "protected_traf_without_samples"):
        assert name in good
    front, behind = good["senc_in_front_of_the_truns"], good["senc_behind_the_truns"]
    assert front.find("senc")[0] < front.find("trun")[0] and behind.find("senc")[0] > behind.find("trun")[0]
    two = good["two_truns_under_one_senc_behind"]
    assert len([x for x in two.marks if x[0].endswith("/trun")]) == 2 * len([x for x in two.marks if x[0].endswith("/senc")])
    assert status["senc_version_1"][0] == status["senc_overridden_parameters"][0] == status["senc_subsamples"][0] == X.UNSUPPORTED
    assert status["senc_entries_leave_the_box"][0] == status["senc_count_leaves_the_box"][0] == status["senc_count_below_the_truns"][0] == status["senc_of_4_bytes"][0] == X.INVALID
    assert status["protected_traf_without_senc"][0] == status["sbgp_seig"][0] == status["sgpd_seig"][0] == X.UNSUPPORTED
    # the key
    assert status["no_key"][0] == status["key_of_another_kid"][0] == X.NO_KEY
    # the keystream
    assert good["wrap_inside_three_blocks"].ivs[0] == CC.WRAP_IV and len(good["wrap_inside_three_blocks"].clear[0]) == 48
    assert good["sizes_0_1_15_16_17_33"].sizes == [0, 1, 15, 16, 17, 33]
    assert [(s + 15) // 16 for s in good["piece_edges"].sizes] == [63, 64, 65, 128, 129]
