"""The fused call, from an Ogg file to PCM (ohgpu_ogg_vorbis_process_host): the Ogg batch into a middle arena that stays on the device,
one small read of its packet records, the Vorbis batch over those rows.  The files are tests/vorbis_cases.ogg's (what tests/golden/vorbis
pins).  Fed from the first page, a stream's three header packets are passed over and the rest is the model's; fed from where
ohgpu_vorbis_head says the audio begins, the same; and a file taken in two calls -- the second beginning at the last packet the first
consumed, by that packet's own record -- writes what one call writes."""
import numpy as np
import pytest

import vorbis_cases as VC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu
NAMES = ["stereo_256_2048", "six_128_512", "encoder_256", "mono_8192"]
ROUTES = [pytest.param(0, id="fft"), pytest.param(1, id="plain")]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.set_kernel_variant(0)
    c.close()


def tables(names, starts):
    """Descriptors for the files one after the other; starts[i] = (page_offset, segment, seq) or None for the file's first byte."""
    n = len(names)
    ogg, vor = np.zeros(n, dtype=capi.OGG_STREAM_DESC), np.zeros(n, dtype=capi.VORBIS_STREAM_DESC)
    src, images, at_mid, at_dst, at_pkt = bytearray(), [], 0, 0, 0
    for i, name in enumerate(names):
        data = VC.ogg(name)
        head = capi.vorbis_head(data)
        start = starts[i] or (0, 0, 0)
        o, v = ogg[i], vor[i]
        o["src_offset"], o["src_bytes"] = len(src) + start[0], len(data) - start[0]
        o["first_page_segment"], o["expect_seq"], o["serial"] = start[1], start[2], head["serial"]
        o["dst_offset"], o["dst_capacity"] = at_mid, len(data)
        o["packet_first"], o["packet_capacity"] = at_pkt, len(VC.stream(name).packets) + 3
        ch, cap = int(head["info"]["channels"]), VC.expected(name)[2].shape[1]
        v["image_offset"], v["image_bytes"] = sum(im.size for im in images), head["image"].size
        v["dst_offset"], v["max_samples"] = at_dst, cap
        images.append(head["image"])
        src += data
        at_mid += (len(data) + 15) & ~15
        at_dst += (cap * ch * 2 + 3) & ~3
        at_pkt += int(o["packet_capacity"])
    return ogg, vor, np.concatenate(images), np.frombuffer(bytes(src) + bytes(4), dtype=np.uint8).copy(), at_mid, at_dst, at_pkt


@pytest.mark.parametrize("variant", ROUTES)
@pytest.mark.parametrize("from_head", [False, True], ids=["first_page", "audio_page"])
def test_ogg_files_to_pcm(ctx, from_head, variant):
    starts = []
    for name in NAMES:
        head = capi.vorbis_head(VC.ogg(name))
        starts.append((head["page_offset"], head["segment"], head["seq"]) if from_head else None)
    ogg, vor, images, src, mid_bytes, dst_bytes, n_packets = tables(NAMES, starts)
    dst = np.full(dst_bytes, 0x5A, dtype=np.uint8)
    ctx.set_kernel_variant(variant)
    try:
        ores, orecs, sres, pres = ctx.ogg_vorbis_process_host(ogg, vor, n_packets, images, src, mid_bytes, dst)
    finally:
        ctx.set_kernel_variant(0)
    for i, name in enumerate(NAMES):
        recs, _, pcm = VC.expected(name)
        lead = 0 if from_head else 3
        first = int(ogg["packet_first"][i])
        assert int(ores["status"][i]) == 0 and int(ores["packets"][i]) == len(recs) + lead and int(ores["eos_seen"][i]) == 1
        assert int(ores["last_granule"][i]) == pcm.shape[1]                                # (the fixture's granules are the model's sample counts)
        assert (pres["status"][first:first + lead] == capi.VORBIS_HEADER).all()
        got = [(int(r["status"]), int(r["mode"]), int(r["blocksize"]), int(r["samples"]), int(r["position"])) for r in pres[first + lead:first + lead + len(recs)]]
        assert got == [tuple(int(v) for v in r) for r in recs]
        assert int(sres["samples"][i]) == pcm.shape[1] and int(sres["packets_ok"][i]) == (len(recs) if from_head else 0)
        ch, at = pcm.shape[0], int(vor["dst_offset"][i])
        mine = dst[at:at + pcm.shape[1] * ch * 2].view(">i2").astype(np.int32).reshape(-1, ch).T
        assert int(np.abs(mine - pcm).max()) <= 1, name


def test_a_file_in_two_calls_resumes_at_the_last_packet_consumed(ctx):
    name = "stereo_256_2048"
    data, pcm = VC.ogg(name), VC.expected(name)[2]
    ogg, vor, images, src, mid_bytes, dst_bytes, n_packets = tables([name], [None])
    whole = np.zeros(dst_bytes, dtype=np.uint8)
    _, orecs, sres, _ = ctx.ogg_vorbis_process_host(ogg, vor, n_packets, images, src, mid_bytes, whole)
    # the first call gets the file up to a page boundary near its middle; the second begins at the record of the last packet the first consumed
    cut = data.index(b"OggS", len(data) // 2)
    o1 = ogg.copy()
    o1["src_bytes"] = cut
    part1 = np.zeros(dst_bytes, dtype=np.uint8)
    r1, recs1, s1, _ = ctx.ogg_vorbis_process_host(o1, vor, n_packets, images, src, mid_bytes, part1)
    last = recs1[int(r1["packets"][0]) - 1]
    o2 = ogg.copy()
    o2["src_offset"], o2["src_bytes"] = int(last["page_offset"]), len(data) - int(last["page_offset"])
    o2["first_page_segment"], o2["expect_seq"] = int(last["segment"]), int(last["page_seq"])
    part2 = np.zeros(dst_bytes, dtype=np.uint8)
    _, _, s2, _ = ctx.ogg_vorbis_process_host(o2, vor, n_packets, images, src, mid_bytes, part2)
    a, b = int(s1["samples"][0]), int(s2["samples"][0])
    assert a > 0 and b > 0 and a + b == pcm.shape[1] == int(sres["samples"][0])
    assert np.array_equal(np.concatenate([part1[:a * 4], part2[:b * 4]]), whole[:(a + b) * 4])
