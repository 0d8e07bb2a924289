"""The fused call for chained streams, from Ogg bytes to PCM (ohgpu_ogg_vorbis_links_process_host): the Ogg batch with
OHGPU_OGG_FOLLOW_LINKS, one small read, the packet records cut at their links on the host, a head parsed and an image made per new
link, ONE Vorbis batch over every link of every stream.  The files are the committed chains of tests/golden/vorbis (blocks of 64 / 128
in front of 128 / 512, of 1024 / 2048, one channel in front of six and of eight; about six audio packets a link).  Under both routes
the link rows must be the models' and every link's PCM within 1 LSB of tests/vorbis_textbook.py's -- DESIGN.md 5.23's bound, derived
there for a stream, and a link is a stream: by V3 its first packet primes, nothing overlaps across links."""
import numpy as np
import pytest

import chained_cases as KC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu
ROUTES = [pytest.param(0, id="fft"), pytest.param(1, id="plain")]
BIG = 1 << 30


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.set_kernel_variant(0)
    c.close()


class Tables:
    """Descriptors for files laid one after the other, each fed from its first byte with its first link's image; capacities[i]: the
    bytes of stream i's region (None: room for every link); planar[i]: OHGPU_VORBIS_OUT_PLANAR32."""

    def __init__(self, files, capacities=None, planar=None):
        n = len(files)
        self.files = files
        self.ogg, self.vor = np.zeros(n, dtype=capi.OGG_STREAM_DESC), np.zeros(n, dtype=capi.VORBIS_STREAM_DESC)
        self.caps = np.zeros(n, dtype="<u8")
        self.want = []                                    # per stream: [(row dict, bound, pcm)]
        src, images, at_mid, at_dst, at_pkt = bytearray(), [], 0, 0, 0
        for i, data in enumerate(files):
            links, m = KC.links_of(data)
            head = capi.vorbis_head(data[:links[1][1]] if len(links) > 1 else data)
            planes = bool(planar and planar[i])
            o, v = self.ogg[i], self.vor[i]
            o["src_offset"], o["src_bytes"], o["serial"] = len(src), len(data), head["serial"]
            o["dst_offset"], o["dst_capacity"] = at_mid, len(data)
            o["packet_first"], o["packet_capacity"] = at_pkt, len(m["packets"]) + 2
            v["image_offset"], v["image_bytes"] = sum(im.size for im in images), head["image"].size
            v["dst_offset"], v["max_samples"], v["flags"] = at_dst, BIG, capi.VORBIS_OUT_PLANAR32 if planes else 0
            images.append(head["image"])
            decoded = [KC.decode_link(packets) for _, _, _, packets in links]
            sized = [len(packets) * setup.bs[1] // 2 for (_, _, _, packets), (setup, _, _) in zip(links, decoded)]
            frames = [setup.channels * (4 if planes else 2) for setup, _, _ in decoded]
            room = sum((s * f + 3) & ~3 for s, f in zip(sized, frames)) if not capacities or capacities[i] is None else capacities[i]
            self.caps[i] = room
            cursor, full, rows = at_dst, False, []
            for j, ((serial, at, first, packets), (setup, _, _)) in enumerate(zip(links, decoded)):
                left = 0 if full or cursor >= at_dst + room else (at_dst + room - cursor) // frames[j]
                bound = min(sized[j], left)
                full = full or bound < sized[j]
                _, _, pcm = KC.decode_link(packets, max_samples=bound)
                rows.append((dict(stream=i, serial=serial, page_offset=capi.VORBIS_LINK_CONTINUED if j == 0 else at, first_packet=at_pkt + first, n_packets=len(packets),
                                  head=0, channels=setup.channels, sample_rate=setup.rate, blocksize_short=setup.bs[0], blocksize_long=setup.bs[1], reserved=0,
                                  dst_offset=cursor, samples=pcm.shape[1]), bound, pcm))
                cursor += (bound * frames[j] + 3) & ~3
            self.want.append(rows)
            src += data
            at_mid += (len(data) + 15) & ~15
            at_dst += (room + 3) & ~3
            at_pkt += int(o["packet_capacity"])
        self.images, self.src = np.concatenate(images), np.frombuffer(bytes(src) + bytes(4), dtype=np.uint8).copy()
        self.mid_bytes, self.dst_bytes, self.n_packets = at_mid, at_dst, at_pkt

    def run(self, ctx, variant=0):
        dst = np.full(self.dst_bytes, 0x5A, dtype=np.uint8)
        ctx.set_kernel_variant(variant)
        try:
            ores, orecs, links, pres = ctx.ogg_vorbis_links_process_host(self.ogg, self.vor, self.caps, self.n_packets, self.images, self.src, self.mid_bytes, dst)
        finally:
            ctx.set_kernel_variant(0)
        return ores, orecs, links, pres, dst

    def check(self, links, dst):
        want = [row for rows in self.want for row in rows]
        assert len(links) == len(want)
        worst = 0
        for got, (row, bound, pcm) in zip(links, want):
            assert {f: int(got[f]) for f in row} == row
            ch, at, n = pcm.shape[0], row["dst_offset"], pcm.shape[1]
            if int(self.vor["flags"][row["stream"]]) & capi.VORBIS_OUT_PLANAR32:
                mine = np.stack([dst[at + c * bound * 4:at + c * bound * 4 + n * 4].view("<i4") for c in range(ch)]).astype(np.int64)
            else:
                mine = dst[at:at + n * ch * 2].view(">i2").astype(np.int64).reshape(-1, ch).T
            if n:
                worst = max(worst, int(np.abs(mine - pcm).max()))
        return worst


@pytest.mark.parametrize("variant", ROUTES)
def test_the_committed_chains_to_pcm(ctx, variant):
    """All six in one batch: 14 links of 1, 2, 6 and 8 channels and five block-size pairs behind one Vorbis batch."""
    chains = sorted(KC.CHAINS)
    t = Tables([KC.golden(c) for c in chains])
    table = KC.golden_table()
    for c, rows in zip(chains, t.want):                                  # the models here are the committed ones
        assert [(r["serial"], r["n_packets"], r["samples"]) for r, _, _ in rows] == [(x["serial"], x["packets"], x["samples"]) for x in table[c]["links"]]
    ores, orecs, links, pres, dst = t.run(ctx, variant)
    assert [int(r["status"]) for r in ores] == [0] * len(chains) and [int(x) for x in ores.view(capi.OGG_STREAM_RESULT_LINKS)["links"]] == [len(KC.CHAINS[c]) - 1 for c in chains]
    worst = t.check(links, dst)
    print("worst difference to the model, LSB:", worst)
    assert worst <= 1
    for rows in t.want:                                                  # a link's headers are passed over, its first audio packet primes
        for row, _, _ in rows:
            k = row["first_packet"]
            assert (pres["status"][k:k + 3] == capi.VORBIS_HEADER).all() and int(pres["samples"][k + 3]) == 0 and int(pres["status"][k + 3]) == capi.VORBIS_OK


@pytest.mark.parametrize("variant", ROUTES)
def test_a_mono_link_and_an_eight_channel_link_in_one_batch(ctx, variant):
    """The mixed-image case, alone and in both output forms: blocks of 64 / 128 and of 64 / 256, one channel and eight."""
    data = KC.golden("chain_mono_eight")
    t = Tables([data, data], planar=[False, True])
    assert [[r["channels"] for r, _, _ in rows] for rows in t.want] == [[1, 8, 1]] * 2
    _, _, links, _, dst = t.run(ctx, variant)
    assert t.check(links, dst) <= 1


def test_a_range_that_ends_inside_a_links_setup_packet(ctx):
    data = KC.golden("chain_six_128_512")
    (_, _, _, first), (_, at, _, second) = KC.links_of(data)[0]
    setup_page = at + 58                                                 # the link's first page: 27 + 1 + 30 bytes
    cut = data[:setup_page + 200]
    assert len(second[2]["data"]) > 400 and KC.links_of(cut)[1]["status"] == 0
    t = Tables([data])
    t.ogg["src_bytes"][0] = len(cut)
    t.src[len(cut):] = 0xEE
    ores, orecs, links, pres, dst = t.run(ctx)
    assert len(links) == 2 and int(ores["packets"][0]) == len(first) + 1 and int(ores["bytes_consumed"][0]) == setup_page
    row, bound, pcm = t.want[0][0]
    assert {f: int(links[0][f]) for f in row} == row
    assert (int(links[1]["head"]), int(links[1]["page_offset"]), int(links[1]["n_packets"]), int(links[1]["samples"]), int(links[1]["serial"])) == \
        (capi.VORBIS_LINK_HEAD_OPEN, at, 1, 0, 0x502)
    mine = dst[:pcm.shape[1] * 2].view(">i2").astype(np.int64)
    assert int(np.abs(mine - pcm[0]).max()) <= 1 and (dst[int(links[1]["dst_offset"]):] == 0x5A).all()


def test_a_destination_too_small_for_the_second_link(ctx):
    """chain_mono_eight's region holds the first link and 100 frames and 7 bytes more: the second link gets 100 samples, the third none."""
    data = KC.golden("chain_mono_eight")
    first_link = 9 * 64 * 2
    t = Tables([data, KC.golden("chain_negative_g0")], capacities=[first_link + 100 * 16 + 7, None])
    assert [bound for _, bound, _ in t.want[0]] == [9 * 64, 100, 0] and [r["samples"] for r, _, _ in t.want[0]] == [240, 100, 0]
    _, _, links, _, dst = t.run(ctx)
    assert t.check(links, dst) <= 1
    end = first_link + 100 * 16
    assert (dst[end:int(t.vor["dst_offset"][1])] == 0x5A).all()         # nothing behind what the second link was given


def test_fewer_rows_than_links(ctx):
    t = Tables([KC.golden("chain_mono_eight")])
    ores, orecs, (links, count), pres = ctx.ogg_vorbis_links_process_host(t.ogg, t.vor, t.caps, t.n_packets, t.images, t.src, t.mid_bytes,
                                                                          np.zeros(t.dst_bytes, dtype=np.uint8), links_capacity=2)
    assert count == 3 and [int(x) for x in links["serial"]] == [0x601, 0x602]
