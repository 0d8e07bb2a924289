"""The chained Ogg Vorbis files the links tests share, and what the models say of them.  A chain is a list of links, each a prefix of a
stream of tests/vorbis_cases.py wrapped in pages of its own serial: the identification header alone on a first page, comment and setup
on the next, the audio on pages of a few packets, granule positions that start where the link says (granule0; negative: the
specification's start trim) and a last page that may claim fewer samples than its packets deliver (trim).  expected() cuts a file at
its links with tests/ogg_links_textbook.py and decodes every link with tests/vorbis_textbook.py."""
import functools
import gzip
import hashlib
import json
import os

import numpy as np

import ogg_cases as OC
import ogg_links_textbook as LX
import ogg_textbook as OX
import vorbis_cases as VC
import vorbis_frames as VF
import vorbis_textbook as TB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vorbis")

#  name: [(stream of vorbis_cases, serial, audio packets, granule0, trim)]
CHAINS = {
    # the four held against Tremor (streams of VC.TREMOR_SHAPES)
    "chain_mono_stereo":   [("tremor_mono_64_128", 0x101, 7, 0, 0), ("tremor_stereo_1024_2048", 0x102, 6, 0, 0)],
    "chain_million":       [("tremor_mono_64_128", 0x201, 7, 0, 0), ("tremor_six_128_256", 0x202, 6, 1000000, 0)],
    "chain_trimmed":       [("tremor_six_128_256", 0x301, 7, 0, 37), ("tremor_mono_64_128", 0x302, 8, 0, 0)],
    "chain_negative_g0":   [("tremor_mono_64_128", 0x401, 6, 0, 0), ("tremor_mono_64_128", 0x402, 9, -20, 0)],
    # blocks of 128 / 512 behind 64 / 128, and the mixed pair: one channel in front of eight, three links
    "chain_six_128_512":   [("mono_64_128", 0x501, 7, 0, 0), ("six_128_512", 0x502, 6, 0, 0)],
    "chain_mono_eight":    [("mono_64_128", 0x601, 6, 0, 0), ("eight_64_256", 0x602, 6, 0, 5), ("mono_64_128", 0x603, 5, 500, 0)],
}
TREMOR_CHAINS = ("chain_mono_stereo", "chain_million", "chain_trimmed", "chain_negative_g0")
PACKETS_A_PAGE = 3


@functools.lru_cache(maxsize=None)
def link_decoded(name, n_audio):
    st = VC.stream(name)
    return TB.decode_stream(st.model, list(st.packets[:n_audio]))


def link_pages(name, serial, n_audio, granule0, trim, seq0=0):
    st = VC.stream(name)
    recs, _, _ = link_decoded(name, n_audio)
    granules = [granule0 + r[4] + r[3] for r in recs]
    granules[-1] -= trim
    pages = OC.mux([st.ident], serial, seq0, bos=True, eos=False, granules=[0])
    pages += OC.mux([VF.COMMENT, st.setup], serial, seq0 + len(pages), bos=False, eos=False, granules=[0, 0])
    audio = list(st.packets[:n_audio])
    for a in range(0, n_audio, PACKETS_A_PAGE):                          # a few packets a page, whatever their sizes
        part = audio[a:a + PACKETS_A_PAGE]
        pages += OC.mux(part, serial, seq0 + len(pages), granules=granules[a:a + PACKETS_A_PAGE], bos=False, eos=a + PACKETS_A_PAGE >= n_audio)
    return pages


@functools.lru_cache(maxsize=None)
def ogg(chain):
    return b"".join(b"".join(link_pages(*link)) for link in CHAINS[chain])


@functools.lru_cache(maxsize=None)
def links_of(data):
    """The file cut at its links by the Ogg model: [(serial, page_offset, first record, [packet dicts])], and the model's answer."""
    m = LX.demux(data, flags=OX.ANY_SERIAL | OX.ANY_SEQ | LX.FOLLOW_LINKS, magic=LX.VORBIS_MAGIC)
    cuts = [0] + [k for k, pk in enumerate(m["packets"]) if pk["flags"] & LX.PACKET_LINK] + [len(m["packets"])]
    out = []
    for a, b in zip(cuts, cuts[1:]):
        if a == b:
            continue
        at = m["packets"][a]["page_offset"]
        out.append((int.from_bytes(data[at + 14:at + 18], "little"), at, a, m["packets"][a:b]))
    return out, m


def decode_link(packets, max_samples=None):
    """A link's packets, its three headers first -> (Setup, records, pcm)"""
    datas = [pk["data"] for pk in packets]
    setup = TB.parse_headers(datas[0], datas[2])
    recs, _, pcm = TB.decode_stream(setup, datas, max_samples)
    return setup, recs, pcm


def played(chain):
    """What a player puts out of every link by the granule positions (the host element's rule, and the reference's): per link (channels,
    rate, pcm) with the end trim and the start trim applied.  g0 = the first granule-bearing audio page's granule minus what the
    packets up to its last deliver; the last page keeps granule - g0 samples; a negative g0 drops -g0 samples as Tremor does (below)."""
    out = []
    links, _ = links_of(ogg(chain))
    for (_, _, _, packets), (name, _, n_audio, granule0, trim) in zip(links, CHAINS[chain]):
        setup, recs, pcm = decode_link(packets)
        done = np.cumsum([r[3] for r in recs])
        k = next(k for k, pk in enumerate(packets) if k >= 3 and pk["granule"] != -1)
        g0 = packets[k]["granule"] - int(done[k])
        assert g0 == granule0
        keep = min(packets[-1]["granule"] - g0, pcm.shape[1])
        assert keep == pcm.shape[1] - trim
        # a negative g0 (fewer samples claimed by the first page than its packets deliver): Tremor's vorbis_synthesis_blockin learns it
        # at the packet that carries the granule, when the packets before it have been read already, and drops the excess from the
        # front of THAT packet's output, no more than it has (tests/test_chained_tremor.py decides this)
        start = int(done[k - 1])
        drop = min(max(0, -g0), recs[k][3])
        out.append((setup.channels, setup.rate, np.concatenate([pcm[:, :start], pcm[:, start + drop:keep]], axis=1)))
    return out


def golden_table():
    with open(os.path.join(GOLDEN, "chains.json")) as f:
        return json.load(f)


def golden(chain):
    with gzip.open(os.path.join(GOLDEN, chain + ".ogg.gz"), "rb") as f:
        return f.read()


def table_entry(chain):
    links, m = links_of(ogg(chain))
    rows = []
    for serial, at, first, packets in links:
        setup, recs, pcm = decode_link(packets)
        rows.append(dict(serial=serial, page_offset=at, first_packet=first, packets=len(packets), channels=setup.channels, rate=setup.rate,
                         blocks=list(setup.bs), samples=int(pcm.shape[1]), pcm_md5=hashlib.md5(VC.pcm_s16be(pcm)).hexdigest()))
    return dict(bytes=len(ogg(chain)), links=rows)
