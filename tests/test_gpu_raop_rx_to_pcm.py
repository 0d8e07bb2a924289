"""Datagrams to PCM through the fused call (ohgpu_raop_rx_alac_process_host): the Apple Lossless sessions of
tests/golden/raop_textbook.json, their packets sent as RAOP datagrams that a fixed seed shuffles, thins and doubles, the missing ones
answered with 0x56-wrapped resends, fed in several ticks the way a caller does it -- the PENDING datagrams of a tick queued by `order`
in front of the next, state_out as state_in, the destination moved on by what came out.  Once every resend has arrived the PCM is the
PCM the fixtures were encoded from, with nothing missing.  The receiver's own answers are held to the model tick by tick.  Then the
plaintext form, and a wrong key between two good streams.  Both routes."""
import numpy as np
import pytest

import alac_textbook as T
import raop_cases as AC
import raop_rx_cases as RC
import raop_rx_textbook as RX
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu
FIRST_SEQ = (65534, 7, 40000, 65533)          # two of the four sessions cross the 65535 -> 0 wrap


@pytest.fixture(scope="module", params=[0, 1], ids=["wave", "plain"])
def ctx(request):
    c = capi.Context(0)
    c.set_kernel_variant(request.param)
    yield c
    c.close()


def ticks_of(k, s, seed):
    """the session's packets as datagrams in three ticks: damaged arrival, the answers to the resend requests, a late straggler"""
    rng = RC.Lcg(seed)
    seqs = [(FIRST_SEQ[k] + j) & 0xffff for j in range(len(s["payloads"]))]
    gram = {q: RC.A(q, payload=p) for q, p in zip(seqs, s["payloads"])}
    answer = {q: RC.R(q, payload=p, version=0, ptype=0) for q, p in zip(seqs, s["payloads"])}
    lost = seqs[1 + rng.below(len(seqs) - 2)]                                  # neither the first nor the last
    first = [RC.S(seqs[0] * 352, 11025), gram[seqs[0]]]
    at = seqs.index(lost)
    first += [gram[q] for q in seqs[1:at]]
    for q in sorted(seqs[at + 1:], key=lambda q: rng.below(1000)):             # behind the gap: shuffled
        first.append(gram[q])
        if rng.below(2):
            first.append(gram[q])      # ... and doubled on the audio port while it waits (a double of a frame that went out would be a restart)
    second = [answer[seqs[0]], answer[lost], answer[lost]]                     # an answer nobody asked for, the one that was, and it again
    third = [answer[seqs[-1]], (RC.other_gram(0x55), RX.CONTROL)]
    return [first, second, third], lost


def desc_of(s, flags, dst_offset, key=None):
    d = np.zeros(1, dtype=capi.RAOP_STREAM_DESC)
    for f in ("frame_length", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "max_frame_bytes", "avg_bit_rate", "sample_rate"):
        d[f] = s["cfg"][f]
    d["dst_offset"], d["flags"] = dst_offset, flags
    d["aes_key"], d["aes_iv"] = list(key or s["key"]), list(s["iv"])
    return d


def frame_bytes(s):
    return s["cfg"]["channels"] * (s["cfg"]["bit_depth"] // 8)


def room_of(s):
    """what the Apple Lossless batch asks for: a whole frame_length of samples a packet (a session's last packet may hold fewer)"""
    return len(s["payloads"]) * s["cfg"]["frame_length"] * frame_bytes(s)


def test_damaged_sessions_come_out_as_the_pcm_they_were_encoded_from(ctx):
    sessions = AC.sessions()
    plans = [ticks_of(k, s, 90 + k) for k, s in enumerate(sessions)]
    room = [room_of(s) + 64 for s in sessions]
    base = [sum(room[:k]) for k in range(len(sessions))]
    dst = np.full(sum(room), 0xA5, dtype=np.uint8)
    state = [RX.new_state() for _ in sessions]
    carried = [[] for _ in sessions]
    done = [0 for _ in sessions]                                               # packets out so far
    asked = [None for _ in sessions]
    for tick in range(3):
        streams = [RC.stream(carried[k] + plans[k][0][tick], state[k], 5) for k in range(len(sessions))]
        job = RC.Job(streams)
        descs = np.concatenate([desc_of(s, T.PACKED_LE, base[k] + done[k] * s["cfg"]["frame_length"] * frame_bytes(s)) for k, s in enumerate(sessions)])
        sres, recs, rows, ares, pres = ctx.raop_rx_alac_process_host(job.d_streams, descs, job.d_grams, np.frombuffer(job.src, dtype=np.uint8), dst)
        RC.assert_same(sres, recs, rows, job)                                  # the receiver's share is the model's
        for k, (s, res) in enumerate(zip(sessions, job.results)):
            first = int(job.d_streams["first_datagram"][k])
            assert all(int(pres["status"][first + j]) == T.OK and int(pres["samples"][first + j]) > 0 for j in range(res["n_output"]))
            done[k] += res["n_output"]
            state[k] = res["state_out"]
            carried[k] = [streams[k]["grams"][i] for i in res["pending"]]
            if tick == 0:
                asked[k] = res["ranges"]
    for k, s in enumerate(sessions):
        lost = plans[k][1]
        # the request at the end of the first tick names the lost packet (with the reference's `end - 1` of a waiting frame 0)
        assert asked[k][0] == (lost, (((lost + 1) & 0xffff) - 1) & 0xffffffff), (asked[k], lost)
        assert done[k] == len(s["payloads"]) and not carried[k] and state[k]["running"] == 1
        pcm = s["fx"]["pcm"]
        assert dst[base[k]:base[k] + len(pcm)].tobytes() == pcm, s["fixture"]
        assert (dst[base[k] + len(pcm):base[k] + room[k]] == 0xA5).all()


def test_the_plaintext_form_and_a_wrong_key_between_two_good_streams(ctx):
    a, b, c = AC.sessions()[0], AC.sessions()[1], AC.sessions()[2]
    wrong = bytes([b["key"][0] ^ 0x10]) + b["key"][1:]

    def in_order(s, first, extra):
        return [RC.A((first + j) & 0xffff, payload=p) for j, p in enumerate(s["payloads"])] + extra

    streams = [RC.stream(in_order(a, 65534, [RC.R(65534, payload=b"again")]), None, 5), RC.stream(in_order(b, 100, []), None, 5), RC.stream(in_order(c, 9, [RC.A(9)]), None, 5),
               RC.stream(in_order(a, 300, [RC.S(0, 11025)]), None, 5)]
    job = RC.Job(streams)
    size = [room_of(a), room_of(b), room_of(c), len(job.src) + 16]
    base = [0, size[0], size[0] + size[1], size[0] + size[1] + size[2]]
    dst = np.full(sum(size), 0xA5, dtype=np.uint8)
    descs = np.concatenate([desc_of(a, T.PACKED_LE, base[0]), desc_of(b, T.PACKED_LE, base[1], wrong), desc_of(c, T.PACKED_LE, base[2]), desc_of(a, AC.PLAINTEXT, base[3])])
    sres, recs, rows, ares, pres = ctx.raop_rx_alac_process_host(job.d_streams, descs, job.d_grams, np.frombuffer(job.src, dtype=np.uint8), dst)
    RC.assert_same(sres, recs, rows, job)
    assert [r["n_output"] for r in job.results] == [4, 4, 4, 4] and job.results[2]["stop_reason"] == RX.STOP_RESTARTED
    for k, s in ((0, a), (2, c)):
        pcm = s["fx"]["pcm"]
        assert dst[base[k]:base[k] + len(pcm)].tobytes() == pcm and (dst[base[k] + len(pcm):base[k] + size[k]] == 0xA5).all()
    assert dst[base[1]:base[1] + len(b["fx"]["pcm"])].tobytes() != b["fx"]["pcm"]          # the wrong key's stream is whatever its bytes decode to, the neighbours are exact
    # the plaintext stream: packet p at dst_offset + (its payload's place - the first payload's place), decrypted; nothing between
    first = int(job.d_streams["first_datagram"][3])
    want = np.full(size[3], 0xA5, dtype=np.uint8)
    place0 = int(rows["src_offset"][first])
    for j, p in enumerate(a["payloads"]):
        at = int(rows["src_offset"][first + j]) - place0
        want[at:at + len(p)] = np.frombuffer(AC.decrypt_cached(a["key"], a["iv"], p), dtype=np.uint8)
    assert dst[base[3]:].tobytes() == want.tobytes()
