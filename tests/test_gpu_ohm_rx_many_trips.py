"""The Songcast receiver's kernels over work lists longer than a launch holds.

  gather    ohm_rx_gather_kernel is the persistent one: a wave per datagram, workgroups of 4 waves, the launch capped at 8 workgroups
            a CU (ohm_rx_gather_blocks); every wave goes round the datagram table in strides of the launch's waves.  What a launch
            holds is the larger of that cap and what the CUs keep resident: max(8 x 4, 32) x CUs waves.  The table here has more than
            2 x that + 67 datagrams, so every wave makes two trips and the lowest-numbered ones a third; the items are the smallest the kernel admits
            (0..70 audio bytes: no whole line, one, or a few, at seeded lengths and alignments), duplicates among them that a wave
            must skip.
  parse     ohm_rx_parse_kernel and ohm_rx_sequence_kernel are NOT persistent -- a lane per datagram / per stream, the launch sized to
            the table (ceil(datagrams / 256) workgroups, ceil(streams / 64)) -- so they have no trip to go round; the same table runs
            through them and the dispositions of all its records are compared.

The need is asserted before anything runs.  Every 61st datagram is checked against the pure-Python model (tests/ohm_rx_textbook.py:
its record, and its audio where the record says it went); the whole destination arena against a numpy restatement -- the payload
slices of the source arena, concatenated in frame order."""
import numpy as np
import pytest

import ohm_rx_cases as RC
import ohm_rx_textbook as RX
import ohm_textbook as OT
from device_shape import MAX_WAVES_PER_CU, compute_units
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

GATHER_WAVES, GATHER_GROUPS_PER_CU = 4, 8       # kRxWaves, kGatherGroupsPerCu
SAMPLE_EVERY = 61
FILL, N_STREAMS = 0xA5, 24


def gather_need(cus):
    return 2 * max(GATHER_GROUPS_PER_CU * GATHER_WAVES, MAX_WAVES_PER_CU) * cus + 67


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def build(cus):
    rng = np.random.default_rng(77000 + cus)
    lcg = RC.Lcg(77 + cus)
    per_stream = gather_need(cus) // N_STREAMS + 2
    grams, tables, runs = [], [], []                                       # per stream: datagrams in arrival order; (frame rank, is a copy)
    for i in range(N_STREAMS):
        first = (0, 5, 0xffffff00, 0xfffffffe)[i % 4]
        codec = bytes(rng.integers(65, 91, int(rng.integers(0, 30)), dtype=np.uint8))
        payload = [rng.integers(0, 256, int(rng.integers(0, 71)), dtype=np.uint8).tobytes() for _ in range(per_stream)]
        order = RC.window_shuffle(list(range(per_stream)), lcg, reach=5)
        mine, tags = [], []
        for j in order:
            mine.append(RC.audio_gram((first + j) & 0xffffffff, payload[j], codec=codec, depth=8, channels=1))
            tags.append((j, False))
            if rng.random() < 0.03:
                mine.append(RC.audio_gram((first + j) & 0xffffffff, b"copy", flags=OT.FLAG_LOSSLESS | OT.FLAG_RESENT, codec=codec, depth=8, channels=1))
                tags.append((j, True))
        grams.append(mine)
        tables.append(tags)
        runs.append(b"".join(payload))
    # the arenas: datagrams round robin, at seeded multiples of 4; runs back to back with odd gaps
    src, where = bytearray(), [[0] * len(g) for g in grams]
    for k in range(max(len(g) for g in grams)):
        for i, g in enumerate(grams):
            if k < len(g):
                src += bytes(-len(src) % 4 + 4 * int(rng.integers(0, 3)))
                where[i][k] = len(src)
                src += g[k]
    streams = np.zeros(N_STREAMS, dtype=capi.OHM_RX_STREAM)
    table = np.zeros(sum(len(g) for g in grams), dtype=capi.OHM_RX_DATAGRAM)
    at, q = 7, 0
    for i, g in enumerate(grams):
        s = streams[i]
        s["first_datagram"], s["n_datagrams"], s["dst_offset"], s["dst_capacity"] = q, len(g), at, sum(len(x) - 58 for x in g)
        s["last_sample_start"], s["stream_msg_due"] = 0xffffffff, 1
        for k, x in enumerate(g):
            table[q + k]["src_offset"], table[q + k]["bytes"] = where[i][k], len(x)
        q += len(g)
        at += int(s["dst_capacity"]) + 3 + i
    return dict(grams=grams, tags=tables, runs=runs, src=np.frombuffer(bytes(src), dtype=np.uint8), streams=streams, table=table, dst_bytes=at)


def test_the_gather_goes_round_its_table_and_the_parse_covers_it(ctx):
    cus = compute_units()
    case = build(cus)
    n = case["table"].size
    outputs = sum(1 for tags in case["tags"] for _, copy in tags if not copy)
    assert outputs > gather_need(cus) and gather_need(cus) == 2 * max(8 * 4, 32) * cus + 67, (outputs, cus)
    assert min(-(-n // GATHER_WAVES), cus * GATHER_GROUPS_PER_CU) == cus * GATHER_GROUPS_PER_CU            # the launch IS capped
    capi.ohm_rx_batch_check(case["streams"], case["table"], case["src"].size, case["dst_bytes"])
    d_src, d_dst = ctx.upload(case["src"]), ctx.malloc(case["dst_bytes"])
    b = ctx.ohm_rx_batch(case["streams"], case["table"], case["src"].size, case["dst_bytes"])
    try:
        arenas = []
        for _ in range(2):
            ctx.memset(d_dst, FILL, case["dst_bytes"])
            ctx.ohm_rx_run(b, d_src, d_dst)
            sres, recs = ctx.ohm_rx_results(b, N_STREAMS, n)
            arenas.append(ctx.download(d_dst, case["dst_bytes"]))
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    # the numpy restatement: every stream's payloads in frame order, FILL elsewhere
    want = np.full(case["dst_bytes"], FILL, dtype=np.uint8)
    for s, run in zip(case["streams"], case["runs"]):
        want[int(s["dst_offset"]):int(s["dst_offset"]) + len(run)] = np.frombuffer(run, dtype=np.uint8)
    for k, got in enumerate(arenas):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"run {k + 1}: {bad.size} of {want.size} bytes differ, first at {bad[:8].tolist()}"
    # every record's disposition and order from the construction
    q = 0
    for i, tags in enumerate(case["tags"]):
        mine = recs[q:q + len(tags)]
        assert [int(d) for d in mine["disposition"]] == [capi.OHM_RX_DUPLICATE if copy else capi.OHM_RX_OUTPUT for _, copy in tags], i
        assert [int(o) for o, (_, copy) in zip(mine["order"], tags) if not copy] == [j for j, copy in tags if not copy], i
        assert int(sres[i]["n_output"]) == sum(1 for _, c in tags if not c) and int(sres[i]["out_bytes"]) == len(case["runs"][i])
        assert int(sres[i]["n_pending"]) == 0 and int(sres[i]["stop_reason"]) == 0
        q += len(tags)
    # every 61st datagram against the pure-Python model
    flat = [(i, k) for i, g in enumerate(case["grams"]) for k in range(len(g))]
    for q in range(0, n, SAMPLE_EVERY):
        i, k = flat[q]
        gram, r = case["grams"][i][k], recs[q]
        model = RX.parse(gram)
        assert int(r["status"]) == model["status"] == RX.OK
        assert all(int(r[name]) == model[name] for name in RX.HEADER_FIELDS + ("audio_offset", "audio_bytes", "msg_type")), q
        assert bytes(r["codec"][:model["codec_bytes"]]) == model["codec"]
        if int(r["disposition"]) == capi.OHM_RX_OUTPUT:
            at = int(r["dst_offset"])
            assert arenas[0][at:at + model["audio_bytes"]].tobytes() == gram[model["audio_offset"]:], q
