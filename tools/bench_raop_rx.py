"""bench_raop_rx.py -- the RAOP receiver on the device (ohgpu_raop_rx_batch_run): what parse, sequence and table cost, and
what the wave sequencer gains over the plain one.

`--streams` streams of `--seconds` seconds of 352-frame packets at 44.1 kHz (1253 packets for 10 s), each datagram 12 header bytes and
`PAYLOAD` payload bytes in a slot of its own at a multiple of 16 of the source arena; every stream starts at a seeded sequence number, so
some wrap.  Two shapes: `in_order`, and `late_1pct`, where a seeded 1 % of the packets arrive up to 40 places late, each followed by its
0x56-wrapped resend (max_frames 50; a drawn packet is left in place while the late one before it is still out, so that no repair
overflows: `late_packets` says how many were moved).  The baseline is the plain route of the same build -- a lane per stream running
the serial text, the design of the Songcast receiver's sequencer -- not another program: two batches over the same tables, one created
under ohgpu_set_kernel_variant(1), run in alternating pairs in one process after `--warmup` pairs; each phase from device events, medians
over `--runs` pairs.  Both routes' results, records and rows are compared with each other, and every stream's rows with the packets in
sequence order.  One JSON line.

    python tools/bench_raop_rx.py --streams 256 --seconds 10 [--out profiles/raop_rx_summary.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAYLOAD = 1028
SLOT = (16 + PAYLOAD + 15) // 16 * 16
SSRC = 0x1234abcd


def build(n_streams, n_packets, late):
    """-> (source arena, stream table, datagram table, per stream the datagram index of each packet's first arrival in sequence order)"""
    from ohpipeline_amd import capi
    rng = np.random.default_rng(2100 + late)
    orders = []
    for _ in range(n_streams):
        order = np.arange(n_packets)
        resent = np.zeros(0, dtype=np.int64)
        if late:
            drawn = np.flatnonzero(rng.random(n_packets) < 0.01)
            delay = rng.integers(1, 41, size=drawn.size)
            keep, free_from = [], 1                             # (a late packet is taken only once the one before it has arrived: no two repairs overlap)
            for j, p in enumerate(drawn.tolist()):
                if p >= free_from:
                    keep.append(j)
                    free_from = p + int(delay[j]) + 2
            moved, delay = drawn[keep], delay[keep]
            key = order.astype(np.float64)
            key[moved] += delay + 0.5
            order = order[np.argsort(key, kind="stable")]
            resent = moved
        arrival = []
        is_resent = set(resent.tolist())
        for p in order.tolist():
            arrival.append((p, False))
            if p in is_resent:
                arrival.append((p, True))
        orders.append(arrival)
    total = sum(len(a) for a in orders)
    src = np.zeros(total * SLOT, dtype=np.uint8)
    slots = src.reshape(total, SLOT)
    streams = np.zeros(n_streams, dtype=capi.RAOP_RX_STREAM)
    grams = np.zeros(total, dtype=capi.RAOP_RX_DATAGRAM)
    grams["src_offset"] = np.arange(total, dtype=np.uint64) * SLOT
    first_of, q = [], 0
    for i, arrival in enumerate(orders):
        first_seq = int(rng.integers(0, 65536))
        packet = np.array([p for p, _ in arrival], dtype=np.int64)
        resend = np.array([r for _, r in arrival], dtype=bool)
        n = len(arrival)
        rows = slots[q:q + n]
        head = np.zeros((n, 12), dtype=np.uint8)
        head[:, 0], head[:, 1] = 0x80, 0x60
        head[:, 2:4] = ((first_seq + packet) & 0xffff).astype(">u2").view(np.uint8).reshape(-1, 2)
        head[:, 4:8] = ((packet * 352) & 0xffffffff).astype(">u4").view(np.uint8).reshape(-1, 4)
        head[:, 8:12] = np.frombuffer(SSRC.to_bytes(4, "big"), dtype=np.uint8)
        rows[~resend, :12] = head[~resend]
        rows[resend, 0:4] = np.array([0x80, 0xd6, 0, 1], dtype=np.uint8)
        rows[resend, 4:16] = head[resend]
        g = grams[q:q + n]
        g["bytes"] = np.where(resend, 16 + PAYLOAD, 12 + PAYLOAD)
        g["port"] = resend
        s = streams[i]
        s["first_datagram"], s["n_datagrams"], s["max_frames"] = q, n, 50
        where = np.zeros(n_packets, dtype=np.int64)
        for k in range(n - 1, -1, -1):
            where[packet[k]] = k                                # the first arrival of each packet
        first_of.append(where)
        q += n
    return src, streams, grams, first_of


def late_count(grams):
    return int((grams["port"] == 1).sum())


def measure(ctx, label, n_streams, n_packets, late, args):
    from ohpipeline_amd import capi
    src, streams, grams, first_of = build(n_streams, n_packets, late)
    capi.raop_rx_batch_check(streams, grams, src.size)
    d_src = ctx.upload(src)
    batches = {}
    for route, variant in (("wave", 0), ("plain", 1)):
        ctx.set_kernel_variant(variant)
        try:
            batches[route] = ctx.raop_rx_batch(streams, grams, src.size)
        finally:
            ctx.set_kernel_variant(0)
    phases = {route: [] for route in batches}
    try:
        for k in range(args.warmup + args.runs):
            for route in (("wave", "plain") if k % 2 == 0 else ("plain", "wave")):      # alternating pairs
                ctx.raop_rx_run(batches[route], d_src)
                ctx.raop_rx_results(batches[route], n_streams, 0)
                phases[route].append(ctx.raop_rx_phase_ms(batches[route]))
        answers = {}
        for route, b in batches.items():
            sres, recs = ctx.raop_rx_results(b, n_streams, grams.size)
            answers[route] = (sres, recs, ctx.raop_rx_packets(b, grams.size))
    finally:
        for b in batches.values():
            ctx.batch_destroy(b)
        ctx.free(d_src)
    sres, recs, rows = answers["wave"]
    same = all(a.tobytes() == b.tobytes() for a, b in zip(answers["wave"], answers["plain"]))
    ok = bool(np.all(sres["n_output"] == n_packets) and np.all(sres["n_pending"] == 0) and np.all(sres["stop_reason"] == 0))
    for i in range(n_streams):
        first = int(streams[i]["first_datagram"])
        at = first + first_of[i]
        want = grams["src_offset"][at] + np.where(grams["port"][at] == 1, 16, 12).astype(np.uint64)
        ok = ok and np.array_equal(rows["src_offset"][first:first + n_packets], want)
    out = dict(shape=label, streams=n_streams, packets=n_packets, datagrams=int(grams.size), late_packets=late_count(grams), check=ok, routes_agree=same)
    for route in ("wave", "plain"):
        ms = np.median(np.array(phases[route][args.warmup:]), axis=0)
        out[route] = dict(parse_ms=round(float(ms[0]), 4), sequence_ms=round(float(ms[1]), 4), table_ms=round(float(ms[2]), 4), total_ms=round(float(ms.sum()), 4),
                          sequence_ns_per_datagram=round(float(ms[1]) * 1e6 / grams.size, 2), datagrams_per_s=round(grams.size / (float(ms.sum()) * 1e-3)))
    out["sequence_plain_over_wave"] = round(out["plain"]["sequence_ms"] / out["wave"]["sequence_ms"], 2)
    out["total_plain_over_wave"] = round(out["plain"]["total_ms"] / out["wave"]["total_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_packets = int(round(args.seconds * 44100 / 352))
    from ohpipeline_amd import capi
    with capi.Context(0) as ctx:
        result = dict(bench="raop_rx", device=ctx.name(), payload_bytes=PAYLOAD, shapes=[measure(ctx, "in_order", args.streams, n_packets, 0, args),
                                                                                       measure(ctx, "late_1pct", args.streams, n_packets, 1, args)])
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n```\n" + line + "\n```\n")


if __name__ == "__main__":
    main()
