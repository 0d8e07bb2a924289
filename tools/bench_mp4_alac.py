"""bench_mp4_alac.py -- the MPEG-4 container layer in front of the Apple Lossless decoder (ohgpu_mp4_*).

`--files` .m4a files of `--seconds` seconds of 44.1 kHz stereo 16-bit: the packets of the committed encoder-made fixture
tests/golden/alac/stereo16_fl4096, tiled (every file starts at another packet) and muxed by the tests' own muxer (tests/mp4_cases.py:
moov first, stco, `--per-chunk` samples a chunk).  Measured, in ALTERNATING pairs after `--sustain` seconds of back-to-back runs:
  - the container batch alone on both routes (run + results + both tables home), and its phases from device events: walk, tile sums,
    carries, expand on the fused route, the single launch on the plain one;
  - ohgpu_mp4_alac_process_host: file bytes in, PCM out;
  - ohgpu_alac_process_host over the same bytes with a packet table made on the host from the muxer's own record: what a caller had
    to do before this layer existed (and its table costs that caller a parser this figure does not include).
Every file's PCM is checked against what the fixture was encoded from.  Prints one JSON line and writes `--out`.

    python tools/bench_mp4_alac.py --files 256 --seconds 10 [--out profiles/mp4_summary.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIXTURE = "stereo16_fl4096"
PHASES = ("walk", "sums", "carries", "expand")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--per-chunk", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--sustain", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mp4_summary.md"))
    args = ap.parse_args()

    import alac_cases as AC
    import mp4_cases as MC
    from ohpipeline_amd import capi
    fx = AC.load_fixture(FIXTURE)
    cfg = fx["cfg"]
    fl, ch, rate = cfg["frame_length"], cfg["channels"], cfg["sample_rate"]
    full = fx["packets"][:-1]
    per_file = -(-int(round(args.seconds * rate)) // fl)
    unit = ch * (cfg["bit_depth"] // 8)
    pcm = [fx["pcm"][k * fl * unit:(k + 1) * fl * unit] for k in range(len(full))]
    muxed = [MC.mux([full[(r + k) % len(full)] for k in range(per_file)], fx["cookie"], per_chunk=[args.per_chunk]) for r in range(len(full))]
    expected = [b"".join(pcm[(r + k) % len(full)] for k in range(per_file)) for r in range(len(full))]

    n = args.files
    mp4, alac = np.zeros(n, dtype=capi.MP4_STREAM_DESC), np.zeros(n, dtype=capi.ALAC_STREAM_DESC)
    table = np.zeros(n * per_file, dtype=capi.ALAC_PACKET)                  # the host-made table: the muxer's record
    src, span = bytearray(), per_file * fl * unit
    for i in range(n):
        m = muxed[i % len(muxed)]
        mp4[i]["src_offset"], mp4[i]["src_bytes"], mp4[i]["packet_first"], mp4[i]["packet_capacity"] = len(src), len(m.data), i * per_file, per_file
        for k in ("frame_length", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "sample_rate"):
            alac[i][k] = cfg[k]
        alac[i]["first_packet"], alac[i]["n_packets"], alac[i]["dst_offset"], alac[i]["flags"] = i * per_file, per_file, i * span, capi.ALAC_OUT_PACKED_LE
        table["src_offset"][i * per_file:(i + 1) * per_file] = np.array(m.offsets, dtype=np.uint64) + len(src)
        table["bytes"][i * per_file:(i + 1) * per_file] = m.sizes
        src += m.data
    src = np.frombuffer(bytes(src), dtype=np.uint8)
    dst = np.zeros(n * span, dtype=np.uint8)

    def files_exact(buf):
        return sum(buf[i * span:(i + 1) * span].tobytes() == expected[i % len(expected)] for i in range(n))

    with capi.Context(0) as ctx:
        d_src = ctx.upload(src)
        batches = {}
        for route, variant in (("fused", 0), ("plain", 1)):
            ctx.set_kernel_variant(variant)
            batches[route] = ctx.mp4_batch(mp4, len(table), src.size)
            assert ctx.batch_paths(batches[route])["mp4_route"] == (capi.MP4_ROUTE_PLAIN if variant else capi.MP4_ROUTE_FUSED)
        ctx.set_kernel_variant(0)
        t0, sustained = time.perf_counter(), 0
        while sustained == 0 or time.perf_counter() - t0 < args.sustain:
            ctx.mp4_run(batches["fused"], d_src)
            ctx.mp4_results(batches["fused"], n, len(table))
            sustained += 1
        walls = {k: [] for k in ("fused", "plain", "mp4_alac", "alac_host_table")}
        phases = {"fused": [], "plain": []}
        tables_equal, exact = {}, {}
        steady = True
        for _ in range(args.pairs):
            before = ctx.device_allocations()
            for route in ("fused", "plain"):
                t = time.perf_counter()
                ctx.mp4_run(batches[route], d_src)
                res, pk, sm = ctx.mp4_results(batches[route], n, len(table))
                walls[route].append(time.perf_counter() - t)
                phases[route].append(ctx.mp4_phase_ms(batches[route]))
                tables_equal[route] = bool((res["status"] == capi.MP4_OK).all() and pk.tobytes() == table.tobytes())
            steady = steady and ctx.device_allocations() == before      # (the batches' runs; the host-buffer calls below keep arenas of their own)
            dst[:] = 0
            t = time.perf_counter()
            out = ctx.mp4_alac_process_host(mp4, alac, len(table), src, dst)
            walls["mp4_alac"].append(time.perf_counter() - t)
            exact.setdefault("mp4_alac", files_exact(dst) if (out[4]["status"] == capi.ALAC_OK).all() else 0)
            dst[:] = 0
            t = time.perf_counter()
            ctx.alac_process_host(alac, table, src, dst)
            walls["alac_host_table"].append(time.perf_counter() - t)
            exact.setdefault("alac_host_table", files_exact(dst))
        for b in batches.values():
            ctx.batch_destroy(b)
        ctx.free(d_src)
        name = ctx.name()

    result = {"what": "MPEG-4 container in front of Apple Lossless", "device": name, "files": n, "seconds": args.seconds, "packets": int(len(table)),
              "file_bytes": int(src.size), "samples_per_chunk": args.per_chunk, "pairs": args.pairs, "sustain_runs": sustained}
    for route in ("fused", "plain"):
        ph = np.median(np.array(phases[route]), axis=0)
        result[route] = {"run_ms": round(float(np.median(walls[route])) * 1e3, 3), "phase_ms": {k: round(float(v), 4) for k, v in zip(PHASES, ph)},
                         "table_equal_to_the_muxers_record": tables_equal[route]}
    for k in ("mp4_alac", "alac_host_table"):
        result[k] = {"call_ms": round(float(np.median(walls[k])) * 1e3, 3), "files_equal_to_the_encoded_pcm": int(exact[k])}
    result["container_share_of_the_fused_call"] = round(sum(result["fused"]["phase_ms"].values()) / result["mp4_alac"]["call_ms"], 4)
    all_ok = bool(all(tables_equal.values()) and all(v == n for v in exact.values()))
    result.update({"all_ok": all_ok, "steady_state_allocates_nothing": bool(steady)})
    print(json.dumps(result))

    f, p = result["fused"], result["plain"]
    lines = ["# MPEG-4 container in front of Apple Lossless (`tools/bench_mp4_alac.py`)", "",
             f"{n} files x {args.seconds:g} s of 44.1 kHz stereo 16-bit ({len(table)} packets of {fl} samples, {src.size / 1e6:.1f} MB of files, {args.per_chunk} samples a "
             f"chunk), tiled from `tests/golden/alac/{FIXTURE}` and muxed by `tests/mp4_cases.py`; {name}; medians of {args.pairs} alternating pairs after "
             f"{sustained} sustain runs.", "",
             "| container batch | run + results + tables home, ms | walk ms | tile sums ms | carries ms | expand ms | packet table equal to the muxer's record |",
             "|---|---|---|---|---|---|---|"]
    for route, r in (("fused", f), ("plain", p)):
        ph = r["phase_ms"]
        lines.append(f"| {route} | {r['run_ms']} | {ph['walk']} | {ph['sums']} | {ph['carries']} | {ph['expand']} | {r['table_equal_to_the_muxers_record']} |")
    lines += ["", "The plain route is one launch: its time is reported under walk.", "",
              "| host-buffer call | ms | files equal to the encoded PCM |", "|---|---|---|",
              f"| `ohgpu_mp4_alac_process_host`: file bytes in, PCM out | {result['mp4_alac']['call_ms']} | {result['mp4_alac']['files_equal_to_the_encoded_pcm']} / {n} |",
              f"| `ohgpu_alac_process_host`, the same bytes, a packet table made on the host | {result['alac_host_table']['call_ms']} | "
              f"{result['alac_host_table']['files_equal_to_the_encoded_pcm']} / {n} |", "",
              f"The fused route's four phases are {100 * result['container_share_of_the_fused_call']:.2f} % of the fused call.  "
              f"Steady state allocates nothing: {steady}.  Everything OK: {all_ok}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
