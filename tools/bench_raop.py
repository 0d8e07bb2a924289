"""bench_raop.py -- RAOP audio on the device (ohgpu_raop_batch_run): what the decrypt phase costs.

`--streams` streams of `--seconds` seconds of 44.1 kHz stereo 16-bit, the packets of tools/bench_alac_decode.py (tiled from the
committed fixture tests/golden/alac/stereo16_fl4096), each at a multiple of 4 in the arena, encrypted under per-stream keys as a RAOP
sender encrypts them (tools/raop_host_cpu.cpp, FIPS-197's Cipher written straightforwardly).  In ONE process: a RAOP batch over the
encrypted arena and an Apple Lossless batch over the same packets in the clear, run in ALTERNATING pairs after `--sustain` seconds
of back-to-back runs: wall clock around run + results, and each phase from device events.  Every stream's planes are checked against
the PCM the fixture was encoded from, on both.  Beside them, where the system has a libcrypto, its AES_cbc_encrypt decrypting the same
payloads on `--host-threads` threads: the SYSTEM's library with hardware AES, not the reference (which calls the same function, one
packet at a time, on the protocol thread).  Prints one JSON line and writes `--out`.

    python tools/bench_raop.py --streams 256 --seconds 10 [--out profiles/raop_summary.md]

The LDS bank-conflict share of the decrypt kernel comes from a run of its own, counters only:
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d DIR -- python tools/bench_raop.py --runs-only 3
and is handed to the next run with `--pmc-dir DIR` (raop_decrypt_kernel's rows are summed)."""
import argparse
import csv
import ctypes.util
import glob
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = ("decrypt", "entropy", "predict", "store")


def helper():
    build = os.path.join(ROOT, "tools", "build")
    os.makedirs(build, exist_ok=True)
    exe, text = os.path.join(build, "raop_host_cpu"), os.path.join(ROOT, "tools", "raop_host_cpu.cpp")
    core = os.path.join(ROOT, "ohpipeline_amd", "csrc", "raop_aes_core.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(text), os.path.getmtime(core)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", text, "-o", exe, "-ldl"])
    return exe, build


def job_blob(secrets, table, n_packets_per_stream, arena):
    rows = b"".join(struct.pack("<QII", int(p["src_offset"]), int(p["bytes"]), k // n_packets_per_stream) for k, p in enumerate(table))
    return struct.pack("<IIQ", len(secrets), len(table), arena.size) + b"".join(secrets) + rows + arena.tobytes()


def pmc_share(directory):
    """(conflict cycles, active cycles) of raop_decrypt_kernel in a rocprofv3 --pmc CSV directory"""
    sums = {}
    for path in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if "raop_decrypt_kernel" in row.get("Kernel_Name", ""):
                    sums[row["Counter_Name"]] = sums.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    return sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--sustain", type=float, default=1.0)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--runs-only", type=int, default=0, help="run the RAOP batch this many times and leave: for a counters-only profiler run")
    ap.add_argument("--pmc-dir", default=None, help="a rocprofv3 --pmc output directory of a --runs-only run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raop_summary.md"))
    args = ap.parse_args()

    import alac_cases as AC
    import bench_alac_decode as BA
    from ohpipeline_amd import capi
    fx = AC.load_fixture(BA.FIXTURE)
    cfg = fx["cfg"]
    fl, ch, rate = cfg["frame_length"], cfg["channels"], cfg["sample_rate"]
    per_stream = -(-int(round(args.seconds * rate)) // fl)
    descs, table, packed, dst_bytes = BA.workload(capi, fx, args.streams, per_stream)
    # the same packets, each at a multiple of 4
    clear = np.zeros(int(sum((int(b) + 3) // 4 * 4 for b in table["bytes"])), dtype=np.uint8)
    at = 0
    for p in table:
        clear[at:at + int(p["bytes"])] = packed[int(p["src_offset"]):int(p["src_offset"]) + int(p["bytes"])]
        p["src_offset"] = at
        at += (int(p["bytes"]) + 3) // 4 * 4
    payload_bytes = int(table["bytes"].sum())
    rng = AC.Lcg(2026)
    secrets = [bytes(rng.next() & 0xff for _ in range(32)) for _ in range(args.streams)]
    exe, build = helper()
    job, enc = os.path.join(build, "raop_job.bin"), os.path.join(build, "raop_enc.bin")
    with open(job, "wb") as f:
        f.write(job_blob(secrets, table, per_stream, clear))
    subprocess.check_output([exe, "encrypt", job, enc, str(args.host_threads)])
    sent = np.fromfile(enc, dtype=np.uint8)
    os.remove(job)
    os.remove(enc)
    rdescs = np.zeros(args.streams, dtype=capi.RAOP_STREAM_DESC)
    for name in capi.ALAC_STREAM_DESC.names:
        rdescs[name] = descs[name]
    for s, secret in enumerate(secrets):
        rdescs[s]["aes_key"], rdescs[s]["aes_iv"] = list(secret[:16]), list(secret[16:])
    total = args.streams * per_stream * fl
    n_full = len(fx["packets"]) - 1
    pcm = np.array(fx["samples"], dtype=np.int32)[:n_full * fl].reshape(n_full, fl, ch)
    expected = [np.concatenate([pcm[(r + k) % n_full] for k in range(per_stream)]).T for r in range(n_full)]

    with capi.Context(0) as ctx:
        d_sent, d_clear, d_dst = ctx.upload(sent), ctx.upload(clear), ctx.malloc(dst_bytes)
        raop = ctx.raop_batch(rdescs, table, sent.size, dst_bytes)
        alac = ctx.alac_batch(descs, table, clear.size, dst_bytes)
        if args.runs_only:
            for _ in range(args.runs_only):
                ctx.raop_run(raop, d_sent, d_dst)
                ctx.raop_results(raop, args.streams, len(table))
            ctx.batch_destroy(raop); ctx.batch_destroy(alac)
            ctx.free(d_sent); ctx.free(d_clear); ctx.free(d_dst)
            return 0
        t0, sustained = time.perf_counter(), 0
        while sustained == 0 or time.perf_counter() - t0 < args.sustain:
            ctx.raop_run(raop, d_sent, d_dst)
            ctx.raop_results(raop, args.streams, len(table))
            sustained += 1
        allocs = ctx.device_allocations()
        walls, phases, checked, ok = {"raop": [], "alac": []}, {"raop": [], "alac": []}, {}, True
        for _ in range(args.pairs):
            for which in ("raop", "alac"):
                if which not in checked:
                    ctx.memset(d_dst, 0, dst_bytes)
                    ctx.sync()
                t = time.perf_counter()
                if which == "raop":
                    ctx.raop_run(raop, d_sent, d_dst)
                    sres, pres = ctx.raop_results(raop, args.streams, len(table))
                else:
                    ctx.alac_run(alac, d_clear, d_dst)
                    sres, pres = ctx.alac_results(alac, args.streams, len(table))
                walls[which].append(time.perf_counter() - t)
                phases[which].append(ctx.raop_phase_ms(raop) if which == "raop" else (0.0,) + ctx.alac_phase_ms(alac))
                ok = ok and bool((pres["status"] == capi.ALAC_OK).all() and (sres["samples"] == per_stream * fl).all())
                if which not in checked:
                    out = ctx.download(d_dst, dst_bytes).view("<i4").reshape(args.streams, ch, per_stream * fl)
                    checked[which] = sum(bool(np.array_equal(out[s], expected[s % n_full])) for s in range(args.streams))
        steady = ctx.device_allocations() == allocs
        ctx.batch_destroy(raop); ctx.batch_destroy(alac)
        ctx.free(d_sent); ctx.free(d_clear); ctx.free(d_dst)
        name = ctx.name()

    host = None
    library = ctypes.util.find_library("crypto")
    if library:
        with open(job, "wb") as f:
            f.write(job_blob(secrets, table, per_stream, sent))
        answer = subprocess.check_output([exe, "libcrypto", job, str(args.host_threads), library], text=True).split()[0]
        os.remove(job)
        host = None if answer == "absent" else float(answer)

    result = {"what": "RAOP audio: AES-128-CBC decrypt in front of the Apple Lossless decode, datagram payloads -> TInt32 planes", "device": name,
              "streams": args.streams, "seconds": args.seconds, "samples_total": total, "packets": int(len(table)), "payload_bytes": payload_bytes, "frame_length": fl}
    for which in ("raop", "alac"):
        wall = float(np.median(walls[which]))
        ph = np.median(np.array(phases[which]), axis=0)
        result[which] = {"run_ms": round(wall * 1e3, 3), "device_ms": round(float(ph.sum()), 3), "phase_ms": {k: round(float(v), 3) for k, v in zip(PHASES, ph)},
                         "streams_equal_to_the_encoded_pcm": int(checked[which])}
    r = result["raop"]
    result["cost_of_the_feature"] = {"run_ms": round(r["run_ms"] - result["alac"]["run_ms"], 3), "device_ms": round(r["device_ms"] - result["alac"]["device_ms"], 3),
                                     "run_ratio": round(r["run_ms"] / result["alac"]["run_ms"], 3)}
    result["decrypt"] = {"ms": r["phase_ms"]["decrypt"], "payload_GB_per_s": round(payload_bytes / (r["phase_ms"]["decrypt"] * 1e-3) / 1e9, 1)}
    result["longest_phase"] = max(PHASES, key=lambda k: r["phase_ms"][k])
    result["shortest_phase"] = min(PHASES, key=lambda k: r["phase_ms"][k])
    if args.pmc_dir:
        sums = pmc_share(args.pmc_dir)
        result["decrypt"]["pmc"] = sums
        if sums.get("SQ_LDS_IDX_ACTIVE"):
            result["decrypt"]["lds_bank_conflict_share"] = round(sums.get("SQ_LDS_BANK_CONFLICT", 0.0) / sums["SQ_LDS_IDX_ACTIVE"], 3)
    if host is not None:
        result["system_libcrypto"] = {"what": "the system's libcrypto (AES_cbc_encrypt, hardware AES where the CPU has it), not the reference", "threads": args.host_threads,
                                      "ms": round(host * 1e3, 3), "payload_GB_per_s": round(payload_bytes / host / 1e9, 1)}
    all_ok = bool(ok and all(checked[w] == args.streams for w in checked))
    result.update({"all_ok": all_ok, "steady_state_allocates_nothing": bool(steady), "sustain_runs": sustained, "pairs": args.pairs})
    print(json.dumps(result))

    a = result["alac"]
    lines = ["# RAOP audio on the device (`tools/bench_raop.py`)", "",
             f"{args.streams} streams x {args.seconds:g} s of 44.1 kHz stereo 16-bit ({len(table)} packets of {fl} samples, {payload_bytes / 1e6:.1f} MB of payload, "
             f"{total / 1e6:.1f} M samples per channel): the packets of `tools/bench_alac_decode.py`, each at a multiple of 4, encrypted under {args.streams} keys; {name}; "
             f"medians of {args.pairs} alternating pairs (RAOP batch, Apple Lossless batch over the same packets in the clear, one process) after {sustained} sustain runs.  "
             "Phases from device events, run + results from the wall clock.", "",
             "| batch | run + results, ms | device ms | decrypt ms | entropy ms | predict ms | store ms | streams equal to the encoded PCM |", "|---|---|---|---|---|---|---|---|"]
    for which, label in (("raop", "`ohgpu_raop_batch_run` (encrypted)"), ("alac", "`ohgpu_alac_batch_run` (in the clear)")):
        x = result[which]
        lines.append(f"| {label} | {x['run_ms']} | {x['device_ms']} | {x['phase_ms']['decrypt'] if which == 'raop' else '-'} | {x['phase_ms']['entropy']} | "
                     f"{x['phase_ms']['predict']} | {x['phase_ms']['store']} | {x['streams_equal_to_the_encoded_pcm']} / {args.streams} |")
    c = result["cost_of_the_feature"]
    lines += ["", f"(a) The cost of the feature: {c['run_ms']} ms of run + results ({c['run_ratio']}x the run in the clear), {c['device_ms']} ms of device time "
              f"({r['device_ms']} against {a['device_ms']}).", "",
              f"(b) The decrypt phase: {result['decrypt']['ms']} ms, {result['decrypt']['payload_GB_per_s']} GB/s of payload; the longest of the four phases is "
              f"**{result['longest_phase']}**, the shortest **{result['shortest_phase']}**."]
    if "lds_bank_conflict_share" in result["decrypt"]:
        lines[-1] += (f"  LDS bank conflicts, from one counters-only `rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE` run of `--runs-only`: "
                      f"{result['decrypt']['lds_bank_conflict_share']} of the kernel's LDS-active cycles (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE).")
    else:
        lines[-1] += "  The LDS bank-conflict share was not taken in this run (no `--pmc-dir`)."
    if host is not None:
        h = result["system_libcrypto"]
        lines += ["", f"(c) The system's libcrypto (`AES_cbc_encrypt`, hardware AES where the CPU has it) decrypting the same payloads on {args.host_threads} threads: {h['ms']} ms, "
                  f"{h['payload_GB_per_s']} GB/s.  That is the system library, not the reference, which calls it one packet at a time on the protocol thread."]
    else:
        lines += ["", "(c) No libcrypto on this machine: no host figure."]
    lines += ["", f"Steady state allocates nothing: {steady}.  Everything OK: {all_ok}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
