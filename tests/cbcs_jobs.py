"""The jobs of the second protected MPEG-4 family's tests, each made once and each with an assertion, from the model's own outputs, that
it reaches what it is for -- so that a fixture that shrinks fails there and does not quietly stop testing a path.
tests/test_cbcs_core_cpu.py takes every job through the sanitised CPU driver; tests/test_gpu_cbcs_textbook.py takes the same jobs to
the device."""
import functools

import cbcs_cases as BC
import cbcs_textbook as BX
import cenc_cases as CC

TILE, SLOT_UNITS, CRYPT_WAVES, CRYPT_GROUPS_PER_CU = 1024, 64, 4, 8      # kTile, cbcs::kLaneUnits, kProtWaves, kProtGroupsPerCu (csrc/protected_shell.h)
TRIPS = 5


def slots_of(d):
    """the documented rule: a stream has room for dst_capacity / 16 + packet_capacity + 3 subsample_capacity units, and none if either of the first two is 0"""
    if not d["dst_capacity"] or not d["packet_capacity"]:
        return 0
    return (int(d["dst_capacity"]) // 16 + int(d["packet_capacity"]) + 3 * int(d["subsample_capacity"]) + SLOT_UNITS - 1) // SLOT_UNITS


@functools.lru_cache(maxsize=None)
def named_job():
    good, bad = BC.named_good(), BC.named_malformed()
    streams = [BC.stream(m, gather_first_row=k % 3) for k, m in enumerate(good.values())]
    streams += [BC.stream(data, codecs=codecs, have_key=have_key, kid=kid) for data, _, _, codecs, have_key, kid in bad.values()]
    # parts that do not sum to their sample in a run BEYOND run_capacity: INVALID all the same, and so is the stream with room for both runs
    m = BC.build([40, 50, 60, 70], counts=[2, 2], iv_size=16, layout=lambda i, size: [(4, size - 4)], seed=33)
    senc = m.find("senc", 1)
    wrong = BC.FC.patched(m, senc[1] + 8 + 16 + 2 + 2, 55)          # (the second traf's first entry: 4 clear bytes, 56 protected)
    streams += [BC.stream(wrong, capacity=4, run_capacity=1, sub_capacity=8), BC.stream(wrong, capacity=4, run_capacity=2, sub_capacity=8)]
    job = BC.Job(streams)
    job.beyond = (BX.INVALID, senc[0])
    return job


def assert_named(job, results):
    good, bad = BC.named_good(), BC.named_malformed()
    for m, f in zip(job.models, good.values()):
        assert m["status"] == BX.OK and m["samples_available"] == f.n and m["subsamples"] == f.subsamples
    got = [(int(r["cenc"]["mp4f"]["status"]), int(r["cenc"]["mp4f"]["error_offset"])) for r in results[len(good):]]
    assert got == [(status, at) for _, status, at, _, _, _ in bad.values()] + [job.beyond] * 2
    assert [(m["status"], m["error_offset"]) for m in job.models[-2:]] == [job.beyond] * 2
    assert {int(r["cenc"]["mp4f"]["status"]) for r in results} >= {BX.OK, BX.INVALID, BX.UNSUPPORTED, BX.NO_KEY}
    assert {(int(r["cenc"]["iv_size"]), int(r["constant_iv_size"])) for r in results} >= {(8, 0), (16, 0), (0, 8), (0, 16), (0, 0)}
    assert {(int(r["crypt_blocks"]), int(r["skip_blocks"])) for r in results} >= set(BC.PATTERNS)
    assert {int(r["cenc"]["scheme"]) for r in results} >= {0, BX.code(b"cenc"), BX.code(b"cbcs")}
    assert sum(1 for m in job.models if m["blocks"]) >= 20


ALIGNED_FILES = {"cbcs_edge_parts": BC.EDGE_PARTS, "cbcs_parts_of_63_to_129_blocks": tuple(16 * b for b in BC.PIECE_BLOCKS),
                 "cenc_edge_parts_alac": BC.EDGE_PARTS, "cenc_keystream_offsets_and_the_wrap": BC.CTR_PARTS}
SRC_ALIGN, DST_ALIGN = (0, 1, 7, 14), (0, 3, 8, 15)


@functools.lru_cache(maxsize=None)
def alignment_job():
    """every file that carries a named protected-part size, each laid at all sixteen pairs of four source and four destination
    alignments: stream i holds file i % 4 at pair i // 4"""
    good = BC.named_good()
    files = [good[name] for name in ALIGNED_FILES]
    job = BC.Job([BC.stream(files[i % 4]) for i in range(64)], align=lambda i: SRC_ALIGN[i // 4 % 4], dst_align=lambda i: DST_ALIGN[i // 16])
    job.files = [files[i % 4] for i in range(64)]
    return job


def part_places(job):
    """-> {(file, protected bytes of a part, its sample, its entry): {(source address % 16, destination address % 16) of the part's first
    byte, a pair a stream that holds the file}}, from the muxer's record of the entries, the files' sample places and the model's rows"""
    names = list(ALIGNED_FILES)
    out = {}
    for i, (d, m, f) in enumerate(zip(job.descs, job.models, job.files)):
        for row, entries in enumerate(f.entries):
            at = 0
            for e, (clear, prot) in enumerate(entries or [(0, f.sizes[row])]):
                src = int(d["src_offset"]) + f.offsets[row] + at + clear
                dst = int(d["dst_offset"]) + m["clear_rows"][row][0] + at + clear
                out.setdefault((names[i % 4], prot, row, e), set()).add((src % 16, dst % 16))
                at += clear + prot
    return out


def assert_alignments(job):
    assert {(int(d["src_offset"]) % 16, int(d["dst_offset"]) % 16) for d in job.descs} == {(a, b) for a in SRC_ALIGN for b in DST_ALIGN}
    for m, f in zip(job.models, job.files):
        BC.check_against_record(m, f)
    places = part_places(job)
    for name, sizes in ALIGNED_FILES.items():
        for size in sizes:
            # (the parts of 64 and 128 blocks are written with a tail of 5 bytes behind their whole blocks)
            mine = [v for (n, p, _, _), v in places.items() if n == name and (p == size or (size % 1024 == 0 and p == size + 5))]
            assert mine, (name, size)
            for pairs in mine:      # every such part lies at sixteen pairs, four residues on either side, odd destination addresses among them
                assert len(pairs) == 16 and len({a for a, _ in pairs}) == 4 == len({b for _, b in pairs}) and any(b % 2 for _, b in pairs), (name, size, sorted(pairs))


@functools.lru_cache(maxsize=None)
def capacity_job():
    """gather_first_row inside a traf; subsample_capacity one short, a few rows' worth and none; packet and run capacities below the
    counts; rooms too small; prefixes of a stream cut inside a senc and inside the second fragment's samples"""
    good = BC.named_good()
    two, many = good["two_truns_under_one_subsample_senc_front"], good["cbcs_counts_0_1_2_3_17"]
    streams = [BC.stream(two, gather_first_row=row) for row in (0, 3, 5, 6, 70)]
    streams += [BC.stream(two, sub_capacity=two.subsamples - 1), BC.stream(two, sub_capacity=11), BC.stream(two, sub_capacity=0), BC.stream(two, sub_capacity=11, gather_first_row=5)]
    streams += [BC.stream(many, sub_capacity=k) for k in (22, 6, 5, 0)]
    streams += [BC.stream(two, capacity=40, run_capacity=1), BC.stream(two, capacity=4), BC.stream(two, dst_capacity=sum(two.sizes) - 1), BC.stream(two, dst_capacity=0),
                BC.stream(two, capacity=0, run_capacity=0, sub_capacity=0)]
    split = good["cbcs_parts_of_63_to_129_blocks"]
    senc = split.find("senc")
    streams += [BC.stream(split.data[:cut], capacity=split.n, run_capacity=len(split.runs), key=split.key, kid=split.kid, sub_capacity=split.subsamples)
                for cut in (senc[1] + 20, split.segment_ends[0] + 40, split.offsets[3] + 100)]
    return BC.Job(streams)


def assert_capacities(job):
    m = job.models
    assert [x["samples_available"] for x in m[5:9]] == [70, 5, 0, 5] and [x["subsamples"] for x in m[5:9]] == [140, 10, 0, 10]
    assert m[5]["bytes_gathered"] and m[6]["bytes_gathered"] and not m[7]["bytes_gathered"] and not m[8]["bytes_gathered"] and m[5]["samples"] == 71
    assert [x["samples_available"] for x in m[9:13]] == [4, 4, 3, 1] and [x["subsamples"] for x in m[9:13]] == [6, 6, 3, 0]
    assert m[13]["samples_available"] == 5 and m[14]["samples_available"] == 4 and not m[15]["bytes_gathered"]
    assert m[-3]["samples"] == 0 and m[-2]["samples"] == 3 and m[-1]["samples_refused"] and m[-1]["bytes_gathered"]
    assert all(x["status"] == BX.OK for x in m)


def tile_file(n, seed, **options):
    """n samples of cenc_cases.tile_sizes(); a sample of 8 bytes or more has two entries (the first ends in a clear part of 3 bytes), every
    seventh none"""
    sizes = CC.tile_sizes(n, seed, options.pop("hollow", False))
    sizes[-1] = 40                          # (the last row, alone in its tile for 1025 and 2049 samples, has work)
    entries = [None if i % 7 == 0 or size < 8 else [(3, size - 8), (5, 0)] for i, size in enumerate(sizes)]
    return BC.build(sizes, layout=BC.split_layout(entries), seed=seed, **options)


@functools.lru_cache(maxsize=None)
def tile_job():
    """1025 and 2049 samples with subsample entries, so that the chain and the prefixes cross rows 1024 and 2048; 3077 of which tile 1
    holds no byte; short streams between them"""
    files = [tile_file(1025, 51, pattern=(1, 9), iv_size=8, key=BC.key_of(1), kid=BC.kid_of(1)),
             tile_file(2049, 52, scheme=BC.CENC, iv_size=16, runs_of=[[1019, 1030]], senc="front", key=BC.key_of(2), kid=BC.kid_of(2)),
             tile_file(3077, 53, hollow=True, counts=[1500, 1577], constant_iv=bytes(range(16)), pattern=(1, 1), key=BC.key_of(3), kid=BC.kid_of(3))]
    good = BC.named_good()
    short = [good["cbcs_edge_parts"], good["sibling_clear_plain_flac"], good["cenc_counts_0_1_2_3_17"]]
    streams = [BC.stream(short[0])]
    for k, m in enumerate(files):
        streams += [BC.stream(m), BC.stream(short[k])]
    streams += [BC.stream(files[1], gather_first_row=1025), BC.stream(files[1], sub_capacity=files[1].subsamples - 1), BC.stream(files[0], gather_first_row=1024)]
    job = BC.Job(streams, align=lambda i: (0, 1, 7, 14)[i % 4], dst_align=lambda i: (0, 3, 8, 15)[i // 2 % 4])
    job.files = files
    return job


def tile_units(model, f):
    """the work units of every tile of the stream's rows, restated from the muxer's record of the entries"""
    out = []
    ctr = f.scheme == BC.CENC
    for t in range(0, len(model["clear_rows"]), TILE):
        units = 0
        for row in range(t, min(t + TILE, len(model["clear_rows"]))):
            size = model["clear_rows"][row][1]
            used = 0
            for clear, prot in (f.entries[row] or [(0, size)]) if size or f.entries[row] else []:
                units += (clear + 15) // 16 + ((used % 16 + prot + 15) // 16 if ctr and prot else (prot + 15) // 16)
                used += prot
        out.append(units)
    return out


def assert_tiles(job):
    big = [job.models[i] for i in (1, 3, 5)]
    assert [m["samples_available"] for m in big] == [1025, 2049, 3077] and all(m["status"] == BX.OK for m in job.models)
    per_tile = [tile_units(m, f) for m, f in zip(big, job.files)]
    assert [len(t) for t in per_tile] == [2, 3, 4] and all(t[0] and t[-1] for t in per_tile) and per_tile[2][1] == 0 and per_tile[2][2]      # a tile with no work between two
    assert all(m["subsamples"] > 1024 for m in big)
    assert job.models[8]["samples_available"] == 2048 and job.models[8]["subsamples"] == job.files[1].subsamples - 2 and job.models[8]["bytes_gathered"]


@functools.lru_cache(maxsize=None)
def mixed_files():
    """seven small files a stream of which fits one chunk slot: `cbcs` whole and with entries under a pattern, `cenc` with entries and
    whole, a constant IV, a clear one -- under five keys"""
    out = [BC.build([16 * 5 + 3, 40], pattern=(1, 1), iv_size=16, layout=BC.split_layout([[(3, 16 * 5)], None]), seed=61, key=BC.key_of(11), kid=BC.kid_of(11)),
           BC.build([90, 33, 7], scheme=BC.CENC, iv_size=8, layout=BC.split_layout([[(5, 40), (5, 40)], [(0, 33)], None]), seed=62, key=BC.key_of(12), kid=BC.kid_of(12)),
           BC.build([48, 100], scheme=BC.CENC, iv_size=16, listed=False, seed=63, key=BC.key_of(13), kid=BC.kid_of(13)),
           BC.build([16 * 12, 20], constant_iv=bytes(range(8)), pattern=(1, 9), senc=None, seed=64, key=BC.key_of(14), kid=BC.kid_of(14)),
           BC.named_good()["sibling_clear_plain_flac"],
           BC.build([64, 17, 1], codec=BC.ALAC, iv_size=8, listed=False, seed=65, key=BC.key_of(15), kid=BC.kid_of(15)),
           BC.build([35, 36, 37], scheme=BC.CENC, codec=BC.ALAC, iv_size=8, layout=lambda i, size: [(i, size - i)], seed=66, key=BC.key_of(11), kid=BC.kid_of(11))]
    return out


@functools.lru_cache(maxsize=None)
def mixed_job():
    """one batch interleaving `cbcs`, `cenc` with entries, `cenc` without, clear, NO_KEY and malformed streams under five keys"""
    files, bad = mixed_files(), BC.named_malformed()
    wrong = [bad[name] for name in ("scheme_cens", "parts_below_the_sample", "constant_iv_of_4_bytes", "last_entry_leaves_the_senc")]
    streams = []
    for k in range(28):
        streams.append(BC.stream(files[k % 7], have_key=k % 5 != 4))
        if k % 6 == 2:
            data, _, _, codecs, have_key, kid = wrong[k // 6 % 4]
            streams.append(BC.stream(data, codecs=codecs, have_key=have_key, kid=kid))
    return BC.Job(streams)


def assert_mixed(job):
    statuses = [m["status"] for m in job.models]
    assert statuses.count(BX.NO_KEY) >= 4 and statuses.count(BX.INVALID) >= 2 and statuses.count(BX.UNSUPPORTED) >= 2 and statuses.count(BX.OK) >= 18
    ok = [m for m in job.models if m["status"] == BX.OK]
    assert len({m["kid"] for m in ok if m["is_protected"]}) == 5 and {m["scheme"] for m in ok} == {0, BX.code(b"cenc"), BX.code(b"cbcs")}
    assert any(m["subsamples"] for m in ok if m["scheme"] == BX.code(b"cenc")) and any(not m["subsamples"] and m["blocks"] for m in ok if m["scheme"] == BX.code(b"cenc"))


@functools.lru_cache(maxsize=None)
def damage_job():
    """150 files of fixed-seed damage, a stream each"""
    return BC.Job([BC.stream(data, capacity=80, run_capacity=4, dst_capacity=len(data), key=f.key, kid=f.kid, sub_capacity=150) for data, f in BC.damaged(150)])


def assert_damage(job):
    statuses = [m["status"] for m in job.models]
    assert statuses.count(BX.OK) >= 60 and statuses.count(BX.INVALID) >= 10 and statuses.count(BX.UNSUPPORTED) >= 3 and BX.NO_KEY in statuses, [statuses.count(s) for s in range(8)]


@functools.lru_cache(maxsize=None)
def many_trip_job(cus):
    """-> (Job, slots): a work list of at least TRIPS x W chunk slots for a device of `cus` CUs, W = 8 x 4 x cus the waves of the capped
    launch.  Streams of one slot over the seven files of mixed_files(): the stream at slot g takes file (g % W + 3 (g // W)) % 7, so the
    wave of residue g % W meets another file -- another schedule, and among any four of the seven another scheme -- on every trip.  In
    the third trip every 23rd stream has room for three slots of which one works: the waves that come to the other two jump.  The
    model runs once per distinct (file, capacities)."""
    files = mixed_files()
    W = CRYPT_GROUPS_PER_CU * CRYPT_WAVES * cus
    streams, models, cache, slots = [], [], {}, 0
    while slots < TRIPS * W + 3:
        r, trip = slots % W, slots // W
        k = (r + 3 * trip) % 7
        f = files[k]
        room = sum(f.sizes) + (16 * 2 * SLOT_UNITS if trip == 2 and r % 23 == 22 and r + 2 < W else 0)
        s = BC.stream(f, dst_capacity=room)
        key = (k, room)
        if key not in cache:
            cache[key] = BX.demux(s["data"], 3, s["capacity"], s["run_capacity"], 0, room, kid=s["kid"], key=s["key"], subsample_capacity=s["sub_capacity"])
        streams.append(s)
        models.append(cache[key])
        slots += (room // 16 + s["capacity"] + 3 * s["sub_capacity"] + SLOT_UNITS - 1) // SLOT_UNITS
    return BC.Job(streams, models=models), slots


def assert_trips(cus, job, slots):
    """every wave of the capped launch works in at least four slots, under two schemes and two keys or more, and some waves jump"""
    W = CRYPT_GROUPS_PER_CU * CRYPT_WAVES * cus
    per_slot = []
    for i, (d, m) in enumerate(zip(job.descs, job.models)):
        n = slots_of(d)
        assert n in (1, 3) and m["status"] == BX.OK and m["bytes_gathered"]
        per_slot += [(m["scheme"], m["kid"] if m["is_protected"] else None, k == 0) for k in range(n)]
    assert len(per_slot) == slots >= TRIPS * W and min((slots + CRYPT_WAVES - 1) // CRYPT_WAVES, CRYPT_GROUPS_PER_CU * cus) * CRYPT_WAVES == W
    jumps = 0
    for r in range(W):
        mine = per_slot[r::W]
        working = [x for x in mine if x[2]]
        assert len(working) >= 4 and len({x[0] for x in working}) >= 2 and len({x[1] for x in working} - {None}) >= 2, (r, mine)
        jumps += any(not x[2] for x in mine)
    assert jumps >= W // 16
