"""The builders of tests/cenc_cases.py that the device tests lean on, without a device: the files of more than one tile hold what
their docstrings say, the model reads back the muxer's own record of them, and the work list of many_trip_job meets every condition
of tests/test_gpu_cenc_textbook.py's trip test at assumed CU counts of 1, 8, 256 and 304 -- so that the references alone are shown
to reach the paths before anything goes to a GPU, and a builder that changes fails here first.

The conditions on the work list, W = trip_waves(cus) = max(8 x 4, 32 resident) x CUs waves:
  1. the slot count by the documented rule is the builder's, it is 3 W + 67 at the least, and the launch -- min(ceil(slots / 4),
     8 CUs) workgroups of four waves -- is capped;
  2. every residue mod W has two working slots and more, two of them of protected streams under different keys; in a quarter of the
     residues and more a clear working slot lies between two protected ones (met at 38 to 62 in a hundred under TRIP_SEED);
  3. W / 8 waves and more meet a slot that does not work and a working one later: they jump and then do real work;
  4. the list has no period and the four waves of a workgroup meet different streams, keys and a clear stream in one trip.
Building the list for 256 CUs (33 740 streams, 41 027 slots, a source arena of 30 MB and a destination arena of 12 MB) takes 2.3 s."""
import numpy as np
import pytest

import cenc_cases as CC
import cenc_textbook as CX

CUS = [1, 8, 256, 304]
TILE = CC.TILE


def test_files_of_more_than_one_tile_hold_what_they_are_for():
    files = CC.multi_tile_files()
    assert CC.multi_tile_files() is files and CC.multi_tile_jobs() is CC.multi_tile_jobs()          # made once
    assert sorted(m.n for m in files.values())[:6] == list(CC.TILE_COUNTS[:6]) and {m.n for m in files.values()} == set(CC.TILE_COUNTS)
    for name, m in files.items():
        assert set(m.sizes) <= set(CC.EDGE_SIZES) | set(CC.RARE_SIZES), name
        assert 2 <= sum(1 for s in m.sizes if s in CC.RARE_SIZES) <= 12, name                       # rare: the model's AES is scalar Python
        assert all(m.sizes[row] == 0 for row in (TILE - 1, TILE) if row < m.n), name
        if m.n > TILE + 2:
            assert {s for s in m.sizes[TILE:] if s in CC.RARE_SIZES} == set(CC.RARE_SIZES) or "empty" in name, name
    hollow = files["samples_3077_tile_1_empty"]
    assert not any(hollow.sizes[TILE:2 * TILE]) and any(hollow.sizes[:TILE]) and any(hollow.sizes[2 * TILE:3 * TILE]) and any(hollow.sizes[3 * TILE:])
    two = files["samples_2049_two_truns_under_one_senc"]
    assert [(r[2], r[3]) for r in two.runs] == [(0, 1019), (1019, 1030)] and len([x for x in two.marks if x[0].endswith("/senc")]) == 1
    many = files["samples_3077_fragments_of_700"]
    assert [r[3] for r in many.runs] == [703, 689, 711, 697, 277] and len([x for x in many.marks if x[0].endswith("/senc")]) == 5
    # a tile holds the end of one run and the start of the next: a run begins inside tiles 1 and 2, far from the run's first sample
    assert {r[2] // TILE for r in many.runs[1:]} >= {1, 2} and all(r[2] % TILE for r in many.runs[1:])
    protected = [m for m in files.values() if m.protected]
    assert len({m.key for m in protected}) >= 3 and {len(m.ivs[0]) for m in protected} == {8, 16} and len(protected) == len(files) - 2
    assert {m.codec for m in files.values()} == {CC.FLAC, CC.ALAC}


def test_the_model_reads_back_the_muxers_record_of_every_big_file():
    for name, job in CC.multi_tile_jobs().items():
        CC.assert_reaches(name, job)
    job = CC.multi_tile_jobs()["every_count"]
    for i, m in zip(job.big, CC.multi_tile_files().values()):
        model = job.models[i]
        assert model["gathered"] == b"".join(m.clear) and [size for _, size in model["clear_rows"]] == m.sizes
        assert model["run_rows"] == m.runs and model["blocks"] == (sum((s + 15) // 16 for s in m.sizes) if m.protected else 0)
        assert bytes(job.src[int(job.descs[i]["src_offset"]):][:len(m.data)]) == m.data
        if m.protected:                                                                             # the file itself holds other bytes than the clear ones
            assert b"".join(m.data[o:o + s] for o, s in zip(m.offsets, m.sizes)) != model["gathered"]
    # a descriptor that starts behind row 0 gathers the tail of the same clear bytes
    job = CC.multi_tile_jobs()["descriptors"]
    whole = {m.data: b"".join(m.clear) for m in CC.multi_tile_files().values()}
    sizes = {m.data: m.sizes for m in CC.multi_tile_files().values()}
    seen = 0
    for i in job.big:
        s, model = job.streams[i], job.models[i]
        if s["data"] in whole and model["bytes_gathered"]:
            skip = sum(sizes[s["data"]][:s["gather_first_row"]])
            assert model["gathered"] == whole[s["data"]][skip:skip + model["bytes_gathered"]]
            seen += 1
    assert seen >= 18


def test_the_pool_of_the_work_list():
    small, medium, big = CC.trip_pool()
    assert len(small) == 16 and all(1 <= m.n <= 4 and sum((s + 15) // 16 for s in m.sizes) <= 32 for m in small)
    protected = [m for m in small if m.protected]
    assert len(protected) == 12 and len({m.key for m in protected}) == 12 == len({m.kid for m in protected}) and {len(m.ivs[0]) for m in protected} == {8, 16}
    assert len({m.data for m in small + medium + big}) == 21 and {m.codec for m in small} == {CC.FLAC, CC.ALAC}
    assert any(b"enca" in m.data for m in small if not m.protected) and any(b"enca" not in m.data for m in small if not m.protected)
    blocks = [sum((s + 15) // 16 for s in m.sizes) for m in medium + big]
    assert all(64 < b <= 128 for b in blocks[:2]) and all(130 <= b <= 200 for b in blocks[2:]) and blocks[-1] > 192 >= blocks[-2]
    assert len({m.key for m in protected + [m for m in medium + big if m.protected]}) == 15


@pytest.mark.parametrize("cus", CUS)
def test_the_work_list_outgrows_the_launch(cus):
    job, slots, per_slot = CC.many_trip_job(cus)
    assert CC.many_trip_job(cus)[0] is job                                                          # made once
    c = CC.assert_trips(cus, job, slots, per_slot)                                                  # items 1 and 2
    W = c["W"]
    assert W == 32 * cus and slots >= CC.TRIPS * W + 67
    assert c["clear_between"] >= W * 3 // 8                                                         # (a quarter is the condition: room to spare)
    assert c["jumps"] >= W // 8                                                                     # item 3
    # item 4: no constant difference and no period in chunk_first; a workgroup's four waves in different streams in one trip
    steps = np.diff(c["chunk_first"])
    assert int(c["chunk_first"][-1]) == slots and len(set(steps.tolist())) >= (6 if cus >= 8 else 3)
    assert not any(np.array_equal(steps[q:], steps[:-q]) for q in list(range(1, 4097)) + [W, 2 * W] if q <= steps.size // 2)
    several = sorted({int(v) for v in steps if v > 1})
    assert all(W % v and v % W for v in several) and (cus < 256 or (several[0] == 3 and several[-1] >= 30)), several
    assert c["mixed_groups"] >= W // 8 and c["mixed_with_clear"] >= W // 16
    boundaries = c["chunk_first"][1:-1]
    assert int((boundaries % 4 != 0).sum()) >= boundaries.size // 2                                 # streams end and begin inside a workgroup's four slots
    # the streams by the number of their slots that work
    working, total = {}, {}
    for i, works, _ in per_slot:
        working[i], total[i] = working.get(i, 0) + works, total.get(i, 0) + 1
    jumpers = [i for i in total if total[i] > working[i]]
    assert len(jumpers) >= slots // 80 and {1} <= {working[i] for i in jumpers} <= {1, 2, 4} and {1} <= {working[i] for i in total if total[i] == working[i]} <= {1, 3}
    assert cus < 256 or ({working[i] for i in jumpers} == {1, 2, 4} and 3 in {working[i] for i in total if total[i] == working[i]})      # three and four slots filled in a row
    assert all(m["status"] == CX.OK and m["bytes_gathered"] for m in job.models)
    assert len({id(m) for m in job.models}) <= 700 and len(job.models) == len(job.streams) >= slots // 2          # the model ran some hundred times
    # the working flags against the rows the model gathers, stream by stream: slot k works when 64 k < B
    for i in jumpers[:50] + list(range(0, len(job.streams), 997)):
        blocks = sum((size + 15) // 16 for _, size in job.models[i]["clear_rows"])
        assert working[i] == min(total[i], (blocks + 63) // 64) and total[i] == CC.slots_of(int(job.descs[i]["dst_capacity"]), int(job.descs[i]["packet_capacity"]))
    assert job.src.size < 48 << 20 and job.dst_bytes < 24 << 20
