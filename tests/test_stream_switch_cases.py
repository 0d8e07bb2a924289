"""What makes tests/test_gpu_stream_switch.py able to fail, checked without a device: for each of the fifteen families whose batch keeps
per-run device records, the one set of tables of tests/stream_switch_cases.py passes the library's own validation, and the models'
answers for its two source arenas X and Y differ -- inside EVERY stream's output range of the destination arena, in the results of at
least one stream, and, for the families that give their tables (the three without a destination arena -- mp4, adts, raop_rx -- have
nothing else), in every table.  A run that met the other run's records, or bytes of the other arena, cannot come out right by accident.
Vorbis's PCM is held to its model within 1 LSB on the device: there "differ" means more than 2 LSB apart in a sample of the range."""
import numpy as np
import pytest

import stream_switch_cases as SC

TABLES = {"mp4": 2, "mp4f": 3, "cenc": 3, "cbcs": 3, "vorbis": 1, "ts": 1, "adts": 1, "raop_rx": 2}       # how many tables a family's model gives
LSB_APART = 2                                                                                           # (the device's tolerance is 1 LSB to either side of the model)


def test_fifteen_families():
    assert len(SC.FAMILIES) == len(set(SC.FAMILIES)) == 15 and set(SC.BOTH_ROUTES) <= set(SC.FAMILIES)


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_the_tables_pass_the_librarys_check(family):
    p = SC.pair(family)
    p.check()                                                          # (raises OhGpuError on a bad table; the arenas' sizes are both runs')
    assert p.src["X"].size == p.src["Y"].size > 0 and not np.array_equal(p.src["X"], p.src["Y"])


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_x_and_y_differ_in_every_streams_output(family):
    p = SC.pair(family)
    if p.tables is not None or family in TABLES:
        assert len(p.tables["X"]) == len(p.tables["Y"]) == TABLES[family] and all(x != y for x, y in zip(p.tables["X"], p.tables["Y"]))
    if p.dst0 is None:
        assert family in ("mp4", "adts", "raop_rx")
        return
    x, y = p.want["X"], p.want["Y"]
    assert x.size == y.size == p.dst0.size and 2 <= len(p.ranges) <= 4
    assert p.sample_types is None or len(p.sample_types) == len(p.ranges)
    covered = np.zeros(x.size, dtype=bool)
    for k, (off, n) in enumerate(p.ranges):
        assert n > 0 and off + n <= x.size and not covered[off:off + n].any()
        covered[off:off + n] = True
        if p.sample_types is None:
            assert np.any(x[off:off + n] != y[off:off + n]), (family, off, n)
        else:
            xs, ys = (a[off:off + n].view(p.sample_types[k]).astype(np.int64) for a in (x, y))
            assert np.abs(xs - ys).max() > LSB_APART, (family, off, n)
            for w in "XY":                                             # what a run writes lies inside the ranges, and is not the fill throughout
                assert p.written[w][off:off + n].any() and np.any(p.want[w][off:off + n][p.written[w][off:off + n]] != p.dst0[off:off + n][p.written[w][off:off + n]])
        assert np.any(x[off:off + n] != p.dst0[off:off + n]) or np.any(y[off:off + n] != p.dst0[off:off + n]), (family, off, n)
    assert np.array_equal(x[~covered], p.dst0[~covered]) and np.array_equal(y[~covered], p.dst0[~covered])      # the guards stay the fill
    assert covered.sum() < x.size
    if p.written is not None:
        for w in "XY":
            assert not p.written[w][~covered].any() and np.array_equal(p.want[w][~p.written[w]], p.dst0[~p.written[w]])


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_the_results_differ(family):
    p = SC.pair(family)
    assert p.summary["X"] != p.summary["Y"]
