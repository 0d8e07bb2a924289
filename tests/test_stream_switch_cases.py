"""What makes tests/test_gpu_stream_switch.py able to fail, checked without a device: for each of the eight families whose batch keeps
per-run device records, the one set of tables of tests/stream_switch_cases.py passes the library's own validation, and the models'
answers for its two source arenas X and Y differ -- inside EVERY stream's output range of the destination arena, in the results of at
least one stream, and for MPEG-4 (which has no destination arena) in both tables.  A run that met the other run's records, or bytes of
the other arena, cannot come out right by accident."""
import numpy as np
import pytest

import stream_switch_cases as SC


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_the_tables_pass_the_librarys_check(family):
    p = SC.pair(family)
    p.check()                                                          # (raises OhGpuError on a bad table; the arenas' sizes are both runs')
    assert p.src["X"].size == p.src["Y"].size > 0 and not np.array_equal(p.src["X"], p.src["Y"])


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_x_and_y_differ_in_every_streams_output(family):
    p = SC.pair(family)
    if p.dst0 is None:
        assert family == "mp4" and all(x != y for x, y in zip(p.tables["X"], p.tables["Y"])) and len(p.tables["X"]) == 2
        return
    x, y = p.want["X"], p.want["Y"]
    assert x.size == y.size == p.dst0.size and 2 <= len(p.ranges) <= 4
    covered = np.zeros(x.size, dtype=bool)
    for off, n in p.ranges:
        assert n > 0 and off + n <= x.size and not covered[off:off + n].any()
        covered[off:off + n] = True
        assert np.any(x[off:off + n] != y[off:off + n]), (family, off, n)
        assert np.any(x[off:off + n] != p.dst0[off:off + n]) or np.any(y[off:off + n] != p.dst0[off:off + n]), (family, off, n)
    assert np.array_equal(x[~covered], p.dst0[~covered]) and np.array_equal(y[~covered], p.dst0[~covered])      # the guards stay the fill
    assert covered.sum() < x.size


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_the_results_differ(family):
    p = SC.pair(family)
    assert p.summary["X"] != p.summary["Y"]
