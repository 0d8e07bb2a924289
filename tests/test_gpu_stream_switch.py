"""A decoder's or demultiplexer's batch on streams other than the context's own, for the fifteen families whose batch keeps per-run
device records (flac, alac, raop, ohm_rx, ogg, mp4, iff, dsd_file; mp4f, cenc, cbcs, vorbis, ts, adts, raop_rx: counters, candidate and
piece lists, records, row tables, scratch rows).  Their runs never
refuse a stream: a run on another stream than the last one's first waits, on the host, for the batch's last run (run_begin,
csrc/api_common.h) -- on the event that run recorded at its end, because the earlier stream may have been destroyed by then.

One batch and two source arenas X and Y per family (tests/stream_switch_cases.py; tests/test_stream_switch_cases.py shows on the CPU
that every stream's output differs between the two): a run that met the other run's records, or a wait that was left out, cannot give
the model's bytes by accident.  The WHOLE destination arenas are compared with the models', the results and tables too -- the whole
tables of the seven newer families, so that a row run X wrote and run Y does not must be back at the table's fill.  Everything is exact
but Vorbis's PCM, which tests/test_gpu_vorbis_textbook.py bounds at 1 LSB from the model: there every byte a run does not write is
compared exactly, every sample within 1 LSB, the spectra bit for bit, and every later run over X with the first one byte for byte.
The seven newer families run on both routes: the launches, and the plain route (kernel variant 1 at create), whose per-run state is
its own."""
import gc
import time

import numpy as np
import pytest

import stream_switch_cases as SC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

FILL_BYTES, FILL_COPIES = 256 << 20, 4       # what keeps stream A busy while run Y is issued: 1 GiB from pinned memory (see the first test)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scratch(ctx):
    """(device block, pinned host block) of FILL_BYTES each: a copy from pinned memory is queued, the call returns at once"""
    dev, host = ctx.malloc(FILL_BYTES), ctx.malloc_host(FILL_BYTES)
    host[:] = 0x3C
    yield dev, host
    ctx.free(dev)
    ctx.free_host(host)


class Rig:
    """One family's batch, both source arenas and a destination arena for each on the device, two streams of the caller's.  variant:
    None -- the batch is created as the context stands --, or the kernel variant it is created under (0: the launches, 1: the plain
    route, which keeps per-run state of its own), asserted through the family's own paths call; the context is back at 0 afterwards."""

    def __init__(self, ctx, family, variant=None):
        self.ctx, self.p = ctx, SC.pair(family)
        p = self.p
        p.check()
        self.d_src = {w: ctx.upload(p.src[w]) for w in "XY"}
        self.d_dst = {w: ctx.upload(p.dst0) if p.dst0 is not None else None for w in "XY"}
        if variant is None:
            self.batch = p.create(ctx)
        else:
            ctx.set_kernel_variant(variant)
            try:
                self.batch = p.create(ctx)
            finally:
                ctx.set_kernel_variant(0)
            assert p.route(ctx, self.batch) == (2 if variant else 1)
        self.streams = {"A": ctx.stream_create(), "B": ctx.stream_create()}
        self.label = family + {None: "", 0: " (launches)", 1: " (plain)"}[variant]
        self.first_x = None                      # (Vorbis: the arena of the first checked run over X)

    def refill(self, which):
        if self.p.dst0 is not None:
            self.ctx.copy_h2d(self.d_dst[which], self.p.dst0)
            self.ctx.sync()

    def run(self, which, stream):
        self.p.run(self.ctx, self.batch, self.d_src[which], self.d_dst[which], stream)

    def arena_is_the_models(self, which):
        if self.p.dst0 is None:
            return
        p = self.p
        got, want = self.ctx.download(self.d_dst[which], p.dst0.size), p.want[which]
        if p.sample_types is None:
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"arena {which}: {bad.size} of {want.size} bytes differ, the first at {bad[:8].tolist()}"
            return
        # Vorbis: every byte the model does not write is the fill, exactly; inside a stream's range the samples lie within 1 LSB
        bad = np.flatnonzero((got != want) & ~p.written[which])
        assert bad.size == 0, f"arena {which}: {bad.size} bytes differ that the run does not write, the first at {bad[:8].tolist()}"
        for (off, n), kind in zip(p.ranges, p.sample_types):
            mine, model = (a[off:off + n].view(kind).astype(np.int64) for a in (got, want))
            worst = int(np.abs(mine - model).max())
            assert worst <= 1, f"arena {which}, the range at {off}: a sample {worst} LSB from the model's"
        return got

    def checked(self, which, stream):
        """a run from a fresh arena, waited for and compared: the arena, the results, the tables"""
        self.refill(which)
        self.run(which, stream)
        self.ctx.sync(stream)
        got = self.arena_is_the_models(which)
        self.p.verify(self.ctx, self.batch, which)
        if got is not None and which == "X":     # (beside the model, not in its place: a run over X writes what the first one wrote)
            if self.first_x is None:
                self.first_x = got
            assert np.array_equal(got, self.first_x), "a later run over X wrote other bytes than the first"

    def destroy_stream(self, name):
        self.ctx.stream_destroy(self.streams.pop(name))

    def close(self):
        ctx = self.ctx
        ctx.batch_destroy(self.batch)
        for s in self.streams.values():
            ctx.stream_destroy(s)
        for d in list(self.d_src.values()) + list(self.d_dst.values()):
            if d is not None:
                ctx.free(d)


@pytest.fixture
def rig(ctx, request):
    r = Rig(ctx, *request.param)
    yield r
    r.close()


def _cases():
    """the first eight families as they were; the newer ones on both routes"""
    out = []
    for family in SC.FAMILIES:
        if family in SC.BOTH_ROUTES:
            out += [pytest.param((family, 0), id=f"{family}-launches"), pytest.param((family, 1), id=f"{family}-plain")]
        else:
            out.append(pytest.param((family, None), id=family))
    return out


families = pytest.mark.parametrize("rig", _cases(), indirect=True)


@families
def test_a_run_on_another_stream_waits_for_the_last(ctx, scratch, rig):
    """A fill is queued on stream A, run X behind it, and AT ONCE run Y on stream B: run X has not finished (for every family but
    FLAC not begun) when run Y is issued, so run Y's first launches -- which clear the counters and overwrite the records run X works
    with -- would meet it, were it not for the host's wait at the top of run Y.  Both arenas must be the models', and the batch's
    results and tables those of run Y, the last.

    The fill proves nothing unless it outlasts the host's way to run Y: the interval on the device (an event in front of the fill,
    one behind run X) must be longer than the host's (from before the first event record to just before the call of run Y), or the
    test fails.  MPEG-4, ADTS and the RAOP receiver have no destination arena: their tables are read after each of the two waits, and
    are run Y's both times.

    The fill is four copies of 256 MiB from pinned memory, each a call of 5 us that keeps the stream busy for 4.7 ms.  A device fill
    (ohgpu_memset) does not do: measured on an MI355X, 1 GiB of it is over in 0.16 ms, while the host needs 0.65-0.8 ms to issue
    run X when the family's kernels have not run in the process yet (and a tenth of that when they have).  Measured once, in that
    cold state and with ONE copy of 256 MiB (host / device interval, ms): alac 0.65 / 5.47, raop 0.69 / 5.50, ohm_rx 0.67 / 4.74,
    ogg 0.68 / 4.75, mp4 0.81 / 4.78, iff 0.66 / 4.73 -- less than ten times, hence four copies; with the four, inside the whole
    suite: alac 0.08 / 19.5, raop 0.09 / 19.6, ohm_rx 0.07 / 18.8, ogg 0.10 / 18.8, mp4 0.11 / 18.9, iff 0.06 / 18.8.  The seven newer
    families, measured with the four copies, on the launches' route and then the plain one.  Cold (this file first in the process; the
    plain route comes second, adts behind ts, whose code object it shares): mp4f 0.82 / 18.9 and 0.07 / 20.0, cenc 0.81 / 19.2 and
    0.09 / 19.0, cbcs 0.89 / 19.1 and 0.08 / 19.3, vorbis 0.75 / 28.9 and 0.09 / 29.1, ts 0.77 / 18.8 and 0.07 / 18.9, adts 0.07 / 18.8
    and 0.07 / 18.8, raop_rx 0.66 / 19.0 and 0.09 / 18.8 -- no host interval above a twentieth of the device's, so the four copies stay.
    Inside the whole suite: mp4f 0.11 / 18.9 and 0.10 / 20.0, cenc 0.13 / 19.2 and 0.09 / 19.0, cbcs 0.13 / 19.1 and 0.09 / 19.3,
    vorbis 0.13 / 30.4 and 0.12 / 29.4, ts 0.12 / 18.8 and 0.09 / 18.9, adts 0.11 / 18.8 and 0.09 / 18.8, raop_rx 0.10 / 18.8 and
    0.10 / 18.8.  FLAC is
    another matter: its run waits on the host for the scan, so its host interval holds the fill whatever the fill's size (19.0 / 35.2;
    4.85 / 21.2 with one copy), and what is still running when run Y is issued is what run X queued behind that wait, the probe and
    restoration of frames of 4096 samples (tests/stream_switch_cases.py).  With run_begin's wait taken out of a scratch build, once,
    the test failed for all seven families there were then: FLAC's arena X came out wrong, the other six held run X's results at
    the end.  (No such build was run for the families added since: records that race can index out of bounds.)"""
    r, a, b = rig, rig.streams["A"], rig.streams["B"]
    e0, e1 = ctx.event(), ctx.event()
    r.refill("X")
    r.refill("Y")
    ctx.sync(a)
    ctx.sync(b)
    gc.disable()
    try:
        t0 = time.perf_counter()
        ctx.record(e0, a)
        for _ in range(FILL_COPIES):
            ctx.copy_h2d(scratch[0], scratch[1], stream=a)
        r.run("X", a)
        ctx.record(e1, a)
        t1 = time.perf_counter()
        r.run("Y", b)
    finally:
        gc.enable()
    ctx.sync(a)
    if r.p.dst0 is None:
        r.p.verify(ctx, r.batch, "Y")
    ctx.sync(b)
    host_ms, device_ms = (t1 - t0) * 1e3, ctx.elapsed_ms(e0, e1)
    ctx.event_destroy(e0)
    ctx.event_destroy(e1)
    print(f"\n{r.label}: host interval {host_ms:.3f} ms, device interval {device_ms:.3f} ms")
    r.arena_is_the_models("X")
    r.arena_is_the_models("Y")
    r.p.verify(ctx, r.batch, "Y")
    assert host_ms < device_ms, f"run X was over before run Y was issued ({host_ms:.3f} ms on the host, {device_ms:.3f} ms on the device): nothing was shown"


@families
def test_the_earlier_stream_may_be_gone(ctx, rig):
    """Run X on stream A, wait for A, destroy A: run Y on stream B must not ask anything of A's handle.  It returns OK (capi raises
    otherwise) and matches the model, and so does run X on the context's own stream after it; neither allocates on the device."""
    r = rig
    r.checked("X", r.streams["A"])
    r.destroy_stream("A")
    r.checked("Y", r.streams["B"])
    allocs = ctx.device_allocations()
    r.checked("X", None)
    assert ctx.device_allocations() == allocs


@families
def test_back_and_forth_allocates_nothing(ctx, rig):
    r = rig
    allocs = []
    for which, name in (("X", "A"), ("Y", "B"), ("X", "A")):
        r.checked(which, r.streams[name])
        allocs.append(ctx.device_allocations())
    assert allocs[1] == allocs[2], allocs
