"""The shell the three lossless decoder families of the C ABI share (ohgpu_flac_*, ohgpu_alac_*, ohgpu_raop_*: csrc/api_common.h),
where tests/test_gpu_batch_lifecycle.py and tests/test_gpu_alac_lifecycle.py do not reach: what the results and the phase times say
of a batch that has not run, what the results say of a wrong count, that a host-buffer call with a null buffer is refused before it
counts as a call, and what a RAOP host-buffer call moves over the link.  Every expectation was first observed on the library as it
was while each family had a shell of its own: the file pins that behaviour, not the sharing.

The batches are the smallest there are:

    flac   tests/golden/flac_decode/tiny_s16_stereo_44k1_b16.flac, one stream
    alac   tests/alac_cases.handmade: hand_stereo8 -- one stereo packet of eight samples, frame length 64, planes
    raop   two streams: that packet encrypted under a fixed key and IV, planes; and a PLAINTEXT stream of payloads of 20, 0 and 12
           bytes (one block with a tail, nothing, a tail only)

The same three pins for the families that came behind the shared shell and keep three tables or a spectrum beside their results:

    mp4f, cenc, cbcs   one gathered file of three samples in one run (tests/mp4f_cases.py, cenc_cases.py, cbcs_cases.py); the run, packet
           and sample tables are each asked for before a run and with a wrong count
    vorbis tests/vorbis_cases.py's mono_64_128, packets [0, 4); ohgpu_vorbis_batch_spectrum before a run and out of range"""
import ctypes as C

import numpy as np
import pytest

import alac_cases as AC
import alac_textbook as T
import cbcs_cases as BC
import cenc_cases as CC
import flac_cases as FC
import mp4f_cases as MF
import raop_cases as RC
import raop_textbook as R
import vorbis_cases as VC
import vorbis_frames as VF
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

FRAGMENTED = ("mp4f", "cenc", "cbcs")
FAMILIES = ("flac", "alac", "raop") + FRAGMENTED + ("vorbis",)
KEY, IV = bytes(range(16)), bytes(range(16, 32))
KEY2, IV2 = bytes(range(32, 48)), bytes(range(48, 64))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class Case:
    """One batch: `head` = the arguments between the context and the source (create: the arena sizes), `counts` = (streams, packets)
    (FLAC: (streams,)), the source arena and the destination arena's size."""

    def __init__(self, family, head, keep, counts, src, dst_bytes, tables=()):
        self.family, self.head, self.keep, self.counts, self.src, self.dst_bytes = family, head, keep, counts, src, dst_bytes
        self.tables = tables                    # the fragmented families: (the call's suffix, the row type, the batch's row count) of results, runs, packets, samples


class Fixtures:
    def __init__(self):
        self.ctx = capi.Context(0)
        cookie, (packet,) = AC.handmade()["hand_stereo8"]
        cfg = T.parse_config(cookie)
        assert (cfg["channels"], cfg["frame_length"]) == (2, 64)
        self.cases = {"flac": self._flac(FC.whole(FC.fixture("tiny_s16_stereo_44k1_b16"))), "alac": self._alac(cfg, packet)}
        self.job = RC.Job([RC.stream(KEY, IV, [R.encrypt_packet(KEY, IV, packet)], T.PLANAR, cfg),
                           RC.stream(KEY2, IV2, [bytes(range(100, 120)), b"", bytes(range(200, 212))])])
        descs, packets = RC.capi_tables(self.job)
        self.cases["raop"] = Case("raop", (_ptr(descs), descs.size, _ptr(packets), packets.size), [descs, packets], (descs.size, packets.size),
                                  np.frombuffer(self.job.src, dtype=np.uint8), len(self.job.dst0))

        for family, job, result in (("mp4f", MF.Job([MF.stream(MF.simple([3]))]), capi.MP4F_STREAM_RESULT), ("cenc", CC.Job([CC.stream(CC.simple([3]))]), capi.CENC_STREAM_RESULT),
                                    ("cbcs", BC.Job([BC.stream(BC.build([40, 50, 64], iv_size=16, listed=False))]), capi.CBCS_STREAM_RESULT)):
            head = (_ptr(job.descs), 1, job.n_packets, job.n_runs) + ((job.n_subsamples,) if family == "cbcs" else ())
            tables = (("results", result, 1), ("runs", capi.MP4F_RUN, job.n_runs), ("packets", capi.ALAC_PACKET, job.n_packets), ("samples", capi.MP4_SAMPLE, job.n_packets))
            self.cases[family] = Case(family, head, [job.descs], (1, job.n_packets, job.n_runs), job.src, job.dst_bytes, tables)
        blob, descs, packets, src, dst_bytes, _ = VF.batch_tables(capi, [VC.stream("mono_64_128")], ranges=[(0, 4)])
        self.cases["vorbis"] = Case("vorbis", (_ptr(descs), 1, _ptr(packets), packets.size, _ptr(blob), blob.size), [descs, packets, blob], (1, packets.size), src, dst_bytes)

    def close(self):
        self.ctx.close()

    def _flac(self, c):
        d = np.zeros(1, dtype=capi.FLAC_STREAM_DESC)
        audio = np.frombuffer(c.data[c.offset:c.offset + c.src_bytes], dtype=np.uint8)
        d["src_bytes"], d["dst_plane_stride"], d["first_sample"], d["max_samples"] = audio.size, c.max_samples * 4, c.first_sample, c.max_samples
        d["sample_rate"], d["blocksize"], d["max_blocksize"], d["channels"], d["bits"], d["flags"] = c.rate, c.blocksize, c.max_blocksize, c.channels, c.bits, c.flags
        return Case("flac", (_ptr(d), 1), [d], (1,), audio.copy(), FC.arena_bytes(c))

    def _alac(self, cfg, packet):
        d, p = np.zeros(1, dtype=capi.ALAC_STREAM_DESC), np.zeros(1, dtype=capi.ALAC_PACKET)
        for k in ("frame_length", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "sample_rate"):
            d[k] = cfg[k]
        d["n_packets"], d["dst_plane_stride"], p["bytes"] = 1, cfg["frame_length"] * 4, len(packet)
        return Case("alac", (_ptr(d), 1, _ptr(p), 1), [d, p], (1, 1), np.frombuffer(packet, dtype=np.uint8), 2 * cfg["frame_length"] * 4)

    def create(self, family):
        case = self.cases[family]
        b = C.c_void_p()
        capi.check(getattr(capi.lib(), f"ohgpu_{family}_batch_create")(self.ctx.handle, *case.head, case.src.size, case.dst_bytes, C.byref(b)))
        return case, b

    def results(self, family, batch, counts):
        """ohgpu_<family>_batch_results with room for `counts` results -> the library's code"""
        if family == "flac":
            res = np.zeros(counts[0], dtype=capi.FLAC_STREAM_RESULT)
            return capi.lib().ohgpu_flac_batch_results(self.ctx.handle, batch, _ptr(res), res.size)
        if family in FRAGMENTED:
            return self.fetch(family, batch, "results", self.cases[family].tables[0][1], counts[0])
        kinds = (capi.VORBIS_STREAM_RESULT, capi.VORBIS_PACKET_RESULT) if family == "vorbis" else (capi.ALAC_STREAM_RESULT, capi.ALAC_PACKET_RESULT)
        sres, pres = np.zeros(counts[0], dtype=kinds[0]), np.zeros(counts[1], dtype=kinds[1])
        return getattr(capi.lib(), f"ohgpu_{family}_batch_results")(self.ctx.handle, batch, _ptr(sres), sres.size, _ptr(pres), pres.size)

    def fetch(self, family, batch, suffix, kind, count):
        """ohgpu_<family>_batch_<suffix> with room for `count` rows -> the library's code"""
        rows = np.zeros(count, dtype=kind)
        return getattr(capi.lib(), f"ohgpu_{family}_batch_{suffix}")(self.ctx.handle, batch, _ptr(rows), rows.size)

    def spectrum(self, batch, packet, channel, n_values):
        out = np.zeros(max(n_values, 1), dtype=np.float32)
        return capi.lib().ohgpu_vorbis_batch_spectrum(self.ctx.handle, batch, packet, channel, _ptr(out), n_values)


@pytest.fixture(scope="module")
def fx():
    f = Fixtures()
    yield f
    f.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_a_batch_that_has_not_run(fx, family):
    case, b = fx.create(family)
    try:
        assert fx.results(family, b, case.counts) == capi.ERR_INVALID
        assert capi.last_error() == f"ohgpu_{family}_batch_results: the batch has not run"
        ms = (C.c_float * 8)()                                        # (the families have three to six phases)
        assert getattr(capi.lib(), f"ohgpu_{family}_batch_phase_ms")(fx.ctx.handle, b, ms) == capi.ERR_INVALID
        assert capi.last_error() == f"ohgpu_{family}_batch_phase_ms: the batch has not run"
        for suffix, kind, count in case.tables:                       # every table of its own
            assert count > 0 and fx.fetch(family, b, suffix, kind, count) == capi.ERR_INVALID
            assert capi.last_error() == f"ohgpu_{family}_batch_{suffix}: the batch has not run"
        if family == "vorbis":                                        # a mono stream of four packets, rows of 64 values
            assert fx.spectrum(b, 0, 0, 32) == capi.ERR_INVALID
            assert capi.last_error() == "ohgpu_vorbis_batch_spectrum: the batch has not run"
            assert fx.spectrum(b, 4, 0, 32) == capi.ERR_INVALID
            assert capi.last_error() == "ohgpu_vorbis_batch_spectrum: packet 4 of 4"
            assert fx.spectrum(b, 0, 1, 32) == capi.ERR_INVALID
            assert capi.last_error() == "ohgpu_vorbis_batch_spectrum: channel 1, 32 values (the stream has 1 channels and rows of 64)"
            assert fx.spectrum(b, 0, 0, 65) == capi.ERR_INVALID
            assert capi.last_error() == "ohgpu_vorbis_batch_spectrum: channel 0, 65 values (the stream has 1 channels and rows of 64)"
    finally:
        fx.ctx.batch_destroy(b)


@pytest.mark.parametrize("family", FAMILIES)
def test_results_with_a_wrong_count(fx, family):
    case, b = fx.create(family)
    try:
        assert fx.results(family, b, (case.counts[0] + 1,) + case.counts[1:]) == capi.ERR_INVALID
        assert "room for" in capi.last_error(), capi.last_error()
        for suffix, kind, count in case.tables:                       # a row too many, a row too few: each table says what it has
            for wrong in (count + 1, count - 1):
                assert fx.fetch(family, b, suffix, kind, wrong) == capi.ERR_INVALID
                noun = "results, the batch has 1 streams" if suffix == "results" else f"rows, the batch's table has {count}"
                assert capi.last_error() == f"ohgpu_{family}_batch_{suffix}: room for {wrong} {noun}", capi.last_error()
        if family == "vorbis":
            assert fx.results(family, b, (case.counts[0], case.counts[1] - 1)) == capi.ERR_INVALID
            assert capi.last_error() == "ohgpu_vorbis_batch_results: room for 3 packet results, the batch has 4 packets"
    finally:
        fx.ctx.batch_destroy(b)


@pytest.mark.parametrize("family", FAMILIES)
def test_process_host_with_a_null_buffer(fx, family):
    case = fx.cases[family]
    dst = np.zeros(case.dst_bytes, dtype=np.uint8)
    tail = (None, None, 0, None) if family == "flac" else (None,) * 4 if family in FRAGMENTED else (None, None)
    before = fx.ctx.host_transfer_stats()
    code = getattr(capi.lib(), f"ohgpu_{family}_process_host")(fx.ctx.handle, *case.head, None, case.src.size, _ptr(dst), dst.size, *tail)
    assert case.src.size > 0 and code == capi.ERR_INVALID
    assert capi.last_error() == f"ohgpu_{family}_process_host: null buffer"
    assert fx.ctx.host_transfer_stats() == before


def test_raop_process_host_moves_what_was_decoded_and_the_payloads(fx):
    job, case = fx.job, fx.cases["raop"]
    descs, packets = case.keep
    dst = np.frombuffer(job.dst0, dtype=np.uint8).copy()
    before = fx.ctx.host_transfer_stats()
    sres, pres = fx.ctx.raop_process_host(descs, packets, case.src, dst)
    after = fx.ctx.host_transfer_stats()
    assert np.array_equal(dst, np.frombuffer(job.want, dtype=np.uint8)) and job.want != job.dst0
    assert [(int(p["status"]), int(p["samples"])) for p in pres] == [tuple(w) for w in job.want_packets] == [(T.OK, 8)] + [(T.OK, 0)] * 3
    assert [(int(s["packets_ok"]), int(s["samples"]), int(s["first_bad_status"])) for s in sres] == job.want_streams()
    # eight decoded samples in two planes, then the plaintext payloads' bytes and nothing between them
    assert {k: after[k] - before[k] for k in after} == {"calls": 1, "src_calls": 0, "h2d_bytes": len(job.src), "d2h_bytes": 2 * 8 * 4 + 32}
