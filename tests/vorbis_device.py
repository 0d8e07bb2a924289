"""What the Vorbis device tests share (tests/test_gpu_vorbis_textbook.py, tests/test_gpu_vorbis_damage.py): one batch over device arenas
with the route asserted, the packet records against the model's, a stream's samples out of the destination arena."""
import numpy as np

import vorbis_frames as VF
from ohpipeline_amd import capi

FILL = 0xA5


def run_batch(ctx, variant, streams, planar=False, max_samples=None, ranges=None, spectra=False):
    """One batch over `streams` on device arenas: (stream results, packet results, destination bytes, descs, spectrum reader's results)."""
    blob, descs, packets, src, dst_bytes, infos = VF.batch_tables(capi, streams, planar, max_samples, ranges)
    ctx.set_kernel_variant(variant)
    b = ctx.vorbis_batch(descs, packets, blob, src.size, dst_bytes)
    ctx.set_kernel_variant(0)
    assert ctx.batch_paths(b)["vorbis_route"] == (2 if variant == 1 else 1) and ctx.vorbis_paths(b)["route"] == ctx.batch_paths(b)["vorbis_route"]
    d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
    ctx.memset(d_dst, FILL, dst_bytes)
    ctx.vorbis_run(b, d_src, d_dst)
    res, pres = ctx.vorbis_results(b, descs.size, packets.size)
    got = ctx.download(d_dst, dst_bytes)
    spec = {}
    if spectra:
        for p in range(packets.size):
            if pres[p]["status"] == capi.VORBIS_OK:
                i = int(np.searchsorted(descs["first_packet"], p, side="right")) - 1
                for c in range(int(infos[i]["channels"])):
                    spec[(p, c)] = ctx.vorbis_spectrum(b, p, c, int(pres[p]["blocksize"]) // 2)
    ctx.batch_destroy(b)
    ctx.free(d_src)
    ctx.free(d_dst)
    return res, pres, got, descs, spec


def check_records(pres, recs):
    got = [(int(r["status"]), int(r["mode"]), int(r["blocksize"]), int(r["samples"]), int(r["position"])) for r in pres]
    assert got == [tuple(int(v) for v in r) for r in recs]
    assert not pres["reserved"].any()


def stream_pcm(got, desc, channels, samples, planar=False):
    """(int32 [channels][samples] the stream wrote, the bytes of its destination behind them)"""
    at = int(desc["dst_offset"])
    if planar:
        stride = int(desc["dst_plane_stride"])
        return np.stack([got[at + c * stride:at + c * stride + samples * 4].view("<i4") for c in range(channels)]).astype(np.int32), None
    raw = got[at:at + samples * channels * 2].view(">i2").astype(np.int32).reshape(samples, channels).T
    rest = got[at + samples * channels * 2:at + int(desc["max_samples"]) * channels * 2]
    return raw, rest
