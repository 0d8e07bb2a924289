"""A DSD file to a PCM driver without a host pass over the audio: DSF file bytes (made here) -> the DSF packer (ohgpu_dsd_*) -> the
pipeline's DSD format -> DSD -> PCM at 88.2 kHz (ohgpu_dsd_pcm_*) -> the 88.2 -> 48 kHz resampler with a ramp (ohgpu_src_*) -> S24.
Each stage reads the device arena the stage before wrote; only the file goes up and only the last arena comes down.  The result must
equal the composition of the three textbook models (tests/dsd_textbook.py, tests/dsd_pcm_textbook.py, tests/src_textbook.py)."""
import numpy as np
import pytest

import dsd_pcm_cases as DC
import dsd_pcm_textbook as DP
import dsd_textbook as DT
import src_textbook as ST
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

FILL = 0xA5
KEY = (32, 16)                       # DSD64 -> 88.2 kHz
W, P = 6, 2
CHUNKS = 4096                        # two DSF block pairs: 65536 bits a channel, 2048 frames at 88.2 kHz


@pytest.mark.parametrize("variant", [0, 1], ids=["tuned", "v1"])
def test_dsf_file_to_48k_s24(variant):
    rng = np.random.default_rng(9800)
    dsf = np.frombuffer(DT.dsf_image(rng.bytes(2 * CHUNKS), rng.bytes(2 * CHUNKS)), dtype=np.uint8)
    pack = np.array([(0, 0, CHUNKS, capi.DSD_DSF, 0, W, P, [0] * 8)], dtype=capi.DSD_DESC)
    dsd_bytes = CHUNKS * (4 + P)
    frames = CHUNKS * 16 // KEY[0]
    conv = np.array([(0, 0, CHUNKS, 0, 0, frames, 0, 0, W, P, capi.ENDIAN_BIG, 0, [0] * 12)], dtype=capi.DSD_PCM_MSG_DESC)
    pcm_bytes = frames * 6
    L, M, coef = capi.src_design(88200, 48000, 24, 9.0, 20000.0)
    n_out = ST.out_frames(L, M, frames)
    cut = n_out // 3
    rows = [(0, 0, frames, 0, 0, cut, capi.RAMP_MAX, 0, 256, 2, 24, capi.ENDIAN_BIG, 24, capi.ENDIAN_BIG, capi.FLAG_RAMP, 0),
            (0, 0, frames, cut, 6 * cut + 2, n_out - cut, 0, 0, 256, 2, 24, capi.ENDIAN_BIG, 24, capi.ENDIAN_LITTLE, 0, 0)]
    src_descs = np.array(rows, dtype=capi.SRC_MSG_DESC)
    out_bytes = 6 * n_out + 2 + 3

    want_dsd = np.frombuffer(DT.batch_bytes(pack, dsf.tobytes(), dsd_bytes, FILL), dtype=np.uint8)
    want_pcm = DP.batch_bytes(conv, DC.coef(KEY), KEY[0], want_dsd, pcm_bytes, FILL)
    want = ST.batch_bytes(coef, L, M, 24, src_descs, want_pcm, out_bytes, capi.ramp_table(), FILL)

    with capi.Context(0) as ctx:
        ctx.set_kernel_variant(variant)
        d_file, d_dsd, d_pcm, d_out = ctx.upload(dsf), ctx.malloc(dsd_bytes), ctx.malloc(pcm_bytes), ctx.malloc(out_bytes)
        ctx.memset(d_out, FILL, out_bytes)
        filt, src = ctx.dsd_pcm_create(KEY[0], KEY[1], DC.coef(KEY)), ctx.src_create(L, M, 24, coef)
        b1 = ctx.dsd_batch(pack, dsf.size, dsd_bytes)
        b2 = ctx.dsd_pcm_batch(filt, conv, dsd_bytes, pcm_bytes)
        b3 = ctx.src_batch(src, src_descs, pcm_bytes, out_bytes)
        try:
            assert ctx.dsd_pcm_batch_paths(b2) == {"fast_descs": 1 - variant, "plain_descs": variant, "launches": 1}
            ctx.dsd_run(b1, d_file, d_dsd)                                 # one stream: each stage queues behind the last
            ctx.dsd_pcm_run(b2, d_dsd, d_pcm)
            ctx.src_run(b3, d_pcm, d_out)
            got = ctx.download(d_out, out_bytes)
            mid = ctx.download(d_pcm, pcm_bytes)
        finally:
            for b in (b1, b2, b3):
                ctx.batch_destroy(b)
            ctx.dsd_pcm_destroy(filt)
            ctx.src_destroy(src)
            for p in (d_file, d_dsd, d_pcm, d_out):
                ctx.free(p)
    assert np.array_equal(mid, want_pcm), "the 88.2 kHz stage"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} differing bytes, first at {bad[:6].tolist()}"
    assert (want == FILL).sum() >= 5
