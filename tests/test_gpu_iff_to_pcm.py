"""A check of the PCM file layer that does not rest on its model: for little-endian 16- and 24-bit WAV files, the new family's
big-endian output fed to the existing ohgpu_pcm_process_host as a big-endian source must give the same bytes as the audio taken
straight from the file and fed to the same call as a little-endian source (row a1: the swap fused into the message path)."""
import numpy as np
import pytest

import iff_cases as IC
import oracle_lib as O
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sample_bytes", [2, 3], ids=["wav16", "wav24"])
def test_the_files_audio_reaches_the_message_path_either_way(sample_bytes):
    frames, channels = 1237, 2
    files = [IC.wav(IC.samples(frames, channels, sample_bytes, 70 + k), channels, before_fmt=[IC.junk(b"JUNK", k)]) for k in range(3)]
    job = IC.Job([IC.stream(w) for w in files])
    frame = channels * sample_bytes
    with capi.Context(0) as ctx:
        big = np.full(job.dst_bytes, IC.FILL, dtype=np.uint8)
        results = ctx.iff_process_host(job.descs, job.src, big)
        assert all(int(r["status"]) == capi.IFF_OK and int(r["frames_written"]) == frames and int(r["src_endian"]) == capi.ENDIAN_LITTLE for r in results)

        def through_the_message_path(src, offsets, endian):
            d = np.zeros(len(offsets), dtype=O.MSG_DESC)
            for k, off in enumerate(offsets):
                d[k] = (off, k * frames * frame, frames, 0, 0, 256, channels, 8 * sample_bytes, endian, 8 * sample_bytes, O.ENDIAN_BIG, 0)
            out = np.zeros(len(offsets) * frames * frame, dtype=np.uint8)
            ctx.pcm_process_host(d, np.ascontiguousarray(src), out)
            return out

        from_new = through_the_message_path(big, [int(d["dst_offset"]) for d in job.descs], O.ENDIAN_BIG)
        from_file = through_the_message_path(job.src, [int(d["src_offset"]) + w.data_offset for d, w in zip(job.descs, files)], O.ENDIAN_LITTLE)
    assert np.array_equal(from_new, from_file)
    assert from_new.tobytes() == b"".join(w.pcm() for w in files)             # (and both are the writer's samples)
