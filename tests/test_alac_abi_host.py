"""The host-only half of the Apple Lossless ABI: ohgpu_alac_config_parse, with and without the atoms older files put in front of
the configuration, and the descriptor validation of ohgpu_alac_batch_create (ohgpu_alac_batch_check) -- each refusal with its code
and text, without a device."""
import numpy as np
import pytest

import alac_cases as AC
import alac_frames as F
import alac_textbook as T
from ohpipeline_amd import capi


def tables(n_packets=3, packet_bytes=100, **over):
    d = np.zeros(1, dtype=capi.ALAC_STREAM_DESC)
    base = dict(frame_length=256, bit_depth=16, pb=40, mb=10, kb=14, channels=2, max_run=255, sample_rate=44100, first_packet=0,
                n_packets=n_packets, dst_offset=0, dst_plane_stride=n_packets * 256 * 4, flags=0)
    base.update(over)
    for k, v in base.items():
        d[k] = v
    p = np.zeros(n_packets, dtype=capi.ALAC_PACKET)
    p["src_offset"] = np.arange(n_packets) * packet_bytes
    p["bytes"] = packet_bytes
    return d, p


@pytest.mark.parametrize("frma", [False, True])
@pytest.mark.parametrize("alac", [False, True])
def test_config_parse_with_and_without_the_atoms(frma, alac):
    for fx in AC.fixtures():
        got = capi.alac_config_parse(F.wrapped(fx["cookie"], frma, alac))
        assert {k: int(got[k]) for k in fx["cfg"]} == fx["cfg"] and got["compatible_version"] == 0
    odd = F.cookie(12345, 24, 7, sample_rate=192000, pb=1, mb=2, kb=3, max_run=0x1234)
    got = capi.alac_config_parse(F.wrapped(odd, frma, alac))
    assert {k: int(got[k]) for k in T.parse_config(odd)} == T.parse_config(odd)


def test_config_parse_refusals():
    good = F.cookie(4096, 16, 2)
    for bad, text in ((good[:23], "takes 24"), (F.wrapped(good)[:47], "takes 24"), (b"", "null argument"), (F.cookie(4096, 16, 2, version=1), "compatible version 1")):
        with pytest.raises(capi.OhGpuError) as e:
            capi.alac_config_parse(bad)
        assert e.value.code == capi.ERR_INVALID and text in str(e.value), str(e.value)


def test_descriptor_validation_without_a_device():
    plane = 3 * 256 * 4
    capi.alac_batch_check(*tables(), 300, 2 * plane)
    capi.alac_batch_check(*tables(bit_depth=20), 300, 2 * plane)               # accepted: its packets come back UNSUPPORTED
    capi.alac_batch_check(*tables(flags=capi.ALAC_OUT_PACKED_LE, dst_plane_stride=0), 300, 3 * 256 * 4)
    capi.alac_batch_check(*tables(flags=capi.ALAC_OUT_PACKED_BE, dst_plane_stride=0, bit_depth=24), 300, 3 * 256 * 6)
    capi.alac_batch_check(*tables(channels=8, frame_length=16384, n_packets=1, dst_plane_stride=65536, packet_bytes=16384 * 8 * 5 + 64), 16384 * 8 * 5 + 64, 8 * 65536)
    capi.alac_batch_check(np.zeros(0, dtype=capi.ALAC_STREAM_DESC), np.zeros(0, dtype=capi.ALAC_PACKET), 0, 0)
    for (d, p), sa, da, code, text in (
        (tables(), 299, 2 * plane, capi.ERR_BOUNDS, "source arena"),
        (tables(), 300, 2 * plane - 1, capi.ERR_BOUNDS, "destination arena"),
        (tables(flags=capi.ALAC_OUT_PACKED_LE, dst_plane_stride=0, bit_depth=32), 300, 3 * 256 * 8 - 1, capi.ERR_BOUNDS, "destination arena"),
        (tables(channels=0), 300, 2 * plane, capi.ERR_INVALID, "channels 0 outside 1..8"),
        (tables(channels=9), 300, 9 * plane, capi.ERR_INVALID, "channels 9 outside 1..8"),
        (tables(frame_length=0), 300, 2 * plane, capi.ERR_INVALID, "frame length 0 outside 1..16384"),
        (tables(frame_length=16385), 300, 2 ** 30, capi.ERR_INVALID, "frame length 16385 outside 1..16384"),
        (tables(packet_bytes=256 * 2 * 5 + 65), 3 * (256 * 2 * 5 + 65), 2 * plane, capi.ERR_INVALID, "at most frame length x channels x 5 + 64 = 2624"),
        (tables(bit_depth=8), 300, 2 * plane, capi.ERR_UNSUPPORTED, "bit depth 8"),
        (tables(compatible_version=1), 300, 2 * plane, capi.ERR_INVALID, "compatible version 1"),
        (tables(flags=3), 300, 2 * plane, capi.ERR_INVALID, "flags"),
        (tables(flags=4), 300, 2 * plane, capi.ERR_INVALID, "flags"),
        (tables(flags=capi.ALAC_OUT_PACKED_LE), 300, 2 * plane, capi.ERR_INVALID, "packed"),
        (tables(dst_offset=2), 300, 3 * plane, capi.ERR_INVALID, "multiples of 4"),
        (tables(dst_plane_stride=plane + 2), 300, 3 * plane, capi.ERR_INVALID, "multiples of 4"),
        (tables(dst_plane_stride=plane - 4), 300, 3 * plane, capi.ERR_INVALID, "planes overlap"),
        (tables(first_packet=1, n_packets=2), 300, 2 * plane, capi.ERR_INVALID, "where the table goes on at 0"),
        (tables(n_packets=2)[:1] + (tables()[1],), 300, 2 * plane, capi.ERR_INVALID, "take 2 packets of a table of 3"),
    ):
        with pytest.raises(capi.OhGpuError) as e:
            capi.alac_batch_check(d, p, sa, da)
        assert e.value.code == code and text in str(e.value), str(e.value)
    d, p = tables()
    p["reserved"][1] = 7
    with pytest.raises(capi.OhGpuError) as e:
        capi.alac_batch_check(d, p, 300, 2 * plane)
    assert e.value.code == capi.ERR_INVALID and "reserved" in str(e.value)
