"""Writes tests/golden/ts: two small transport streams made by the tests' own muxer (tests/ts_cases.py), and what the model
(tests/ts_textbook.py) says of them -- pinned, so that a change to the muxer or the model that moves either shows up as a diff here.

    python tests/golden/make_ts_fixtures.py
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ts_cases as TC          # noqa: E402
import ts_textbook as TX       # noqa: E402


def main():
    out = os.path.join(HERE, "ts")
    os.makedirs(out, exist_ok=True)
    rng = TC.Lcg(4711)
    streams = {}
    packets, _ = TC.segment(rng, 40)
    streams["segment_40_frames"] = b"".join(packets)
    packets, _ = TC.segment(rng, 24, frames_per_pes=1, tables_every=9)
    cut = b"".join(packets)
    streams["segment_cut_in_a_packet"] = cut[:len(cut) - 100]
    index = dict(crc_123456789=TX.crc(b"123456789"), pat_section=TC.pat()[:-4].hex(), streams={})
    for name, data in streams.items():
        with gzip.GzipFile(os.path.join(out, name + ".ts.gz"), "wb", mtime=0) as f:
            f.write(data)
        m = TX.demux(data)
        a = TX.adts_chain(m["run"], TX.RECOGNISE)
        index["streams"][name] = dict(status=m["status"], packets=m["packets"], audio_pid=m["audio_pid"], pes_packets=len(m["pes"]), bytes_delivered=len(m["run"]),
                                      run_fnv1a32=TC.fnv1a32(m["run"]), adts_status=a["status"], adts_frames=len(a["frames"]), adts_bytes_consumed=a["bytes_consumed"])
    with open(os.path.join(out, "streams.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
