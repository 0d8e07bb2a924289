"""What the Songcast sender's GPU tests share (tests/test_gpu_ohm_textbook.py, tests/test_gpu_far_offsets.py): the batch builder --
streams, frames and fragments, each frame's expected datagram from tests/ohm_textbook.py with the fragments' audio from
tests/pcm_textbook.py -- and the run on both routes.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import ohm_textbook as OT
import oracle_lib as O
import pcm_textbook as PT
from ohpipeline_amd import capi

LE, BE = O.ENDIAN_LITTLE, O.ENDIAN_BIG
FILL = 0xA5


class Batch:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.streams, self.frames, self.fragments, self.src, self.expected = [], [], [], [], []
        self.src_bytes = self.dst_bytes = 0

    def stream(self, rate, bits, ch, endian=BE, codec=b"PCM", volume=0, total=0):
        s = np.zeros(1, dtype=capi.OHM_STREAM)
        s["samples_total"], s["sample_rate"], s["bit_rate"], s["volume_offset"] = total, rate, rate * bits * ch, volume
        s["src_channels"], s["src_bits"], s["codec_bytes"], s["src_endian"] = ch, bits, len(codec), endian
        s["codec"][0, :len(codec)] = np.frombuffer(codec, dtype=np.uint8)
        self.streams.append(s)
        wire_ch, wire_bits = OT.wire_format(ch, bits)
        return dict(index=len(self.streams) - 1, rate=rate, bits=bits, ch=ch, endian=endian,
                    header=OT.stream_header(total, rate, rate * bits * ch, volume, wire_bits, wire_ch, codec),
                    max_samples=min(rate * 5 // 1000, OT.MAX_SAMPLE_BYTES // (wire_ch * wire_bits // 8)))

    def frame(self, st, fragments, flags=capi.OHM_FLAG_LOSSLESS, frame_no=0, net=0, latency=0, start=0, gap=0):
        """fragments: [(n_frames, kind)] with kind in plain / ramp / silence / att."""
        audio, first = b"", len(self.fragments)
        for k, (n, kind) in enumerate(fragments):
            g = np.zeros(1, dtype=capi.OHM_FRAGMENT)
            g["n_frames"], g["attenuation"] = n, 256
            ramp = [(16384, 0), (0, 16384), (8191, 8190), (12345, 54)][(first + k) % 4]
            if kind == "ramp":
                g["flags"], g["ramp_start"], g["ramp_end"] = O.FLAG_RAMP, ramp[0], ramp[1]
            elif kind == "silence":
                g["flags"] = O.FLAG_SILENCE
            elif kind == "att":
                assert st["bits"] == 16
                g["attenuation"] = [100, 0, 255][(first + k) % 3]
            nbytes = n * st["ch"] * st["bits"] // 8
            if kind != "silence":
                pad = (first + k) % 5                                      # arbitrary source alignment
                self.src.append(self.rng.integers(0, 256, pad + nbytes, dtype=np.uint8))
                g["src_offset"] = self.src_bytes + pad
                self.src_bytes += pad + nbytes
            self.fragments.append(g)
            d = dict(src_offset=int(g["src_offset"][0]), dst_offset=0, n_frames=n, ramp_start=int(g["ramp_start"][0]),
                     ramp_end=int(g["ramp_end"][0]), attenuation=int(g["attenuation"][0]), channels=st["ch"], src_bits=st["bits"],
                     src_endian=st["endian"], dst_bits=st["bits"], dst_endian=BE, flags=int(g["flags"][0]))
            audio += OT.sender_audio(PT.process_message(d, self._src_so_far()), st["ch"], st["bits"])
        samples = sum(n for n, _ in fragments)
        fr = np.zeros(1, dtype=capi.OHM_FRAME_DESC)
        fr["dst_offset"], fr["sample_start"], fr["stream"], fr["frame"] = self.dst_bytes, start, st["index"], frame_no
        fr["network_timestamp"], fr["media_latency"], fr["first_fragment"], fr["n_fragments"], fr["flags"] = net, latency, first, len(fragments), flags
        self.frames.append(fr)
        gram = OT.audio_frame(flags, samples, frame_no, net, latency, start, st["header"], audio)
        self.expected.append((self.dst_bytes, np.frombuffer(gram, dtype=np.uint8)))
        self.dst_bytes += len(gram) + gap

    def _src_so_far(self):
        if len(self.src) > 1:
            self.src = [np.concatenate(self.src)]
        return self.src[0] if self.src else np.zeros(1, dtype=np.uint8)

    def run(self, ctx, variants=(0, 1)):
        src = self._src_so_far()
        streams, frames, fragments = np.concatenate(self.streams), np.concatenate(self.frames), np.concatenate(self.fragments)
        dst_bytes = self.dst_bytes + 3
        want = np.full(dst_bytes, FILL, dtype=np.uint8)
        for off, gram in self.expected:
            want[off:off + gram.size] = gram
        d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
        b, outs = None, {}
        try:
            b = ctx.ohm_batch(streams, frames, fragments, src.size, dst_bytes)
            paths = ctx.batch_paths(b)
            for v in variants:
                ctx.set_kernel_variant(v)
                ctx.memset(d_dst, FILL, dst_bytes)
                ctx.ohm_run(b, d_src, d_dst)
                outs[v] = ctx.download(d_dst, dst_bytes)
        finally:
            ctx.set_kernel_variant(0)
            if b is not None:
                ctx.batch_destroy(b)
            ctx.free(d_src)
            ctx.free(d_dst)
        for v, out in outs.items():
            if np.array_equal(out, want):
                continue
            for k, (off, gram) in enumerate(self.expected):
                got = out[off:off + gram.size]
                if not np.array_equal(got, gram):
                    bad = int(np.flatnonzero(got != gram)[0])
                    raise AssertionError(f"variant {v}: frame {k} at {off}: byte {bad} of {gram.size}: got {got[bad]:#x}, want {gram[bad]:#x} ({paths})")
            raise AssertionError(f"variant {v}: bytes outside every frame were modified ({paths})")
        return paths
