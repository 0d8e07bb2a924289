"""What the pulled resampler's GPU tests share (tests/test_gpu_src_pull.py, tests/test_gpu_far_positions.py, tests/test_gpu_far_offsets.py)
and tests/test_far_cases.py checks without a device: the arena builder, the expected bytes from the numpy model
(tests/src_pull_model.py), and the streams of far positions.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import src_pull_model as PM
from ohpipeline_amd import capi

S = 8


class Arena:
    """Streams' input laid out in one source arena, their messages' outputs back to back in one destination arena."""

    def __init__(self):
        self.src = bytearray()
        self.descs = []
        self.dst_bytes = 0

    def add_input(self, data):
        off = len(self.src)
        self.src += bytes(data)
        self.src += bytes((-len(self.src)) % 16)
        return off

    def add_msg(self, src_offset, src_frame0, src_frames, pos, frac, step, n, ch, sb, se, db, de, flags=0, ramp=(0, 0)):
        d = np.zeros(1, dtype=capi.SRC_PULL_MSG_DESC)[0]
        d["src_offset"], d["src_frame0"], d["src_frames"] = src_offset, src_frame0, src_frames
        d["pos_frame"], d["pos_frac"], d["step"], d["n_frames"] = pos, frac, step, n
        d["dst_offset"] = self.dst_bytes
        d["ramp_start"], d["ramp_end"], d["attenuation"] = ramp[0], ramp[1], capi.UNITY_ATTENUATION
        d["channels"], d["src_bits"], d["src_endian"], d["dst_bits"], d["dst_endian"], d["flags"] = ch, sb, se, db, de, flags
        self.descs.append(d)
        self.dst_bytes += n * ch * db // 8

    def arrays(self):
        return np.frombuffer(bytes(self.src) or b"\0", dtype=np.uint8).copy(), np.array(self.descs, dtype=capi.SRC_PULL_MSG_DESC)


def expected(table, descs, src, dst_bytes, ramp_table):
    want = np.zeros(dst_bytes, dtype=np.uint8)
    for d in descs:
        b = PM.message_bytes(table, S, d, src, ramp_table)
        want[int(d["dst_offset"]):int(d["dst_offset"]) + b.size] = b
    return want


def stream(arena, rng, ch, sb, se, db, de, T, steps, sizes, in_frames, flags_of=lambda m: 0, ramps_of=lambda m: (0, 0), pos0=(0, 0)):
    """One stream of random packed input whose messages take the given sizes and steps in turn, each reading the whole input."""
    data = rng.integers(0, 256, size=in_frames * ch * sb // 8, dtype=np.uint8)
    off = arena.add_input(data)
    pos, frac = pos0
    for m, (st, n) in enumerate(zip(steps, sizes)):
        first, frames = PM.window(pos, frac, st, n, T)
        if first + frames > in_frames:
            break
        arena.add_msg(off, 0, in_frames, pos, frac, st, n, ch, sb, se, db, de, flags_of(m), ramps_of(m))
        pos, frac = PM.advance(pos, frac, st, n)


# ---------------------------------------------------------------- far positions
FAR_NEAR0 = 4096                                   # where a far stream's near twin is entered: mid-stream, past every filter's history
FAR_SIZES = (300, 1, 257, 77)                      # the messages of one far stream, in turn (more than one tile of 256; one output)
FAR_FRAC = (1 << 32) - 5                           # with any step >= 5 the first output's fraction carries into the frame


def far_pos_frames(T):
    """label -> pos_frame of a far stream's first message: pos_frame passes 2^31 and 2^32 inside that message (after 150 of its 300
    outputs, roughly: 137 input frames at 44.1 -> 48); the window's first frame pos_frame - (T - 1) still below 2^32 with pos_frame
    above; and the stream that ends at the ABI's limit, its last message reading up to frame 2^48 - 1."""
    return {"frame_2p31": (1 << 31) - 137, "frame_2p32": (1 << 32) - 137, "window_2p32": (1 << 32) + T // 2, "below_2p48": (1 << 48) - 700,
            "at_2p48": 1 << 48}                        # (one message: the last pos_frame the creation admits)


def far_streams(T, far, rate_in=44100, ppm=300):
    """(arena, labels): one stream per far_pos_frames(T) entry x (stereo, five channels), each message's input window packed by
    itself (src_frame0 = the window's first frame), the first message entered at FAR_FRAC.  far = False: the same streams entered
    at FAR_NEAR0 -- the same bytes, the same layout, only pos_frame and src_frame0 moved: the resampler is translation invariant, so
    the expected bytes are the same."""
    rng = np.random.default_rng(4800 + T)
    a, labels = Arena(), []
    step = PM.step_of(rate_in, 48000, PM.multiplier_of(ppm))
    for label, far_pos in far_pos_frames(T).items():
        for k, ch in enumerate((2, 5)):
            pos, frac = (far_pos if far else FAR_NEAR0), FAR_FRAC
            for m, n in enumerate(FAR_SIZES[:1] if label == "at_2p48" else FAR_SIZES):
                first, frames = PM.window(pos, frac, step, n, T)
                off = a.add_input(rng.integers(0, 256, size=frames * ch * 3, dtype=np.uint8))
                a.add_msg(off, first, frames, pos, frac, step, n, ch, 24, PM.ENDIAN_LITTLE if k else PM.ENDIAN_BIG, 24, PM.ENDIAN_BIG,
                          PM.FLAG_RAMP if m == 2 else 0, (16384, 3000))
                labels.append(f"{label}/{ch}ch/m{m}")
                pos, frac = PM.advance(pos, frac, step, n)
    return a, labels
