"""The DSD -> PCM cases that tests/test_dsd_pcm_core_cpu.py (csrc/dsd_pcm_core.h on the CPU) and tests/test_gpu_dsd_pcm_textbook.py (both
kernels) share: the designs, a batch builder, and the batches.  The expected bytes come from tests/dsd_pcm_textbook.py, once per batch.

Shapes: the smallest at which the code can go wrong.  A tile is 512 frames (kDsdPcmTile): n_frames goes round 16 and round 512 and
over two tiles; out_frame0 = 0 reads idle history, 7 and 1001 are mid-stream (7 with part of its history before the stream start
for the longer filters); P = 0, 2, 4; odd source offsets; destination offsets that are no multiple of 4; both byte orders; every
ramp pair of test_gpu_src_textbook.RAMPS and none; inputs of seeded noise (pad bytes random too: they must not be looked at), all
ones (clamps high), all zeros (the lowest value), 0x69 and 0xAA."""
import hashlib

import numpy as np

import dsd_pcm_textbook as DP
from ohpipeline_amd import capi

FILL = 0xA5
kMax = 1 << 14
RAMPS = [(kMax, 0), (0, kMax), (kMax, 8192), (8191, 8190), (5, 5), (kMax, kMax), (0, 0), (12345, 54), (17, 16001)]   # test_gpu_src_textbook.RAMPS
FORMATS = [(2, 0), (6, 2), (8, 4)]                                  # (W, P)
# (dsd_rate, pcm_rate, T): D = 8 is one table of eight look-ups, (64, 16) the longest filter the fast route holds
DESIGNS = {(8, 8): (2822400, 352800, 8), (16, 24): (2822400, 176400, 24), (32, 16): (2822400, 88200, 16), (64, 16): (5644800, 88200, 16)}
BETA, F_PASS = 14.0, 20000.0
INPUTS = ("noise", "ones", "zeros", "idle", "aa")
N_FRAMES = (1, 15, 16, 17, 511, 512, 513, 1025)
OUT0 = (0, 7, 1001)

_COEF = {}


def coef(key, gain=1.0):
    if (key, gain) not in _COEF:
        dsd_rate, pcm_rate, T = DESIGNS[key]
        _COEF[(key, gain)] = DP.design(dsd_rate, pcm_rate, T, BETA, F_PASS, gain)[1]
    return _COEF[(key, gain)]


class Batch:
    """Messages laid one after another: each one's window of chunks into the source arena, its frames into the destination."""

    def __init__(self, key, seed, src_lead=0, dst_lead=0):
        self.D, self.T = key
        self.rng = np.random.default_rng(seed)
        self.src = bytearray(self.rng.bytes(src_lead))
        self.rows, self.dp = [], dst_lead

    def add(self, out0, n, fmt=(2, 0), kind="noise", ramp=None, endian=capi.ENDIAN_BIG, before=0, after=0, src_gap=0, dst_gap=0):
        """`before` / `after`: chunks held beyond the window on either side (never read)."""
        W, P = fmt
        lo, hi = DP.window(out0, n, self.D, self.T)
        c0 = max(lo - before, 0)
        chunks = hi + after - c0
        if kind == "noise":
            raw = self.rng.bytes(chunks * (4 + P))
        else:
            byte = {"ones": 0xFF, "zeros": 0x00, "idle": 0x69, "aa": 0xAA}[kind]
            raw = DP.pack_chunks(np.unpackbits(np.full((2, 2 * chunks), byte, dtype=np.uint8), axis=1), P)
        self.src += self.rng.bytes(src_gap)
        so = len(self.src)
        self.src += raw
        do = self.dp + dst_gap
        start, end = ramp if ramp else (0, 0)
        self.rows.append((so, c0, chunks, out0, do, n, start, end, W, P, endian, capi.FLAG_RAMP if ramp else 0, [0] * 12))
        self.dp = do + 6 * n
        return self

    def finish(self, label, dst_tail=0):
        return Case(label, (self.D, self.T), np.array(self.rows, dtype=capi.DSD_PCM_MSG_DESC), np.frombuffer(bytes(self.src), dtype=np.uint8),
                    self.dp + dst_tail)


class Case:
    def __init__(self, label, key, descs, src, dst_bytes):
        self.label, self.key, self.descs, self.src, self.dst_bytes = label, key, descs, src, dst_bytes
        self._want = None

    def want(self):
        """The model's whole destination arena (computed once)."""
        if self._want is None:
            self._want = DP.batch_bytes(self.descs, coef(self.key), self.key[0], self.src, self.dst_bytes, FILL)
            self._want.setflags(write=False)
        return self._want

    def sha(self):
        return hashlib.sha256(self.want().tobytes()).hexdigest()


_CASES = {}


def shapes(key):
    """Every n_frames x out_frame0, the format, the byte order, the ramp and the input rotating; odd offsets on both sides."""
    if ("shapes", key) not in _CASES:
        b, k = Batch(key, 9100 + key[0] + key[1], src_lead=1, dst_lead=3), 0
        for n in N_FRAMES:
            for out0 in OUT0:
                ramp = RAMPS[k % len(RAMPS)] if k % 3 else None
                b.add(out0, n, FORMATS[k % 3], INPUTS[k % 5] if k % 2 else "noise", ramp, capi.ENDIAN_LITTLE if k % 4 == 1 else capi.ENDIAN_BIG,
                      before=k % 3, after=k % 2, src_gap=2 * (k % 2) + (k % 3 == 0), dst_gap=1 + k % 3)
                k += 1
        _CASES[("shapes", key)] = b.finish(f"shapes D={key[0]} T={key[1]}", dst_tail=5)
    return _CASES[("shapes", key)]


def inputs(key):
    """Every input x out_frame0 at 17 frames, ramped with every pair and unramped, big- and little-endian."""
    if ("inputs", key) not in _CASES:
        b, k = Batch(key, 9200 + key[0], src_lead=3, dst_lead=1), 0
        for kind in INPUTS:
            for out0 in OUT0:
                for ramp in [None] + RAMPS:
                    b.add(out0, 17, FORMATS[k % 3], kind, ramp, capi.ENDIAN_LITTLE if k % 2 else capi.ENDIAN_BIG, src_gap=k % 2, dst_gap=k % 4)
                    k += 1
        _CASES[("inputs", key)] = b.finish(f"inputs D={key[0]} T={key[1]}", dst_tail=2)
    return _CASES[("inputs", key)]


def mixed(key=(32, 16)):
    """64 streams x 2048 frames of mixed P, a stream in four messages of 512, every fourth stream from its start."""
    if ("mixed", key) not in _CASES:
        b = Batch(key, 9300)
        for s in range(64):
            base = 0 if s % 4 == 0 else 2048 * (1 + s % 5) + s
            for m in range(4):
                b.add(base + 512 * m, 512, FORMATS[s % 3], "noise", RAMPS[(s + m) % len(RAMPS)] if (s + m) % 2 else None,
                      capi.ENDIAN_LITTLE if s % 2 else capi.ENDIAN_BIG, dst_gap=(s + m) % 2)
        _CASES[("mixed", key)] = b.finish("mixed 64 x 2048")
    return _CASES[("mixed", key)]


FAR_NEAR0 = 64          # where the near twin of a far message starts (plus the far position's parity): past every filter's history


def far_positions(key):
    """label -> (out_frame0, n_frames): the stream's bit index out_frame0 * D passes 2^32 at the message's frame 9, inside a tile,
    and so do its byte index (bits / 8: what the fast kernel counts in) and its chunk index (bits / 16); out_frame0 itself passes
    2^31 inside the first tile and 2^32 inside the second; the message whose last frame is the last below 2^40; and the one frame
    at out_frame0 = 2^40, the last value the creation admits (2^40 + 1 is refused)."""
    D = key[0]
    return {"bit_2p32": ((1 << 32) // D - 9, 513), "byte_2p32": ((1 << 35) // D - 9, 513), "chunk_2p32": ((1 << 36) // D - 9, 17),
            "frame_2p31": ((1 << 31) - 9, 513), "frame_2p32": ((1 << 32) - 521, 1025),
            "below_2p40": ((1 << 40) - 513, 513), "at_2p40": (1 << 40, 1), "bit_2p32_short": ((1 << 32) // D - 9, 17)}


def positions(key, far):
    """The messages of far_positions(key) (far) or their near twins: the same frames of the same streams, moved down by an even
    number of frames to FAR_NEAR0, so that only out_frame0 and src_chunk0 differ between the two batches -- the source bytes, the
    layout and, the conversion being translation invariant (an even shift keeps the chunks' and the idle pattern's phase), the
    expected destination bytes are the same."""
    if ("positions", key, far) not in _CASES:
        b = Batch(key, 9600 + key[0] + key[1], src_lead=1, dst_lead=3)
        for k, (label, (out0, n)) in enumerate(far_positions(key).items()):
            ramp = RAMPS[k % len(RAMPS)] if k % 2 else None
            b.add(out0 if far else FAR_NEAR0 + out0 % 2, n, FORMATS[k % 3], "noise", ramp, capi.ENDIAN_LITTLE if k % 3 == 1 else capi.ENDIAN_BIG,
                  before=k % 3, after=k % 2, src_gap=k % 2, dst_gap=1 + k % 3)
        _CASES[("positions", key, far)] = b.finish(f"{'far' if far else 'near'} positions D={key[0]} T={key[1]}", dst_tail=5)
    return _CASES[("positions", key, far)]


def every_case():
    return [f(key) for key in DESIGNS for f in (shapes, inputs)] + [mixed()]


def every_far_case():
    return [positions(key, far) for key in DESIGNS for far in (False, True)]
