"""What the DSD line kernels' GPU tests share (tests/test_gpu_dsd_textbook.py, tests/test_gpu_far_offsets.py): the batch builder, the
planner's documented rule restated (`planned`), and the expected destination arena from tests/dsd_textbook.py.  TEST INFRASTRUCTURE
ONLY."""
import hashlib

import numpy as np

import dsd_textbook as DT
from ohpipeline_amd import capi

FILL = 0xA5
PASS, DSF, DFF, RAW = capi.DSD_PASS, capi.DSD_DSF, capi.DSD_DFF, capi.DSD_RAW
KINDS = {PASS: "pass", DSF: "dsf", DFF: "dff", RAW: "raw"}
FORMATS = [(1, 0), (2, 0), (6, 2), (8, 4)]                                 # every (W, P) in use; (3, 0) and (12, 8) ride along
MORE_FORMATS = FORMATS + [(3, 0), (12, 8)]
CUTS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1025, 2047, 2048, 2049, 2055, 2056, 2057, 4095, 4096, 4097, 4104, 6151)


class Batch:
    """Descriptors laid one after another into a source arena of seeded bytes and a destination arena: `sres` / `dres` = the
    offsets' residues mod 16 (None: wherever the last one ended), `gap` = untouched bytes before the output."""

    def __init__(self, seed, src_lead=0, dst_lead=0):
        self.rng = np.random.default_rng(seed)
        self.src = bytearray(self.rng.bytes(src_lead))
        self.rows, self.dp = [], dst_lead

    def add(self, kind, W, P, n, sres=None, dres=None, gap=0, silence=False):
        need, out = DT.layout(kind, W, P, n, silence)
        if sres is not None:
            self.src += self.rng.bytes((sres - len(self.src)) % 16)
        so = len(self.src)
        self.src += self.rng.bytes(need)
        do = self.dp + gap
        if dres is not None:
            do += (dres - do) % 16
        self.rows.append((so, do, n, kind, capi.DSD_FLAG_SILENCE if silence else 0, W, P, [0] * 8))
        self.dp = do + out
        return self

    def empty(self, kind=DFF, W=6, P=2, silence=False):
        """A descriptor of no chunks, its offsets far beyond both arenas: accepted, writes nothing."""
        self.rows.append((1 << 40, (1 << 41) + 1, 0, kind, capi.DSD_FLAG_SILENCE if silence else 0, W, P, [0] * 8))
        return self

    def finish(self, dst_tail=0):
        return np.array(self.rows, dtype=capi.DSD_DESC), np.frombuffer(bytes(self.src), dtype=np.uint8), self.dp + dst_tail


def whole(n, per_block):
    """n rounded up to whole blocks."""
    return -(-n // per_block) * per_block


def planned(descs):
    """The documented rule (module docstring): (wide, generic, launches)."""
    wide = generic = 0
    for d in descs:
        n, P = int(d["n_chunks"]), int(d["pad_bytes_per_chunk"])
        if n == 0:
            continue
        silent = bool(d["flags"] & capi.DSD_FLAG_SILENCE)
        aligned = int(d["dst_offset"]) % 16 == 0 and (silent or int(d["src_offset"]) % 16 == 0)
        if silent:
            body = DT.layout(int(d["kind"]), int(d["sample_block_words"]), P, n, True)[1] >= 16
        elif d["kind"] == PASS:
            body = n * (4 + P) >= 16
        else:
            body = P <= 4 and n >= 8
        if aligned and body:
            wide += 1
        else:
            generic += 1
    return {"wide_descs": wide, "generic_descs": generic, "launches": 1 if wide + generic else 0}


_WANT = {}


def expected(descs, src, dst_bytes):
    """(kept per input: `vctx` runs every test twice on the same seeded bytes, and the model is slow)"""
    key = hashlib.sha256(descs.tobytes() + src.tobytes() + dst_bytes.to_bytes(8, "little")).digest()
    if key not in _WANT:
        _WANT[key] = np.frombuffer(DT.batch_bytes(descs, src.tobytes(), dst_bytes, FILL), dtype=np.uint8)
    return _WANT[key]
