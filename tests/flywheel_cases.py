"""The FlywheelRamper inputs that tests/test_flywheel_textbook.py (CPU: model == oracle, and the model's undefined division is
never reached) and tests/test_gpu_flywheel_textbook.py (device) share.  Fixed seeds, numpy only: no oracle, no library.

A request is a dict: sample_rate, channels, in_samples, channel_bytes, out_frames, block_frames, blob (the `channels` training
planes of channel_bytes each, big-endian 32-bit, oldest sample first) and a name."""
import numpy as np

KINDS = ("noise", "sine", "dc", "square", "zero", "impulse", "alternating")
JIFFIES_PER_MS = 56448
JIFFIES_PER_SAMPLE = {7350: 7680, 8000: 7056, 11025: 5120, 16000: 3528, 22050: 2560, 32000: 1764, 44100: 1280, 48000: 1176,
                      88200: 640, 96000: 588, 176400: 320, 192000: 294, 352800: 160, 384000: 147}    # 56448000 / rate
RATES = (44100, 48000, 88200, 96000, 176400, 192000, 384000, 32000, 7350)


def decimation(rate):
    return 4 if rate in (176400, 192000) else (2 if rate in (88200, 96000) else 1)


def plane(kind, seed, n, rate):
    """n big-endian 32-bit samples of one channel, as uint8."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "noise":
        v = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64)
    elif kind == "sine":
        f = 400.0 + float(rng.integers(0, 3000))
        x = 0.7 * np.sin(2 * np.pi * f * t / rate + 0.1 * (seed % 7)) + 0.1 * np.sin(2 * np.pi * 5003.0 * t / rate)
        v = np.round(x * (2 ** 31 - 1)).astype(np.int64)
    elif kind == "dc":
        v = np.full(n, int(rng.integers(-2 ** 31, 2 ** 31)), dtype=np.int64)
    elif kind == "square":                                      # full scale, period 6: the 16-bit sums wrap
        v = np.where((t // 3) % 2 == 0, 2 ** 31 - 1, -2 ** 31).astype(np.int64)
    elif kind == "zero":                                        # sn == 0: every coefficient stays 0
        v = np.zeros(n, dtype=np.int64)
    elif kind == "impulse":                                     # a single non-zero sample
        v = np.zeros(n, dtype=np.int64)
        v[int(rng.integers(0, n))] = int(rng.integers(-2 ** 31, 2 ** 31)) | 0x10000
    elif kind == "alternating":                                 # +/- full scale every sample: t1 / t2 wrap in 16 bits
        v = np.where(t % 2 == 0, 2 ** 31 - 1, -2 ** 31).astype(np.int64)
    else:
        raise ValueError(kind)
    return v.astype(np.int32).astype(">i4").view(np.uint8)


def request(name, seed, rate, channels, kind, in_samples=None, extra=0, out_frames=None, block_frames=None):
    """Defaults are the StarvationRamper's: 1 ms of training, 20 ms out in 1 ms blocks (StarvationRamper.cpp:374-375)."""
    per_ms = JIFFIES_PER_MS // JIFFIES_PER_SAMPLE[rate]
    in_samples = per_ms if in_samples is None else in_samples
    out_frames = 20 * per_ms if out_frames is None else out_frames
    block_frames = per_ms if block_frames is None else block_frames
    kinds = [kind] * channels if kind != "mixed" else [KINDS[(seed + c) % len(KINDS)] for c in range(channels)]
    planes = [plane(kinds[c], seed * 16 + c, in_samples + extra, rate) for c in range(channels)]
    return dict(name=name, sample_rate=rate, channels=channels, in_samples=in_samples, channel_bytes=(in_samples + extra) * 4,
                out_frames=out_frames, block_frames=block_frames, blob=np.concatenate(planes))


def input_classes():
    """Every input class at every decimation factor, then the shape edges: in_samples from degree + 1 (after decimation) up,
    out_frames that no block divides, out_frames below one block, a block of one frame, more training bytes than samples."""
    reqs, seed = [], 100
    for kind in KINDS + ("mixed",):
        for rate, ch in ((44100, 2), (96000, 3), (192000, 1), (384000, 2)):
            seed += 1
            reqs.append(request(f"{kind}_{rate}_{ch}ch", seed, rate, ch, kind, out_frames=3 * (JIFFIES_PER_MS // JIFFIES_PER_SAMPLE[rate]) + 5))
    for rate in RATES:
        dec = decimation(rate)
        for in_samples in (4 * dec, 4 * dec + 1, 5 * dec, 5 * dec + dec - 1, 7 * dec + 1, 33):
            seed += 1
            reqs.append(request(f"short_{rate}_{in_samples}", seed, rate, 1 + seed % 3, ("noise", "sine", "mixed")[seed % 3],
                                in_samples=in_samples, extra=seed % 3, out_frames=37, block_frames=10))
    for rate, out_frames, block in ((44100, 100, 44), (96000, 97, 96), (192000, 50, 192), (176400, 177, 176), (88200, 7, 1),
                                    (48000, 1, 48), (192000, 3, 2), (96000, 5, 3), (176400, 1000, 7)):
        seed += 1
        reqs.append(request(f"blocks_{rate}_{out_frames}_{block}", seed, rate, 2 + seed % 2, "noise", out_frames=out_frames, block_frames=block))
    for ch in range(1, 11):
        seed += 1
        reqs.append(request(f"channels_{ch}", seed, RATES[ch % len(RATES)], ch, "mixed", out_frames=61, block_frames=16))
    return reqs


def lanes_batch(n_lanes, seed):
    """Requests whose channel counts (1..10, mixed) add up to exactly n_lanes, mixed rates (a different decimated count per lane),
    short outputs."""
    reqs, left, k = [], n_lanes, 0
    while left > 0:
        ch = min(left, 1 + (seed + 3 * k) % 10)
        rate = RATES[(seed + k) % len(RATES)]
        reqs.append(request(f"lanes{n_lanes}_{k}", seed * 10000 + k, rate, ch, ("noise", "sine", "mixed", "square")[k % 4],
                            extra=k % 2, out_frames=23 + k % 9, block_frames=5 + k % 7))
        left -= ch
        k += 1
    assert sum(r["channels"] for r in reqs) == n_lanes
    return reqs


LANE_COUNTS = (1, 63, 64, 65, 3000)


def layout(reqs, unaligned=True):
    """Packs the requests' planes into one source arena and their outputs into one destination arena, at odd offsets when
    `unaligned`.  Returns (src, [(src_offset, dst_offset)], dst_bytes)."""
    parts, offs, sp, dp = [], [], 0, 0
    for k, r in enumerate(reqs):
        pad = (k * 3) % 5 if unaligned else 0
        parts.append(np.full(pad, 0x5A, dtype=np.uint8))
        sp += pad
        offs.append((sp, dp + (k % 4 if unaligned else 0)))
        parts.append(r["blob"])
        sp += r["blob"].size
        dp += r["out_frames"] * r["channels"] * 4 + (8 if unaligned else 0)
    return np.concatenate(parts), offs, dp
