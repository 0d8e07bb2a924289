# LDS bank-conflict model (MI355X_MICROARCH.md): ds_read_b64: 2 groups of 32 lanes, 64 banks of 4 B; cost of a group = max over banks of distinct dword addresses
import itertools
def read_b64_cycles(addrs):   # addrs: 64 byte addresses (4-aligned), each reads 8 bytes
    tot = 0
    for grp in (range(0, 32), range(32, 64)):
        banks = {}
        for l in grp:
            for dw in (addrs[l] // 4, addrs[l] // 4 + 1):
                banks.setdefault(dw % 64, set()).add(dw)
        tot += max(len(v) for v in banks.values())
    return tot
def write_b16_cycles(addrs):  # 2 groups of 32, 32 banks
    tot = 0
    for grp in (range(0, 32), range(32, 64)):
        banks = {}
        for l in grp:
            dw = addrs[l] // 4
            banks.setdefault(dw % 32, set()).add(dw)
        tot += max(len(v) for v in banks.values())
    return tot

# ---- the 16-byte forms, and the stereo S24 split of src_mfma_wg_kernel.hip: the lane roles it has, and two it was measured against ----
# ("LDS work per tile": both conflict-free roles were built, bit-exact, and no faster on the GPU -- the kernel keeps lane = row)
# ds_read_b128: four groups of sixteen lanes, NOT contiguous (MI355X_MICROARCH.md, LDS), 64 banks; ds_write_b128: eight groups of
# eight contiguous lanes, 32 banks; ds_read2_b32: two ds_read_b32 (2 x 32 lanes, 32 banks)
B128_GROUP_A = [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27]
B128_GROUP_B = [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]
B128_GROUPS = [B128_GROUP_A, B128_GROUP_B, [l + 32 for l in B128_GROUP_A], [l + 32 for l in B128_GROUP_B]]
def _group_cycles(addrs, lanes, dwords, banks_n):
    """LDS cycles of one lane group: the most distinct dword addresses any bank is asked for (the same address is a broadcast)."""
    banks = {}
    for l in lanes:
        if addrs[l] is None: continue                      # (a lane that sits the instruction out)
        for k in range(dwords):
            dw = addrs[l] // 4 + k
            banks.setdefault(dw % banks_n, set()).add(dw)
    return max((len(v) for v in banks.values()), default=0)
def read_b128_cycles(addrs):
    assert all(a is None or a % 16 == 0 for a in addrs)
    return sum(_group_cycles(addrs, grp, 4, 64) for grp in B128_GROUPS)
def write_b128_cycles(addrs):
    assert all(a is None or a % 16 == 0 for a in addrs)
    return sum(_group_cycles(addrs, range(8 * k, 8 * k + 8), 4, 32) for k in range(8))
def read_b32_cycles(addrs):
    return sum(_group_cycles(addrs, grp, 1, 32) for grp in (range(0, 32), range(32, 64)))
def read_b64_group_cycles(addrs):                          # as read_b64_cycles, lanes may sit out
    return sum(_group_cycles(addrs, grp, 2, 64) for grp in (range(0, 32), range(32, 64)))

ST_ROWS, ST_HC, ST_ROW_IN, ST_HALF, ST_CHUNK = 16, 24, 1152, 256, 512    # stereo: pair-rows of a pass, half chunks of a row, WgGeom::kRowIn, kHalf, kChunk
def stereo_lane_task(wave, lane, rnd):
    """Tried, not kept -- every row's image 16-byte aligned, 1152 bytes apart, lanes by ds_read_b128's groups: (row, half chunk) of a
    lane in round 0 (every wave) and round 1 (waves 0 and 1), or None."""
    q = (lane & 31) >> 2
    grp = 2 * (lane >> 5) + ((0x96 >> q) & 1)
    idx = 4 * (q >> 1) + (lane & 3)
    assert B128_GROUPS[grp][idx] == lane                 # the arithmetic above IS the table of lane groups
    if rnd == 0:
        return wave + 4 * grp, 2 * (idx & 3) + ((idx >> 2) & 1) + 8 * (idx >> 3)
    if wave >= 2:
        return None
    return 2 * wave + 4 * grp + (idx >> 3), 16 + 2 * (idx & 3) + ((idx >> 2) & 1)
def stereo_union_lane_task(wave, lane, rnd):
    """The kernel's roles on the union run: lane = row, sixteen lanes a half chunk."""
    tid = 64 * wave + lane
    hc = tid // 16 + 16 * rnd
    return (tid % 16, hc) if hc < ST_HC else None
def stereo_union_group_task(wave, lane, rnd):
    """Tried, not kept -- the union run, a half wave = rows a, a + 2, a + 4, a + 6 x eight half chunks: at 882 bytes a row, rows two
    apart start one bank further on and eight half chunks meet eight banks four apart; eight contiguous lanes are those four rows x
    half chunks h and h + 2 (swizzle 1)."""
    b = (lane & 31) >> 2
    hcl = (b & 4) | ((b & 1) << 1) | ((b >> 1) & 1)
    g = 2 * wave + (lane >> 5)
    row = (g & 1) + 8 * ((g >> 1) & 1) + 2 * (lane & 3)
    if rnd == 0:
        return row, 8 * (g >> 2) + hcl
    return (row, 16 + hcl) if wave < 2 else None
def stereo_plane_slot(row, hc, swizzle=0):
    """Byte offset in a digit plane of the 16 bytes of (row, half chunk): [chunk][half][column tile][row 8][16 bytes], odd chunks with
    their column tiles swapped; `swizzle`: a row's slot XORed with chunk & swizzle (0: the kernel's layout)."""
    c = hc >> 1
    return c * ST_CHUNK + (((hc & 1) * ST_HALF + row * 16) ^ ((c & 1) * 128) ^ ((c & swizzle) * 16))
def stereo_split_model(task=stereo_union_lane_task, aligned=False, row_src_bytes=882, swizzle=0):
    """{"tasks": every (row, half chunk) once?, "read_cycles", "read_ideal", "store_cycles", "store_ideal"} of a pass's split."""
    seen, rc, ri, sc, si = [], 0, 0, 0, 0
    for rnd in (0, 1):
        for wave in range(4):
            tasks = [task(wave, l, rnd) for l in range(64)]
            if all(t is None for t in tasks): continue
            seen += [t for t in tasks if t is not None]
            if aligned:                                     # three ds_read_b128 of the row's own image
                for k in range(3):
                    rc += read_b128_cycles([None if t is None else t[0] * ST_ROW_IN + t[1] * 48 + 16 * k for t in tasks]); ri += 4
            else:                                           # thirteen dwords around 48 bytes at an even address of the union run
                for k in range(13):
                    rc += read_b32_cycles([None if t is None else ((t[0] * row_src_bytes + t[1] * 48) & ~3) + 4 * k for t in tasks]); ri += 2
            sc += write_b128_cycles([None if t is None else stereo_plane_slot(t[0], t[1], swizzle) for t in tasks]); si += 8
    return {"tasks_once": sorted(seen) == [(r, h) for r in range(ST_ROWS) for h in range(ST_HC)], "read_cycles": rc, "read_ideal": ri, "store_cycles": sc, "store_ideal": si}
def stereo_tile_read_model(swizzle=0):
    """The tiles' ds_read_b64 (issue_planes): lane (g, n) of column tile ct reads 8 bytes of row 8 ct + n / 2, chunk kc + g, either half:
    (cycles, ideal) over every kc and ct, and whether every lane finds the bytes the split stored for it."""
    cyc, ideal, right = 0, 0, True
    for kc in range(9):
        for ct in range(2):
            for half in (0, 1):
                addrs = []
                for l in range(64):
                    g, n = l >> 4, l & 15
                    c = kc + g
                    a = c * ST_CHUNK + ((ct * 128 + n * 8) ^ ((c & 1) * 128) ^ ((c & swizzle) * 16)) + half * ST_HALF
                    right &= a == stereo_plane_slot(8 * ct + n // 2, 2 * c + half, swizzle) + 8 * (n & 1)
                    addrs.append(a)
                cyc += read_b64_group_cycles(addrs); ideal += 2
    return cyc, ideal, right
def stereo_report():
    for name, kw in (("union run, lane = row (the kernel)", dict()),
                     ("union run, half wave = 4 rows x 8 half chunks, slots ^ (chunk & 1) (tried)", dict(task=stereo_union_group_task, swizzle=1)),
                     ("aligned rows, lane = row", dict(aligned=True)),
                     ("aligned rows, lanes by LDS group, no swizzle", dict(task=stereo_lane_task, aligned=True)),
                     ("aligned rows, lanes by LDS group, slots ^ (chunk & 3) (tried)", dict(task=stereo_lane_task, aligned=True, swizzle=3))):
        print("stereo split, %s: %s" % (name, stereo_split_model(**kw)))
    print("stereo tile reads (cycles, ideal, addresses agree) by swizzle:", {sw: stereo_tile_read_model(sw) for sw in (0, 1, 3)})

def six_channel_report():
    global PAIRS, kFb, row_src, kRowOut
    PAIRS, kFb, row_src = 3, 18, 147 * 18
    def split_reads(mapping):
        tot = 0; n = 0
        for wave in range(4):
            for rnd in range(2):
                for m in range(4):
                    for odd in (0, 1):
                        addrs = []
                        for l in range(64):
                            sp_row, hc_local = mapping(l)
                            hc = 4 * wave + hc_local + 16 * rnd
                            if hc >= 24: hc = 4 * wave + hc_local      # inactive lanes: whatever
                            used = min(sp_row, 14)
                            srow, pair = used // 3, used % 3
                            byte0 = srow * row_src + 6 * pair + hc * 8 * kFb + odd * kFb
                            addrs.append((byte0 & ~3) + 2 * kFb * m)
                        tot += read_b64_cycles(addrs); n += 1
        return tot / n
    cur = lambda l: (l % 16, l // 16)
    alt = lambda l: ((l & 7) | ((l >> 2) & 8), (l >> 3) & 3)
    alt2 = lambda l: ((l & 3) | ((l >> 2) & 12), (l >> 2) & 3)
    print("split reads, avg LDS cycles per ds_read_b64 (ideal 2): current %.2f  alt(8 rows x 4 hc per half) %.2f  alt2(4 rows x 4 hc ...) %.2f" % (split_reads(cur), split_reads(alt), split_reads(alt2)))
    # epilogue stores: lane (g, n): pr = ct*8 + 2g + q, sr = pr // 3; at = sr*kRowOut + 6*(pr - 3 sr) + kFb*n + 16*kFb*step ; three b16 at +0, +2, +4
    kRowOut = 160 * kFb
    def epi(pad_row=0, frame_pitch=kFb):
        tot = 0; n = 0
        for ct in range(2):
            for q in range(2):
                for off in (0, 2, 4):
                    addrs = []
                    for l in range(64):
                        g, nn = l >> 4, l & 15
                        pr = ct * 8 + 2 * g + q; sr = pr // 3
                        addrs.append(sr * (kRowOut + pad_row) + 6 * (pr - 3 * sr) + frame_pitch * nn + off)
                    tot += write_b16_cycles(addrs); n += 1
        return tot / n
    print("epilogue b16 stores, avg LDS cycles (ideal 2): now %.2f ; row pad 16: %.2f; row pad 64: %.2f" % (epi(), epi(16), epi(64)))
    print("--- by channel count")
    for P in (1, 3, 4):
        PAIRS, kFb = P, 6 * P
        row_src = 147 * kFb; kRowOut = 160 * kFb
        def epiP(pad_row=0):
            tot = 0; n = 0
            for ct in range(2):
                for q in range(2):
                    for off in (0, 2, 4):
                        addrs = []
                        for l in range(64):
                            g, nn = l >> 4, l & 15
                            pr = ct * 8 + 2 * g + q; sr = pr // P
                            addrs.append(sr * (kRowOut + pad_row) + 6 * (pr - P * sr) + kFb * nn + off)
                        tot += write_b16_cycles(addrs); n += 1
            return tot / n
        print("PAIRS", P, "epilogue b16: now %.2f" % epiP(), " pads:", {p: round(epiP(p), 2) for p in (4, 8, 16, 32, 64, 128)})
    print("--- six channels: row pitch sweep (16-byte aligned pitches)")
    PAIRS, kFb = 3, 18
    kRowOut = 160 * kFb
    res = {}
    for pad in range(0, 513, 16):
        tot = 0; n = 0
        for ct in range(2):
            for q in range(2):
                for off in (0, 2, 4):
                    addrs = []
                    for l in range(64):
                        g, nn = l >> 4, l & 15
                        pr = ct * 8 + 2 * g + q; sr = pr // 3
                        addrs.append(sr * (kRowOut + pad) + 6 * (pr - 3 * sr) + kFb * nn + off)
                    tot += write_b16_cycles(addrs); n += 1
        res[pad] = tot / n
    print({k: round(v, 2) for k, v in res.items() if v <= 4.01})
    # what limits: within a 32-lane group: g in {0,1} (or {2,3}), n 0..15: two (row, pair) x 16 frames 18 B apart: 16 frames span 288 B = 72 dwords over 32 banks
    for P, kFb in ((1, 6), (3, 18), (4, 24)):
        addrs = [kFb * nn for nn in range(16)]
        banks = {}
        for a in addrs:
            banks.setdefault((a // 4) % 32, set()).add(a // 4)
        print("one row's 16 frames, kFb", kFb, "max dwords per bank:", max(len(v) for v in banks.values()))

if __name__ == "__main__":
    stereo_report()
    six_channel_report()
