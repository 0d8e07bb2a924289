// dsd_perm.h -- the compile-time byte permutation of the DSD packers: which source byte each byte of a lane's eight output chunks is,
// and the one v_perm_b32 per output dword that follows from it.  csrc/dsd_line_kernel.hip (audio runs the caller has found) and
// csrc/dsd_file_kernel.hip (DSF and DFF files, through csrc/dsd_file_core.h) share it; the selectors are plain constant expressions,
// so the file layer's CPU driver evaluates the same table.
#pragma once

#include <stdint.h>

#include "../../include/ohgpu.h"

namespace ohgpu {

// Where byte t of a lane's 8 * (4 + P) output bytes comes from: -1 for padding, else 4 * (input dword) + (byte of it), the input
// being the lane's eight dwords in[0..7] -- DSF: in[0..3] the left plane's sixteen bytes, in[4..7] the right plane's, each dword
// already bit-reversed, so that source byte b of a dword sits at 3 - b; DFF and Raw: dword c is chunk c's four source bytes.
static constexpr int dsd_src_of(int kind, int P, int t)
{
    const int cs = 4 + P, c = t / cs, o = t % cs, h = P / 2;
    int ch = 0, i = 0;
    if (o < h) return -1;
    if (o < h + 2) { ch = 0; i = o - h; }
    else if (o < 2 * h + 2) return -1;
    else { ch = 1; i = o - 2 * h - 2; }
    if (kind == OHGPU_DSD_DSF) return (ch * 4 + c / 2) * 4 + (3 - ((c & 1) * 2 + i));
    if (kind == OHGPU_DSD_DFF) return c * 4 + ch + 2 * i;               // s0 s2 | s1 s3
    return c * 4 + ch * 2 + i;                                          // s0 s1 | s2 s3
}

struct DsdPerm { int lo, hi; uint32_t sel; bool ok; };
// Output dword D as v_perm_b32 {in[hi] (selector bytes 4-7), in[lo] (0-3)}; 0x0c selects a zero byte.
static constexpr DsdPerm dsd_perm(int kind, int P, int D)
{
    DsdPerm p{-1, -1, 0, true};
    for (int k = 0; k < 4; k++) {
        const int s = dsd_src_of(kind, P, 4 * D + k);
        uint32_t code = 0x0c;
        if (s >= 0) {
            const int dw = s >> 2, by = s & 3;
            if (p.lo < 0 || p.lo == dw) { p.lo = dw; code = (uint32_t)by; }
            else if (p.hi < 0 || p.hi == dw) { p.hi = dw; code = 4u + (uint32_t)by; }
            else p.ok = false;
        }
        p.sel |= code << (8 * k);
    }
    if (p.lo < 0) p.lo = 0;
    if (p.hi < 0) p.hi = p.lo;
    return p;
}

#if defined(__HIPCC__)
typedef uint32_t dv4 __attribute__((ext_vector_type(4)));

template <int KIND, int P, int D>
__device__ __forceinline__ uint32_t dsd_out_dword(const uint32_t (&in)[8])
{
    constexpr DsdPerm p = dsd_perm(KIND, P, D);
    static_assert(p.ok, "an output dword draws on at most two input dwords");
    return __builtin_amdgcn_perm(in[p.hi], in[p.lo], p.sel);
}

template <int KIND, int P, int V>
__device__ __forceinline__ void dsd_store_vec(const uint32_t (&in)[8], uint8_t* out)
{
    const dv4 o = {dsd_out_dword<KIND, P, 4 * V>(in), dsd_out_dword<KIND, P, 4 * V + 1>(in), dsd_out_dword<KIND, P, 4 * V + 2>(in),
                   dsd_out_dword<KIND, P, 4 * V + 3>(in)};
    __builtin_nontemporal_store(o, (dv4*)(out + 16 * V));               // written once, never read here
}
#endif

}  // namespace ohgpu
