// dsd_pcm_core.h -- DSD -> PCM straight from the specification (include/ohgpu.h): one output value at a time, one bit at a
// time.  The text is __host__ __device__: dsd_pcm_kernel_v1 (csrc/dsd_pcm_kernel.hip) runs it on the device, and
// tests/cpp/dsd_pcm_core_driver.cpp builds it for the CPU under AddressSanitizer and UBSan and holds it to tests/dsd_pcm_textbook.py.
// The ramp and the pack are the expressions of pcm_device.h (ramp_index, ramp_word at three bytes, store_word) restated without
// device intrinsics, so that the CPU build runs them too; the fast kernel's epilogue uses pcm_device.h itself.
#pragma once

#include <stdint.h>

#include "../../include/ohgpu.h"

#if defined(__HIPCC__)
#define DSDPCM_HD __host__ __device__ inline
#else
#define DSDPCM_HD inline
#endif

namespace dsdpcm {

// Bit n of channel ch (0: left) of a stream whose chunk `chunk0` starts at win; P pad bytes per chunk.  n < 0: the idle pattern.
DSDPCM_HD uint32_t stream_bit(const uint8_t* win, uint64_t chunk0, uint32_t P, uint32_t ch, int64_t n)
{
    if (n < 0) return (OHGPU_DSD_SILENCE_BYTE >> (7u - (uint32_t)(n & 7))) & 1u;      // (two's complement: n & 7 is the non-negative modulo)
    const uint64_t j = (uint64_t)n >> 4;
    const uint32_t r = (uint32_t)n & 15u;
    const uint8_t byte = win[(j - chunk0) * (4u + P) + (ch ? P + 2u : P / 2u) + (r >> 3)];
    return ((uint32_t)byte >> (7u - (r & 7u))) & 1u;
}

// y of output frame m: every partial sum stays below sum|coef| < 2^30
DSDPCM_HD int32_t output_s24(const int32_t* coef, uint32_t N, uint32_t D, const uint8_t* win, uint64_t chunk0, uint32_t P, uint32_t ch, uint64_t m)
{
    const int64_t newest = (int64_t)((m + 1u) * D) - 1;
    int32_t acc = 0;
    for (uint32_t k = 0; k < N; k++) acc += stream_bit(win, chunk0, P, ch, newest - (int64_t)k) ? coef[k] : -coef[k];
    const int32_t y = (acc + 16) >> 5;
    return y > 8388607 ? 8388607 : (y < -8388608 ? -8388608 : y);
}

// RampApplicator's 24-bit case (Msg.cpp:835-895) on an S24 value: frame i of n, the table's 512 Q15 entries.  The ramped 24 bits.
DSDPCM_HD uint32_t ramp_s24(int32_t y, uint32_t i, uint32_t n, uint32_t start, uint32_t end, const uint16_t* table)
{
    const int32_t total = (int32_t)start - (int32_t)end;
    uint32_t ramp = n == 1 ? start : start - (uint32_t)(((int32_t)i * total) / (int32_t)(n - 1u));
    ramp &= 0xffffu;
    uint32_t idx = (OHGPU_RAMP_MAX - ramp + 16u) >> 5;
    if (idx > 511u) idx = 511u;
    const int32_t s16 = y >> 8;                                       // the top 16 of the 24 bits, signed
    const int32_t r = (s16 * (int32_t)table[idx]) >> 15;
    return ((uint32_t)r & 0xffffu) << 8;                              // the low byte is zeroed
}

DSDPCM_HD void store_s24(uint8_t* p, uint32_t v, bool little)
{
    if (little) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); }
    else        { p[0] = (uint8_t)(v >> 16); p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)v; }
}

// Output value q = 2 * frame + channel of message d, frames counted from the message's first
DSDPCM_HD void convert_value(const ohgpu_dsd_pcm_msg_desc& d, const int32_t* coef, uint32_t N, uint32_t D, const uint8_t* src,
                             uint8_t* dst, const uint16_t* ramp_table, uint64_t q)
{
    const uint32_t i = (uint32_t)(q >> 1), ch = (uint32_t)q & 1u;
    const int32_t y = output_s24(coef, N, D, src + d.src_offset, d.src_chunk0, d.pad_bytes_per_chunk, ch, d.out_frame0 + i);
    uint32_t v = (uint32_t)y & 0xffffffu;
    if (d.flags & OHGPU_FLAG_RAMP) v = ramp_s24(y, i, d.n_frames, d.ramp_start, d.ramp_end, ramp_table);
    store_s24(dst + d.dst_offset + q * 3u, v, d.dst_endian == OHGPU_ENDIAN_LITTLE);
}

}  // namespace dsdpcm
