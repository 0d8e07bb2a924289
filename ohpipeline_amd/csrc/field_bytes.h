// field_bytes.h -- the one reader of header fields for the container walks (csrc/mp4_box_core.h with csrc/mp4_frag_core.h,
// csrc/iff_chunk_core.h, csrc/dsd_file_core.h): a field of 1, 2, 4 or 8 bytes, little- or big-endian, at any address.  g++ and hipcc both
// compile it, as they do the cores: the kernels run this text on the device, the cores' CPU drivers and tests/cpp/field_bytes_driver.cpp
// run it under the sanitizers.  (csrc/ogg_page_core.h's le32(p) and csrc/ohm_rx_core.h's ld32 / be32(p) have another contract -- an
// address the caller has aligned, or plain bytes with no switch -- and are not this reader.)
//
// The caller has made sure that [pos, pos + width) lies inside the stream.  On the device, or with OHGPU_ALIGNED_READS defined (the CPU
// drivers build both readers), a field is read as the aligned dword(s) that hold it, joined by shifts, so that every dword load is
// aligned whatever the field's address (four byte loads in a row are merged by the compiler into one dword load at the field's own
// address) -- and never a dword that holds none of its bytes.  The dwords that hold a stream's first and last bytes reach up to three
// bytes beyond it: include/ohgpu.h states that as the source arena's requirement, and it rests on this reader and on nothing else.
// Otherwise a field is read byte by byte.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define FIELD_HD __host__ __device__ __forceinline__
#else
#define FIELD_HD inline
#endif

namespace fieldbytes {

constexpr uint32_t fourcc(char a, char b, char c, char d) { return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint8_t)d; }

#if defined(__HIP_DEVICE_COMPILE__) || defined(OHGPU_ALIGNED_READS)
FIELD_HD uint32_t u8(const uint8_t* p, uint64_t pos)
{
    const uintptr_t a = (uintptr_t)(p + pos);
    return (*(const uint32_t*)(a & ~(uintptr_t)3) >> ((uint32_t)(a & 3u) * 8u)) & 0xffu;
}
FIELD_HD uint32_t le16(const uint8_t* p, uint64_t pos)
{
    const uintptr_t a = (uintptr_t)(p + pos);
    const uint32_t* w = (const uint32_t*)(a & ~(uintptr_t)3);
    const uint32_t shift = (uint32_t)(a & 3u) * 8u;
    uint32_t v = w[0] >> shift;
    if (shift == 24u) v |= w[1] << 8;                 // the one address mod 4 at which the field has a byte in the next dword
    return v & 0xffffu;
}
FIELD_HD uint32_t le32(const uint8_t* p, uint64_t pos)
{
    const uintptr_t a = (uintptr_t)(p + pos);
    const uint32_t* w = (const uint32_t*)(a & ~(uintptr_t)3);
    const uint32_t shift = (uint32_t)(a & 3u) * 8u;
    uint32_t v = w[0];
    if (shift) v = (v >> shift) | (w[1] << (32u - shift));
    return v;
}
#else
FIELD_HD uint32_t u8(const uint8_t* p, uint64_t pos) { return p[pos]; }
FIELD_HD uint32_t le16(const uint8_t* p, uint64_t pos) { return (uint32_t)p[pos] | ((uint32_t)p[pos + 1] << 8); }
FIELD_HD uint32_t le32(const uint8_t* p, uint64_t pos) { return (uint32_t)p[pos] | ((uint32_t)p[pos + 1] << 8) | ((uint32_t)p[pos + 2] << 16) | ((uint32_t)p[pos + 3] << 24); }
#endif
FIELD_HD uint32_t be16(const uint8_t* p, uint64_t pos) { const uint32_t v = le16(p, pos); return ((v & 0xffu) << 8) | (v >> 8); }
FIELD_HD uint32_t be32(const uint8_t* p, uint64_t pos) { return __builtin_bswap32(le32(p, pos)); }
FIELD_HD uint64_t le64(const uint8_t* p, uint64_t pos) { return (uint64_t)le32(p, pos) | ((uint64_t)le32(p, pos + 4) << 32); }
FIELD_HD uint64_t be64(const uint8_t* p, uint64_t pos) { return ((uint64_t)be32(p, pos) << 32) | be32(p, pos + 4); }

}  // namespace fieldbytes
