// field_bytes_driver.cpp -- csrc/field_bytes.h's reader on the CPU, for tests/test_field_bytes_cpu.py (built with
// -fsanitize=address,undefined -fno-sanitize-recover=all, once as it is -- byte reads -- and once with -DOHGPU_ALIGNED_READS, the
// device's reader).  Every width (u8, le16 / be16, le32 / be32, le64 / be64) is read at offsets 0 to 7 of one 16-byte pattern, so at
// every address mod 4, and compared with the value assembled here from the bytes.  Each read is made from a heap block of its own that
// begins with the dword that holds the field's first byte and ends exactly at the end of the dword that holds its last: a reader that
// touches a dword that holds none of the field's bytes, in front or behind, is AddressSanitizer's to report.  Prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../ohpipeline_amd/csrc/field_bytes.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s (offset %u)\n", __FILE__, __LINE__, #cond, off); exit(1); } \
    } while (0)

namespace {

// (every byte differs, most have the top bit set: a sign extension or a swapped pair shows)
const uint8_t kPattern[16] = {0x81, 0x92, 0xa3, 0xb4, 0xc5, 0xd6, 0xe7, 0xf8, 0x09, 0x1a, 0x2b, 0x3c, 0x4d, 0x5e, 0x6f, 0x70};

uint64_t by_hand(uint32_t off, uint32_t width, bool little)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < width; k++) v |= (uint64_t)kPattern[off + k] << (8u * (little ? k : width - 1u - k));
    return v;
}

// the dwords of the pattern that hold [off, off + width), alone in a heap block; *pos: where the field lies in it
uint8_t* holding_dwords(uint32_t off, uint32_t width, uint64_t* pos)
{
    const uint32_t first = off & ~3u, end = (off + width + 3u) & ~3u;
    uint8_t* const block = (uint8_t*)malloc(end - first);                // (aligned for any type, so for a dword)
    if (!block) exit(1);
    memcpy(block, kPattern + first, end - first);
    *pos = off - first;
    return block;
}

}  // namespace

int main()
{
    using namespace fieldbytes;
    static_assert(fourcc('f', 'L', 'a', 'C') == 0x664c6143u && fourcc('\xff', 'D', 'S', '\x80') == 0xff445380u, "fourcc: the first character is the top byte");
    for (uint32_t off = 0; off < 8; off++) {
        uint64_t pos = 0;
        uint8_t* p = holding_dwords(off, 1, &pos);
        CHECK(u8(p, pos) == by_hand(off, 1, true));
        CHECK(u8(p + pos, 0) == by_hand(off, 1, true));
        free(p);
        p = holding_dwords(off, 2, &pos);
        CHECK(le16(p, pos) == by_hand(off, 2, true) && be16(p, pos) == by_hand(off, 2, false));
        CHECK(le16(p + pos, 0) == by_hand(off, 2, true) && be16(p + pos, 0) == by_hand(off, 2, false));
        free(p);
        p = holding_dwords(off, 4, &pos);
        CHECK(le32(p, pos) == by_hand(off, 4, true) && be32(p, pos) == by_hand(off, 4, false));
        CHECK(le32(p + pos, 0) == by_hand(off, 4, true) && be32(p + pos, 0) == by_hand(off, 4, false));
        free(p);
        p = holding_dwords(off, 8, &pos);
        CHECK(le64(p, pos) == by_hand(off, 8, true) && be64(p, pos) == by_hand(off, 8, false));
        CHECK(le64(p + pos, 0) == by_hand(off, 8, true) && be64(p + pos, 0) == by_hand(off, 8, false));
        free(p);
    }
    printf("ok\n");
    return 0;
}
