// dsd_pcm_core_driver.cpp -- csrc/dsd_pcm_core.h on the CPU: every output value of every message of a file of batches through
// dsdpcm::convert_value, the call csrc/dsd_pcm_kernel.hip's plain kernel makes per thread.  tests/test_dsd_pcm_core_cpu.py builds this
// with -fsanitize=address,undefined and holds the whole destination arenas against tests/dsd_pcm_textbook.py.
// Every buffer is allocated at exactly its declared size, so that a load or a store outside a range is a sanitizer report.
//
// in:  u16 ramp_table[512]; u32 n; then per batch { u32 D, T, n_descs, fill; u64 src_bytes, dst_bytes; i32 coef[D * T];
//      ohgpu_dsd_pcm_msg_desc descs[n_descs]; src_bytes of source arena }
// out: per batch its destination arena
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dsd_pcm_core.h"

struct Head { uint32_t D, T, n_descs, fill; uint64_t src_bytes, dst_bytes; };

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    uint16_t table[512];
    uint32_t n = 0;
    if (fread(table, 2, 512, in) != 512 || fread(&n, 4, 1, in) != 1) return 2;
    for (uint32_t k = 0; k < n; k++) {
        Head h;
        if (fread(&h, sizeof(h), 1, in) != 1) return 2;
        const uint32_t N = h.D * h.T;
        int32_t* coef = (int32_t*)malloc(N * sizeof(int32_t));
        ohgpu_dsd_pcm_msg_desc* descs = (ohgpu_dsd_pcm_msg_desc*)malloc(h.n_descs ? h.n_descs * sizeof(ohgpu_dsd_pcm_msg_desc) : 1);
        uint8_t* src = (uint8_t*)malloc(h.src_bytes ? h.src_bytes : 1);
        uint8_t* dst = (uint8_t*)malloc(h.dst_bytes ? h.dst_bytes : 1);
        if (fread(coef, sizeof(int32_t), N, in) != N) return 2;
        if (h.n_descs && fread(descs, sizeof(ohgpu_dsd_pcm_msg_desc), h.n_descs, in) != h.n_descs) return 2;
        if (h.src_bytes && fread(src, 1, h.src_bytes, in) != h.src_bytes) return 2;
        memset(dst, (int)h.fill, h.dst_bytes);
        for (uint32_t i = 0; i < h.n_descs; i++)
            for (uint64_t q = 0; q < 2ull * descs[i].n_frames; q++) dsdpcm::convert_value(descs[i], coef, N, h.D, src, dst, table, q);
        if (h.dst_bytes && fwrite(dst, 1, h.dst_bytes, out) != h.dst_bytes) return 2;
        free(coef); free(descs); free(src); free(dst);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
