/* vorbis_tremor_driver.c -- Tremor's packet interface over a case file of tests/test_vorbis_core_cpu.py (u32 bytes + identification
 * packet, u32 bytes + setup packet, u32 n, then n times u32 bytes + packet): the three headers in (the comment header is made here, empty),
 * every audio packet through vorbis_synthesis / vorbis_synthesis_blockin, and what vorbis_synthesis_pcmout gives written to the output
 * file as interleaved 16-bit little-endian samples, converted as Tremor's own file reader converts them (>> 9, clipped to 16 bits).
 * tests/test_vorbis_tremor.py compiles it with Tremor and its libogg into pytest's temporary directory.  A packet Tremor refuses is
 * passed over.  Exit status 0 and "OK <samples a channel>" on success, 3 when Tremor refuses a header. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <ogg/ogg.h>
#include "ivorbiscodec.h"

static unsigned char* blob(FILE* f, long* n)
{
    unsigned char len[4];
    if (fread(len, 1, 4, f) != 4) { fprintf(stderr, "case file too short\n"); exit(2); }
    *n = (long)len[0] | ((long)len[1] << 8) | ((long)len[2] << 16) | ((long)len[3] << 24);
    unsigned char* p = malloc(*n ? (size_t)*n : 1);
    if (*n && fread(p, 1, (size_t)*n, f) != (size_t)*n) { fprintf(stderr, "case file too short\n"); exit(2); }
    return p;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s case out\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!f || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    static unsigned char comment[] = {3, 'v', 'o', 'r', 'b', 'i', 's', 0, 0, 0, 0, 0, 0, 0, 0, 1};
    vorbis_info vi;
    vorbis_comment vc;
    vorbis_info_init(&vi);
    vorbis_comment_init(&vc);
    ogg_packet op;
    memset(&op, 0, sizeof(op));
    long n = 0;
    for (int h = 0; h < 3; h++) {
        op.packet = h == 1 ? comment : blob(f, &n);
        op.bytes = h == 1 ? (long)sizeof(comment) : n;
        op.b_o_s = h == 0;
        op.packetno = h;
        const int rc = vorbis_synthesis_headerin(&vi, &vc, &op);
        if (rc != 0) { fprintf(stderr, "Tremor refuses header %d: %d\n", h, rc); return 3; }
    }
    vorbis_dsp_state vd;
    vorbis_block vb;
    if (vorbis_synthesis_init(&vd, &vi) != 0) { fprintf(stderr, "vorbis_synthesis_init failed\n"); return 3; }
    vorbis_block_init(&vd, &vb);
    unsigned char len[4];
    if (fread(len, 1, 4, f) != 4) return 2;
    const long packets = (long)len[0] | ((long)len[1] << 8) | ((long)len[2] << 16) | ((long)len[3] << 24);
    long total = 0;
    for (long k = 0; k < packets; k++) {
        op.packet = blob(f, &n);
        op.bytes = n;
        op.b_o_s = 0;
        op.packetno = 3 + k;
        op.granulepos = -1;
        if (vorbis_synthesis(&vb, &op) == 0) vorbis_synthesis_blockin(&vd, &vb);
        ogg_int32_t** pcm;
        int samples;
        while ((samples = vorbis_synthesis_pcmout(&vd, &pcm)) > 0) {
            for (int i = 0; i < samples; i++)
                for (int c = 0; c < vi.channels; c++) {
                    long v = pcm[c][i] >> 9;
                    if (v > 32767) v = 32767;
                    if (v < -32768) v = -32768;
                    const unsigned char two[2] = {(unsigned char)(v & 0xff), (unsigned char)((v >> 8) & 0xff)};
                    fwrite(two, 1, 2, out);
                }
            total += samples;
            vorbis_synthesis_read(&vd, samples);
        }
        free(op.packet);
    }
    fclose(out);
    printf("OK %ld\n", total);
    return 0;
}
