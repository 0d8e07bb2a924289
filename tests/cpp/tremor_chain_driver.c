/* tremor_chain_driver.c -- Tremor's FILE interface (vorbisfile.c) over a chained Ogg Vorbis file, as the reference's CodecVorbis
 * drives it: callbacks that cannot seek, ov_read until it answers 0, OV_HOLE passed over as CodecVorbis::Process passes it over
 * ("attempting to continue decoding", Codec/Vorbis.cpp:388-391).  Per read one line "<bitstream index> <channels> <rate> <bytes>"
 * on the standard output (ov_info asked after every read, as CodecVorbis::Process asks it at a new bitstream), the samples -- 16-bit,
 * interleaved, as ov_read writes them on this host: little-endian -- appended to the output file.
 * tests/test_chained_tremor.py compiles it with Tremor, vorbisfile.c among it, and its libogg into pytest's temporary directory.
 * Exit status 0 and a last line "OK <reads> <holes>"; 3 when Tremor refuses the file, 4 when a read answers an error. */
#include <stdio.h>

#include "ivorbisfile.h"   /* (brings ivorbiscodec.h and ogg/ogg.h along) */

static size_t read_bytes(void* to, size_t size, size_t n, void* source) { return fread(to, size, n, (FILE*)source); }
static int no_seek(void* source, ogg_int64_t offset, int whence) { (void)source; (void)offset; (void)whence; return -1; }
static int no_close(void* source) { (void)source; return 0; }
static long no_tell(void* source) { (void)source; return -1; }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s file.ogg out.pcm\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    ov_callbacks cb;
    cb.read_func = read_bytes; cb.seek_func = no_seek; cb.close_func = no_close; cb.tell_func = no_tell;
    OggVorbis_File chain;
    const int rc = ov_open_callbacks(in, &chain, NULL, 0, cb);
    if (rc != 0) { fprintf(stderr, "ov_open_callbacks: %d\n", rc); return 3; }
    static char buffer[8192];
    long reads = 0, holes = 0;
    long n = 1;
    while (n != 0) {
        int bitstream = -1;
        n = ov_read(&chain, buffer, (int)sizeof(buffer), &bitstream);
        if (n == 0) continue;
        if (n == OV_HOLE) { holes++; continue; }
        if (n < 0) { fprintf(stderr, "ov_read: %ld\n", n); return 4; }
        const vorbis_info* vi = ov_info(&chain, -1);
        printf("%d %d %ld %ld\n", bitstream, vi->channels, vi->rate, n);
        fwrite(buffer, 1, (size_t)n, out);
        reads++;
    }
    fclose(out);
    ov_clear(&chain);
    fclose(in);
    printf("OK %ld %ld\n", reads, holes);
    return 0;
}
