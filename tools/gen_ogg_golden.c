/* gen_ogg_golden.c -- records what an Ogg page library's own writer and reader make of a dozen sessions, for tests/golden/ogg.
 * It calls the <ogg/ogg.h> interface and nothing else; tests/golden/make_ogg_fixtures.py compiles it against the reference tree's
 * copy of that library and runs it.  The binary is never committed.
 *   gen_ogg_golden OUTDIR     writes OUTDIR/NAME.ogg per session and OUTDIR/sessions.json
 * The reader expects page 0 first, as a stream state does after ogg_stream_init; where a session says any_seq it was reset first.
 * A session's bytes are muxed by the library's writer (packet k's byte i is (7 i + 13 k) & 255), then changed by hand where the
 * session says so -- a page dropped, a bit flipped, two bytes put in, the version or a flag patched and the checksum set again, the
 * end cut off.  The record is what the library's reader yields for one serial, page by page as libFLAC's Ogg layer drives it:
 *   ["sync"]                         ogg_sync_pageout returned -1
 *   ["refused", serial, seq, ver]    ogg_stream_pagein refused the page
 *   ["hole"]                         ogg_stream_packetout returned -1
 *   ["packet", bytes, granule, b_o_s, e_o_s, fnv1a32 of the bytes]
 */
#include <ogg/ogg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct { unsigned char* p; size_t n, cap; size_t page_at[64]; int pages; } Bytes;

static void put(Bytes* b, const void* src, size_t n)
{
    if (b->n + n > b->cap) { b->cap = (b->n + n) * 2 + 1024; b->p = (unsigned char*)realloc(b->p, b->cap); }
    memcpy(b->p + b->n, src, n);
    b->n += n;
}
static void put_page(Bytes* b, const ogg_page* og)
{
    if (b->pages < 64) b->page_at[b->pages] = b->n;
    b->pages++;
    put(b, og->header, (size_t)og->header_len);
    put(b, og->body, (size_t)og->body_len);
}
/* one logical stream: packets of the given sizes; flush[k] != 0 ends the page behind packet k */
static void mux(Bytes* out, int serial, const long* sizes, const int* flush, int n, int first_k)
{
    ogg_stream_state os;
    ogg_page og;
    int k;
    ogg_stream_init(&os, serial);
    for (k = 0; k < n; k++) {
        ogg_packet op;
        long i;
        unsigned char* data = (unsigned char*)malloc(sizes[k] ? (size_t)sizes[k] : 1);
        for (i = 0; i < sizes[k]; i++) data[i] = (unsigned char)((7 * i + 13 * (k + first_k)) & 255);
        memset(&op, 0, sizeof op);
        op.packet = data; op.bytes = sizes[k]; op.b_o_s = k == 0; op.e_o_s = k == n - 1;
        op.granulepos = 1000 * (ogg_int64_t)(k + 1); op.packetno = k;
        ogg_stream_packetin(&os, &op);
        free(data);
        while (ogg_stream_pageout(&os, &og) > 0) put_page(out, &og);
        if (flush && flush[k]) while (ogg_stream_flush(&os, &og) > 0) put_page(out, &og);
    }
    while (ogg_stream_flush(&os, &og) > 0) put_page(out, &og);
    ogg_stream_clear(&os);
}
/* the page at page_at[k], as the library sees it, for ogg_page_checksum_set */
static void reseal(Bytes* b, int k)
{
    ogg_page og;
    unsigned char* h = b->p + b->page_at[k];
    int s, body = 0;
    for (s = 0; s < h[26]; s++) body += h[27 + s];
    og.header = h; og.header_len = 27 + h[26];
    og.body = h + og.header_len; og.body_len = body;
    ogg_page_checksum_set(&og);
}
static void cut(Bytes* b, size_t from, size_t to)          /* bytes [from, to) go */
{
    memmove(b->p + from, b->p + to, b->n - to);
    b->n -= to - from;
}
static size_t page_end(const Bytes* b, int k) { return k + 1 < b->pages ? b->page_at[k + 1] : b->n; }

static unsigned fnv(const unsigned char* p, long n)
{
    unsigned h = 2166136261u;
    long i;
    for (i = 0; i < n; i++) { h ^= p[i]; h *= 16777619u; }
    return h;
}
static void read_back(const Bytes* b, int serial, int any_seq, FILE* js)
{
    ogg_sync_state oy;
    ogg_stream_state os;
    ogg_page og;
    ogg_packet op;
    size_t fed = 0;
    int first = 1, r;
    ogg_sync_init(&oy);
    ogg_stream_init(&os, serial);
    if (any_seq) ogg_stream_reset(&os);              /* as after a flush of the layer above: no page number is expected */
    for (;;) {
        r = ogg_sync_pageout(&oy, &og);
        if (r == 0) {
            size_t n = b->n - fed < 4096 ? b->n - fed : 4096;
            if (!n) break;
            memcpy(ogg_sync_buffer(&oy, (long)n), b->p + fed, n);
            ogg_sync_wrote(&oy, (long)n);
            fed += n;
            continue;
        }
        if (r < 0) { fprintf(js, "%s[\"sync\"]", first ? "" : ", "); first = 0; continue; }
        if (ogg_stream_pagein(&os, &og) != 0) {
            fprintf(js, "%s[\"refused\", %d, %ld, %d]", first ? "" : ", ", ogg_page_serialno(&og), ogg_page_pageno(&og), ogg_page_version(&og));
            first = 0;
            continue;
        }
        while ((r = ogg_stream_packetout(&os, &op)) != 0) {
            if (r < 0) fprintf(js, "%s[\"hole\"]", first ? "" : ", ");
            else fprintf(js, "%s[\"packet\", %ld, %lld, %d, %d, %u]", first ? "" : ", ", op.bytes, (long long)op.granulepos, op.b_o_s ? 1 : 0, op.e_o_s ? 1 : 0, fnv(op.packet, op.bytes));
            first = 0;
        }
    }
    ogg_stream_clear(&os);
    ogg_sync_clear(&oy);
}

static const char* g_dir;
static FILE* g_js;
static int g_first = 1;
static void finish(const char* name, Bytes* b, int serial, int any_seq, int keep, const char* what)
{
    char path[1024];
    FILE* f;
    snprintf(path, sizeof path, "%s/%s.ogg", g_dir, name);
    f = fopen(path, "wb");
    if (!f) { perror(path); exit(1); }
    fwrite(b->p, 1, b->n, f);
    fclose(f);
    fprintf(g_js, "%s\n  \"%s\": {\"serial\": %d, \"any_seq\": %d, \"bytes\": %lu, \"what\": \"%s\", \"events\": [", g_first ? "" : ",", name, serial, any_seq, (unsigned long)b->n, what);
    read_back(b, serial, any_seq, g_js);
    fprintf(g_js, "]}");
    g_first = 0;
    if (keep) return;
    free(b->p);
    memset(b, 0, sizeof *b);
}

int main(int argc, char** argv)
{
    Bytes b;
    char path[1024];
    if (argc != 2) { fprintf(stderr, "usage: %s OUTDIR\n", argv[0]); return 2; }
    g_dir = argv[1];
    snprintf(path, sizeof path, "%s/sessions.json", g_dir);
    g_js = fopen(path, "w");
    if (!g_js) { perror(path); return 1; }
    fprintf(g_js, "{\"sessions\": {");
    memset(&b, 0, sizeof b);

    { const long s[] = {0, 1, 254, 255, 256, 510, 65030};
      mux(&b, 0x1234, s, NULL, 7, 0); finish("sizes", &b, 0x1234, 0, 0, "packets of 0, 1, 254, 255, 256, 510 and 65030 bytes"); }
    { const long s[] = {10, 131000, 20};
      mux(&b, 0x1234, s, NULL, 3, 0); finish("three_pages", &b, 0x1234, 0, 0, "a packet over three pages, the middle one completing nothing"); }
    { const long s[] = {510, 765, 5}; const int fl[] = {1, 1, 1};
      mux(&b, 0x1234, s, fl, 3, 0); finish("ends_on_255k", &b, 0x1234, 0, 0, "pages that end exactly on packets of 255 k bytes"); }
    { const long s1[] = {300, 20, 70}, s2[] = {40, 600, 9}; const int fl[] = {1, 1, 1};
      Bytes x, y; int k;
      memset(&x, 0, sizeof x); memset(&y, 0, sizeof y);
      mux(&x, 0x1234, s1, fl, 3, 0); mux(&y, 0x4321, s2, fl, 3, 3);
      for (k = 0; k < 3; k++) { put(&b, x.p + x.page_at[k], page_end(&x, k) - x.page_at[k]); put(&b, y.p + y.page_at[k], page_end(&y, k) - y.page_at[k]); }
      free(x.p); free(y.p);
      finish("two_serials", &b, 0x1234, 0, 0, "two logical streams, their pages interleaved"); }
    { const long s[] = {30, 40, 50}; const int fl[] = {1, 1, 1};
      mux(&b, 0x1234, s, fl, 3, 0); b.p[b.page_at[1] + 4] = 1; reseal(&b, 1);
      finish("version_1", &b, 0x1234, 0, 0, "the second page says version 1 and has a good checksum"); }
    { const long s[] = {100, 100, 70000, 50}; const int fl[] = {1, 1, 0, 1};
      mux(&b, 0x1234, s, fl, 4, 0); cut(&b, b.page_at[2], page_end(&b, 2));
      finish("gap", &b, 0x1234, 0, 0, "the page a long packet begins on is missing"); }
    { const long s[] = {100, 100, 100}; const int fl[] = {1, 1, 1};
      mux(&b, 0x1234, s, fl, 3, 0); b.p[b.page_at[1] + 40] ^= 0x10;
      finish("flipped_bit", &b, 0x1234, 0, 0, "one bit of the second page's body is flipped"); }
    { const long s[] = {100, 100, 100}; const int fl[] = {1, 1, 1};
      unsigned char tail[4096]; size_t n;
      mux(&b, 0x1234, s, fl, 3, 0);
      n = b.n - b.page_at[1]; memcpy(tail, b.p + b.page_at[1], n); b.n = b.page_at[1];
      put(&b, "\0\1", 2); put(&b, tail, n);
      finish("junk", &b, 0x1234, 0, 0, "two bytes between the first page and the second"); }
    { const long s[] = {70000, 30, 40}; const int fl[] = {0, 1, 1};
      mux(&b, 0x1234, s, fl, 3, 0); cut(&b, 0, b.page_at[1]);
      finish("continued_first", &b, 0x1234, 1, 1, "the stream begins with a page that continues a packet; no page number is expected");
      finish("continued_first_from_0", &b, 0x1234, 0, 0, "the same bytes where page 0 is expected"); }
    { const long s[] = {100, 100, 100}; const int fl[] = {1, 1, 1};
      mux(&b, 0x1234, s, fl, 3, 0); b.n -= 11;
      finish("truncated", &b, 0x1234, 0, 0, "the last page lacks its last 11 bytes"); }
    { const long s[] = {70000, 5};
      mux(&b, 0x1234, s, NULL, 2, 0); b.p[b.page_at[0] + 5] |= 4; reseal(&b, 0);
      finish("eos_255", &b, 0x1234, 0, 0, "the first page ends on a segment of 255 and says it is the last"); }
    { long s[40]; int k;
      for (k = 0; k < 40; k++) s[k] = (k * 137) % 700;
      mux(&b, 0x1234, s, NULL, 40, 0); finish("many_small", &b, 0x1234, 0, 0, "forty packets, paged as the writer likes"); }

    fprintf(g_js, "\n}}\n");
    fclose(g_js);
    return 0;
}
