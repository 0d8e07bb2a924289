// vorbis_core_driver.cpp -- csrc/vorbis_core.h on the CPU, stand-alone (no Python, no device): tests/test_vorbis_core_cpu.py builds it with
// -fsanitize=address,undefined and runs it on streams of tests/vorbis_frames.py with what tests/vorbis_textbook.py expects.
//   case file:    u32 bytes + identification packet, u32 bytes + setup packet, u32 n, then n times u32 bytes + packet
//   expect file:  per packet u32 status, mode, block, samples and u64 position; for an OK packet channels x block / 2 float32 of spectrum
//   pcm file:     the model's samples, int32, interleaved by channel
// It parses the setup, reads every packet's head, sums the positions, decodes floors and residue, draws the curves and multiplies:
// records and spectrum must be EXACTLY the model's (two values that are both not a number count as equal).  Then the core's serial
// synthesis -- the direct-form DCT-IV, the unfolding, the window, the overlap-add and the rounding -- must give the model's PCM within
// 1 LSB.  Exit status 0 and "OK <packets>" on success.
//
//   driver case expect max_samples pcm      one case
//   driver --many file                      many cases from one file: u32 n, then per case
//       u32 bytes + label, u32 parse (0: the model accepts the headers, 1: it refuses them), u32 pcm (1: the model's PCM within 1 LSB,
//       2: V6 alone -- every stored sample is 0 where the sum is not a number, clamped where it is beyond 16 bits, else within half a
//       step of it), u64 max_samples, u32 bytes + case, u32 bytes + expect, u32 bytes + pcm (the last two empty for a refused case)
//     For every case whose headers the core refuses it prints "PARSE <label> <code>".  A case in which the core and the model differ --
//     the parse's answer, an image vorbiscore::image_valid does not pass, a record, a spectrum value, the PCM -- is reported by its
//     label, the first ten of them.  Exit status 0 and "OK <cases>" when there is none.
#include <cmath>
#include <map>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ohpipeline_amd/csrc/vorbis_core.h"

using namespace vorbiscore;

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> out;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return out;
}

struct Cursor {
    const std::vector<uint8_t>& d;
    size_t at = 0;
    template <typename T> T take() { T v; if (at + sizeof(T) > d.size()) { fprintf(stderr, "file too short\n"); exit(2); } memcpy(&v, &d[at], sizeof(T)); at += sizeof(T); return v; }
    std::vector<uint8_t> blob() { const uint32_t n = take<uint32_t>(); if (at + n > d.size()) { fprintf(stderr, "file too short\n"); exit(2); } std::vector<uint8_t> v(d.begin() + (long)at, d.begin() + (long)(at + n)); at += n; return v; }
};

enum { kPcmModel = 1, kPcmV6 = 2 };
enum { kSame = 0, kDiffers = 1, kRefused = 2 };

// One case against what the model expects.  kRefused: the core refuses the headers (*code says how); kDiffers: something is not the
// model's, said on stderr behind `label`; kSame with *packets the case's count.
static int run_case(const char* label, const std::vector<uint8_t>& cs, const std::vector<uint8_t>& ex, const std::vector<uint8_t>& pc, uint64_t max_samples, uint32_t pcm_mode,
                    int* code, uint32_t* n_packets)
{
    Cursor c{cs}, e{ex};
    const std::vector<uint8_t> ident = c.blob(), setup = c.blob();
    std::vector<uint32_t> img;
    ParsedInfo info;
    const char* why = "";
    const int rc = parse_setup(ident.data(), ident.size(), setup.data(), setup.size(), &img, &info, &why);
    *code = rc;
    if (rc != kParseOk) { if (!label[0]) fprintf(stderr, "parse_setup: %d (%s)\n", rc, why); return kRefused; }
    if (!image_valid(img.data(), (uint64_t)img.size() * 4u)) { fprintf(stderr, "%sthe parsed image does not pass image_valid\n", label); return kDiffers; }
    const uint32_t n = c.take<uint32_t>();
    *n_packets = n;
    std::vector<std::vector<uint8_t>> packets(n);
    for (auto& p : packets) { p = c.blob(); if (p.empty()) p.reserve(1); }      // (exactly the packet's bytes: the sanitizer sees a load past them)
    std::vector<Rec> recs(n);
    for (uint32_t i = 0; i < n; i++) head_packet(img.data(), packets[i].data(), (uint32_t)packets[i].size(), &recs[i]);
    Stream s;
    memset(&s, 0, sizeof(s));
    s.n_packets = n; s.max_samples = max_samples; s.channels = info.channels; s.bs0 = info.bs0; s.bs1 = info.bs1;
    scan_stream(s, recs.data());
    float db[256];
    db_table(db);
    const Image& im = image_head(img.data());
    std::vector<uint8_t> cls(im.class_bytes ? im.class_bytes : 1);
    int bad = 0;
    // the tables the batch makes: the window's slopes and the cosine of 8N points, by block size
    std::map<uint32_t, std::vector<float>> slopes, cos8;
    for (uint32_t bs : {info.bs0, info.bs1}) {
        slopes[bs].resize(bs / 2u);
        window_slope(bs, slopes[bs].data());
        cos8[bs].resize(4u * bs);
        for (uint32_t j = 0; j < 4u * bs; j++) cos8[bs][j] = (float)std::cos(2.0 * 3.14159265358979323846 * j / (4.0 * bs));
    }
    std::vector<std::vector<float>> blocks(n);                          // per OK packet: channels x block, windowed
    for (uint32_t i = 0; i < n && bad < 10; i++) {
        const Rec& r = recs[i];
        const uint32_t status = e.take<uint32_t>(), mode = e.take<uint32_t>(), block = e.take<uint32_t>(), samples = e.take<uint32_t>();
        const uint64_t position = e.take<uint64_t>();
        if (r.status != status || r.mode != mode || r.blocksize != block || r.samples != samples || r.position != position) {
            fprintf(stderr, "%spacket %u: record (%u %u %u %u %llu), the model (%u %u %u %u %llu)\n", label, i, r.status, r.mode, r.blocksize, r.samples,
                    (unsigned long long)r.position, status, mode, block, samples, (unsigned long long)position);
            bad++;
            break;                                                       // (the expect file cannot be followed behind a record that differs)
        }
        if (r.status != kOk) continue;
        const uint32_t half = r.blocksize / 2u;
        std::vector<float> rows((size_t)info.channels * half, 0.0f);       // exactly the block's: the sanitizer sees a store past it
        std::vector<FloorOut> floors(info.channels);
        decode_packet(img.data(), packets[i].data(), (uint32_t)packets[i].size(), r, Rows{rows.data(), half}, floors.data(), cls.data());
        const Mapping& map = image_mapping(img.data(), image_mode(img.data(), r.mode).mapping);
        for (uint32_t ch = 0; ch < info.channels; ch++) {
            float* row = rows.data() + (size_t)ch * half;
            if (!floors[ch].used) { for (uint32_t x = 0; x < half; x++) row[x] = 0.0f; }
            else {
                const Floor& fl = image_floor(img.data(), map.sub_floor[map.mux[ch]]);
                Segment segs[64];
                int32_t tx, ty;
                const uint32_t ns = floor_segments(fl, floors[ch], segs, &tx, &ty);
                for (uint32_t k = 0; k < ns; k++) draw_segment(segs[k], (int32_t)half, [&](int32_t x, int32_t y) { row[x] = row[x] * db[y]; });
                for (uint32_t x = (uint32_t)tx; x < half; x++) row[x] = row[x] * db[ty];
            }
            for (uint32_t x = 0; x < half; x++) {
                const float want = e.take<float>();
                if (memcmp(&want, &row[x], 4) != 0 && !(want != want && row[x] != row[x]) && bad < 10) {
                    fprintf(stderr, "%spacket %u channel %u value %u: %.9g, the model %.9g\n", label, i, ch, x, row[x], want);
                    bad++;
                }
            }
            const uint32_t bs = r.blocksize;
            std::vector<float> u(half);
            for (uint32_t x = 0; x < half; x++) u[x] = dct4_direct(row, half, cos8[bs].data(), x);
            blocks[i].resize((size_t)info.channels * bs);
            for (uint32_t x = 0; x < bs; x++)
                blocks[i][(size_t)ch * bs + x] = unfold_at(u.data(), half, x) * window_at(x, bs, info.bs0, image_mode(img.data(), r.mode).blockflag != 0, r.prev_flag != 0, r.next_flag != 0,
                                                                                             slopes[bs].data(), slopes[info.bs0].data());
        }
    }
    Cursor pcm{pc};
    int worst = 0, v6 = 0;
    for (uint32_t i = 0; i < n && !bad; i++) {
        const Rec& r = recs[i];
        if (r.status != kOk) continue;
        for (uint32_t j = 0; j < r.samples; j++)
            for (uint32_t ch = 0; ch < info.channels; ch++) {
                const float sum = overlap_at(blocks[r.prev_packet].data() + (size_t)ch * r.prev_block, r.prev_block, blocks[i].data() + (size_t)ch * r.blocksize, r.blocksize, j);
                const int32_t got = to_pcm16(sum);
                const int32_t want = pcm.take<int32_t>();
                if (pcm_mode == kPcmV6) {
                    const double x = (double)sum * 32768.0;
                    const bool ok = sum != sum ? got == 0 : x >= 32767.0 ? got == 32767 : x <= -32768.0 ? got == -32768 : std::fabs((double)got - x) <= 0.5 + 1e-3;
                    if (!ok && v6++ < 3) fprintf(stderr, "%spacket %u sample %u channel %u: %.9g stored as %d, which is not V6's\n", label, i, j, ch, sum, got);
                    continue;
                }
                const int d = got > want ? got - want : want - got;
                if (d > worst) worst = d;
            }
    }
    if (!bad && (pcm.at != pc.size() || worst > 1 || v6)) { fprintf(stderr, "%sPCM: largest difference %d LSB, %zu of %zu bytes compared, %d samples against V6\n", label, worst, pcm.at, pc.size(), v6); bad++; }
    return bad ? kDiffers : kSame;
}

static int run_many(const char* path)
{
    const std::vector<uint8_t> all = slurp(path);
    Cursor f{all};
    const uint32_t n = f.take<uint32_t>();
    int differ = 0;
    for (uint32_t i = 0; i < n; i++) {
        const std::vector<uint8_t> name = f.blob();
        const std::string label(name.begin(), name.end());
        const uint32_t refused_by_model = f.take<uint32_t>(), pcm_mode = f.take<uint32_t>();
        const uint64_t max_samples = f.take<uint64_t>();
        const std::vector<uint8_t> cs = f.blob(), ex = f.blob(), pc = f.blob();
        if (differ >= 10) continue;
        int code = 0;
        uint32_t packets = 0;
        const std::string prefix = label + ": ";
        const int r = run_case(prefix.c_str(), cs, ex, pc, max_samples, pcm_mode, &code, &packets);
        if (r == kRefused) printf("PARSE %s %d\n", label.c_str(), code);
        if (r == kDiffers) differ++;
        else if ((r == kRefused) != (refused_by_model != 0)) { fprintf(stderr, "%s: the core %s the headers, the model %s them\n", label.c_str(), r == kRefused ? "refuses" : "accepts", refused_by_model ? "refuses" : "accepts"); differ++; }
    }
    if (differ) return 1;
    printf("OK %u\n", n);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "--many")) return run_many(argv[2]);
    if (argc != 5) { fprintf(stderr, "usage: %s case expect max_samples pcm | %s --many file\n", argv[0], argv[0]); return 2; }
    const std::vector<uint8_t> cs = slurp(argv[1]), ex = slurp(argv[2]), pc = slurp(argv[4]);
    int code = 0;
    uint32_t packets = 0;
    if (run_case("", cs, ex, pc, strtoull(argv[3], nullptr, 10), kPcmModel, &code, &packets) != kSame) return 1;
    printf("OK %u\n", packets);
    return 0;
}
