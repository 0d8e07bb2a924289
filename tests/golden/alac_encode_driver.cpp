// alac_encode_driver.cpp -- turns interleaved host-endian PCM into Apple Lossless packets with the reference tree's own encoder, for
// tests/golden/make_alac_fixtures.py.  It is compiled into a temporary directory against the reference's codec sources, where those
// exist; no test builds or runs it.
//   alac_encode_driver BITS CHANNELS RATE FRAME_LENGTH FAST PCM_IN PACKETS_OUT META_OUT
// META_OUT: the magic cookie in hex on the first line, then one packet size per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ALACAudioTypes.h"
#include "ALACEncoder.h"

int main(int argc, char** argv)
{
    if (argc != 9) { fprintf(stderr, "usage: %s BITS CHANNELS RATE FRAME_LENGTH FAST PCM_IN PACKETS_OUT META_OUT\n", argv[0]); return 2; }
    const unsigned bits = atoi(argv[1]), channels = atoi(argv[2]), rate = atoi(argv[3]), frame_length = atoi(argv[4]);
    const bool fast = atoi(argv[5]) != 0;
    const unsigned flag = bits == 16 ? 1 : bits == 24 ? 3 : bits == 32 ? 4 : 0;
    if (!flag || channels < 1 || channels > 8 || frame_length < 1) { fprintf(stderr, "bad format\n"); return 2; }
    FILE* in = fopen(argv[6], "rb");
    FILE* out = fopen(argv[7], "wb");
    FILE* meta = fopen(argv[8], "w");
    if (!in || !out || !meta) { perror("open"); return 1; }
    std::vector<unsigned char> pcm;
    for (int c; (c = fgetc(in)) != EOF;) pcm.push_back((unsigned char)c);

    const unsigned frame_bytes = channels * (bits / 8);
    AudioFormatDescription pcm_fmt, alac_fmt;
    memset(&pcm_fmt, 0, sizeof pcm_fmt);
    memset(&alac_fmt, 0, sizeof alac_fmt);
    pcm_fmt.mSampleRate = rate; pcm_fmt.mFormatID = kALACFormatLinearPCM; pcm_fmt.mFormatFlags = kALACFormatFlagsNativeEndian | kALACFormatFlagIsSignedInteger | kALACFormatFlagIsPacked;
    pcm_fmt.mBytesPerPacket = frame_bytes; pcm_fmt.mFramesPerPacket = 1; pcm_fmt.mBytesPerFrame = frame_bytes;
    pcm_fmt.mChannelsPerFrame = channels; pcm_fmt.mBitsPerChannel = bits;
    alac_fmt.mSampleRate = rate; alac_fmt.mFormatID = kALACFormatAppleLossless; alac_fmt.mFormatFlags = flag;
    alac_fmt.mFramesPerPacket = frame_length; alac_fmt.mChannelsPerFrame = channels;

    ALACEncoder enc;
    enc.SetFrameSize(frame_length);
    enc.SetFastMode(fast);
    if (enc.InitializeEncoder(alac_fmt) != 0) { fprintf(stderr, "InitializeEncoder failed\n"); return 1; }
    unsigned char cookie[256];
    uint32_t cookie_bytes = sizeof cookie;
    enc.GetMagicCookie(cookie, &cookie_bytes);
    for (uint32_t i = 0; i < cookie_bytes; i++) fprintf(meta, "%02x", cookie[i]);
    fprintf(meta, "\n");

    std::vector<unsigned char> packet((size_t)frame_length * channels * 5 + 64), chunk((size_t)frame_length * frame_bytes);
    for (size_t at = 0; at < pcm.size(); at += chunk.size()) {
        const size_t take = pcm.size() - at < chunk.size() ? pcm.size() - at : chunk.size();
        memset(chunk.data(), 0, chunk.size());
        memcpy(chunk.data(), pcm.data() + at, take);
        int32_t n = (int32_t)take;
        if (enc.Encode(pcm_fmt, alac_fmt, chunk.data(), packet.data(), &n) != 0) { fprintf(stderr, "Encode failed\n"); return 1; }
        fwrite(packet.data(), 1, (size_t)n, out);
        fprintf(meta, "%d\n", n);
    }
    enc.Finish();
    fclose(in); fclose(out); fclose(meta);
    return 0;
}
