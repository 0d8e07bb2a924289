// raop_host_cpu.cpp -- the host side of tools/bench_raop.py.
//   raop_host_cpu encrypt JOB OUT THREADS            encrypts the job's packets as a RAOP sender does (AES-128-CBC over the whole blocks
//                                                    of each packet from the stream's IV, the tail in the clear): FIPS-197's Cipher,
//                                                    straightforward, with the S-box of csrc/raop_aes_core.h's computed tables
//   raop_host_cpu libcrypto JOB THREADS LIBRARY      times the SYSTEM's libcrypto (AES_set_decrypt_key + AES_cbc_encrypt, hardware AES
//                                                    where the CPU has it) decrypting the job's packets in place on THREADS threads;
//                                                    prints seconds, or "absent" when the library or its symbols are not there
// JOB: u32 n_streams, n_packets; u64 bytes; per stream 16 key bytes and 16 IV bytes; per packet u64 offset, u32 bytes, u32 stream;
//      the arena.
#include <dlfcn.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../ohpipeline_amd/csrc/raop_aes_core.h"

using namespace raopcore;

static constexpr Tables kTables = make_tables();

struct Pk { uint64_t offset; uint32_t bytes, stream; };

static void forward_keys(const uint8_t key[16], uint8_t rk[176])
{
    memcpy(rk, key, 16);
    uint8_t rcon = 1;
    for (int i = 4; i < 44; i++) {
        uint8_t t[4];
        memcpy(t, rk + 4 * (i - 1), 4);
        if (i % 4 == 0) {
            const uint8_t first = t[0];
            t[0] = (uint8_t)(kTables.sbox[t[1]] ^ rcon); t[1] = kTables.sbox[t[2]]; t[2] = kTables.sbox[t[3]]; t[3] = kTables.sbox[first];
            rcon = gf_mul(rcon, 2);
        }
        for (int b = 0; b < 4; b++) rk[4 * i + b] = (uint8_t)(rk[4 * (i - 4) + b] ^ t[b]);
    }
}

static void forward_block(const uint8_t rk[176], uint8_t s[16])
{
    for (int b = 0; b < 16; b++) s[b] ^= rk[b];
    for (int r = 1; r <= 10; r++) {
        uint8_t t[16];
        for (int c = 0; c < 4; c++) for (int row = 0; row < 4; row++) t[4 * c + row] = kTables.sbox[s[4 * ((c + row) % 4) + row]];      // SubBytes, ShiftRows
        for (int c = 0; c < 4 && r != 10; c++) {
            const uint8_t a0 = t[4 * c], a1 = t[4 * c + 1], a2 = t[4 * c + 2], a3 = t[4 * c + 3];
            t[4 * c] = (uint8_t)(gf_mul(a0, 2) ^ gf_mul(a1, 3) ^ a2 ^ a3);
            t[4 * c + 1] = (uint8_t)(a0 ^ gf_mul(a1, 2) ^ gf_mul(a2, 3) ^ a3);
            t[4 * c + 2] = (uint8_t)(a0 ^ a1 ^ gf_mul(a2, 2) ^ gf_mul(a3, 3));
            t[4 * c + 3] = (uint8_t)(gf_mul(a0, 3) ^ a1 ^ a2 ^ gf_mul(a3, 2));
        }
        for (int b = 0; b < 16; b++) s[b] = (uint8_t)(t[b] ^ rk[16 * r + b]);
    }
}

int main(int argc, char** argv)
{
    if (argc < 5) { fprintf(stderr, "usage: %s encrypt JOB OUT THREADS | libcrypto JOB THREADS LIBRARY\n", argv[0]); return 2; }
    const bool encrypt = strcmp(argv[1], "encrypt") == 0;
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    uint32_t counts[2];
    uint64_t bytes;
    if (fread(counts, 4, 2, f) != 2 || fread(&bytes, 8, 1, f) != 1) return 1;
    std::vector<uint8_t> secrets((size_t)counts[0] * 32), arena(bytes);
    std::vector<Pk> packets(counts[1]);
    if (fread(secrets.data(), 32, counts[0], f) != counts[0] || fread(packets.data(), sizeof(Pk), counts[1], f) != counts[1] || fread(arena.data(), 1, bytes, f) != bytes) return 1;
    fclose(f);
    const int threads = atoi(argv[encrypt ? 4 : 3]);

    typedef int (*SetKey)(const unsigned char*, int, void*);
    typedef void (*Cbc)(const unsigned char*, unsigned char*, size_t, const void*, unsigned char*, int);
    SetKey set_key = nullptr;
    Cbc cbc = nullptr;
    if (!encrypt) {
        void* lib = dlopen(argv[4], RTLD_NOW);
        if (lib) { set_key = (SetKey)dlsym(lib, "AES_set_decrypt_key"); cbc = (Cbc)dlsym(lib, "AES_cbc_encrypt"); }
        if (!set_key || !cbc) { printf("absent\n"); return 0; }
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            for (size_t i = (size_t)t; i < packets.size(); i += (size_t)threads) {
                const Pk& p = packets[i];
                uint8_t* at = arena.data() + p.offset;
                const uint8_t* secret = &secrets[(size_t)p.stream * 32];
                if (encrypt) {
                    uint8_t rk[176], prev[16];
                    forward_keys(secret, rk);
                    memcpy(prev, secret + 16, 16);
                    for (uint32_t b = 0; b + 16 <= p.bytes; b += 16) {
                        for (int k = 0; k < 16; k++) at[b + k] ^= prev[k];
                        forward_block(rk, at + b);
                        memcpy(prev, at + b, 16);
                    }
                } else {
                    alignas(16) unsigned char schedule[256], iv[16];
                    set_key(secret, 128, schedule);
                    memcpy(iv, secret + 16, 16);
                    cbc(at, at, p.bytes / 16 * 16, schedule, iv, 0);
                }
            }
        });
    for (std::thread& t : pool) t.join();
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (encrypt) {
        f = fopen(argv[3], "wb");
        if (!f) { perror(argv[3]); return 1; }
        fwrite(arena.data(), 1, arena.size(), f);
        fclose(f);
    }
    printf("%.6f\n", seconds);
    return 0;
}
