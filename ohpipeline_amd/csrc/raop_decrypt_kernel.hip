// raop_decrypt_kernel.hip -- RAOP's AES-128-CBC decryption on the device (the cipher's text is csrc/raop_aes_core.h).
// CBC decryption has no chain: block j needs ciphertext blocks j and j - 1 only.  The work table (made at creation) holds one record
// per piece -- up to 64 consecutive blocks of one packet --; a wave takes a piece and a lane a block, so the stream, its key and its
// IV are the same for the whole wave: the piece and the round keys are read through a wave-uniform index and stay in scalar
// registers.  A workgroup is four waves; it stages Td0 (1 KB) and the inverse S-box (256 B) into the LDS once.  The table reads are
// data-dependent, so LDS bank conflicts are part of the cost (5.13 has the measurement).  A lane loads its own block and the one
// before it (which its neighbour has just pulled into the cache), in dwords: the C ABI guarantees 4-byte alignment.  The piece with
// a packet's last block copies the bytes % 16 tail, a byte per lane.
// Every load and store lies inside a packet range that ohgpu_raop_batch_check validated against the arenas, or inside the batch's
// own plaintext scratch, which raop_plan sized from the same table.
#include <hip/hip_runtime.h>

#include <cstring>

#include "api_common.h"

namespace ohgpu {

using namespace raopcore;

constexpr uint32_t kRaopThreads = 256, kRaopWaves = kRaopThreads / 64;

constexpr Tables kRaopHostTables = make_tables();
__constant__ const Tables kRaopTables = kRaopHostTables;

const Tables& raop_tables() { return kRaopHostTables; }

__global__ __launch_bounds__(kRaopThreads) void raop_decrypt_kernel(const Piece* __restrict__ pieces, uint32_t n_pieces, const uint32_t* __restrict__ keys,
                                                                    const uint8_t* __restrict__ src, uint8_t* __restrict__ scratch, uint8_t* __restrict__ dst)
{
    __shared__ uint32_t td0[256];
    __shared__ uint8_t isbox[256];
    td0[threadIdx.x] = kRaopTables.td0[threadIdx.x];
    isbox[threadIdx.x] = kRaopTables.isbox[threadIdx.x];
    __syncthreads();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u);      // (the same in every lane: says so to the compiler)
    const uint32_t i = blockIdx.x * kRaopWaves + wave;
    if (i >= n_pieces) return;
    const Piece pc = pieces[i];
    piece_lane(pc, threadIdx.x % 64u, keys + (size_t)pc.key * kKeyWords, src, pc.to_arena ? dst : scratch, td0, isbox);
}

int raop_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const Job* jobs, size_t n_jobs)
{
    RaopState& r = *b->raop;
    std::vector<Piece> pieces;
    plan_pieces(jobs, n_jobs, &pieces);
    r.n_pieces = (uint32_t)pieces.size();
    OHGPU_TRY(state_events(r, 1));
    if (pieces.empty()) return OHGPU_OK;
    r.keys_bytes = r.keys.size() * sizeof(uint32_t);
    OHGPU_TRY(dev_array(ctx, r, &r.d_pieces, pieces.size(), pieces.data()));
    OHGPU_TRY(dev_array(ctx, r, &r.d_keys, r.keys.size(), r.keys.data()));
    OHGPU_TRY(dev_array<uint8_t>(ctx, r, &r.d_plain, r.plain_bytes));
    return OHGPU_OK;
}

void raop_free(ohgpu_ctx* ctx, ohgpu_batch* b)
{
    if (b->raop) {
        RaopState& r = *b->raop;
        (void)hipDeviceSynchronize();
        // the expanded keys do not outlive the batch: the device array is cleared before its block goes back to the cache, the host copy too
        if (r.d_keys) (void)hipMemset(r.d_keys, 0, r.keys_bytes);
        for (uint32_t& w : r.keys) *(volatile uint32_t*)&w = 0;
    }
    state_free(ctx, b->raop);
    state_free(ctx, b->alac);
}

int raop_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    const RaopState& r = *b->raop;
    AlacState& a = *b->alac;
    OHGPU_TRY(run_begin(a, s));      // (the scratch serves one run at a time)
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(r.ev[0], s));
    if (r.n_pieces) {
        hipLaunchKernelGGL(raop_decrypt_kernel, dim3((r.n_pieces + kRaopWaves - 1) / kRaopWaves), dim3(kRaopThreads), 0, s, (const Piece*)r.d_pieces, r.n_pieces,
                           (const uint32_t*)r.d_keys, src, (uint8_t*)r.d_plain, dst);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return OHGPU_OK;
}

}  // namespace ohgpu
