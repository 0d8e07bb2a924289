// src_mfma_kernel.hip -- the host tables of the matrix-pipe resampler (src_mfma_wg_kernel.hip), and the arithmetic they serve:
// the coefficients' digit tables, the steps' accumulator biases and their A-operand images (build_mfma_tables, build_mfma_images,
// build_mfma_halfband; the C ABI hands them out as ohgpu_src_mfma_tables).  Round 4's unit-per-wave kernel was written in this
// file; the workgroup kernel serves every layout it did.
//
// Why.  The lean kernel (src_lean_kernel.hip) computes an output as 32 dependent v_fmac_f64 per lane; three rounds of work on
// it ended at 0.37-0.40 of the HBM roofline with the per-output loop, not the memory system, as the bound.
// The sums are exact integers, y = sum_k c[p][k] x[n0 - k] with Q28 coefficients and 24-bit samples, so they can be written in
// base-256 digits, x = d0 + d1 2^8 + d2 2^16, c = e0 + e1 2^8 + e2 2^16 + e3 2^24, and then
//      y = sum_{s = 0..5} 2^(8 s) S_s,      S_s = sum over i + j = s of  sum_k d_i[k] e_j[k]
// where every S_s is an int8 dot product.  A TILE is 16 consecutive output frames of 16 columns (a column = one channel of
// one block row); the 16 windows of a tile lie inside one run of 64 input frames, so with the coefficients laid out as a
// banded 16 x 64 matrix per digit a tile is twelve v_mfma_i32_16x16x64_i8 into six accumulators -- 0.75 matrix-pipe cycles
// per output subsample against the 2 vector-pipe cycles of 32 fp64 FMAs -- and the per-output vector work shrinks from 44
// instructions (32 taps + 12) to about 15 (recombination 10, pack 3, digit planes 2.5), all of them 32-bit integer.
//
// The tables.
//   * COEFFICIENT DIGITS: balanced base-256 digits of each Q28 coefficient (coef_digits), one padded 96-byte row per phase and
//     digit with the taps reversed, so that the 16 bytes an output's A operand needs for a chunk of its window are one run.
//   * SAMPLE DIGITS.  The low two bytes of a sample are used as OFFSET digits, u - 128 = u ^ 0x80 read as int8 (no carry
//     chain; the top byte is the signed digit as it stands): x = [s8(b0^0x80) + 2^8 s8(b1^0x80) + 2^16 s8(b2)] + 128 * 257,
//     and the constant's share of an output, 32896 * sum_k c[p][k], is a per-phase constant the host folds -- together with
//     the rounding 2^27 -- into the accumulators' INITIAL VALUES (MfStep::b0..b2).  Raw zero bytes are the value 0, so frames
//     before a stream's start are zero bytes.
//   * STEPS: a step is 16 consecutive outputs of a row, the same for every row (rows start at phase 0); its window is four
//     chunks of 16 input frames starting on a chunk boundary (MfStep::kc), and output m's A row starts at MfStep::aoff[m].
//   * IMAGES: the A operands of a step, lane-linear (4 KB a step, [digit][lane][16 bytes]), so that the kernel reads them as
//     whole pieces rather than gathering rows per lane.
//   * RECOMBINATION in 32-bit integers (mf_recombine_head / _tail, src_mfma_common.h): T0 = S0 + (S1 << 8), T1 = S2 + (S3 << 8),
//     T2 = S4 + (S5 << 8) (each below 2^30), U = T1 + (T0 >> 16), W = T2 + (U >> 16), y = (W << 4) | bits 12..15 of U =
//     floor(acc / 2^28) exactly (the low 16 bits of T0 and the low 12 of U cannot carry into bit 28), then a clamp.
// Bit-exact against the integer model (oracle/ohp_pipeline.c) like the kernels before it: same sum, same rounding.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ohgpu_internal.h"
#include "pcm_device.h"
#include "src_mfma_common.h"

namespace ohgpu {

// ---- host: the tables ----
// Balanced base-256 digits of a Q28 coefficient: c = e0 + e1 2^8 + e2 2^16 + e3 2^24, e0..e2 in [-128, 127].  False when the top
// digit -- what is left after the three balanced ones -- is no int8: the coefficients from -(128 << 24) - 0x808080 to
// (127 << 24) + 0x7f7f7f have digits (a value above that carries into a top digit of 128, which the cast would wrap to -128).
static bool coef_digits(int32_t c, int8_t e[4])
{
    int64_t v = c;
    for (int j = 0; j < 3; j++) {
        const int d = (int)(int8_t)(uint8_t)(v & 0xff);
        e[j] = (int8_t)d;
        v = (v - d) >> 8;
    }
    e[3] = (int8_t)v;
    return v >= -128 && v <= 127;
}

bool build_mfma_tables(uint32_t L, uint32_t M, uint32_t T, const int32_t* coef_q28, uint32_t L_blk, uint32_t kb_cap,
                       std::vector<uint8_t>* adig, std::vector<MfStep>* steps)
{
    if (T != 32 || L == 0 || M == 0 || L_blk == 0 || (L_blk % 16) != 0 || (L_blk % L) != 0 || kb_cap == 0) return false;
    for (size_t i = 0; i < (size_t)L * T; i++) {
        int8_t e[4];
        if (!coef_digits(coef_q28[i], e)) return false;                                           // the top digit is an int8
    }
    adig->assign((size_t)4 * L * 96, 0);
    std::vector<int64_t> bias(L);
    for (uint32_t p = 0; p < L; p++) {
        int64_t sum = 0;
        for (uint32_t k = 0; k < 32; k++) {
            const int32_t c = coef_q28[(size_t)p * T + k];
            sum += c;
            int8_t e[4];
            coef_digits(c, e);
            for (int j = 0; j < 4; j++) (*adig)[((size_t)j * L + p) * 96 + (63 - k)] = (uint8_t)e[j];
        }
        // the offset digits' constant (128 + 128 * 256 per sample) and the rounding
        bias[p] = 32896 * sum + ((int64_t)1 << 27);
        if (bias[p] < -((int64_t)1 << 44) || bias[p] > ((int64_t)1 << 44)) return false;      // (its bits 16.. ride in ONE accumulator: MfStep)
    }
    const uint32_t n_steps = (L_blk / 16) * kb_cap;
    steps->assign(n_steps, MfStep());
    for (uint32_t t = 0; t < n_steps; t++) {
        MfStep& s = (*steps)[t];
        memset(&s, 0, sizeof(s));
        const uint64_t n0_first = ((uint64_t)16 * t * M) / L;         // newest input frame of the step's first output (row-relative)
        const uint64_t k0 = ((n0_first + 1) / 16) * 16;               // the window: frames k0 .. k0 + 63 in a' = frame + 32
        s.kc = (uint32_t)(k0 / 16);
        for (uint32_t m = 0; m < 16; m++) {
            const uint64_t tm = ((uint64_t)16 * t + m) * M;
            const uint64_t n0 = tm / L;
            const uint32_t p = (uint32_t)(tm % L);
            const int64_t o = 31 + (int64_t)k0 - (int64_t)n0;         // row offset of K = 0
            if (o < 0 || o > 32) return false;                        // (a ratio this tiling does not hold: 15 M / L must stay below 17)
            s.aoff[m] = p * 96 + (uint32_t)o;
            s.b0[m] = (uint32_t)(bias[p] & 0xffff);
            s.b1[m] = (uint32_t)(int32_t)(bias[p] >> 16);
            s.b2[m] = 0;
        }
    }
    return true;
}

// The half-band 2:1 decimator (L = 1, M = 2, T = 64 stored taps of which the even ones and the centre tap 31 are not zero) on the
// same tiles.  y[j] = sum_m c[2 m] x[2 j - 2 m] + c[31] x[2 j - 31]: with the row's image starting 64 frames before the block
// (image frame a = frame + 64), its EVEN frames e = a / 2 and its ODD frames o = (a - 1) / 2 as two sample streams, output j
// meets e = 32 + j - m (m = 0..31) and o = j + 16.  A step of 16 outputs j = 16 s + n therefore reads even samples 16 s ..
// 16 s + 47 -- three aligned chunks, K groups 0..2 -- and the ONE odd chunk s + 1, sample n for output n -- K group 3, a diagonal.
// One coefficient image serves every step (the phase never changes): [digit 4][lane = 16 g + n][16 bytes], and one bias.
bool build_mfma_halfband(const int32_t* coef_q28, uint32_t L_blk, std::vector<MfStep>* steps, std::vector<uint8_t>* amat)
{
    if (L_blk == 0 || (L_blk % 16) != 0) return false;
    int64_t sum = 0;
    for (uint32_t k = 0; k < 64; k++) {
        const int32_t c = coef_q28[k];
        int8_t e4[4];
        if (!coef_digits(c, e4)) return false;                                                    // the top digit is an int8
        if ((k & 1u) && k != 31 && c != 0) return false;                                          // not a half-band filter
        sum += c;
    }
    const int64_t bias = 32896 * sum + ((int64_t)1 << 27);
    if (bias < -((int64_t)1 << 44) || bias > ((int64_t)1 << 44)) return false;
    amat->assign(kMfStepImage, 0);
    for (uint32_t gq = 0; gq < 4; gq++)
        for (uint32_t n = 0; n < 16; n++)
            for (uint32_t i = 0; i < 16; i++) {
                int32_t c = 0;
                if (gq < 3) {
                    const int m_tap = 32 + (int)n - 16 * (int)gq - (int)i;                          // even sample 16 (s + gq) + i against output 16 s + n
                    if (m_tap >= 0 && m_tap <= 31) c = coef_q28[2 * m_tap];
                } else if (i == n) {
                    c = coef_q28[31];
                }
                int8_t e[4];
                coef_digits(c, e);
                for (int j = 0; j < 4; j++) (*amat)[(size_t)j * 1024 + (gq * 16 + n) * 16 + i] = (uint8_t)e[j];
            }
    steps->assign(L_blk / 16, MfStep());
    for (uint32_t t = 0; t < L_blk / 16; t++) {
        MfStep& st = (*steps)[t];
        memset(&st, 0, sizeof(st));
        st.kc = t;                                                                                // even chunks t .. t + 2, odd chunk t + 1
        for (uint32_t m = 0; m < 16; m++) {
            st.b0[m] = (uint32_t)(bias & 0xffff);
            st.b1[m] = (uint32_t)(int32_t)(bias >> 16);
            st.b2[m] = 0;
        }
    }
    return true;
}

// The kernel's A operands, lane-linear: [step][coefficient digit][lane = 16 g + m][16 bytes] = the 16 bytes of output m's padded
// coefficient row that meet frames 16 (kc + g) .. + 15 of the step's window (MfStep::aoff).
void build_mfma_images(const std::vector<uint8_t>& adig, const std::vector<MfStep>& steps, uint32_t L, std::vector<uint8_t>* amat)
{
    amat->assign(steps.size() * (size_t)kMfStepImage, 0);
    for (size_t t = 0; t < steps.size(); t++)
        for (uint32_t j = 0; j < 4; j++)
            for (uint32_t gq = 0; gq < 4; gq++)
                for (uint32_t m = 0; m < 16; m++)
                    memcpy(amat->data() + t * kMfStepImage + j * 1024 + (gq * 16 + m) * 16,
                           adig.data() + (size_t)j * L * 96 + steps[t].aoff[m] + 16 * gq, 16);
}

bool src_mfma_supported(uint32_t T, uint32_t ch, uint32_t sb, uint32_t db)
{
    return T == 32 && ch == 2 && sb == 3 && db == 3;
}

}  // namespace ohgpu
