// host_design.cpp -- host-side tables the device kernels consume: the RampArray multipliers and the
// polyphase resampler's Q28 coefficients.  Product code (never calls into oracle/).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ohgpu_internal.h"

namespace ohgpu {

// RampArray.h:7-74 describes its 512 Q15 entries as "a ramp down curve over 0 to -60dB".  Every entry
// equals min(0x7FFF, round(32768 * (1 - i/512)^2.5)); with n = 512 - i that is round(sqrt(n^5 / 2^15)),
// which is evaluated here in exact integer arithmetic so that no libm rounding can move an entry.
// tests/test_capi_loads.py compares all 512 with the values extracted from the reference header.
void build_ramp_table(uint16_t out[512])
{
    for (uint32_t i = 0; i < 512; i++) {
        const uint64_t n = 512u - i;
        const uint64_t n5 = n * n * n * n * n;
        // v = round-half-up(sqrt(n5 / 2^15)): the largest v with (2v - 1)^2 * 2^13 <= n5
        uint64_t lo = 0, hi = 32768;
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) / 2;
            const uint64_t t = 2 * mid - 1;
            if (t * t * 8192u <= n5) lo = mid; else hi = mid - 1;
        }
        out[i] = (uint16_t)(lo > 32767u ? 32767u : lo);
    }
}

static uint32_t gcd_u32(uint32_t a, uint32_t b)
{
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}

static double bessel_i0(double x)
{
    double sum = 1.0, term = 1.0;
    const double q = x * x * 0.25;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-20) break;
    }
    return sum;
}

// Resampler specification (DESIGN.md "Resampler"; the reference has no sample-rate converter):
//   L/M = rate_out/rate_in reduced, N = L*T prototype taps, Kaiser(beta)-windowed sinc,
//   stop edge f_stop = rate_out - f_pass, cutoff midway, DC gain L, Q28 rounding half up,
//   polyphase order coef[p*T + k] = h[p + k*L].
//   An integer decimator (L = 1) gets an ODD length, N = T - 1, centred on a tap (a type I linear-phase filter, whole-sample
//   delay), stored with coef[T - 1] = 0.  For 2:1 (96 -> 48 kHz: cutoff midway between 20 and 28 kHz = exactly a quarter of the
//   input rate) that prototype is a HALF-BAND filter: sinc(d / 2) vanishes at every even distance d from the centre, so every
//   second coefficient is exactly zero after the Q28 rounding and an output needs T / 2 products plus the centre tap
//   (src_lean_kernel's half-band instantiations; any other kernel just multiplies by the zeros).
int design_src(uint32_t rate_in, uint32_t rate_out, uint32_t T, double beta, double f_pass,
               std::vector<int32_t>* coef_q28, uint32_t* L_out, uint32_t* M_out)
{
    if (rate_in == 0 || rate_out == 0 || T == 0) return set_error(OHGPU_ERR_INVALID, "src design: zero rate or taps");
    const uint32_t g = gcd_u32(rate_in, rate_out);
    const uint32_t L = rate_out / g, M = rate_in / g;
    if ((uint64_t)L * T > (1u << 22)) return set_error(OHGPU_ERR_INVALID, "src design: L*T too large (%u*%u)", L, T);
    *L_out = L;
    *M_out = M;
    if (coef_q28 == nullptr) return OHGPU_OK;
    const uint32_t N = (L == 1 && T > 1) ? T - 1 : L * T;
    double f_stop = (double)rate_out - f_pass;
    // (from 2x on, as design_src_pull: at exactly 2x the output's rule would put the cutoff at the input rate)
    if (f_stop > (double)rate_in - f_pass && rate_out >= 2 * rate_in) f_stop = (double)rate_in - f_pass;
    const double fs_up = (double)L * (double)rate_in;
    const double fc = 0.5 * (f_pass + f_stop);
    const double wc = 2.0 * fc / fs_up;
    const double centre = 0.5 * (double)(N - 1);
    const double i0b = bessel_i0(beta);
    std::vector<double> h(N);
    double sum = 0.0;
    for (uint32_t n = 0; n < N; n++) {
        const double d = (double)n - centre;
        const double x = wc * d;
        const double sinc = (std::fabs(x) < 1e-12) ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        const double r = (centre > 0.0) ? d / centre : 0.0;
        const double arg = 1.0 - r * r;
        const double w = bessel_i0(beta * std::sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
        h[n] = wc * sinc * w;
        sum += h[n];
    }
    const double scale = (double)L / sum;
    coef_q28->assign((size_t)L * T, 0);
    int64_t worst = 0;
    for (uint32_t p = 0; p < L; p++) {
        int64_t sabs = 0;
        for (uint32_t k = 0; k < T; k++) {
            const double v = (p + k * L < N) ? h[p + k * L] * scale : 0.0;
            const int32_t q = (int32_t)std::floor(v * 268435456.0 + 0.5);
            (*coef_q28)[p * T + k] = q;
            sabs += q < 0 ? -(int64_t)q : (int64_t)q;
        }
        if (sabs > worst) worst = sabs;
    }
    // sum|c| < 2^30 and |x| <= 2^23 keep every partial sum an integer below 2^53: fp64 accumulation is then exact
    if (worst >= ((int64_t)1 << 30))
        return set_error(OHGPU_ERR_INVALID, "src design: sum|c| = %lld breaks the exact-accumulation bound", (long long)worst);
    return OHGPU_OK;
}

// The DSD -> PCM decimator: D = dsd_rate / pcm_rate in {8, 16, 32, 64}, T taps per output a multiple of 8 in 8 .. 64,
// N = D * T stored coefficients.  The rule is the integer decimator's above at the DSD rate: an odd length N - 1 centred on a tap,
// stored with coef[N - 1] = 0; stop edge pcm_rate - f_pass, cutoff midway; scaled to sum = gain, Q28 rounding half up.
int check_dsd_pcm_filter(uint32_t D, uint32_t T, const int32_t* coef_q28, const char* who)
{
    if ((D != 8 && D != 16 && D != 32 && D != 64) || T < 8 || T > 64 || T % 8 != 0)
        return set_error(OHGPU_ERR_INVALID, "%s: decimation %u (8, 16, 32 or 64) with %u taps per output (a multiple of 8 in 8 .. 64)", who, D, T);
    if (!coef_q28) return OHGPU_OK;
    int64_t sabs = 0;
    for (uint32_t k = 0; k < D * T; k++) sabs += coef_q28[k] < 0 ? -(int64_t)coef_q28[k] : (int64_t)coef_q28[k];
    // one-bit samples are +-1: sum|c| < 2^30 keeps every partial sum, and the last one with the rounding added, inside 32 bits
    if (sabs >= ((int64_t)1 << 30)) return set_error(OHGPU_ERR_INVALID, "%s: sum|c| = %lld breaks the 32-bit accumulation bound 2^30", who, (long long)sabs);
    return OHGPU_OK;
}

int design_dsd_pcm(uint32_t dsd_rate, uint32_t pcm_rate, uint32_t T, double beta, double f_pass, double gain,
                   std::vector<int32_t>* coef_q28, uint32_t* D_out)
{
    if (dsd_rate == 0 || pcm_rate == 0 || dsd_rate % pcm_rate != 0)
        return set_error(OHGPU_ERR_INVALID, "dsd pcm design: %u -> %u is not a whole decimation", dsd_rate, pcm_rate);
    const uint32_t D = dsd_rate / pcm_rate;
    int err = check_dsd_pcm_filter(D, T, nullptr, "dsd pcm design");
    if (err != OHGPU_OK) return err;
    *D_out = D;
    if (coef_q28 == nullptr) return OHGPU_OK;
    const double f_stop = (double)pcm_rate - f_pass;
    if (!(f_pass > 0.0) || !(f_stop > f_pass) || !(beta >= 0.0) || !(gain > 0.0) || !(gain < 4.0))
        return set_error(OHGPU_ERR_INVALID, "dsd pcm design: f_pass %g (stop edge %g), beta %g, gain %g", f_pass, f_stop, beta, gain);
    const uint32_t N = D * T - 1;
    const double fc = 0.5 * (f_pass + f_stop);
    const double wc = 2.0 * fc / (double)dsd_rate;
    const double centre = 0.5 * (double)(N - 1);
    const double i0b = bessel_i0(beta);
    std::vector<double> h(N);
    double sum = 0.0;
    for (uint32_t n = 0; n < N; n++) {
        const double d = (double)n - centre;
        const double x = wc * d;
        const double sinc = (std::fabs(x) < 1e-12) ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        const double r = d / centre;
        const double arg = 1.0 - r * r;
        const double w = bessel_i0(beta * std::sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
        h[n] = wc * sinc * w;
        sum += h[n];
    }
    const double scale = gain / sum;
    coef_q28->assign((size_t)D * T, 0);
    for (uint32_t n = 0; n < N; n++) (*coef_q28)[n] = (int32_t)std::floor(h[n] * scale * 268435456.0 + 0.5);
    return check_dsd_pcm_filter(D, T, coef_q28->data(), "dsd pcm design");
}

// The pulled resampler's table.  The prototype h[n], n = 0 .. T*P - 1, is sampled at P = 2^s phases per input
// frame; frequencies below are in cycles per input frame at an input rate pulled anywhere in rate_in * [1 - max_pull, 1 + max_pull]:
// the pass edge at the slowest such rate, the stop edge (DESIGN.md 4's rule) at the fastest, the cutoff midway.  Rows p = 0 .. P of
// T: coef[p*T + k] = round(h[p + k*P] / g_p * 2^28) with g_p = sum_k h[p + k*P] and h[T*P] = 0 (row P is row 0 moved on one tap).
int design_src_pull(uint32_t rate_in, uint32_t rate_out, uint32_t T, uint32_t s, double beta, double f_pass, double max_pull,
                    std::vector<int32_t>* coef_q28)
{
    if (rate_in == 0 || rate_out == 0) return set_error(OHGPU_ERR_INVALID, "src pull design: zero rate");
    if (T != 32 && T != 64) return set_error(OHGPU_ERR_INVALID, "src pull design: %u taps per phase (32 or 64)", T);
    if (s < 1 || s > 16) return set_error(OHGPU_ERR_INVALID, "src pull design: phases_log2 %u outside 1..16", s);
    if (!(max_pull >= 0.0 && max_pull < 0.5) || !(f_pass > 0.0) || !(beta >= 0.0))
        return set_error(OHGPU_ERR_INVALID, "src pull design: max_pull %g, f_pass %g, beta %g", max_pull, f_pass, beta);
    // (from 2x upsampling on the images of the pass band, not the output's alias, set the stop edge: at exactly 2x the output's
    // rule would put the cutoff at the input rate)
    double f_stop = (double)rate_out - f_pass;
    if (f_stop > (double)rate_in - f_pass && rate_out >= 2 * rate_in) f_stop = (double)rate_in - f_pass;
    const double fp = f_pass / ((double)rate_in * (1.0 - max_pull));
    const double fs = f_stop / ((double)rate_in * (1.0 + max_pull));
    if (!(fs > fp)) return set_error(OHGPU_ERR_INVALID, "src pull design: stop edge %g <= pass edge %g (cycles per input frame)", fs, fp);
    const uint32_t P = 1u << s;
    const uint64_t N = (uint64_t)T * P;
    const double fc = 0.5 * (fp + fs);
    const double wc = 2.0 * fc / (double)P;
    const double centre = 0.5 * (double)(N - 1);
    const double i0b = bessel_i0(beta);
    std::vector<double> h(N + 1, 0.0);
    for (uint64_t n = 0; n < N; n++) {
        const double d = (double)n - centre;
        const double x = wc * d;
        const double sinc = (std::fabs(x) < 1e-12) ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        const double r = d / centre;
        const double arg = 1.0 - r * r;
        h[n] = wc * sinc * bessel_i0(beta * std::sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
    }
    // each row p < P is scaled to DC gain 1 on its own (the sampled prototype's phases differ in gain by up to 1e-4 of it: the stop
    // band's aliases), so that every row sums to 2^28 within T / 2; row P is row 0 moved on one tap
    coef_q28->assign((size_t)(P + 1) * T, 0);
    for (uint32_t p = 0; p < P; p++) {
        double row = 0.0;
        for (uint32_t k = 0; k < T; k++) row += h[p + (uint64_t)k * P];
        for (uint32_t k = 0; k < T; k++)
            (*coef_q28)[(size_t)p * T + k] = (int32_t)std::floor(h[p + (uint64_t)k * P] / row * 268435456.0 + 0.5);
    }
    for (uint32_t k = 0; k + 1 < T; k++) (*coef_q28)[(size_t)P * T + k] = (*coef_q28)[k + 1];
    return check_src_pull_table(T, s, coef_q28->data(), "src pull design");
}

// Every interpolated coefficient lies between its two rows' values, so sum_k max(|C[p][k]|, |C[p+1][k]|) < 2^30 keeps |acc| < 2^53
// for S24 input: fp64 accumulation is exact in any order.  The kernel forms the interpolation as mulhi(2 * (C[p+1] - C[p]), w << 15),
// which needs every difference below 2^30 as well.
int check_src_pull_table(uint32_t T, uint32_t s, const int32_t* c, const char* who)
{
    const uint32_t P = 1u << s;
    for (uint32_t p = 0; p < P; p++) {
        int64_t bound = 0;
        for (uint32_t k = 0; k < T; k++) {
            const int64_t a = c[(size_t)p * T + k], b = c[(size_t)(p + 1) * T + k];
            bound += std::max(a < 0 ? -a : a, b < 0 ? -b : b);
            if ((b - a) >= ((int64_t)1 << 30) || (a - b) >= ((int64_t)1 << 30))
                return set_error(OHGPU_ERR_INVALID, "%s: rows %u and %u differ by 2^30 or more at tap %u", who, p, p + 1, k);
        }
        if (bound >= ((int64_t)1 << 30))
            return set_error(OHGPU_ERR_INVALID, "%s: rows %u and %u have sum max|c| = %lld >= 2^30 (exact fp64 accumulation bound)", who, p,
                             p + 1, (long long)bound);
    }
    return OHGPU_OK;
}

}  // namespace ohgpu
