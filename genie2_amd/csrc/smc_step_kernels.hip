// The SMC bookkeeping of one twisted-diffusion step for independent particle systems (include/genie_hip.h: genie_smc_reweight):
// the fork's weight helpers, systematic resampling and the weight update of its loop (genie/sampler/unconditional_smc.py:25-43,
// 237-288, 540-576; genie2_amd/smc.py:212-226 is the PyTorch restatement for one system), for S systems of K particles in one
// call, system-major: particle b belongs to system b / K.
//
// Two launches, no atomics, every sum in a fixed order, float64 throughout after the float32 loads:
//   k_smc_log_w    one work-group per particle: d_b = sum_{n,c} [(x - mean_tw)^2 - (x - mean_un)^2] / (2 sigma^2), summed in the
//                  difference form (mean_un - mean_tw) ((x - mean_tw) + (x - mean_un)) -- the two squares agree to many digits
//                  and their difference is what matters -- per thread in element order, then a butterfly inside each wave and the
//                  waves in wave order; log_w_b = d_b + log_prob_b - log_proposal_b + log_w_acc_b goes to work[b] as a double.
//                  The in/out vectors are read here only, so the second launch can overwrite them.
//   k_smc_gather   grid (particle, tile of 3N floats): every wave of every work-group redoes its system's K-value tail from
//                  `work` (one lane per particle: max, exp, the two sums by butterfly, which leaves bitwise the same value in every
//                  lane; the cumulative sum walked in particle order by every lane, as torch.cumsum does), then the work-group
//                  copies its tile of x_new[ancestor].  The first work-group of a system writes the per-system and per-particle
//                  outputs.  Ancestors are clamped between the first and the last particle of the system with a non-zero weight, so
//                  an index never leaves the system and a particle of weight exactly 0 (log_w = -inf) is never taken.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int SR_THREADS = 256;
constexpr int SR_WAVES = SR_THREADS / 64;
constexpr int SR_TILE = 4 * SR_THREADS;                // floats of x_out one work-group of the gather copies
constexpr int SR_MAX_K = 64;                           // one wave holds a system

__device__ inline double sr_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline double sr_wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(SR_THREADS) void k_smc_log_w(int N, const float* __restrict__ x_new, const float* __restrict__ mean_tw,
                                                          const float* __restrict__ mean_un, const float* __restrict__ sigma,
                                                          const float* __restrict__ log_prob, const float* __restrict__ log_proposal,
                                                          const float* __restrict__ log_w_acc, double* __restrict__ work) {
    __shared__ double red[SR_WAVES];
    const size_t b = blockIdx.x, n3 = 3 * (size_t)N;
    const float *x = x_new + b * n3, *mt = mean_tw + b * n3, *mu = mean_un + b * n3;
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < n3; i += SR_THREADS) {
        const double xi = x[i], ti = mt[i], ui = mu[i];
        acc += (ui - ti) * ((xi - ti) + (xi - ui));
    }
    acc = sr_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double d = red[0];
        for (int w = 1; w < SR_WAVES; ++w) d += red[w];
        const double sg = (double)sigma[0];
        work[b] = ((d / (2.0 * sg * sg) + (double)log_prob[b]) - (double)log_proposal[b]) + (double)log_w_acc[b];
    }
}

__global__ __launch_bounds__(SR_THREADS) void k_smc_gather(int K, int N, const float* __restrict__ x_new, const float* __restrict__ log_prob,
                                                           const float* __restrict__ u, double ess_fraction, const double* __restrict__ work,
                                                           float* __restrict__ log_proposal, float* __restrict__ log_w_acc,
                                                           float* __restrict__ x_out, int32_t* __restrict__ index_out,
                                                           float* __restrict__ ess_out, int32_t* __restrict__ resampled_out) {
    const int b = blockIdx.x, s = b / K, k0 = s * K, lane = threadIdx.x & 63;
    // the tail of system s, one lane per particle; every wave of the work-group does the same arithmetic on the same values
    const bool live = lane < K;
    const double lw = live ? work[k0 + lane] : -INFINITY;
    const bool any_nan = __ballot(lw != lw) != 0ull;
    const double mx = sr_wave_max(lw);
    const double e = live ? exp(lw - mx) : 0.0;                        // (exactly 0 for log_w = -inf)
    const double sum1 = sr_wave_sum(e), sum2 = sr_wave_sum(e * e);
    const double ess = sum1 * sum1 / sum2;
    // a system whose largest log_w is not finite (a NaN counts, as it does for torch.max) stays in place
    const bool ok = !any_nan && isfinite(mx);
    const bool resample = ok && ess < ess_fraction * (double)K;       // (wave-uniform: the sums are bitwise equal in every lane)
    int anc = lane;
    if (resample) {
        const uint64_t nz = __ballot(live && e > 0.0);                // (not empty: the particle at the max has e = 1)
        const double wn = e / sum1, point = (double)u[s] + (double)lane / (double)K;
        double cum = 0.0;
        int below = 0;
        for (int j = 0; j < K; ++j) {                                  // the cumulative sums in particle order, as torch.cumsum
            cum += __shfl(wn, j, 64);
            below += cum < point ? 1 : 0;
        }
        const int first = __ffsll((unsigned long long)nz) - 1, last = 63 - __clzll((long long)nz);
        anc = min(max(below, first), last);
    }
    if (b == k0 && blockIdx.y == 0 && threadIdx.x < 64) {             // the first wave of the system's first work-group writes its outputs
        if (live) {
            const int p = k0 + lane;
            index_out[p] = k0 + anc;
            log_proposal[p] = log_prob[k0 + anc];
            log_w_acc[p] = resample ? 0.f : (float)(((lw - mx) - log(sum1)) + log((double)K));
        }
        if (lane == 0) {
            ess_out[s] = (float)ess;
            resampled_out[s] = resample ? 1 : 0;
        }
    }
    const int from = k0 + __shfl(anc, b - k0, 64);
    const size_t n3 = 3 * (size_t)N;
    const float* src = x_new + (size_t)from * n3;
    float* dst = x_out + (size_t)b * n3;
    const size_t i0 = (size_t)blockIdx.y * SR_TILE;
#pragma unroll
    for (int r = 0; r < SR_TILE / SR_THREADS; ++r) {
        const size_t i = i0 + (size_t)r * SR_THREADS + threadIdx.x;
        if (i < n3) dst[i] = src[i];
    }
}

int sr_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_smc_reweight: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

}  // namespace

size_t genie_smc_reweight_work_bytes(int S, int K, int N) {
    return (S >= 1 && K >= 1 && K <= SR_MAX_K && N >= 1) ? (size_t)S * K * sizeof(double) : 0;
}

int genie_smc_reweight(genie_stream_t stream, int S, int K, int N, const float* x_new, const float* mean_tw, const float* mean_un,
                       const float* sigma, const float* log_prob, const float* u, double ess_fraction, float* log_proposal,
                       float* log_w_acc, float* x_out, int32_t* index_out, float* ess_out, int32_t* resampled_out, void* work,
                       size_t work_bytes) {
    if (!x_new || !mean_tw || !mean_un || !sigma || !log_prob || !u || !log_proposal || !log_w_acc || !x_out || !index_out || !ess_out ||
        !resampled_out || !work)
        return sr_refuse("null pointer");
    if (K < 1 || K > SR_MAX_K) return sr_refuse("K outside 1..64");
    if (S < 1 || N < 1) return sr_refuse("S or N below 1");
    if ((int64_t)S * K > INT32_MAX) return sr_refuse("S * K above 2^31 - 1");
    const size_t n3 = 3 * (size_t)N, B = (size_t)S * K, tiles = (n3 + SR_TILE - 1) / SR_TILE;
    if (tiles > 65535) return sr_refuse("N too large");
    if (!isfinite(ess_fraction)) return sr_refuse("non-finite ess_fraction");
    const uintptr_t xo = reinterpret_cast<uintptr_t>(x_out), xn = reinterpret_cast<uintptr_t>(x_new), xb = B * n3 * sizeof(float);
    if (xo < xn + xb && xn < xo + xb) return sr_refuse("x_out overlaps x_new");
    const uintptr_t lp = reinterpret_cast<uintptr_t>(log_prob), lq = reinterpret_cast<uintptr_t>(log_proposal), lb = B * sizeof(float);
    if (lp < lq + lb && lq < lp + lb) return sr_refuse("log_proposal overlaps log_prob");
    if (work_bytes < genie_smc_reweight_work_bytes(S, K, N)) return sr_refuse("work_bytes below genie_smc_reweight_work_bytes(S, K, N)");
    if (reinterpret_cast<uintptr_t>(work) & 7) return sr_refuse("work not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* lw = static_cast<double*>(work);
    hipLaunchKernelGGL(k_smc_log_w, dim3((unsigned)B), dim3(SR_THREADS), 0, st, N, x_new, mean_tw, mean_un, sigma, log_prob,
                       (const float*)log_proposal, (const float*)log_w_acc, lw);
    hipLaunchKernelGGL(k_smc_gather, dim3((unsigned)B, (unsigned)tiles), dim3(SR_THREADS), 0, st, K, N, x_new, log_prob, u, ess_fraction,
                       (const double*)lw, log_proposal, log_w_acc, x_out, index_out, ess_out, resampled_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
