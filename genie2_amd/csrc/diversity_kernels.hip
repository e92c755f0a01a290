// Diversity potential of twisted-diffusion / SMC sampling (include/genie_hip.h: genie_diversity_potential): the particles of one batch
// repel each other.  The batch x0 [B, N, 3] is S = B / K particle systems of K particles, system-major (sys(b) = b / K); every
// unordered pair of particles of DIFFERENT systems is scored once by the gapless, seeded ascent of csrc/fold_kernels.hip -- the
// particle of the lower index moving, the other one standing in for the reference -- and its one fit gives a gradient to both
// members.  Particles of one system are resampled copies of each other and are never scored.  The reference has no counterpart.
//
// For i < j, sys(i) != sys(j), x = x_i, y = x_j, d0 = d0(N) and the 11 seed windows of genie_pairwise_tm over 0..N-1:
//   n_ij = the largest over the seeds (ties to the lowest) of sum_n g_n of the seed's LAST of n_iter iterations, (R, c_p, c_q) that
//   seed's last fit: genie_fold_potential's procedure, operation for operation;  n_ji := n_ij;  tm = n / N;
//   a_bj = (n_bj - N tm_max)_+,  E_b = (weight / K) sum_{j: sys(j) != sys(b)} a_bj^2,  logp[b] = -E_b / (2 var);
//   grad[b,n] = c ( sum_{j > b} a_bj g_n^2 R^T e_n  -  sum_{j < b} a_bj g_n^2 e_n ),  c = 2 weight / (K var d0^2), with e_n the
//   pair's residual under its stored fit, R (x_lower,n - c_p) - (x_higher,n - c_q): the derivative of logp[b] in x_b alone, every
//   other particle and every fit held fixed.
//
// k_diversity_fit: one 256-thread work-group per unordered pair, pair p = j (j - 1) / 2 + i for i < j, decoded from blockIdx.x; a
// pair inside one system returns at once.  Otherwise k_fold_fit with x_i for the particle and x_j for the reference: the same LDS
// layout (24 N + 344 bytes), the seeds dealt to the four waves, lanes striding over the residues, butterfly sums, the Jacobi solve of
// horn.h in every lane.  Thread 0 writes n, the seed, the fit and the two staged centroids to the pair's DV_FIT floats of `work`, and
// n / N to tm_out[i, j] and tm_out[j, i].
// k_diversity_finish: grid (ceil(N / 256), B), 256 threads, one thread per residue.  Every thread walks the partners j in index
// order, skipping its own system: the hinge, the energy and the report from the stored n (the same bits in every thread), and, for a
// pair with an active hinge only, its residue's residual under the stored fit -- formed from x0 with the operations the fit kernel
// used -- and the moving-side (j > b) or reference-side (j < b) share of the gradient.  Thread 0 of tile 0 writes logp, the report and
// the zeros of tm_out's same-system entries, the diagonal among them.
// No atomics, no scratch, fixed summation trees and orders: two calls on the same inputs are bitwise equal.  Rows n >= N of x0 and
// the same-system slots of `work` are never read; with S = 1 nothing is fitted and `work` is not touched.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"
#include "horn.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int DV_THREADS = 256;
constexpr int DV_WAVES = DV_THREADS / 64;
constexpr int DV_SEEDS = GENIE_TM_SEEDS;
constexpr int DV_MIN_LEN = GENIE_TM_MIN_LENGTH;
constexpr int DV_MAX_LEN = GENIE_TM_MAX_LENGTH;
constexpr int DV_MAX_K = 64;            // particles per system, genie_smc_reweight's
constexpr int DV_FIT = 24;              // floats of `work` per pair, the DV_* below
constexpr int DV_BEST = 17;             // floats a wave leaves in LDS: value, seed, R (9), c_p (3), c_q (3)
enum { DV_N = 0, DV_SEED = 1, DV_ROT = 2, DV_CP = 11, DV_CQ = 14, DV_XCEN = 17, DV_YCEN = 20, DV_UNUSED = 23 };

// dynamic LDS of k_diversity_fit: [xs: 3 N] [ys: 3 N] [part: 3 WAVES] [cen: 6] [best: DV_BEST * WAVES]
size_t dv_lds_bytes(int N) { return sizeof(float) * (6 * (size_t)N + 3 * DV_WAVES + 6 + DV_BEST * DV_WAVES); }

// unordered pairs of B particles, and the slot of pair (i, j), i < j
__host__ __device__ inline size_t dv_pairs(int B) { return (size_t)B * (size_t)(B - 1) / 2; }
__device__ inline size_t dv_slot(int i, int j) { return (size_t)j * (size_t)(j - 1) / 2 + (size_t)i; }

__device__ inline float dv_wave_sum(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// d0 of the TM-score for a normalising length L
__device__ inline float dv_d0(int L) { return L > 15 ? fmaxf(0.5f, 1.24f * cbrtf((float)(L - 15)) - 1.8f) : 0.5f; }

// seed s of a chain of L residues: (start, length) of its window
__device__ inline void dv_window(int s, int L, int& start, int& len) {
    if (s == 0) {
        start = 0;
        len = L;
        return;
    }
    const int k = s < 4 ? 1 : 2, j = s < 4 ? s - 1 : s - 4, n = s < 4 ? 3 : 7;
    len = max((L + (1 << k) - 1) >> k, DV_MIN_LEN);
    start = j * (L - len) / (n - 1);
}

// stages rows 0..L-1 of src in dst, centred on their centroid, which goes to cen[0..2] (a fixed tree: per-thread strided sums,
// butterfly, waves in order)
__device__ inline void dv_stage(const float* __restrict__ src, int L, float* dst, float* part, float* cen) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int n = tid; n < L; n += DV_THREADS) {
        const float x = src[3 * n], y = src[3 * n + 1], z = src[3 * n + 2];
        dst[3 * n] = x;
        dst[3 * n + 1] = y;
        dst[3 * n + 2] = z;
        sx += x;
        sy += y;
        sz += z;
    }
    sx = dv_wave_sum(sx);
    sy = dv_wave_sum(sy);
    sz = dv_wave_sum(sz);
    if (lane == 0) {
        part[3 * w] = sx;
        part[3 * w + 1] = sy;
        part[3 * w + 2] = sz;
    }
    __syncthreads();
    float cx = part[0], cy = part[1], cz = part[2];
    for (int u = 1; u < DV_WAVES; ++u) {
        cx += part[3 * u];
        cy += part[3 * u + 1];
        cz += part[3 * u + 2];
    }
    cx /= (float)L;
    cy /= (float)L;
    cz /= (float)L;
    for (int n = tid; n < L; n += DV_THREADS) {                   // (each thread centres the rows it wrote)
        dst[3 * n] -= cx;
        dst[3 * n + 1] -= cy;
        dst[3 * n + 2] -= cz;
    }
    if (tid == 0) {
        cen[0] = cx;
        cen[1] = cy;
        cen[2] = cz;
    }
    __syncthreads();                                             // (`part` is free again, dst is complete)
}

__global__ __launch_bounds__(DV_THREADS) void k_diversity_fit(int B, int K, int N, const float* __restrict__ x0, int n_iter,
                                                              float* __restrict__ work, float* __restrict__ tm_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dv_smem[];
    // pair p = j (j - 1) / 2 + i, i < j: j from the root (8 p + 1 < 2^24 is exact in float), then set right by at most a step
    const int p = blockIdx.x, tid = threadIdx.x;
    int j = (int)((1.f + sqrtf((float)(8 * p + 1))) * 0.5f);
    while (j * (j - 1) / 2 > p) --j;
    while ((j + 1) * j / 2 <= p) ++j;
    const int i = p - j * (j - 1) / 2;
    if (j >= B || i / K == j / K) return;                        // (the whole work-group: one system's particles do not repel)
    float* xs = reinterpret_cast<float*>(dv_smem);
    float* ys = xs + 3 * (size_t)N;
    float* part = ys + 3 * (size_t)N;
    float* cen = part + 3 * DV_WAVES;
    float* best = cen + 6;
    dv_stage(x0 + (size_t)i * 3 * N, N, xs, part, cen);
    dv_stage(x0 + (size_t)j * 3 * N, N, ys, part, cen + 3);

    const float d0 = dv_d0(N), inv_d0sq = 1.f / (d0 * d0);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    float best_n = -1.f;
    int best_s = INT_MAX;
    float* mine = best + DV_BEST * w;                            // the wave's best fit lives in LDS, not in registers
    if (lane == 0) {                                             // (the identity, should no seed ever win: a score that is NaN everywhere)
        for (int k = 0; k < 15; ++k) mine[2 + k] = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f;
    }

    for (int s = w; s < DV_SEEDS; s += DV_WAVES) {
        int ws, wl;
        dv_window(s, N, ws, wl);

        // the window's centroids
        float c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int n = ws + lane; n < ws + wl; n += 64) {
            c[0] += xs[3 * n];
            c[1] += xs[3 * n + 1];
            c[2] += xs[3 * n + 2];
            c[3] += ys[3 * n];
            c[4] += ys[3 * n + 1];
            c[5] += ys[3 * n + 2];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = dv_wave_sum(c[k]) / (float)wl;
        float cpx = c[0], cpy = c[1], cpz = c[2], cqx = c[3], cqy = c[4], cqz = c[5];

        // the window's correlation about them, and its fit
        float a[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = 0.f;
        for (int n = ws + lane; n < ws + wl; n += 64) {
            const float px = xs[3 * n] - cpx, py = xs[3 * n + 1] - cpy, pz = xs[3 * n + 2] - cpz;
            const float qx = ys[3 * n] - cqx, qy = ys[3 * n + 1] - cqy, qz = ys[3 * n + 2] - cqz;
            a[7] += px * qx;
            a[8] += px * qy;
            a[9] += px * qz;
            a[10] += py * qx;
            a[11] += py * qy;
            a[12] += py * qz;
            a[13] += pz * qx;
            a[14] += pz * qy;
            a[15] += pz * qz;
        }
#pragma unroll
        for (int k = 7; k < 16; ++k) a[k] = dv_wave_sum(a[k]);
        MrMat Rm = mr_rotation(mr_quaternion(MrMat{a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15]}));

        float value = 0.f;
        for (int it = 0; it < n_iter; ++it) {
            // one pass: the distances under (R, c_p, c_q), the score, and the weighted sums of the next fit about (c_p, c_q)
            float sc = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) a[k] = 0.f;
            for (int n = lane; n < N; n += 64) {
                const float px = xs[3 * n] - cpx, py = xs[3 * n + 1] - cpy, pz = xs[3 * n + 2] - cpz;
                const float qx = ys[3 * n] - cqx, qy = ys[3 * n + 1] - cqy, qz = ys[3 * n + 2] - cqz;
                const float ex = (Rm.xx * px + Rm.xy * py + Rm.xz * pz) - qx;
                const float ey = (Rm.yx * px + Rm.yy * py + Rm.yz * pz) - qy;
                const float ez = (Rm.zx * px + Rm.zy * py + Rm.zz * pz) - qz;
                const float d2 = ex * ex + ey * ey + ez * ez;
                const float g = 1.f / (1.f + d2 * inv_d0sq), wt = g * g;
                sc += g;
                a[0] += wt;
                a[1] += wt * px;
                a[2] += wt * py;
                a[3] += wt * pz;
                a[4] += wt * qx;
                a[5] += wt * qy;
                a[6] += wt * qz;
                const float wx = wt * px, wy = wt * py, wz = wt * pz;
                a[7] += wx * qx;
                a[8] += wx * qy;
                a[9] += wx * qz;
                a[10] += wy * qx;
                a[11] += wy * qy;
                a[12] += wy * qz;
                a[13] += wz * qx;
                a[14] += wz * qy;
                a[15] += wz * qz;
            }
            if (it + 1 == n_iter) {                              // (the last iteration is the seed's value: its fit stays)
                value = dv_wave_sum(sc);
                break;
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) a[k] = dv_wave_sum(a[k]);
            const float sw = a[0] > 0.f ? a[0] : 1.f;            // (every weight underflowed: the fit stays put)
            const float mpx = a[1] / sw, mpy = a[2] / sw, mpz = a[3] / sw, mqx = a[4] / sw, mqy = a[5] / sw, mqz = a[6] / sw;
            Rm = mr_rotation(mr_quaternion(MrMat{a[7] - a[1] * mqx, a[8] - a[1] * mqy, a[9] - a[1] * mqz, a[10] - a[2] * mqx,
                                                 a[11] - a[2] * mqy, a[12] - a[2] * mqz, a[13] - a[3] * mqx, a[14] - a[3] * mqy,
                                                 a[15] - a[3] * mqz}));
            cpx += mpx;
            cpy += mpy;
            cpz += mpz;
            cqx += mqx;
            cqy += mqy;
            cqz += mqz;
        }
        if (value > best_n) {                                    // (strictly: the lowest seed of equal values stays; wave-uniform)
            best_n = value;
            best_s = s;
            if (lane == 0) {
                mine[2] = Rm.xx;
                mine[3] = Rm.xy;
                mine[4] = Rm.xz;
                mine[5] = Rm.yx;
                mine[6] = Rm.yy;
                mine[7] = Rm.yz;
                mine[8] = Rm.zx;
                mine[9] = Rm.zy;
                mine[10] = Rm.zz;
                mine[11] = cpx;
                mine[12] = cpy;
                mine[13] = cpz;
                mine[14] = cqx;
                mine[15] = cqy;
                mine[16] = cqz;
            }
        }
    }

    if (lane == 0) {
        mine[0] = best_n;
        mine[1] = __int_as_float(best_s);
    }
    __syncthreads();
    if (tid != 0) return;
    int u = 0;
    float v = best[0];
    int s = __float_as_int(best[1]);
    for (int k = 1; k < DV_WAVES; ++k) {
        const float vk = best[DV_BEST * k];
        const int sk = __float_as_int(best[DV_BEST * k + 1]);
        if (vk > v || (vk == v && sk < s)) {
            v = vk;
            s = sk;
            u = k;
        }
    }
    const float* m = best + DV_BEST * u;
    float* f = work + dv_slot(i, j) * DV_FIT;
    f[DV_N] = v;
    f[DV_SEED] = __int_as_float(s);
    for (int k = 0; k < 15; ++k) f[DV_ROT + k] = m[2 + k];
    for (int k = 0; k < 6; ++k) f[DV_XCEN + k] = cen[k];
    f[DV_UNUSED] = 0.f;
    if (tm_out) {
        const float tm = v / (float)N;
        tm_out[(size_t)i * B + j] = tm;
        tm_out[(size_t)j * B + i] = tm;
    }
}

__global__ __launch_bounds__(DV_THREADS) void k_diversity_finish(int B, int K, int N, const float* __restrict__ x0, float tm_max,
                                                                 float weight, const float* __restrict__ var_p,
                                                                 const float* __restrict__ work, float* __restrict__ logp,
                                                                 float* __restrict__ grad, float* __restrict__ report,
                                                                 float* __restrict__ tm_out) {
    const int b = blockIdx.y, n = blockIdx.x * DV_THREADS + threadIdx.x;
    if (n >= N) return;                                          // (thread 0 of tile 0 is always a residue: N >= 4)
    const bool force = grad != nullptr;
    const int own = b / K;
    const float* xp = x0 + ((size_t)b * N + n) * 3;
    const float xn = xp[0], yn = xp[1], zn = xp[2];
    const float d0 = dv_d0(N), inv_d0sq = 1.f / (d0 * d0), fN = (float)N, bound = fN * tm_max;
    float gx = 0.f, gy = 0.f, gz = 0.f, sum_sq = 0.f, tm_top = 0.f, tm_sum = 0.f;
    int nearest = -1, similar = 0, partners = 0;
    for (int j = 0; j < B; ++j) {                                // (j, and all but the residue's own terms, are the same in every thread)
        if (j / K == own) continue;
        const bool moving = b < j;                               // b moved in the fit of (b, j); it stood still in that of (j, b)
        const float* f = work + (moving ? dv_slot(b, j) : dv_slot(j, b)) * DV_FIT;
        const float nr = f[DV_N], tm = nr / fN;
        const float a = fmaxf(nr - bound, 0.f);
        sum_sq += a * a;
        tm_sum += tm;
        ++partners;
        if (a > 0.f) ++similar;
        if (nearest < 0 || tm > tm_top) {                        // (strictly: the lowest index of equal scores)
            tm_top = tm;
            nearest = j;
        }
        if (a == 0.f || !force) continue;                        // (an idle hinge: exactly nothing)
        const float* op = x0 + ((size_t)j * N + n) * 3;
        const float ox = op[0], oy = op[1], oz = op[2];
        const float mx = moving ? xn : ox, my = moving ? yn : oy, mz = moving ? zn : oz;      // the residue of the chain that moved
        const float sx = moving ? ox : xn, sy = moving ? oy : yn, sz = moving ? oz : zn;      // ... and of the one that stood still
        const float px = (mx - f[DV_XCEN]) - f[DV_CP], py = (my - f[DV_XCEN + 1]) - f[DV_CP + 1], pz = (mz - f[DV_XCEN + 2]) - f[DV_CP + 2];
        const float qx = (sx - f[DV_YCEN]) - f[DV_CQ], qy = (sy - f[DV_YCEN + 1]) - f[DV_CQ + 1], qz = (sz - f[DV_YCEN + 2]) - f[DV_CQ + 2];
        const float* m = f + DV_ROT;                             // xx xy xz yx yy yz zx zy zz
        const float ex = (m[0] * px + m[1] * py + m[2] * pz) - qx;
        const float ey = (m[3] * px + m[4] * py + m[5] * pz) - qy;
        const float ez = (m[6] * px + m[7] * py + m[8] * pz) - qz;
        const float d2 = ex * ex + ey * ey + ez * ez;
        const float g = 1.f / (1.f + d2 * inv_d0sq), c = a * (g * g);
        if (moving) {                                            // + a g^2 R^T e
            gx += c * (m[0] * ex + m[3] * ey + m[6] * ez);
            gy += c * (m[1] * ex + m[4] * ey + m[7] * ez);
            gz += c * (m[2] * ex + m[5] * ey + m[8] * ez);
        } else {                                                 // - a g^2 e
            gx -= c * ex;
            gy -= c * ey;
            gz -= c * ez;
        }
    }
    const float share = weight / (float)K;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const float energy = share * sum_sq;
        if (logp) logp[b] = -energy / (2.f * *var_p);
        if (report) {
            float* out = report + (size_t)b * GENIE_DIVERSITY_REPORT;
            out[0] = tm_top;
            out[1] = (float)nearest;
            out[2] = partners ? tm_sum / (float)partners : 0.f;
            out[3] = (float)similar;
            out[4] = energy;
        }
        if (tm_out)                                              // (the scored entries are the fit kernel's)
            for (int j = own * K; j < own * K + K; ++j) tm_out[(size_t)b * B + j] = 0.f;
    }
    if (!force) return;
    const float sc = 2.f * share * inv_d0sq / *var_p;
    float* out = grad + ((size_t)b * N + n) * 3;
    out[0] = sc * gx;
    out[1] = sc * gy;
    out[2] = sc * gz;
}

int dv_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_diversity_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

}  // namespace

size_t genie_diversity_potential_work_bytes(int B, int K, int N) {
    if (B < 1 || B > GENIE_DIVERSITY_MAX_BATCH || K < 1 || K > DV_MAX_K || B % K != 0 || N < DV_MIN_LEN || N > DV_MAX_LEN) return 0;
    const size_t pairs = dv_pairs(B);
    return (pairs ? pairs : 1) * DV_FIT * sizeof(float);         // (one particle has no pair: a slot nobody touches, so that `work` is never NULL)
}

int genie_diversity_potential(genie_stream_t stream, int B, int K, int N, const float* x0, float tm_max, float weight, int n_iter,
                              const float* var, float* logp_out, float* grad_out, float* report_out, float* tm_out, void* work,
                              size_t work_bytes) {
    if (B < 1 || B > GENIE_DIVERSITY_MAX_BATCH) return dv_refuse("B outside 1..GENIE_DIVERSITY_MAX_BATCH (1448)");
    if (K < 1 || K > DV_MAX_K || B % K != 0) return dv_refuse("K outside 1..64 or not a divisor of B");
    if (N < DV_MIN_LEN || N > DV_MAX_LEN) return dv_refuse("N outside 4..1706");
    if (n_iter < 1 || n_iter > GENIE_TM_MAX_ITER) return dv_refuse("n_iter outside 1..32");
    if (!(tm_max > 0.f && tm_max <= 1.f)) return dv_refuse("tm_max not in (0, 1]");
    if (!(isfinite(weight) && weight >= 0.f)) return dv_refuse("weight not finite or negative");
    if (!x0) return dv_refuse("x0 is NULL");
    if (!var) return dv_refuse("var is NULL");
    if (!logp_out && !grad_out && !report_out && !tm_out)
        return dv_refuse("no output asked for (logp_out, grad_out, report_out and tm_out are NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return dv_refuse("logp_out and grad_out are given together or both NULL");
    if (!work || work_bytes < genie_diversity_potential_work_bytes(B, K, N))
        return dv_refuse("work is NULL or work_bytes below genie_diversity_potential_work_bytes(B, K, N)");
    if (reinterpret_cast<uintptr_t>(work) & 3) return dv_refuse("work not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* fits = static_cast<float*>(work);
    if (B > K)                                                   // (one system: nothing to fit, and the finish reads no fit)
        hipLaunchKernelGGL(k_diversity_fit, dim3((unsigned)dv_pairs(B)), dim3(DV_THREADS), dv_lds_bytes(N), st, B, K, N, x0, n_iter, fits,
                           tm_out);
    hipLaunchKernelGGL(k_diversity_finish, dim3((N + DV_THREADS - 1) / DV_THREADS, B), dim3(DV_THREADS), 0, st, B, K, N, x0, tm_max, weight,
                       var, (const float*)fits, logp_out, grad_out, report_out, tm_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
