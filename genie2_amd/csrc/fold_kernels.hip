// Fold potential of twisted-diffusion / SMC sampling (include/genie_hip.h: genie_fold_potential): the TM-score of every particle to
// every one of R fixed reference backbones of the same length, kept in a range per reference -- above a minimum for a template to
// sample around, below a maximum for folds to stay away from -- with its gradient and a per-particle report, in two launches.  The
// score is the gapless, seeded ascent of csrc/similarity_kernels.hip at offset 0 with the particle moving; the
// reference has no counterpart.
//
// For particle b (x_n), reference r (y_n), n = 0..N-1, d0 = d0(N), and the 11 seed windows of genie_pairwise_tm over 0..N-1:
//   from seed s, n_iter iterations of: (R, c_p, c_q) = the weighted Horn fit (proper rotations only), d_n^2 = |R (x_n - c_p) - (y_n - c_q)|^2
//   for all N residues, g_n = 1 / (1 + d_n^2 / d0^2), next weights g_n^2; the seed's value is sum_n g_n of its LAST iteration;
//   n_r = the largest value over the seeds (ties to the lowest seed), (R*, c_p*, c_q*) that seed's last fit, tm_r = n_r / N;
//   E = sum_r weight_r [ (N lo_r - n_r)_+^2 + (n_r - N hi_r)_+^2 ],  logp[b] = -E / (2 var);
//   grad[b,n] = (2 / (var d0^2)) sum_r k_r g_n^2 R*^T e_n,  e_n = R* (x_n - c_p*) - (y_n - c_q*),  k_r = weight_r ((n_r - N hi_r)_+ - (N lo_r - n_r)_+):
//   the derivative of logp with every pair's winning rigid transform held fixed.
//
// k_fold_fit: grid (R, B), 256 threads.  The work-group of pair (b, r) stages the particle and the reference in LDS, each centred on
// its own centroid (24 N + 344 bytes), and deals the seeds to its four waves, wave w taking s = w, w + 4, w + 8.  Inside a seed the
// lanes stride over the residues exactly as in k_pairwise_tm: one pass forms d_n^2 under the current fit, the score, and the 16
// weighted sums of the next fit about the current fit's centroids; the sums are butterflies inside the wave, so every lane holds the
// same bits and every lane runs the Jacobi solve of horn.h.  Each wave keeps the best (value, seed) of its seeds in seed order and
// that seed's fit in LDS; thread 0 takes the best of the four in wave order, ties to the lowest seed, and writes n_r, the seed, R*,
// c_p*, c_q* (both about the staged centroids) and the two staged centroids to the pair's FD_FIT floats of `work`, and tm_r to
// tm_out.
// k_fold_finish: grid (ceil(N / 256), B), 256 threads, one thread per residue.  Every thread walks the references in index order:
// the hinges, the energy and the report from the stored n_r (the same bits in every thread), and, for a reference with an active
// hinge and a positive weight only, its residue's e_n under the stored fit -- formed from x0 and ref with the operations k_fold_fit
// used -- and its share of the gradient.  Thread 0 of tile 0 writes logp and the report.
// No atomics, no scratch, fixed summation trees and orders: two calls on the same inputs are bitwise equal.  Rows n >= N are never
// read, of x0, ref or work.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"
#include "horn.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int FD_THREADS = 256;
constexpr int FD_WAVES = FD_THREADS / 64;
constexpr int FD_SEEDS = GENIE_TM_SEEDS;
constexpr int FD_MIN_LEN = GENIE_TM_MIN_LENGTH;
constexpr int FD_MAX_LEN = GENIE_TM_MAX_LENGTH;
constexpr int FD_FIT = 24;              // floats of `work` per (particle, reference), the FD_* below
constexpr int FD_BEST = 17;             // floats a wave leaves in LDS: value, seed, R (9), c_p (3), c_q (3)
enum { FD_N = 0, FD_SEED = 1, FD_ROT = 2, FD_CP = 11, FD_CQ = 14, FD_XCEN = 17, FD_YCEN = 20, FD_UNUSED = 23 };

// dynamic LDS of k_fold_fit: [xs: 3 N] [ys: 3 N] [part: 3 WAVES] [cen: 6] [best: FD_BEST * WAVES]
size_t fd_lds_bytes(int N) { return sizeof(float) * (6 * (size_t)N + 3 * FD_WAVES + 6 + FD_BEST * FD_WAVES); }

__device__ inline float fd_wave_sum(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// d0 of the TM-score for a normalising length L
__device__ inline float fd_d0(int L) { return L > 15 ? fmaxf(0.5f, 1.24f * cbrtf((float)(L - 15)) - 1.8f) : 0.5f; }

// seed s of a chain of L residues: (start, length) of its window
__device__ inline void fd_window(int s, int L, int& start, int& len) {
    if (s == 0) {
        start = 0;
        len = L;
        return;
    }
    const int k = s < 4 ? 1 : 2, j = s < 4 ? s - 1 : s - 4, n = s < 4 ? 3 : 7;
    len = max((L + (1 << k) - 1) >> k, FD_MIN_LEN);
    start = j * (L - len) / (n - 1);
}

// stages rows 0..L-1 of src in dst, centred on their centroid, which goes to cen[0..2] (a fixed tree: per-thread strided sums,
// butterfly, waves in order)
__device__ inline void fd_stage(const float* __restrict__ src, int L, float* dst, float* part, float* cen) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int n = tid; n < L; n += FD_THREADS) {
        const float x = src[3 * n], y = src[3 * n + 1], z = src[3 * n + 2];
        dst[3 * n] = x;
        dst[3 * n + 1] = y;
        dst[3 * n + 2] = z;
        sx += x;
        sy += y;
        sz += z;
    }
    sx = fd_wave_sum(sx);
    sy = fd_wave_sum(sy);
    sz = fd_wave_sum(sz);
    if (lane == 0) {
        part[3 * w] = sx;
        part[3 * w + 1] = sy;
        part[3 * w + 2] = sz;
    }
    __syncthreads();
    float cx = part[0], cy = part[1], cz = part[2];
    for (int u = 1; u < FD_WAVES; ++u) {
        cx += part[3 * u];
        cy += part[3 * u + 1];
        cz += part[3 * u + 2];
    }
    cx /= (float)L;
    cy /= (float)L;
    cz /= (float)L;
    for (int n = tid; n < L; n += FD_THREADS) {                   // (each thread centres the rows it wrote)
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

__global__ __launch_bounds__(FD_THREADS) void k_fold_fit(int N, int R, const float* __restrict__ x0, const float* __restrict__ ref,
                                                         int n_iter, float* __restrict__ work, float* __restrict__ tm_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fd_smem[];
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float* xs = reinterpret_cast<float*>(fd_smem);
    float* ys = xs + 3 * (size_t)N;
    float* part = ys + 3 * (size_t)N;
    float* cen = part + 3 * FD_WAVES;
    float* best = cen + 6;
    fd_stage(x0 + (size_t)b * 3 * N, N, xs, part, cen);
    fd_stage(ref + (size_t)r * 3 * N, N, ys, part, cen + 3);

    const float d0 = fd_d0(N), inv_d0sq = 1.f / (d0 * d0);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    float best_n = -1.f;
    int best_s = INT_MAX;
    float* mine = best + FD_BEST * w;                            // the wave's best fit lives in LDS, not in registers
    if (lane == 0) {                                             // (the identity, should no seed ever win: a score that is NaN everywhere)
        for (int k = 0; k < 15; ++k) mine[2 + k] = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f;
    }

    for (int s = w; s < FD_SEEDS; s += FD_WAVES) {
        int ws, wl;
        fd_window(s, N, ws, wl);

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
        for (int k = 0; k < 6; ++k) c[k] = fd_wave_sum(c[k]) / (float)wl;
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
        for (int k = 7; k < 16; ++k) a[k] = fd_wave_sum(a[k]);
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
                value = fd_wave_sum(sc);
                break;
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) a[k] = fd_wave_sum(a[k]);
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
    for (int k = 1; k < FD_WAVES; ++k) {
        const float vk = best[FD_BEST * k];
        const int sk = __float_as_int(best[FD_BEST * k + 1]);
        if (vk > v || (vk == v && sk < s)) {
            v = vk;
            s = sk;
            u = k;
        }
    }
    const float* m = best + FD_BEST * u;
    float* f = work + ((size_t)b * R + r) * FD_FIT;
    f[FD_N] = v;
    f[FD_SEED] = __int_as_float(s);
    for (int k = 0; k < 15; ++k) f[FD_ROT + k] = m[2 + k];
    for (int k = 0; k < 6; ++k) f[FD_XCEN + k] = cen[k];
    f[FD_UNUSED] = 0.f;
    if (tm_out) tm_out[(size_t)b * R + r] = v / (float)N;
}

__global__ __launch_bounds__(FD_THREADS) void k_fold_finish(int N, int R, const float* __restrict__ x0, const float* __restrict__ ref,
                                                            const float* __restrict__ bounds, const float* __restrict__ var_p,
                                                            const float* __restrict__ work, float* __restrict__ logp,
                                                            float* __restrict__ grad, float* __restrict__ report) {
    const int b = blockIdx.y, n = blockIdx.x * FD_THREADS + threadIdx.x;
    const bool live = n < N;
    const bool force = live && grad != nullptr;
    const float* xp = x0 + ((size_t)b * N + (live ? n : 0)) * 3;
    const float xn = xp[0], yn = xp[1], zn = xp[2];
    const float d0 = fd_d0(N), inv_d0sq = 1.f / (d0 * d0), fN = (float)N;
    float gx = 0.f, gy = 0.f, gz = 0.f, energy = 0.f, tm_max = -1.f, tm_low = INFINITY;
    int nearest = 0, violations = 0;
    for (int r = 0; r < R; ++r) {                                // (r, and all but the residue's own terms, are the same in every thread)
        const float* f = work + ((size_t)b * R + r) * FD_FIT;
        const float lo = bounds[3 * r], hi = bounds[3 * r + 1], wt = bounds[3 * r + 2];
        const float nr = f[FD_N], tm = nr / fN;
        const float below = fmaxf(fN * lo - nr, 0.f), above = fmaxf(nr - fN * hi, 0.f);      // (hi = +inf: above is 0)
        energy += wt * (below * below + above * above);
        if (below > 0.f || above > 0.f) ++violations;
        if (tm > tm_max) {                                       // (strictly: the lowest index of equal scores)
            tm_max = tm;
            nearest = r;
        }
        if (lo > 0.f) tm_low = fminf(tm_low, tm);
        const float k = wt * (above - below);
        if (k == 0.f || !force) continue;                        // (both hinges inactive, or weight 0: exactly nothing)
        const float* yp = ref + ((size_t)r * N + n) * 3;
        const float px = (xn - f[FD_XCEN]) - f[FD_CP], py = (yn - f[FD_XCEN + 1]) - f[FD_CP + 1], pz = (zn - f[FD_XCEN + 2]) - f[FD_CP + 2];
        const float qx = (yp[0] - f[FD_YCEN]) - f[FD_CQ], qy = (yp[1] - f[FD_YCEN + 1]) - f[FD_CQ + 1], qz = (yp[2] - f[FD_YCEN + 2]) - f[FD_CQ + 2];
        const float* m = f + FD_ROT;                             // xx xy xz yx yy yz zx zy zz
        const float ex = (m[0] * px + m[1] * py + m[2] * pz) - qx;
        const float ey = (m[3] * px + m[4] * py + m[5] * pz) - qy;
        const float ez = (m[6] * px + m[7] * py + m[8] * pz) - qz;
        const float d2 = ex * ex + ey * ey + ez * ez;
        const float g = 1.f / (1.f + d2 * inv_d0sq), c = k * (g * g);
        gx += c * (m[0] * ex + m[3] * ey + m[6] * ez);
        gy += c * (m[1] * ex + m[4] * ey + m[7] * ez);
        gz += c * (m[2] * ex + m[5] * ey + m[8] * ez);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (logp) logp[b] = -energy / (2.f * *var_p);
        if (report) {
            float* out = report + (size_t)b * GENIE_FOLD_REPORT;
            out[0] = tm_max;
            out[1] = (float)nearest;
            out[2] = tm_low == INFINITY ? 0.f : tm_low;
            out[3] = (float)violations;
            out[4] = energy;
        }
    }
    if (!force) return;
    const float sc = 2.f * inv_d0sq / *var_p;
    float* out = grad + ((size_t)b * N + n) * 3;
    out[0] = sc * gx;
    out[1] = sc * gy;
    out[2] = sc * gz;
}

int fd_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_fold_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

}  // namespace

size_t genie_fold_potential_work_bytes(int B, int N, int R) {
    return (B >= 1 && N >= FD_MIN_LEN && N <= FD_MAX_LEN && R >= 1 && R <= GENIE_FOLD_MAX_REFERENCES)
               ? (size_t)B * (size_t)R * FD_FIT * sizeof(float)
               : 0;
}

int genie_fold_potential(genie_stream_t stream, int B, int N, const float* x0, int R, const float* ref, const float* bounds, int n_iter,
                         const float* var, float* logp_out, float* grad_out, float* report_out, float* tm_out, void* work,
                         size_t work_bytes) {
    if (B < 1 || B > 65535) return fd_refuse("B outside 1..65535");
    if (N < FD_MIN_LEN || N > FD_MAX_LEN) return fd_refuse("N outside 4..1706");
    if (R < 1 || R > GENIE_FOLD_MAX_REFERENCES) return fd_refuse("R outside 1..GENIE_FOLD_MAX_REFERENCES (4096)");
    if (n_iter < 1 || n_iter > GENIE_TM_MAX_ITER) return fd_refuse("n_iter outside 1..32");
    if (!x0) return fd_refuse("x0 is NULL");
    if (!ref) return fd_refuse("ref is NULL");
    if (!bounds) return fd_refuse("bounds is NULL");
    if (!var) return fd_refuse("var is NULL");
    if (!logp_out && !grad_out && !report_out && !tm_out)
        return fd_refuse("no output asked for (logp_out, grad_out, report_out and tm_out are NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return fd_refuse("logp_out and grad_out are given together or both NULL");
    if (!work || work_bytes < genie_fold_potential_work_bytes(B, N, R))
        return fd_refuse("work is NULL or work_bytes below genie_fold_potential_work_bytes(B, N, R)");
    if (reinterpret_cast<uintptr_t>(work) & 3) return fd_refuse("work not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* fits = static_cast<float*>(work);
    hipLaunchKernelGGL(k_fold_fit, dim3(R, B), dim3(FD_THREADS), fd_lds_bytes(N), st, N, R, x0, ref, n_iter, fits, tm_out);
    if (logp_out || report_out)
        hipLaunchKernelGGL(k_fold_finish, dim3((N + FD_THREADS - 1) / FD_THREADS, B), dim3(FD_THREADS), 0, st, N, R, x0, ref, bounds, var,
                           (const float*)fits, logp_out, grad_out, report_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
