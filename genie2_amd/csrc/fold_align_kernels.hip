// Fold potential under gapped alignment (include/genie_hip.h: genie_fold_align_potential): the score of genie_tm_align between every
// particle and every one of R fixed reference backbones of any length, polished over its alignment and kept in a range per reference,
// with its gradient and a per-particle report, in two launches.  It is genie_fold_potential (csrc/fold_kernels.hip)
// with the identity alignment replaced by the alignment genie_tm_align finds (csrc/tmalign_kernels.hip); the header
// states the mathematics, DESIGN.md 7.11 the choices.  The reference has no counterpart.
//
// k_fold_align_fit: grid (R, B), 256 threads, one work-group per (particle, reference) pair; the particle is the query, a = the shorter
// chain moves (equal lengths: the particle), b = the longer one is fixed.  The search is k_tm_align's, written again here (the LDS
// layout, stage 0's item loop, the anti-diagonal wavefront with one owner per row of moves, the traceback by thread 0, the refit by
// wave 0) with one addition: stage 0 visits the offsets 0, s, 2 s, ... and the last one, item t = 11 v + seed for the v-th visited
// offset, so ties still go to the lowest offset and s = 1 is k_tm_align's loop.  Then wave 0 polishes the best stage's fit over its
// aligned pairs -- n_iter weighted Horn steps from the weights g(T*)^2, the LAST iteration kept -- and lane 0 writes n_r, Lnorm, d0
// and the fit to the pair's FA_FIT floats of `work` as (rot, c_x, c_y): rot (x - c_x) ~ y - c_y with x the particle's and y the
// reference's coordinates, whichever chain moved; the centres are the staged centroid plus the fit's own, so k_fold_align_finish
// forms e from differences of nearby numbers.  All threads write the query-indexed map to `work`, inverted through LDS when the
// reference moved.
// k_fold_align_finish: grid (ceil(N / 256), B), 256 threads, one thread per query residue.  Every thread walks the references in index
// order: the hinges, the energy and the report from the stored n_r (the same bits in every thread), and, for a reference with k_r != 0
// and a residue that is aligned, e_i under the stored fit and its share of the gradient.  Thread 0 of tile 0 writes logp and the report.
// LDS of the fit kernel: k_tm_align's, 8 (3 (Na + 1)) + 4 (9 Na + 3 Nb + Na ceil(Nb / 16) + 128) bytes, 59 904 at 362 x 362, the most
// any call inside MAX_CELLS asks for.  No atomics, no scratch, fixed summation trees and orders: two calls on the same inputs are
// bitwise equal.  Only rows below a chain's length are read, so padding never reaches a result.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"
#include "horn.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int FA_THREADS = 256;
constexpr int FA_WAVES = FA_THREADS / 64;
constexpr int FA_SEEDS = GENIE_TM_SEEDS;
constexpr int FA_MIN_LEN = GENIE_TM_MIN_LENGTH;
constexpr int FA_MAX_LEN = GENIE_TMALIGN_MAX_LENGTH;
constexpr int FA_ROWS = 2;                              // table rows per thread: La <= 362 < FA_ROWS * FA_THREADS
constexpr int FA_SLOT = 16;                             // floats of a fit kept in LDS: R (9), c_p (3), c_q (3), the score
constexpr int FA_MISC = 128;                            // floats: part (16), best (8), fits (6 x 16), the traceback's count
constexpr int FA_CUR = 4, FA_BEST = 5;                  // fit slots after the four waves': the stage's starting fit, the best stage's
constexpr int FA_FIT = 20;                              // floats of `work` per pair, the FA_* below
enum { FA_N = 0, FA_LNORM = 1, FA_D0 = 2, FA_ROT = 3, FA_CX = 12, FA_CY = 15, FA_UNUSED = 18 };
static_assert((long long)(FA_ROWS * FA_THREADS) * (FA_ROWS * FA_THREADS) > GENIE_TMALIGN_MAX_CELLS, "a thread owns FA_ROWS rows");

struct FaFit {
    MrMat R;
    float cpx, cpy, cpz, cqx, cqy, cqz;
};

// dynamic LDS for chains padded to Na <= Nb: [dp: 3 x (Na + 1) float2] [a: 3 Na] [T a: 3 Na] [aln cur, prev, best: 3 Na] [b: 3 Nb]
// [misc: 128] [moves: Na ceil(Nb / 16)]
size_t fa_lds_bytes(int Na, int Nb) {
    return sizeof(float) * (6 * ((size_t)Na + 1) + 9 * (size_t)Na + 3 * (size_t)Nb + FA_MISC + (size_t)Na * ((Nb + 15) / 16));
}

__device__ inline float fa_wave_sum(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

__device__ inline float fa_d0(int L) { return L > 15 ? fmaxf(0.5f, 1.24f * cbrtf((float)(L - 15)) - 1.8f) : 0.5f; }

__device__ inline void fa_window(int s, int La, int& start, int& len) {
    if (s == 0) {
        start = 0;
        len = La;
        return;
    }
    const int k = s < 4 ? 1 : 2, j = s < 4 ? s - 1 : s - 4, n = s < 4 ? 3 : 7;
    len = max((La + (1 << k) - 1) >> k, FA_MIN_LEN);
    start = j * (La - len) / (n - 1);
}

// stages rows 0..L-1 of src in dst, centred on their centroid, which every thread returns (a fixed tree, as in tmalign_kernels.hip)
__device__ inline float3 fa_stage(const float* __restrict__ src, int L, float* dst, float* part) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int n = tid; n < L; n += FA_THREADS) {
        const float x = src[3 * n], y = src[3 * n + 1], z = src[3 * n + 2];
        dst[3 * n] = x;
        dst[3 * n + 1] = y;
        dst[3 * n + 2] = z;
        sx += x;
        sy += y;
        sz += z;
    }
    sx = fa_wave_sum(sx);
    sy = fa_wave_sum(sy);
    sz = fa_wave_sum(sz);
    if (lane == 0) {
        part[3 * w] = sx;
        part[3 * w + 1] = sy;
        part[3 * w + 2] = sz;
    }
    __syncthreads();
    float cx = part[0], cy = part[1], cz = part[2];
    for (int u = 1; u < FA_WAVES; ++u) {
        cx += part[3 * u];
        cy += part[3 * u + 1];
        cz += part[3 * u + 2];
    }
    cx /= (float)L;
    cy /= (float)L;
    cz /= (float)L;
    for (int n = tid; n < L; n += FA_THREADS) {
        dst[3 * n] -= cx;
        dst[3 * n + 1] -= cy;
        dst[3 * n + 2] -= cz;
    }
    __syncthreads();
    return make_float3(cx, cy, cz);
}

// One pass of one wave over the pairs (a_n, b_{idx(n)}), idx(n) = o + n (GAPPED false) or aln[n] with aln[n] < 0 left out: the
// distances under (R, c_p, c_q), the sum of g in sc, and in a[0..15] the weighted sums of the next fit about (c_p, c_q), per lane.
template <bool GAPPED>
__device__ inline void fa_pass(const float* as, const float* bs, const int* aln, int o, int La, const MrMat& R, float cpx, float cpy,
                               float cpz, float cqx, float cqy, float cqz, float inv_d0sq, int lane, float& sc, float (&a)[16]) {
    sc = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = 0.f;
    for (int n = lane; n < La; n += 64) {
        const int j = GAPPED ? aln[n] : o + n;
        if (GAPPED && j < 0) continue;
        const float px = as[3 * n] - cpx, py = as[3 * n + 1] - cpy, pz = as[3 * n + 2] - cpz;
        const float qx = bs[3 * j] - cqx, qy = bs[3 * j + 1] - cqy, qz = bs[3 * j + 2] - cqz;
        const float ex = (R.xx * px + R.xy * py + R.xz * pz) - qx;
        const float ey = (R.yx * px + R.yy * py + R.yz * pz) - qy;
        const float ez = (R.zx * px + R.zy * py + R.zz * pz) - qz;
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
}

// the next fit from a pass's sums: the wave's butterflies, the Horn solve in every lane, the centroids moved by the weighted means
__device__ inline void fa_step(float (&a)[16], MrMat& R, float& cpx, float& cpy, float& cpz, float& cqx, float& cqy, float& cqz) {
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = fa_wave_sum(a[k]);
    const float sw = a[0] > 0.f ? a[0] : 1.f;                    // (every weight underflowed: the fit stays put)
    const float mpx = a[1] / sw, mpy = a[2] / sw, mpz = a[3] / sw, mqx = a[4] / sw, mqy = a[5] / sw, mqz = a[6] / sw;
    R = mr_rotation(mr_quaternion(MrMat{a[7] - a[1] * mqx, a[8] - a[1] * mqy, a[9] - a[1] * mqz, a[10] - a[2] * mqx, a[11] - a[2] * mqy,
                                        a[12] - a[2] * mqz, a[13] - a[3] * mqx, a[14] - a[3] * mqy, a[15] - a[3] * mqz}));
    cpx += mpx;
    cpy += mpy;
    cpz += mpz;
    cqx += mqx;
    cqy += mqy;
    cqz += mqz;
}

// One ascent by one wave, k_tm_align's ta_ascent: seeded by the window [ws, ws + wl) of the threading at offset o (GAPPED false) or by
// all wl aligned pairs of aln (GAPPED true); where an iteration's score exceeds `best` (strictly) best takes it and lane 0 stores that
// iteration's fit in the wave's LDS slot `fit`; returns whether one did.
template <bool GAPPED>
__device__ inline bool fa_ascent(const float* as, const float* bs, const int* aln, int o, int La, int ws, int wl, int n_iter,
                                 float inv_d0sq, int lnorm, int lane, float& best, float* fit) {
    const int n0 = GAPPED ? 0 : ws, n1 = GAPPED ? La : ws + wl;
    float c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int n = n0 + lane; n < n1; n += 64) {
        const int j = GAPPED ? aln[n] : o + n;
        if (GAPPED && j < 0) continue;
        c[0] += as[3 * n];
        c[1] += as[3 * n + 1];
        c[2] += as[3 * n + 2];
        c[3] += bs[3 * j];
        c[4] += bs[3 * j + 1];
        c[5] += bs[3 * j + 2];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = fa_wave_sum(c[k]) / (float)wl;
    float cpx = c[0], cpy = c[1], cpz = c[2], cqx = c[3], cqy = c[4], cqz = c[5];

    float a[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = 0.f;
    for (int n = n0 + lane; n < n1; n += 64) {
        const int j = GAPPED ? aln[n] : o + n;
        if (GAPPED && j < 0) continue;
        const float px = as[3 * n] - cpx, py = as[3 * n + 1] - cpy, pz = as[3 * n + 2] - cpz;
        const float qx = bs[3 * j] - cqx, qy = bs[3 * j + 1] - cqy, qz = bs[3 * j + 2] - cqz;
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
    for (int k = 7; k < 16; ++k) a[k] = fa_wave_sum(a[k]);
    MrMat R = mr_rotation(mr_quaternion(MrMat{a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15]}));

    bool improved = false;
    for (int it = 0; it < n_iter; ++it) {
        float sc;
        fa_pass<GAPPED>(as, bs, aln, o, La, R, cpx, cpy, cpz, cqx, cqy, cqz, inv_d0sq, lane, sc, a);
        const float score = fa_wave_sum(sc) / (float)lnorm;
        if (score > best) {
            best = score;
            if (lane == 0) {
                fit[0] = R.xx, fit[1] = R.xy, fit[2] = R.xz, fit[3] = R.yx, fit[4] = R.yy, fit[5] = R.yz, fit[6] = R.zx, fit[7] = R.zy, fit[8] = R.zz;
                fit[9] = cpx, fit[10] = cpy, fit[11] = cpz, fit[12] = cqx, fit[13] = cqy, fit[14] = cqz;
            }
            improved = true;
        }
        if (it + 1 == n_iter) break;
        fa_step(a, R, cpx, cpy, cpz, cqx, cqy, cqz);
    }
    return improved;
}

__device__ inline FaFit fa_get_fit(const float* src) {
    FaFit f;
    f.R = MrMat{src[0], src[1], src[2], src[3], src[4], src[5], src[6], src[7], src[8]};
    f.cpx = src[9];
    f.cpy = src[10];
    f.cpz = src[11];
    f.cqx = src[12];
    f.cqy = src[13];
    f.cqz = src[14];
    return f;
}

// rot x_query + trans ~ x_reference from a fit in the centred frames of a (centroid ca) and b (cb), inverted when the reference moved
__device__ inline void fa_put_transform(const FaFit& f, float3 ca, float3 cb, bool swap, float* ro, float* to) {
    // b' ~ R (a' - c_p) + c_q in the centred frames: b ~ R a + t with t = cb + c_q - R (ca + c_p)
    const MrMat& R = f.R;
    const float ux = ca.x + f.cpx, uy = ca.y + f.cpy, uz = ca.z + f.cpz;
    const float tx = cb.x + f.cqx - (R.xx * ux + R.xy * uy + R.xz * uz);
    const float ty = cb.y + f.cqy - (R.yx * ux + R.yy * uy + R.yz * uz);
    const float tz = cb.z + f.cqz - (R.zx * ux + R.zy * uy + R.zz * uz);
    if (!swap) {
        ro[0] = R.xx, ro[1] = R.xy, ro[2] = R.xz, ro[3] = R.yx, ro[4] = R.yy, ro[5] = R.yz, ro[6] = R.zx, ro[7] = R.zy, ro[8] = R.zz;
        to[0] = tx, to[1] = ty, to[2] = tz;
    } else {                                                      // the reference moved: query = R ref + t, so ref = R^T (query - t)
        ro[0] = R.xx, ro[1] = R.yx, ro[2] = R.zx, ro[3] = R.xy, ro[4] = R.yy, ro[5] = R.zy, ro[6] = R.xz, ro[7] = R.yz, ro[8] = R.zz;
        to[0] = -(R.xx * tx + R.yx * ty + R.zx * tz);
        to[1] = -(R.xy * tx + R.yy * ty + R.zy * tz);
        to[2] = -(R.xz * tx + R.yz * ty + R.zz * tz);
    }
}

__global__ __launch_bounds__(FA_THREADS) void k_fold_align_fit(int N, const float* __restrict__ x0, int Nr, const float* __restrict__ xr,
                                                               const int* __restrict__ lr, int norm, int n_iter, int n_rounds,
                                                               float gap_open, int stride, float* __restrict__ fit_work,
                                                               int* __restrict__ map_work, float* __restrict__ tm_out,
                                                               int* __restrict__ n_aligned_out, int* __restrict__ map_out,
                                                               float* __restrict__ rot_out, float* __restrict__ trans_out,
                                                               float* __restrict__ rot0_out, float* __restrict__ trans0_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fa_smem[];
    const int r = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
    const int R_ = gridDim.x;
    const int Nq = N;
    const int Na = min(Nq, Nr), Nb = max(Nq, Nr);

    // the reference's length indexes LDS and global memory: clamped into 4..Nr whatever the array holds; the particle uses all N rows
    const int Lq = Nq, Lr = min(max(lr[r], FA_MIN_LEN), Nr);
    const bool swap = Lr < Lq;                                   // the shorter chain moves; equal lengths: the particle
    const int La = swap ? Lr : Lq, Lb = swap ? Lq : Lr;          // La <= Na, Lb <= Nb
    const float* pa = swap ? xr + (size_t)r * 3 * Nr : x0 + (size_t)m * 3 * Nq;
    const float* pb = swap ? x0 + (size_t)m * 3 * Nq : xr + (size_t)r * 3 * Nr;

    float2* dp = reinterpret_cast<float2*>(fa_smem);             // three diagonals of (val, path), row i at [i], i = 0..La
    float* as = reinterpret_cast<float*>(dp + 3 * ((size_t)Na + 1));
    float* ta = as + 3 * (size_t)Na;
    int* alnC = reinterpret_cast<int*>(ta + 3 * (size_t)Na);
    int* alnP = alnC + Na;
    int* alnB = alnP + Na;
    float* bs = reinterpret_cast<float*>(alnB + Na);
    float* part = bs + 3 * (size_t)Nb;
    float* best = part + 16;
    float* fits = best + 8;
    int* count = reinterpret_cast<int*>(fits + 6 * FA_SLOT);
    unsigned* moves = reinterpret_cast<unsigned*>(part + FA_MISC);
    const int W = (Lb + 15) >> 4;                                // dwords of a row of moves

    const float3 ca = fa_stage(pa, La, as, part);
    const float3 cb = fa_stage(pb, Lb, bs, part);

    const int lnorm = norm == 0 ? Lq : norm == 1 ? Lr : norm == 2 ? La : Lb;
    const float d0 = fa_d0(lnorm), inv_d0sq = 1.f / (d0 * d0);
    const int n_off = Lb - La + 1;
    const int n_vis = (n_off - 1 + stride - 1) / stride + 1;     // the offsets 0, s, 2 s, ... below the last one, and the last one
    const int n_items = n_vis * FA_SEEDS;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;

    // ---- stage 0: the seeded gapless search over the visited offsets ----
    float v_wave = -1.f;
    int t_wave = INT_MAX;
    if (lane < FA_SLOT) fits[w * FA_SLOT + lane] = lane == 0 || lane == 4 || lane == 8 ? 1.f : 0.f;      // (the identity, should no score compare)
    for (int t = w; t < n_items; t += FA_WAVES) {
        const int v = t / FA_SEEDS, s = t - v * FA_SEEDS;
        const int o = min(v * stride, n_off - 1);
        int ws, wl;
        fa_window(s, La, ws, wl);
        if (fa_ascent<false>(as, bs, nullptr, o, La, ws, wl, n_iter, inv_d0sq, lnorm, lane, v_wave, fits + w * FA_SLOT)) t_wave = t;
    }
    if (lane == 0) {
        best[2 * w] = v_wave;
        best[2 * w + 1] = __int_as_float(t_wave);
    }
    __syncthreads();
    float v_best = best[0];
    int t0 = __float_as_int(best[1]), w0 = 0;
    for (int u = 1; u < FA_WAVES; ++u) {
        const float vu = best[2 * u];
        const int tu = __float_as_int(best[2 * u + 1]);
        if (vu > v_best || (vu == v_best && tu < t0)) {
            v_best = vu;
            t0 = tu;
            w0 = u;
        }
    }
    const int v0 = min(max(t0 / FA_SEEDS, 0), n_vis - 1);        // (indexes LDS; a score that is NaN everywhere leaves t unset)
    const int o0 = min(v0 * stride, n_off - 1);
    if (tid < FA_SLOT) fits[FA_CUR * FA_SLOT + tid] = fits[FA_BEST * FA_SLOT + tid] = fits[w0 * FA_SLOT + tid];
    int cnt_best = La;
    for (int n = tid; n < La; n += FA_THREADS) alnP[n] = alnB[n] = o0 + n;
    for (int k = tid; k < 3; k += FA_THREADS) dp[k * ((size_t)La + 1)] = make_float2(0.f, 0.f);      // row 0 of every diagonal
    __syncthreads();

    // ---- stages 1..n_rounds: fill, trace back, refit ----
    for (int stage = 1; stage <= n_rounds; ++stage) {
        const FaFit f_cur = fa_get_fit(fits + FA_CUR * FA_SLOT);
        for (int n = tid; n < La; n += FA_THREADS) {
            const float px = as[3 * n] - f_cur.cpx, py = as[3 * n + 1] - f_cur.cpy, pz = as[3 * n + 2] - f_cur.cpz;
            ta[3 * n] = (f_cur.R.xx * px + f_cur.R.xy * py + f_cur.R.xz * pz) + f_cur.cqx;
            ta[3 * n + 1] = (f_cur.R.yx * px + f_cur.R.yy * py + f_cur.R.yz * pz) + f_cur.cqy;
            ta[3 * n + 2] = (f_cur.R.zx * px + f_cur.R.zy * py + f_cur.R.zz * pz) + f_cur.cqz;
            alnC[n] = -1;
        }
        __syncthreads();

        float tx[FA_ROWS], ty[FA_ROWS], tz[FA_ROWS], vl[FA_ROWS], pl[FA_ROWS];
        unsigned acc[FA_ROWS];
#pragma unroll
        for (int k = 0; k < FA_ROWS; ++k) {
            const int i = tid + 1 + k * FA_THREADS;
            const int n = min(i, La) - 1;
            tx[k] = ta[3 * n];
            ty[k] = ta[3 * n + 1];
            tz[k] = ta[3 * n + 2];
            vl[k] = 0.f;                                          // val(i, 0) = 0, path(i, 0) = false
            pl[k] = 0.f;
            acc[k] = 0u;
        }
        for (int d = 2; d <= La + Lb; ++d) {
            float2* cur = dp + (d % 3) * ((size_t)La + 1);
            const float2* p1 = dp + ((d + 2) % 3) * ((size_t)La + 1);
            const float2* p2 = dp + ((d + 1) % 3) * ((size_t)La + 1);
#pragma unroll
            for (int k = 0; k < FA_ROWS; ++k) {
                const int i = tid + 1 + k * FA_THREADS, j = d - i;
                if (i <= La && j >= 1 && j <= Lb) {
                    const float ex = tx[k] - bs[3 * (j - 1)], ey = ty[k] - bs[3 * (j - 1) + 1], ez = tz[k] - bs[3 * (j - 1) + 2];
                    const float sij = 1.f / (1.f + (ex * ex + ey * ey + ez * ez) * inv_d0sq);
                    const float2 up = p1[i - 1];
                    const float dg = (j == 1 ? 0.f : p2[i - 1].x) + sij;              // (val(i - 1, 0) = 0 is never stored)
                    const float hh = up.x + (up.y != 0.f ? gap_open : 0.f);
                    const float vv = vl[k] + (pl[k] != 0.f ? gap_open : 0.f);
                    const bool diag = dg >= hh && dg >= vv;
                    const float val = diag ? dg : fmaxf(hh, vv);
                    const unsigned mv = diag ? 0u : vv >= hh ? 2u : 1u;                // 0 diag, 1 up (i - 1), 2 left (j - 1)
                    cur[i] = make_float2(val, diag ? 1.f : 0.f);
                    vl[k] = val;
                    pl[k] = diag ? 1.f : 0.f;
                    const int c = j - 1;
                    acc[k] |= mv << (2 * (c & 15));
                    if ((c & 15) == 15 || c == Lb - 1) {
                        moves[(size_t)(i - 1) * W + (c >> 4)] = acc[k];
                        acc[k] = 0u;
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            int i = La, j = Lb, cnt = 0;
            while (i > 0 && j > 0) {
                const unsigned mv = (moves[(size_t)(i - 1) * W + ((j - 1) >> 4)] >> (2 * ((j - 1) & 15))) & 3u;
                if (mv == 0u) {
                    alnC[i - 1] = j - 1;
                    ++cnt;
                    --i;
                    --j;
                } else if (mv == 1u) {
                    --i;
                } else {
                    --j;
                }
            }
            *count = cnt;
        }
        __syncthreads();
        int differs = 0;
        for (int n = tid; n < La; n += FA_THREADS) differs |= alnC[n] != alnP[n];
        const int cnt = *count;
        if (!__syncthreads_or(differs)) break;                   // the alignment did not move: not fitted
        if (cnt < 3) break;
        if (w == 0) {
            float v = -1.f;
            fa_ascent<true>(as, bs, alnC, 0, La, 0, cnt, n_iter, inv_d0sq, lnorm, lane, v, fits);
            if (lane == 0) fits[15] = v;
        }
        __syncthreads();
        const float v = fits[15];
        const bool better = v > v_best;                          // (strictly: the earliest of equal stages stays)
        if (better) {
            v_best = v;
            cnt_best = cnt;
        }
        if (tid < FA_SLOT - 1) {
            const float f = fits[tid];
            fits[FA_CUR * FA_SLOT + tid] = f;
            if (better) fits[FA_BEST * FA_SLOT + tid] = f;
        }
        for (int n = tid; n < La; n += FA_THREADS) {
            const int c = alnC[n];
            alnP[n] = c;
            if (better) alnB[n] = c;
        }
        __syncthreads();
    }

    // ---- the polish over the best stage's pairs, and the pair's results ----
    const size_t pair = (size_t)m * R_ + r;
    if (w == 0) {
        FaFit f = fa_get_fit(fits + FA_BEST * FA_SLOT);
        if (lane == 0 && rot0_out) fa_put_transform(f, ca, cb, swap, rot0_out + 9 * pair, trans0_out + 3 * pair);
        float a[16], sc;
        for (int it = 0; it < n_iter; ++it) {                    // the weights g(T)^2 of the fit so far, and the fit they give
            fa_pass<true>(as, bs, alnB, 0, La, f.R, f.cpx, f.cpy, f.cpz, f.cqx, f.cqy, f.cqz, inv_d0sq, lane, sc, a);
            fa_step(a, f.R, f.cpx, f.cpy, f.cpz, f.cqx, f.cqy, f.cqz);
        }
        fa_pass<true>(as, bs, alnB, 0, La, f.R, f.cpx, f.cpy, f.cpz, f.cqx, f.cqy, f.cqz, inv_d0sq, lane, sc, a);
        const float n_r = fa_wave_sum(sc);                       // (the last iteration is the value: its fit stays)
        if (lane == 0) {
            float* fw = fit_work + pair * FA_FIT;
            const MrMat& R = f.R;
            const float ux = ca.x + f.cpx, uy = ca.y + f.cpy, uz = ca.z + f.cpz;      // R (a - u) ~ b - v
            const float vx = cb.x + f.cqx, vy = cb.y + f.cqy, vz = cb.z + f.cqz;
            fw[FA_N] = n_r;
            fw[FA_LNORM] = (float)lnorm;
            fw[FA_D0] = d0;
            if (!swap) {
                fw[FA_ROT] = R.xx, fw[FA_ROT + 1] = R.xy, fw[FA_ROT + 2] = R.xz, fw[FA_ROT + 3] = R.yx, fw[FA_ROT + 4] = R.yy;
                fw[FA_ROT + 5] = R.yz, fw[FA_ROT + 6] = R.zx, fw[FA_ROT + 7] = R.zy, fw[FA_ROT + 8] = R.zz;
                fw[FA_CX] = ux, fw[FA_CX + 1] = uy, fw[FA_CX + 2] = uz;
                fw[FA_CY] = vx, fw[FA_CY + 1] = vy, fw[FA_CY + 2] = vz;
            } else {                                              // the reference moved: R^T (x - v) ~ y - u
                fw[FA_ROT] = R.xx, fw[FA_ROT + 1] = R.yx, fw[FA_ROT + 2] = R.zx, fw[FA_ROT + 3] = R.xy, fw[FA_ROT + 4] = R.yy;
                fw[FA_ROT + 5] = R.zy, fw[FA_ROT + 6] = R.xz, fw[FA_ROT + 7] = R.yz, fw[FA_ROT + 8] = R.zz;
                fw[FA_CX] = vx, fw[FA_CX + 1] = vy, fw[FA_CX + 2] = vz;
                fw[FA_CY] = ux, fw[FA_CY + 1] = uy, fw[FA_CY + 2] = uz;
            }
            fw[FA_UNUSED] = 0.f;
            fw[FA_UNUSED + 1] = 0.f;
            if (tm_out) tm_out[pair] = n_r / (float)lnorm;
            if (n_aligned_out) n_aligned_out[pair] = cnt_best;
            if (rot_out) fa_put_transform(f, ca, cb, swap, rot_out + 9 * pair, trans_out + 3 * pair);
        }
    }
    int* mw = map_work + pair * (size_t)Nq;
    int* mo = map_out ? map_out + pair * (size_t)Nq : nullptr;
    if (!swap) {                                                 // La = Nq: the alignment is indexed by the particle's residues
        for (int n = tid; n < Nq; n += FA_THREADS) {
            const int j = alnB[n];
            mw[n] = j;
            if (mo) mo[n] = j;
        }
        return;
    }
    // the reference moved: invert the alignment in LDS (b's coordinates are no longer needed once wave 0 is through), then write it
    __syncthreads();
    int* inv = reinterpret_cast<int*>(bs);                       // Nq = Lb <= Nb ints fit in b's 3 Nb floats
    for (int n = tid; n < Nq; n += FA_THREADS) inv[n] = -1;
    __syncthreads();
    for (int n = tid; n < La; n += FA_THREADS) {
        const int j = alnB[n];
        if (j >= 0) inv[j] = n;
    }
    __syncthreads();
    for (int n = tid; n < Nq; n += FA_THREADS) {
        const int j = inv[n];
        mw[n] = j;
        if (mo) mo[n] = j;
    }
}

__global__ __launch_bounds__(FA_THREADS) void k_fold_align_finish(int N, int R, int Nr, const float* __restrict__ x0,
                                                                  const float* __restrict__ xr, const float* __restrict__ bounds,
                                                                  const float* __restrict__ var_p, const float* __restrict__ fit_work,
                                                                  const int* __restrict__ map_work, float* __restrict__ logp,
                                                                  float* __restrict__ grad, float* __restrict__ report) {
    const int b = blockIdx.y, n = blockIdx.x * FA_THREADS + threadIdx.x;
    const bool live = n < N;
    const bool force = live && grad != nullptr;
    const float* xp = x0 + ((size_t)b * N + (live ? n : 0)) * 3;
    const float xn = xp[0], yn = xp[1], zn = xp[2];
    float gx = 0.f, gy = 0.f, gz = 0.f, energy = 0.f, tm_max = -1.f, tm_low = INFINITY;
    int nearest = 0, violations = 0;
    for (int r = 0; r < R; ++r) {                                // (r, and all but the residue's own terms, are the same in every thread)
        const size_t pair = (size_t)b * R + r;
        const float* f = fit_work + pair * FA_FIT;
        const float lo = bounds[3 * r], hi = bounds[3 * r + 1], wt = bounds[3 * r + 2];
        const float nr = f[FA_N], fL = f[FA_LNORM], tm = nr / fL;
        const float below = fmaxf(fL * lo - nr, 0.f), above = fmaxf(nr - fL * hi, 0.f);      // (hi = +inf: above is 0)
        energy += wt * (below * below + above * above);
        if (below > 0.f || above > 0.f) ++violations;
        if (tm > tm_max) {                                       // (strictly: the lowest index of equal scores)
            tm_max = tm;
            nearest = r;
        }
        if (lo > 0.f) tm_low = fminf(tm_low, tm);
        const float k = wt * (above - below);
        if (k == 0.f || !force) continue;                        // (both hinges inactive, or weight 0: exactly nothing)
        const int j = map_work[pair * (size_t)N + n];
        if (j < 0 || j >= Nr) continue;                          // (an unaligned residue: exactly nothing)
        const float* yp = xr + ((size_t)r * Nr + j) * 3;
        const float d0 = f[FA_D0], inv_d0sq = 1.f / (d0 * d0);
        const float px = xn - f[FA_CX], py = yn - f[FA_CX + 1], pz = zn - f[FA_CX + 2];
        const float qx = yp[0] - f[FA_CY], qy = yp[1] - f[FA_CY + 1], qz = yp[2] - f[FA_CY + 2];
        const float* m = f + FA_ROT;                             // xx xy xz yx yy yz zx zy zz
        const float ex = (m[0] * px + m[1] * py + m[2] * pz) - qx;
        const float ey = (m[3] * px + m[4] * py + m[5] * pz) - qy;
        const float ez = (m[6] * px + m[7] * py + m[8] * pz) - qz;
        const float d2 = ex * ex + ey * ey + ez * ez;
        const float g = 1.f / (1.f + d2 * inv_d0sq), c = (k * inv_d0sq) * (g * g);
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
    const float sc = 2.f / *var_p;
    float* out = grad + ((size_t)b * N + n) * 3;
    out[0] = sc * gx;
    out[1] = sc * gy;
    out[2] = sc * gz;
}

int fa_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_fold_align_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

}  // namespace

size_t genie_fold_align_potential_work_bytes(int B, int N, int R) {
    return (B >= 1 && B <= 65535 && N >= FA_MIN_LEN && N <= FA_MAX_LEN && R >= 1 && R <= GENIE_FOLD_ALIGN_MAX_REFERENCES)
               ? (size_t)B * (size_t)R * ((size_t)FA_FIT + (size_t)N) * sizeof(float)
               : 0;
}

int genie_fold_align_potential(genie_stream_t stream, int B, int N, const float* x0, int R, int Nr, const float* ref, const int* lr,
                               const float* bounds, int norm, int n_iter, int n_rounds, float gap_open, int offset_stride,
                               const float* var, float* logp_out, float* grad_out, float* report_out, float* tm_out, int* n_aligned_out,
                               int* map_out, float* rot_out, float* trans_out, float* rot0_out, float* trans0_out, void* work,
                               size_t work_bytes) {
    if (B < 1 || B > 65535) return fa_refuse("B outside 1..65535");
    if (N < FA_MIN_LEN || N > FA_MAX_LEN) return fa_refuse("N outside 4..1024");
    if (Nr < FA_MIN_LEN || Nr > FA_MAX_LEN) return fa_refuse("Nr outside 4..1024");
    if ((long long)N * Nr > GENIE_TMALIGN_MAX_CELLS) return fa_refuse("N * Nr above 131072 cells");
    if (R < 1 || R > GENIE_FOLD_ALIGN_MAX_REFERENCES) return fa_refuse("R outside 1..GENIE_FOLD_ALIGN_MAX_REFERENCES (1024)");
    if (norm < 0 || norm > 3) return fa_refuse("norm outside 0..3 (query, reference, shorter, longer)");
    if (n_iter < 1 || n_iter > GENIE_TM_MAX_ITER) return fa_refuse("n_iter outside 1..32");
    if (n_rounds < 0 || n_rounds > GENIE_TMALIGN_MAX_ROUNDS) return fa_refuse("n_rounds outside 0..16");
    if (!isfinite(gap_open) || gap_open > 0.f || gap_open < -10.f) return fa_refuse("gap_open is not a finite number in -10..0");
    if (offset_stride < 1 || offset_stride > GENIE_FOLD_ALIGN_MAX_STRIDE) return fa_refuse("offset_stride outside 1..64");
    if (!x0) return fa_refuse("x0 is NULL");
    if (!ref) return fa_refuse("ref is NULL");
    if (!lr) return fa_refuse("lr is NULL");
    if (!bounds) return fa_refuse("bounds is NULL");
    if (!var) return fa_refuse("var is NULL");
    if (!logp_out && !grad_out && !report_out && !tm_out && !n_aligned_out && !map_out && !rot_out && !trans_out && !rot0_out && !trans0_out)
        return fa_refuse("no output asked for (every output pointer is NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return fa_refuse("logp_out and grad_out are given together or both NULL");
    if ((rot_out == nullptr) != (trans_out == nullptr)) return fa_refuse("rot_out and trans_out are given together or both NULL");
    if ((rot0_out == nullptr) != (trans0_out == nullptr)) return fa_refuse("rot0_out and trans0_out are given together or both NULL");
    if (!work || work_bytes < genie_fold_align_potential_work_bytes(B, N, R))
        return fa_refuse("work is NULL or work_bytes below genie_fold_align_potential_work_bytes(B, N, R)");
    if (reinterpret_cast<uintptr_t>(work) & 3) return fa_refuse("work not 4-byte aligned");
    const size_t lds = fa_lds_bytes(N < Nr ? N : Nr, N < Nr ? Nr : N);
    if (lds > 64 * 1024) return fa_refuse("the table does not fit in 64 KB of LDS");      // (no call inside MAX_CELLS reaches this)
    hipStream_t st = (hipStream_t)stream;
    float* fits = static_cast<float*>(work);                     // [B R FA_FIT] floats, then the maps [B R N] ints
    int* maps = reinterpret_cast<int*>(fits + (size_t)B * R * FA_FIT);
    hipLaunchKernelGGL(k_fold_align_fit, dim3(R, B), dim3(FA_THREADS), lds, st, N, x0, Nr, ref, lr, norm, n_iter, n_rounds, gap_open,
                       offset_stride, fits, maps, tm_out, n_aligned_out, map_out, rot_out, trans_out, rot0_out, trans0_out);
    if (logp_out || report_out)
        hipLaunchKernelGGL(k_fold_align_finish, dim3((N + FA_THREADS - 1) / FA_THREADS, B), dim3(FA_THREADS), 0, st, N, R, Nr, x0, ref,
                           bounds, var, (const float*)fits, (const int*)maps, logp_out, grad_out, report_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
