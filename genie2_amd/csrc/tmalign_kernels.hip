// Gapped TM alignment of M queries against R references (include/genie_hip.h: genie_tm_align): the novelty of a design set, and a
// diversity count that is not thrown by an inserted loop.  The score is the project's own (the header states it exactly):
// the seeded gapless search of genie_pairwise_tm (stage 0), then up to n_rounds stages of dynamic programming under the TM objective,
// each refitted over its aligned pairs.  Not a port of the TMalign program, and a lower bound of its score.  The reference has no
// counterpart.
//
// k_tm_align: grid (R, M), 256 threads, one work-group per (query, reference) pair; a = the shorter chain moves (equal lengths: the
// query), b = the longer one is fixed.  Both are staged in LDS, each centred on its own centroid.
//   stage 0    k_pairwise_tm's item loop (similarity_kernels.hip: items t = 11 o + s dealt to the four waves, butterfly sums, the
//              Jacobi solve in every lane) written again here with one addition: a wave keeps the fit (R, c_p, c_q) of its best
//              iteration, and the work-group takes the best wave's in wave order (ties: the lowest t, inside a wave the earliest
//              iteration).
//   a stage    T a (the stage's starting fit applied to a) goes to LDS.  The table is filled as an anti-diagonal wavefront, one
//              work-group barrier per diagonal: thread t owns rows t + 1 and t + 257 (La <= sqrt(MAX_CELLS) = 362), forms S_ij on the fly,
//              keeps its row's previous cell (the V operand) in registers and reads row i - 1 of the two previous diagonals (H, D) from
//              three rolling (val, path) buffers.  The moves, 2 bits a cell, live in LDS row-major, 16 cells a dword; a row has one
//              owner and a dword belongs to one row, so a thread gathers 16 moves in a register and stores the dword once: no
//              read-modify-write, no race.  Thread 0 traces back (at most La + Lb steps); all threads compare the alignment with the
//              previous stage's; wave 0 runs the n_iter ascent over the aligned pairs, the same loop as an item of stage 0.
// The best stage's alignment and fit are kept in LDS; at the end wave 0 forms the rmsd, the threads write map, thread 0 writes the
// scalars and the transform in the callers' frame.  LDS: 8 (3 (La + 1)) + 4 (9 La + 3 Lb + La ceil(Lb / 16) + 128) bytes by the padded
// sizes, 59 904 bytes at 362 x 362, the largest any call inside MAX_CELLS asks for.  No atomics, no global scratch, fixed summation
// trees: two calls on the same inputs are bitwise equal.  Only rows below a chain's length are read, so padding never reaches a result.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"
#include "horn.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int TA_THREADS = 256;
constexpr int TA_WAVES = TA_THREADS / 64;
constexpr int TA_SEEDS = GENIE_TM_SEEDS;
constexpr int TA_MIN_LEN = GENIE_TM_MIN_LENGTH;
constexpr int TA_ROWS = 2;                              // table rows per thread: La <= 362 < TA_ROWS * TA_THREADS
constexpr int TA_FIT = 16;                              // floats of a stored fit: R (9), c_p (3), c_q (3), the score
constexpr int TA_MISC = 128;                            // floats: part (16), best (8), fits (6 x 16), the traceback's count
constexpr int TA_CUR = 4, TA_BEST = 5;                  // fit slots after the four waves': the stage's starting fit, the best stage's
static_assert((long long)(TA_ROWS * TA_THREADS) * (TA_ROWS * TA_THREADS) > GENIE_TMALIGN_MAX_CELLS, "a thread owns TA_ROWS rows");

struct TaFit {
    MrMat R;
    float cpx, cpy, cpz, cqx, cqy, cqz;
};

// dynamic LDS for chains padded to Na <= Nb: [dp: 3 x (Na + 1) float2] [a: 3 Na] [T a: 3 Na] [aln cur, prev, best: 3 Na] [b: 3 Nb]
// [misc: 128] [moves: Na ceil(Nb / 16)]
size_t ta_lds_bytes(int Na, int Nb) {
    return sizeof(float) * (6 * ((size_t)Na + 1) + 9 * (size_t)Na + 3 * (size_t)Nb + TA_MISC + (size_t)Na * ((Nb + 15) / 16));
}

__device__ inline float ta_wave_sum(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

__device__ inline float ta_d0(int L) { return L > 15 ? fmaxf(0.5f, 1.24f * cbrtf((float)(L - 15)) - 1.8f) : 0.5f; }

__device__ inline void ta_window(int s, int La, int& start, int& len) {
    if (s == 0) {
        start = 0;
        len = La;
        return;
    }
    const int k = s < 4 ? 1 : 2, j = s < 4 ? s - 1 : s - 4, n = s < 4 ? 3 : 7;
    len = max((La + (1 << k) - 1) >> k, TA_MIN_LEN);
    start = j * (La - len) / (n - 1);
}

// stages rows 0..L-1 of src in dst, centred on their centroid, which every thread returns (a fixed tree, as in similarity_kernels.hip)
__device__ inline float3 ta_stage(const float* __restrict__ src, int L, float* dst, float* part) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int n = tid; n < L; n += TA_THREADS) {
        const float x = src[3 * n], y = src[3 * n + 1], z = src[3 * n + 2];
        dst[3 * n] = x;
        dst[3 * n + 1] = y;
        dst[3 * n + 2] = z;
        sx += x;
        sy += y;
        sz += z;
    }
    sx = ta_wave_sum(sx);
    sy = ta_wave_sum(sy);
    sz = ta_wave_sum(sz);
    if (lane == 0) {
        part[3 * w] = sx;
        part[3 * w + 1] = sy;
        part[3 * w + 2] = sz;
    }
    __syncthreads();
    float cx = part[0], cy = part[1], cz = part[2];
    for (int u = 1; u < TA_WAVES; ++u) {
        cx += part[3 * u];
        cy += part[3 * u + 1];
        cz += part[3 * u + 2];
    }
    cx /= (float)L;
    cy /= (float)L;
    cz /= (float)L;
    for (int n = tid; n < L; n += TA_THREADS) {
        dst[3 * n] -= cx;
        dst[3 * n + 1] -= cy;
        dst[3 * n + 2] -= cz;
    }
    __syncthreads();
    return make_float3(cx, cy, cz);
}

// One ascent by one wave over the pairs (a_n, b_{idx(n)}): the threading idx(n) = o + n seeded by the window [ws, ws + wl) (GAPPED
// false), or the alignment idx(n) = aln[n], residues with aln[n] < 0 left out, seeded by all wl aligned pairs (GAPPED true).  The
// arithmetic is k_pairwise_tm's.  Where an iteration's score exceeds `best` (strictly: the earliest of equal ones stays), best takes
// it and lane 0 stores that iteration's fit in the wave's LDS slot `fit` (fits are kept out of the registers: the Jacobi solve needs
// them); returns whether one did.
template <bool GAPPED>
__device__ inline bool ta_ascent(const float* as, const float* bs, const int* aln, int o, int La, int ws, int wl, int n_iter,
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
    for (int k = 0; k < 6; ++k) c[k] = ta_wave_sum(c[k]) / (float)wl;
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
    for (int k = 7; k < 16; ++k) a[k] = ta_wave_sum(a[k]);
    MrMat R = mr_rotation(mr_quaternion(MrMat{a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15]}));

    bool improved = false;
    for (int it = 0; it < n_iter; ++it) {
        float sc = 0.f;
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
        const float score = ta_wave_sum(sc) / (float)lnorm;
        if (score > best) {
            best = score;
            if (lane == 0) {
                fit[0] = R.xx, fit[1] = R.xy, fit[2] = R.xz, fit[3] = R.yx, fit[4] = R.yy, fit[5] = R.yz, fit[6] = R.zx, fit[7] = R.zy, fit[8] = R.zz;
                fit[9] = cpx, fit[10] = cpy, fit[11] = cpz, fit[12] = cqx, fit[13] = cqy, fit[14] = cqz;
            }
            improved = true;
        }
        if (it + 1 == n_iter) break;
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = ta_wave_sum(a[k]);
        const float sw = a[0] > 0.f ? a[0] : 1.f;
        const float mpx = a[1] / sw, mpy = a[2] / sw, mpz = a[3] / sw, mqx = a[4] / sw, mqy = a[5] / sw, mqz = a[6] / sw;
        R = mr_rotation(mr_quaternion(MrMat{a[7] - a[1] * mqx, a[8] - a[1] * mqy, a[9] - a[1] * mqz, a[10] - a[2] * mqx,
                                            a[11] - a[2] * mqy, a[12] - a[2] * mqz, a[13] - a[3] * mqx, a[14] - a[3] * mqy,
                                            a[15] - a[3] * mqz}));
        cpx += mpx;
        cpy += mpy;
        cpz += mpz;
        cqx += mqx;
        cqy += mqy;
        cqz += mqz;
    }
    return improved;
}

__device__ inline TaFit ta_get_fit(const float* src) {
    TaFit f;
    f.R = MrMat{src[0], src[1], src[2], src[3], src[4], src[5], src[6], src[7], src[8]};
    f.cpx = src[9];
    f.cpy = src[10];
    f.cpz = src[11];
    f.cqx = src[12];
    f.cqy = src[13];
    f.cqz = src[14];
    return f;
}

__global__ __launch_bounds__(TA_THREADS) void k_tm_align(int Nq, const float* __restrict__ xq, const int* __restrict__ lq, int Nr,
                                                         const float* __restrict__ xr, const int* __restrict__ lr, int norm, int n_iter,
                                                         int n_rounds, float gap_open, float* __restrict__ tm, float* __restrict__ rmsd,
                                                         int* __restrict__ n_aligned, int* __restrict__ rounds, int* __restrict__ map,
                                                         float* __restrict__ rot, float* __restrict__ trans) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ta_smem[];
    const int r = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
    const int R_ = gridDim.x;
    const int Na = min(Nq, Nr), Nb = max(Nq, Nr);

    // lengths index LDS and global memory: clamped into 4..N whatever the arrays hold
    const int Lq = min(max(lq[m], TA_MIN_LEN), Nq), Lr = min(max(lr[r], TA_MIN_LEN), Nr);
    const bool swap = Lr < Lq;                                   // the shorter chain moves; equal lengths: the query
    const int La = swap ? Lr : Lq, Lb = swap ? Lq : Lr;          // La <= Na, Lb <= Nb
    const float* pa = swap ? xr + (size_t)r * 3 * Nr : xq + (size_t)m * 3 * Nq;
    const float* pb = swap ? xq + (size_t)m * 3 * Nq : xr + (size_t)r * 3 * Nr;

    float2* dp = reinterpret_cast<float2*>(ta_smem);             // three diagonals of (val, path), row i at [i], i = 0..La
    float* as = reinterpret_cast<float*>(dp + 3 * ((size_t)Na + 1));
    float* ta = as + 3 * (size_t)Na;
    int* alnC = reinterpret_cast<int*>(ta + 3 * (size_t)Na);
    int* alnP = alnC + Na;
    int* alnB = alnP + Na;
    float* bs = reinterpret_cast<float*>(alnB + Na);
    float* part = bs + 3 * (size_t)Nb;
    float* best = part + 16;
    float* fits = best + 8;
    int* count = reinterpret_cast<int*>(fits + 6 * TA_FIT);
    unsigned* moves = reinterpret_cast<unsigned*>(part + TA_MISC);
    const int W = (Lb + 15) >> 4;                                // dwords of a row of moves

    const float3 ca = ta_stage(pa, La, as, part);
    const float3 cb = ta_stage(pb, Lb, bs, part);

    const int lnorm = norm == 0 ? Lq : norm == 1 ? Lr : norm == 2 ? La : Lb;
    const float d0 = ta_d0(lnorm), inv_d0sq = 1.f / (d0 * d0);
    const int n_off = Lb - La + 1, n_items = n_off * TA_SEEDS;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;

    // ---- stage 0: the seeded gapless search ----
    float v_wave = -1.f;
    int t_wave = INT_MAX;
    if (lane < TA_FIT) fits[w * TA_FIT + lane] = lane == 0 || lane == 4 || lane == 8 ? 1.f : 0.f;      // (the identity, should no score compare)
    for (int t = w; t < n_items; t += TA_WAVES) {
        const int o = t / TA_SEEDS, s = t - o * TA_SEEDS;
        int ws, wl;
        ta_window(s, La, ws, wl);
        if (ta_ascent<false>(as, bs, nullptr, o, La, ws, wl, n_iter, inv_d0sq, lnorm, lane, v_wave, fits + w * TA_FIT)) t_wave = t;
    }
    if (lane == 0) {
        best[2 * w] = v_wave;
        best[2 * w + 1] = __int_as_float(t_wave);
    }
    __syncthreads();
    float v_best = best[0];
    int t0 = __float_as_int(best[1]), w0 = 0;
    for (int u = 1; u < TA_WAVES; ++u) {
        const float vu = best[2 * u];
        const int tu = __float_as_int(best[2 * u + 1]);
        if (vu > v_best || (vu == v_best && tu < t0)) {
            v_best = vu;
            t0 = tu;
            w0 = u;
        }
    }
    const int o0 = min(max(t0 / TA_SEEDS, 0), n_off - 1);        // (indexes LDS; a score that is NaN everywhere leaves t unset)
    if (tid < TA_FIT) fits[TA_CUR * TA_FIT + tid] = fits[TA_BEST * TA_FIT + tid] = fits[w0 * TA_FIT + tid];
    int cnt_best = La, n_fills = 0;
    for (int n = tid; n < La; n += TA_THREADS) alnP[n] = alnB[n] = o0 + n;
    for (int k = tid; k < 3; k += TA_THREADS) dp[k * ((size_t)La + 1)] = make_float2(0.f, 0.f);      // row 0 of every diagonal
    __syncthreads();

    // ---- stages 1..n_rounds: fill, trace back, refit ----
    for (int stage = 1; stage <= n_rounds; ++stage) {
        const TaFit f_cur = ta_get_fit(fits + TA_CUR * TA_FIT);
        for (int n = tid; n < La; n += TA_THREADS) {
            const float px = as[3 * n] - f_cur.cpx, py = as[3 * n + 1] - f_cur.cpy, pz = as[3 * n + 2] - f_cur.cpz;
            ta[3 * n] = (f_cur.R.xx * px + f_cur.R.xy * py + f_cur.R.xz * pz) + f_cur.cqx;
            ta[3 * n + 1] = (f_cur.R.yx * px + f_cur.R.yy * py + f_cur.R.yz * pz) + f_cur.cqy;
            ta[3 * n + 2] = (f_cur.R.zx * px + f_cur.R.zy * py + f_cur.R.zz * pz) + f_cur.cqz;
            alnC[n] = -1;
        }
        __syncthreads();

        float tx[TA_ROWS], ty[TA_ROWS], tz[TA_ROWS], vl[TA_ROWS], pl[TA_ROWS];
        unsigned acc[TA_ROWS];
#pragma unroll
        for (int k = 0; k < TA_ROWS; ++k) {
            const int i = tid + 1 + k * TA_THREADS;
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
            for (int k = 0; k < TA_ROWS; ++k) {
                const int i = tid + 1 + k * TA_THREADS, j = d - i;
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
        ++n_fills;
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
        for (int n = tid; n < La; n += TA_THREADS) differs |= alnC[n] != alnP[n];
        const int cnt = *count;
        if (!__syncthreads_or(differs)) break;                   // the alignment did not move: counted, not fitted
        if (cnt < 3) break;
        if (w == 0) {
            float v = -1.f;
            ta_ascent<true>(as, bs, alnC, 0, La, 0, cnt, n_iter, inv_d0sq, lnorm, lane, v, fits);
            if (lane == 0) fits[15] = v;
        }
        __syncthreads();
        const float v = fits[15];
        const bool better = v > v_best;                          // (strictly: the earliest of equal stages stays)
        if (better) {
            v_best = v;
            cnt_best = cnt;
        }
        if (tid < TA_FIT - 1) {
            const float f = fits[tid];
            fits[TA_CUR * TA_FIT + tid] = f;
            if (better) fits[TA_BEST * TA_FIT + tid] = f;
        }
        for (int n = tid; n < La; n += TA_THREADS) {
            const int c = alnC[n];
            alnP[n] = c;
            if (better) alnB[n] = c;
        }
        __syncthreads();
    }

    // ---- the result ----
    const size_t pair = (size_t)m * R_ + r;
    if (w == 0) {
        const TaFit f_best = ta_get_fit(fits + TA_BEST * TA_FIT);
        float sd = 0.f;
        for (int n = lane; n < La; n += 64) {
            const int j = alnB[n];
            if (j < 0) continue;
            const float px = as[3 * n] - f_best.cpx, py = as[3 * n + 1] - f_best.cpy, pz = as[3 * n + 2] - f_best.cpz;
            const float qx = bs[3 * j] - f_best.cqx, qy = bs[3 * j + 1] - f_best.cqy, qz = bs[3 * j + 2] - f_best.cqz;
            const float ex = (f_best.R.xx * px + f_best.R.xy * py + f_best.R.xz * pz) - qx;
            const float ey = (f_best.R.yx * px + f_best.R.yy * py + f_best.R.yz * pz) - qy;
            const float ez = (f_best.R.zx * px + f_best.R.zy * py + f_best.R.zz * pz) - qz;
            sd += ex * ex + ey * ey + ez * ez;
        }
        sd = ta_wave_sum(sd);
        if (lane == 0) {
            tm[pair] = v_best;
            rmsd[pair] = sqrtf(sd / (float)cnt_best);
            n_aligned[pair] = cnt_best;
            rounds[pair] = n_fills;
            if (rot) {
                // b' ~ R (a' - c_p) + c_q in the centred frames: b ~ R a + t with t = cb + c_q - R (ca + c_p)
                const MrMat& R = f_best.R;
                const float ux = ca.x + f_best.cpx, uy = ca.y + f_best.cpy, uz = ca.z + f_best.cpz;
                const float tx = cb.x + f_best.cqx - (R.xx * ux + R.xy * uy + R.xz * uz);
                const float ty = cb.y + f_best.cqy - (R.yx * ux + R.yy * uy + R.yz * uz);
                const float tz = cb.z + f_best.cqz - (R.zx * ux + R.zy * uy + R.zz * uz);
                float* ro = rot + 9 * pair;
                float* to = trans + 3 * pair;
                if (!swap) {
                    ro[0] = R.xx, ro[1] = R.xy, ro[2] = R.xz, ro[3] = R.yx, ro[4] = R.yy, ro[5] = R.yz, ro[6] = R.zx, ro[7] = R.zy, ro[8] = R.zz;
                    to[0] = tx, to[1] = ty, to[2] = tz;
                } else {                                          // the reference moved: query = R ref + t, so ref = R^T (query - t)
                    ro[0] = R.xx, ro[1] = R.yx, ro[2] = R.zx, ro[3] = R.xy, ro[4] = R.yy, ro[5] = R.zy, ro[6] = R.xz, ro[7] = R.yz, ro[8] = R.zz;
                    to[0] = -(R.xx * tx + R.yx * ty + R.zx * tz);
                    to[1] = -(R.xy * tx + R.yy * ty + R.zy * tz);
                    to[2] = -(R.xz * tx + R.yz * ty + R.zz * tz);
                }
            }
        }
    }
    if (!map) return;
    int* mo = map + pair * (size_t)Nq;
    if (!swap) {
        for (int n = tid; n < Nq; n += TA_THREADS) mo[n] = n < La ? alnB[n] : -1;
        return;
    }
    // the reference moved: invert the alignment in LDS (b's coordinates are no longer needed), then write it in order
    __syncthreads();
    int* inv = reinterpret_cast<int*>(bs);                       // Nq <= Nb ints fit in b's 3 Nb floats
    for (int n = tid; n < Nq; n += TA_THREADS) inv[n] = -1;
    __syncthreads();
    for (int n = tid; n < La; n += TA_THREADS) {
        const int j = alnB[n];
        if (j >= 0) inv[j] = n;
    }
    __syncthreads();
    for (int n = tid; n < Nq; n += TA_THREADS) mo[n] = inv[n];
}

int ta_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_tm_align: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

}  // namespace

int genie_tm_align(genie_stream_t stream, int M, int Nq, const float* xq, const int* lq, int R, int Nr, const float* xr, const int* lr,
                   int norm, int n_iter, int n_rounds, float gap_open, float* tm, float* rmsd, int* n_aligned, int* rounds, int* map,
                   float* rot, float* trans) {
    if (M < 1 || M > 65535) return ta_refuse("M outside 1..65535");
    if (R < 1 || R > 65535) return ta_refuse("R outside 1..65535");
    if (Nq < TA_MIN_LEN || Nq > GENIE_TMALIGN_MAX_LENGTH) return ta_refuse("Nq outside 4..1024");
    if (Nr < TA_MIN_LEN || Nr > GENIE_TMALIGN_MAX_LENGTH) return ta_refuse("Nr outside 4..1024");
    if ((long long)Nq * Nr > GENIE_TMALIGN_MAX_CELLS) return ta_refuse("Nq * Nr above 131072 cells");
    if (norm < 0 || norm > 3) return ta_refuse("norm outside 0..3 (query, reference, shorter, longer)");
    if (n_iter < 1 || n_iter > GENIE_TM_MAX_ITER) return ta_refuse("n_iter outside 1..32");
    if (n_rounds < 0 || n_rounds > GENIE_TMALIGN_MAX_ROUNDS) return ta_refuse("n_rounds outside 0..16");
    if (!isfinite(gap_open) || gap_open > 0.f || gap_open < -10.f) return ta_refuse("gap_open is not a finite number in -10..0");
    if (!xq) return ta_refuse("xq is NULL");
    if (!lq) return ta_refuse("lq is NULL");
    if (!xr) return ta_refuse("xr is NULL");
    if (!lr) return ta_refuse("lr is NULL");
    if (!tm) return ta_refuse("tm is NULL");
    if (!rmsd) return ta_refuse("rmsd is NULL");
    if (!n_aligned) return ta_refuse("n_aligned is NULL");
    if (!rounds) return ta_refuse("rounds is NULL");
    if ((rot == nullptr) != (trans == nullptr)) return ta_refuse("rot and trans are given together or not at all");
    const size_t lds = ta_lds_bytes(Nq < Nr ? Nq : Nr, Nq < Nr ? Nr : Nq);
    if (lds > 64 * 1024) return ta_refuse("the table does not fit in 64 KB of LDS");      // (no call inside MAX_CELLS reaches this)
    hipLaunchKernelGGL(k_tm_align, dim3(R, M), dim3(TA_THREADS), lds, (hipStream_t)stream, Nq, xq, lq, Nr, xr, lr, norm, n_iter, n_rounds,
                       gap_open, tm, rmsd, n_aligned, rounds, map, rot, trans);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
