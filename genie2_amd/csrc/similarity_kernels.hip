// All-pairs TM-score of a design set (include/genie_hip.h: genie_pairwise_tm): how many of the backbones a sampler wrote are different.
// The score is the project's own gapless, seeded form of the TM objective (the header states it exactly), not a port of
// the TMscore or TMalign programs, and a lower bound of theirs.  The reference has no counterpart.
//
// For designs i < j the shorter one moves (a, La residues; equal lengths: the lower index) and the longer one is fixed (b, Lb).  A work
// item is one (offset o, seed s): a_n corresponds to b_{o+n}, the seed is one of 11 windows over a.  From the window's plain
// superposition the item runs n_iter steps of
//   R, c_p, c_q = the weighted fit (Horn's quaternion of sum w p q^T of the centred chains, horn.h)
//   d_n^2 = |R (a_n - c_p) - (b_{o+n} - c_q)|^2 for all La residues,  score = (1 / Lnorm) sum_n 1 / (1 + d_n^2 / d0^2)
//   w_n = (1 / (1 + d_n^2 / d0^2))^2
// and keeps the largest score; tm is the largest over the items, ties to the lowest (o, s); rmsd is sqrt(mean d_n^2) of seed 0's first
// step at the winning offset, which is the plain fit of all aligned residues.
//
// k_pairwise_tm: grid (M, M), 256 threads.  Block (j, i) with i > j returns at once, i == j writes (1, 0, 0).  For i < j the block
// stages both chains in LDS, each centred on its own centroid (12 (La + Lb) bytes of the 28 N + 96 the launch asks for), and deals the
// items t = 11 o + s to its four waves, wave w taking t = w, w + 4, ...  Inside an item the lanes stride over the residues; one pass
// forms d_n^2 under the current fit, the score, and the 16 weighted sums of the next fit (sum w, sum w p', sum w q', sum w p' q'^T),
// with p' and q' taken about the current fit's centroids: as the ascent settles the centroids stop moving and the correction
// sum w p' (sum w q')^T / sum w of the one-pass correlation goes to zero instead of cancelling digits.  (The window fit that starts an
// item takes its centroids in a pass of their own for the same reason.)  The sums are butterflies inside the wave, so every lane holds
// the same bits and every lane runs the Jacobi solve: nothing diverges, nothing is broadcast.  Each wave keeps its best (score, t) and
// writes seed 0's rmsd of its offsets to LDS; thread 0 takes the best of the four in wave order and writes [i, j] and [j, i].  No
// atomics, no scratch buffer, fixed summation trees: two calls on the same inputs are bitwise equal, and the matrices are exactly
// symmetric.  Only rows below a design's length are read, so padding never reaches the result.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"
#include "horn.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int TM_THREADS = 256;
constexpr int TM_WAVES = TM_THREADS / 64;
constexpr int TM_SEEDS = GENIE_TM_SEEDS;
constexpr int TM_MIN_LEN = GENIE_TM_MIN_LENGTH;
constexpr int TM_MAX_LEN = GENIE_TM_MAX_LENGTH;

// dynamic LDS: [a: 3 N] [b: 3 N] [rmsd of seed 0 per offset: N] [part: 4 WAVES] [best: 2 WAVES]
size_t tm_lds_bytes(int N) { return sizeof(float) * (7 * (size_t)N + 6 * TM_WAVES); }

__device__ inline float tm_wave_sum(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// d0 of the TM-score for a normalising length L
__device__ inline float tm_d0(int L) { return L > 15 ? fmaxf(0.5f, 1.24f * cbrtf((float)(L - 15)) - 1.8f) : 0.5f; }

// seed s of a chain of La residues: (start, length) of its window
__device__ inline void tm_window(int s, int La, int& start, int& len) {
    if (s == 0) {
        start = 0;
        len = La;
        return;
    }
    const int k = s < 4 ? 1 : 2, j = s < 4 ? s - 1 : s - 4, n = s < 4 ? 3 : 7;
    len = max((La + (1 << k) - 1) >> k, TM_MIN_LEN);
    start = j * (La - len) / (n - 1);
}

// stages rows 0..L-1 of src in dst, centred on their centroid (a fixed tree: per-thread strided sums, butterfly, waves in order)
__device__ inline void tm_stage(const float* __restrict__ src, int L, float* dst, float* part) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int n = tid; n < L; n += TM_THREADS) {
        const float x = src[3 * n], y = src[3 * n + 1], z = src[3 * n + 2];
        dst[3 * n] = x;
        dst[3 * n + 1] = y;
        dst[3 * n + 2] = z;
        sx += x;
        sy += y;
        sz += z;
    }
    sx = tm_wave_sum(sx);
    sy = tm_wave_sum(sy);
    sz = tm_wave_sum(sz);
    if (lane == 0) {
        part[3 * w] = sx;
        part[3 * w + 1] = sy;
        part[3 * w + 2] = sz;
    }
    __syncthreads();
    float cx = part[0], cy = part[1], cz = part[2];
    for (int u = 1; u < TM_WAVES; ++u) {
        cx += part[3 * u];
        cy += part[3 * u + 1];
        cz += part[3 * u + 2];
    }
    cx /= (float)L;
    cy /= (float)L;
    cz /= (float)L;
    for (int n = tid; n < L; n += TM_THREADS) {                   // (each thread centres the rows it wrote)
        dst[3 * n] -= cx;
        dst[3 * n + 1] -= cy;
        dst[3 * n + 2] -= cz;
    }
    __syncthreads();                                             // (`part` is free again, dst is complete)
}

__global__ __launch_bounds__(TM_THREADS) void k_pairwise_tm(int M, int N, const float* __restrict__ x, const int* __restrict__ length,
                                                            int norm, int n_iter, float* __restrict__ tm, float* __restrict__ rmsd,
                                                            int* __restrict__ offset) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tm_smem[];
    const int j = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    if (i > j) return;
    if (i == j) {
        if (tid == 0) {
            tm[(size_t)i * M + i] = 1.f;
            rmsd[(size_t)i * M + i] = 0.f;
            offset[(size_t)i * M + i] = 0;
        }
        return;
    }
    float* as = reinterpret_cast<float*>(tm_smem);
    float* bs = as + 3 * (size_t)N;
    float* rms = bs + 3 * (size_t)N;
    float* part = rms + N;
    float* best = part + 4 * TM_WAVES;

    // lengths index LDS and global memory: clamped into 4..N whatever the array holds
    const int li = min(max(length[i], TM_MIN_LEN), N), lj = min(max(length[j], TM_MIN_LEN), N);
    const bool swap = lj < li;                                   // the shorter chain moves; equal lengths: the lower index
    const int ia = swap ? j : i, ib = swap ? i : j, La = swap ? lj : li, Lb = swap ? li : lj;
    tm_stage(x + (size_t)ia * 3 * N, La, as, part);
    tm_stage(x + (size_t)ib * 3 * N, Lb, bs, part);

    const int lnorm = norm == 0 ? La : Lb;
    const float d0 = tm_d0(lnorm), inv_d0sq = 1.f / (d0 * d0);
    const int n_off = Lb - La + 1, n_items = n_off * TM_SEEDS;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    float best_tm = -1.f;
    int best_t = INT_MAX;

    for (int t = w; t < n_items; t += TM_WAVES) {
        const int o = t / TM_SEEDS, s = t - o * TM_SEEDS;
        const float* qs = bs + 3 * (size_t)o;
        int ws, wl;
        tm_window(s, La, ws, wl);

        // the window's centroids
        float c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int n = ws + lane; n < ws + wl; n += 64) {
            c[0] += as[3 * n];
            c[1] += as[3 * n + 1];
            c[2] += as[3 * n + 2];
            c[3] += qs[3 * n];
            c[4] += qs[3 * n + 1];
            c[5] += qs[3 * n + 2];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = tm_wave_sum(c[k]) / (float)wl;
        float cpx = c[0], cpy = c[1], cpz = c[2], cqx = c[3], cqy = c[4], cqz = c[5];

        // the window's correlation about them, and its fit
        float a[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = 0.f;
        for (int n = ws + lane; n < ws + wl; n += 64) {
            const float px = as[3 * n] - cpx, py = as[3 * n + 1] - cpy, pz = as[3 * n + 2] - cpz;
            const float qx = qs[3 * n] - cqx, qy = qs[3 * n + 1] - cqy, qz = qs[3 * n + 2] - cqz;
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
        for (int k = 7; k < 16; ++k) a[k] = tm_wave_sum(a[k]);
        MrMat R = mr_rotation(mr_quaternion(MrMat{a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15]}));

        for (int it = 0; it < n_iter; ++it) {
            // one pass: the distances under (R, c_p, c_q), the score, and the weighted sums of the next fit about (c_p, c_q)
            float sc = 0.f, sd = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) a[k] = 0.f;
            for (int n = lane; n < La; n += 64) {
                const float px = as[3 * n] - cpx, py = as[3 * n + 1] - cpy, pz = as[3 * n + 2] - cpz;
                const float qx = qs[3 * n] - cqx, qy = qs[3 * n + 1] - cqy, qz = qs[3 * n + 2] - cqz;
                const float ex = (R.xx * px + R.xy * py + R.xz * pz) - qx;
                const float ey = (R.yx * px + R.yy * py + R.yz * pz) - qy;
                const float ez = (R.zx * px + R.zy * py + R.zz * pz) - qz;
                const float d2 = ex * ex + ey * ey + ez * ez;
                const float g = 1.f / (1.f + d2 * inv_d0sq), wt = g * g;
                sc += g;
                sd += d2;
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
            const float score = tm_wave_sum(sc) / (float)lnorm;    // (divided: identical chains score exactly 1)
            if (s == 0 && it == 0) {                             // (wave-uniform)
                sd = tm_wave_sum(sd);
                if (lane == 0) rms[o] = sqrtf(sd / (float)La);
            }
            if (score > best_tm) {                               // (strictly: the lowest t of equal scores stays)
                best_tm = score;
                best_t = t;
            }
            if (it + 1 == n_iter) break;
#pragma unroll
            for (int k = 0; k < 16; ++k) a[k] = tm_wave_sum(a[k]);
            const float sw = a[0] > 0.f ? a[0] : 1.f;            // (every weight underflowed: the fit stays put)
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
    }

    if (lane == 0) {
        best[2 * w] = best_tm;
        best[2 * w + 1] = __int_as_float(best_t);
    }
    __syncthreads();
    if (tid != 0) return;
    float v = best[0];
    int t = __float_as_int(best[1]);
    for (int u = 1; u < TM_WAVES; ++u) {
        const float vu = best[2 * u];
        const int tu = __float_as_int(best[2 * u + 1]);
        if (vu > v || (vu == v && tu < t)) {
            v = vu;
            t = tu;
        }
    }
    const int o = min(max(t / TM_SEEDS, 0), n_off - 1);          // (indexes LDS; a score that is NaN everywhere leaves t unset)
    const float r = rms[o];
    tm[(size_t)i * M + j] = v;
    tm[(size_t)j * M + i] = v;
    rmsd[(size_t)i * M + j] = r;
    rmsd[(size_t)j * M + i] = r;
    offset[(size_t)i * M + j] = o;
    offset[(size_t)j * M + i] = o;
}

int tm_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_pairwise_tm: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

}  // namespace

int genie_pairwise_tm(genie_stream_t stream, int M, int N, const float* x, const int* length, int norm, int n_iter, float* tm,
                      float* rmsd, int* offset) {
    if (M < 1 || M > 65535) return tm_refuse("M outside 1..65535");
    if (N < TM_MIN_LEN || N > TM_MAX_LEN) return tm_refuse("N outside 4..1706");
    if (n_iter < 1 || n_iter > GENIE_TM_MAX_ITER) return tm_refuse("n_iter outside 1..32");
    if (norm != 0 && norm != 1) return tm_refuse("norm is neither 0 (shorter) nor 1 (longer)");
    if (!x) return tm_refuse("x is NULL");
    if (!length) return tm_refuse("length is NULL");
    if (!tm) return tm_refuse("tm is NULL");
    if (!rmsd) return tm_refuse("rmsd is NULL");
    if (!offset) return tm_refuse("offset is NULL");
    hipLaunchKernelGGL(k_pairwise_tm, dim3(M, M), dim3(TM_THREADS), tm_lds_bytes(N), (hipStream_t)stream, M, N, x, length, norm, n_iter,
                       tm, rmsd, offset);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
