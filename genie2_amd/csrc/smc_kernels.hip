// Motif placement potential of twisted-diffusion / SMC sampling (include/genie_hip.h, genie_motif_potential): the fork's
// motif twisting function, genie/sampler/unconditional_smc.py:303-345 (genie2_amd/smc.py:58-69 is its PyTorch restatement),
// with its gradient, in one pass instead of a Python loop over placements and an autograd walk back through it.
//
// Placement p puts segment s at residues starts[p,s] .. starts[p,s] + seg_len[s] - 1; motif position m runs over the segments
// in order (what x0[:, mask] selects).  For particle b:
//   c_bp(m) = x0[b, r_p(m)] - mean_m x0[b, r_p(m)],   e_bp(m) = c_bp(m) - target[m]
//   score[b,p] = -sum_m |e_bp(m)|^2 / (2 var),   logp[b] = logsumexp_p score[b,p] - log P
//   grad[b,n]  = -sum_p w_bp [n in p] (e_bp(m_p(n)) - mean_m e_bp(m)) / var,   w_bp = softmax_p score[b,:]
// mean_m e_bp(m) = mean_m c_bp(m) - mean_m target[m] = -mean(target) for every (b, p) because c is centred; it is taken in that
// exact form (zero for a centred target, and the entry stays right for one that is not).
//
// Layout: grid (ceil(N / 64), B), 256 threads.  Every work-group of particle b scores all placements (the record (score, centroid)
// of each placement: B * P * M is about 1e5, cheap to repeat per residue tile), reduces max and sum of exp over them in a fixed tree,
// lists the placements whose weight is not exactly 0 in ascending order (scores reach -1e5 with var about 1e-2, so late in the
// trajectory that is one or a few), then gathers the gradient of its 64 residues, one per lane: each wave walks a contiguous quarter
// of the listed placements in order and the four partial sums are added in wave order.  No atomics, no scatter: every output is written once, in a fixed order, so results are
// bitwise reproducible.  Up to MP_LDS_P placements the records live in LDS (one launch); beyond that a first kernel writes them to the
// caller's `work` and the main kernel reads them from there (two launches).  `starts` is trusted (the caller validates it once when it
// builds it); it only ever indexes LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/genie_hip.h"

namespace {

constexpr int MP_THREADS = 256;
constexpr int MP_WAVES = MP_THREADS / 64;
constexpr int MP_TILE = 64;             // residues per work-group in the gather: one per lane
constexpr int MP_LDS_P = 2048;          // placement records (16 B each) kept in LDS; more spill to `work`
constexpr int MP_CHUNK = 64;            // placements per inner partial sum of the gather (two-level f32 summation)
constexpr size_t MP_LDS_MAX = 160 * 1024;

// the active-placement list holds this many entries (P itself when the records stay in LDS)
__host__ __device__ inline int mp_act_cap(int P) { return P < MP_LDS_P ? P : MP_LDS_P; }

// dynamic LDS: [rec: float4 x (SPILL ? 0 : P)] [xs: 3N] [tg: 3M] [part: WAVES*64*3] [red: 2*WAVES] [seg: 2S int] [wcnt: WAVES int]
//              [act: mp_act_cap(P) int]
size_t mp_lds_bytes(int N, int M, int S, int P, int P_lds) {
    return (size_t)P_lds * sizeof(float4) + sizeof(float) * (3 * (size_t)N + 3 * (size_t)M + MP_WAVES * 64 * 3 + 2 * MP_WAVES) +
           sizeof(int) * (2 * (size_t)S + MP_WAVES + mp_act_cap(P));
}

struct MpLds {
    float4* rec;
    float *xs, *tg, *part, *red;
    int *sl, *so, *wcnt, *act;
};

__device__ inline MpLds mp_carve(unsigned char* base, int N, int M, int S, int P_lds) {
    MpLds L;
    L.rec = reinterpret_cast<float4*>(base);
    L.xs = reinterpret_cast<float*>(L.rec + P_lds);
    L.tg = L.xs + 3 * N;
    L.part = L.tg + 3 * M;
    L.red = L.part + MP_WAVES * 64 * 3;
    L.sl = reinterpret_cast<int*>(L.red + 2 * MP_WAVES);
    L.so = L.sl + S;
    L.wcnt = L.so + S;
    L.act = L.wcnt + MP_WAVES;
    return L;
}

// x0[b], the target and the segment table into LDS (segment offsets by one thread, in order)
__device__ inline void mp_stage(const MpLds& L, const float* __restrict__ x0b, const float* __restrict__ target,
                                const int32_t* __restrict__ seg_len, int N, int M, int S) {
    for (int i = threadIdx.x; i < 3 * N; i += MP_THREADS) L.xs[i] = x0b[i];
    for (int i = threadIdx.x; i < 3 * M; i += MP_THREADS) L.tg[i] = target[i];
    if (threadIdx.x == 0) {
        int off = 0;
        for (int s = 0; s < S; ++s) {
            const int n = seg_len[s];
            L.sl[s] = n;
            L.so[s] = off;
            off += n;
        }
    }
}

// (score, centroid) of one placement: the two passes of x0[:, mask] - mean, then - target, squared and summed (smc.py:64-66)
__device__ inline float4 mp_record(const MpLds& L, const int32_t* __restrict__ st, int S, int M, float var) {
    float cx = 0.f, cy = 0.f, cz = 0.f;
    for (int s = 0; s < S; ++s) {
        const int r0 = st[s], n = L.sl[s];
        for (int i = 0; i < n; ++i) {
            const float* x = L.xs + 3 * (r0 + i);
            cx += x[0];
            cy += x[1];
            cz += x[2];
        }
    }
    cx /= (float)M;
    cy /= (float)M;
    cz /= (float)M;
    float q = 0.f;
    for (int s = 0; s < S; ++s) {
        const int r0 = st[s], n = L.sl[s], m0 = L.so[s];
        for (int i = 0; i < n; ++i) {
            const float* x = L.xs + 3 * (r0 + i);
            const float* t = L.tg + 3 * (m0 + i);
            const float ex = (x[0] - cx) - t[0], ey = (x[1] - cy) - t[1], ez = (x[2] - cz) - t[2];
            q += ex * ex + ey * ey + ez * ez;
        }
    }
    return make_float4(-q / (2.f * var), cx, cy, cz);
}

// block-wide reductions in a fixed tree: butterfly inside each wave, then the wave results in wave order (every thread gets lane 0's)
__device__ inline float mp_block_max(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < MP_WAVES; ++w) r = fmaxf(r, red[w]);
    return r;
}

__device__ inline float mp_block_sum(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[MP_WAVES + (threadIdx.x >> 6)] = v;
    __syncthreads();
    float r = red[MP_WAVES];
    for (int w = 1; w < MP_WAVES; ++w) r += red[MP_WAVES + w];
    return r;
}

// large-P path, first launch: one placement per thread, records to work[b, p]
__global__ __launch_bounds__(MP_THREADS) void k_motif_records(const float* __restrict__ x0, int N, int P, int S, int M,
                                                              const int32_t* __restrict__ seg_len, const int32_t* __restrict__ starts,
                                                              const float* __restrict__ target, const float* __restrict__ var,
                                                              float4* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    const int b = blockIdx.y;
    const MpLds L = mp_carve(mp_smem, N, M, S, 0);          // (act / wcnt unused here)
    mp_stage(L, x0 + (size_t)b * 3 * N, target, seg_len, N, M, S);
    __syncthreads();
    const int p = blockIdx.x * MP_THREADS + threadIdx.x;
    if (p < P) work[(size_t)b * P + p] = mp_record(L, starts + (size_t)p * S, S, M, *var);
}

template <bool SPILL>
__global__ __launch_bounds__(MP_THREADS) void k_motif_potential(const float* __restrict__ x0, int N, int P, int S, int M,
                                                                const int32_t* __restrict__ seg_len, const int32_t* __restrict__ starts,
                                                                const float* __restrict__ target, const float* __restrict__ var_p,
                                                                const float4* __restrict__ work, float* __restrict__ logp,
                                                                float* __restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const MpLds L = mp_carve(mp_smem, N, M, S, SPILL ? 0 : P);
    mp_stage(L, x0 + (size_t)b * 3 * N, target, seg_len, N, M, S);
    const float var = *var_p;
    __syncthreads();
    if (!SPILL)
        for (int p = tid; p < P; p += MP_THREADS) L.rec[p] = mp_record(L, starts + (size_t)p * S, S, M, var);
    const float4* rec = SPILL ? work + (size_t)b * P : L.rec;
    __syncthreads();

    // logsumexp with the max taken first: late in the trajectory scores reach -1e5 and the softmax is one-hot
    float mx = -INFINITY;
    for (int p = tid; p < P; p += MP_THREADS) mx = fmaxf(mx, rec[p].x);
    mx = mp_block_max(mx, L.red);
    float se = 0.f;
    for (int p = tid; p < P; p += MP_THREADS) se += expf(rec[p].x - mx);
    se = mp_block_sum(se, L.red);
    if (blockIdx.x == 0 && tid == 0) logp[b] = mx + logf(se) - logf((float)P);

    // -mean_m e = mean(target), the same for every placement
    float tbx = 0.f, tby = 0.f, tbz = 0.f;
    for (int m = 0; m < M; ++m) {
        tbx += L.tg[3 * m];
        tby += L.tg[3 * m + 1];
        tbz += L.tg[3 * m + 2];
    }
    tbx /= (float)M;
    tby /= (float)M;
    tbz /= (float)M;

    // the placements whose weight is not exactly 0, in ascending order (late in the trajectory that is one or a few): ballot +
    // prefix count per wave, per 256-placement chunk.  If there are more than the list holds, the gather walks every placement.
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int cap = mp_act_cap(P);
    int cnt = 0;
    for (int c0 = 0; c0 < P; c0 += MP_THREADS) {
        const int p = c0 + tid;
        const bool on = p < P && expf(rec[p].x - mx) != 0.f;
        const uint64_t bal = __ballot(on);
        if (lane == 0) L.wcnt[w] = __popcll(bal);
        __syncthreads();
        int at = cnt + __popcll(bal & ((1ull << lane) - 1));
        for (int v = 0; v < MP_WAVES; ++v) {
            if (v < w) at += L.wcnt[v];
            cnt += L.wcnt[v];
        }
        if (on && at < cap) L.act[at] = p;
        __syncthreads();
    }
    const bool listed = cnt <= cap;
    const int K = listed ? cnt : P;

    // gather: lane = residue, wave = a contiguous quarter of the (listed) placements (wave-uniform p: the starts are scalar loads)
    const int n = blockIdx.x * MP_TILE + lane;
    const bool live = n < N;
    const float xn = live ? L.xs[3 * n] : 0.f, yn = live ? L.xs[3 * n + 1] : 0.f, zn = live ? L.xs[3 * n + 2] : 0.f;
    const int k0 = (int)((int64_t)K * w / MP_WAVES), k1 = (int)((int64_t)K * (w + 1) / MP_WAVES);
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int c0 = k0; c0 < k1; c0 += MP_CHUNK) {
        const int c1 = min(c0 + MP_CHUNK, k1);
        float bx = 0.f, by = 0.f, bz = 0.f;
        for (int k = c0; k < c1; ++k) {
            const int p = __builtin_amdgcn_readfirstlane(listed ? L.act[k] : k);
            const float4 rp = rec[p];
            const float e = expf(rp.x - mx);          // bitwise the term of `se`
            if (e == 0.f) continue;                   // (wave-uniform)
            const int32_t* st = starts + (size_t)p * S;
            int m = -1;
            for (int s = 0; s < S; ++s) {
                const int d = n - st[s];
                if ((unsigned)d < (unsigned)L.sl[s]) m = L.so[s] + d;
            }
            if (m >= 0) {
                const float* t = L.tg + 3 * m;
                bx += e * (((xn - rp.y) - t[0]) + tbx);
                by += e * (((yn - rp.z) - t[1]) + tby);
                bz += e * (((zn - rp.w) - t[2]) + tbz);
            }
        }
        ax += bx;
        ay += by;
        az += bz;
    }
    float* mine = L.part + 3 * (w * 64 + lane);
    mine[0] = ax;
    mine[1] = ay;
    mine[2] = az;
    __syncthreads();
    if (w == 0 && live) {
        float gx = L.part[3 * lane], gy = L.part[3 * lane + 1], gz = L.part[3 * lane + 2];
        for (int v = 1; v < MP_WAVES; ++v) {
            const float* o = L.part + 3 * (v * 64 + lane);
            gx += o[0];
            gy += o[1];
            gz += o[2];
        }
        const float sc = -1.f / (var * se);
        float* g = grad + ((size_t)b * N + n) * 3;
        g[0] = gx * sc;
        g[1] = gy * sc;
        g[2] = gz * sc;
    }
}

}  // namespace

size_t genie_motif_potential_work_bytes(int B, int P) {
    return (B >= 1 && P > MP_LDS_P) ? (size_t)B * (size_t)P * sizeof(float4) : 0;
}

int genie_motif_potential(genie_stream_t stream, int B, int N, const float* x0, int P, int S, int M, const int32_t* seg_len,
                          const int32_t* starts, const float* target, const float* var, float* logp_out, float* grad_out, void* work,
                          size_t work_bytes) {
    if (!x0 || !seg_len || !starts || !target || !var || !logp_out || !grad_out) return GENIE_E_ARG;
    if (B < 1 || B > 65535 || N < 1 || P < 1 || S < 1 || M < 1 || M > N || S > M || (int64_t)P * S > INT32_MAX) return GENIE_E_ARG;
    const bool spill = P > MP_LDS_P;
    const size_t need = genie_motif_potential_work_bytes(B, P);
    if (spill && (!work || work_bytes < need || (reinterpret_cast<uintptr_t>(work) & 15))) return GENIE_E_ARG;
    const size_t lds = mp_lds_bytes(N, M, S, P, spill ? 0 : P);
    if (lds > MP_LDS_MAX) return GENIE_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((N + MP_TILE - 1) / MP_TILE, B);
    if (spill) {
        if (lds > 64 * 1024) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_motif_records), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_motif_potential<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds);
        }
        float4* rec = static_cast<float4*>(work);
        hipLaunchKernelGGL(k_motif_records, dim3((P + MP_THREADS - 1) / MP_THREADS, B), dim3(MP_THREADS), lds, st, x0, N, P, S, M, seg_len,
                           starts, target, var, rec);
        hipLaunchKernelGGL(k_motif_potential<true>, grid, dim3(MP_THREADS), lds, st, x0, N, P, S, M, seg_len, starts, target, var,
                           (const float4*)rec, logp_out, grad_out);
    } else {
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_motif_potential<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds);
        hipLaunchKernelGGL(k_motif_potential<false>, grid, dim3(MP_THREADS), lds, st, x0, N, P, S, M, seg_len, starts, target, var,
                           (const float4*)nullptr, logp_out, grad_out);
    }
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
