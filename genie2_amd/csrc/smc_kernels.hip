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
// builds it); it only ever indexes LDS.  Two more forms follow, each with its own section below: the superposed one
// (genie_motif_potential_rigid) and the group-wise one for multi-motif problems (genie_motif_potential_grouped).
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

// ---- the superposed (rigid) form: genie_motif_potential_rigid ---------------------------------------------------------------------
// Every placement is compared to the motif in its best-fitting orientation.  With t_c = target - mean(target):
//   R_bp = argmin over proper rotations of sum_m |c_bp(m) - R t_c(m)|^2,   e_bp(m) = c_bp(m) - R_bp t_c(m),   q_bp = sum_m |e_bp(m)|^2
//   score[b,p] = -q_bp / (2 var),   logp[b] = logsumexp_p score[b,p] - log P,   grad[b,n] = -sum_p w_bp [n in p] e_bp(m_p(n)) / var
// (the derivative through R vanishes at the optimum, and sum_m e = 0 because both sides are centred), best[b] = the lowest p with the
// largest score, rmsd[b] = sqrt(q_{b,best} / M).  R is Horn's quaternion: the eigenvector of the largest eigenvalue of the symmetric
// 4x4 matrix built from the correlation sum_m t_c c^T, found by MR_SWEEPS cyclic Jacobi sweeps in float32 with the matrix and the
// eigenvectors in named registers (a quaternion is always a proper rotation: a mirror image does not fit).  q is then summed from the
// residuals with R applied, never as G_x + G_t - 2 lambda, which cancels to nothing exactly when the fit is good.  A collinear
// selection has a double largest eigenvalue: Jacobi still returns one unit eigenvector of it, the score is the same for all of them.
//
// Layout as above with a record (q, centroid, quaternion) of 32 B per placement, MR_LDS_P of them in LDS; the gather rebuilds R from
// the quaternion (wave-uniform).  Without a gradient to write, one work-group per particle does the scoring and the gather is skipped.
constexpr int MR_LDS_P = 1024;          // placement records (32 B each) kept in LDS; more spill to `work`
constexpr int MR_SWEEPS = 6;            // cyclic Jacobi sweeps of the 4x4 (quadratic convergence: 4 reach float32 on these matrices)

// one Jacobi rotation in the (p, q) plane: a_pq -> 0.  (a1p, a1q), (a2p, a2q): the two other rows' entries in columns p and q;
// v*p, v*q: columns p and q of the eigenvector matrix.  (The fit is plain arithmetic, __host__ too: it can be run on the CPU
// against a float64 fit.)
__host__ __device__ __forceinline__ void mr_mix(float& x, float& y, float s, float tau) {
    const float g = x, h = y;
    x = g - s * (h + tau * g);
    y = h + s * (g - tau * h);
}

__host__ __device__ __forceinline__ void mr_rot(float& app, float& aqq, float& apq, float& a1p, float& a1q, float& a2p, float& a2q,
                                                float& v0p, float& v0q, float& v1p, float& v1q, float& v2p, float& v2q, float& v3p,
                                                float& v3q) {
    const float th = (aqq - app) / (2.f * apq);
    float t = copysignf(1.f, th) / (fabsf(th) + sqrtf(th * th + 1.f));      // (th = +-inf gives 0)
    t = apq == 0.f ? 0.f : t;                                               // (and th = 0/0 is never used)
    const float c = 1.f / sqrtf(t * t + 1.f), s = t * c, tau = s / (1.f + c), h = t * apq;
    app -= h;
    aqq += h;
    apq = 0.f;
    mr_mix(a1p, a1q, s, tau);
    mr_mix(a2p, a2q, s, tau);
    mr_mix(v0p, v0q, s, tau);
    mr_mix(v1p, v1q, s, tau);
    mr_mix(v2p, v2q, s, tau);
    mr_mix(v3p, v3q, s, tau);
}

// Horn (1987): the unit quaternion (w, x, y, z) of the proper rotation R that maximises sum_m (R t(m)) . c(m), from S_ab = sum_m t_a c_b
__host__ __device__ __forceinline__ float4 mr_quaternion(float Sxx, float Sxy, float Sxz, float Syx, float Syy, float Syz, float Szx,
                                                         float Szy, float Szz) {
    float a00 = Sxx + Syy + Szz, a01 = Syz - Szy, a02 = Szx - Sxz, a03 = Sxy - Syx;
    float a11 = Sxx - Syy - Szz, a12 = Sxy + Syx, a13 = Szx + Sxz;
    float a22 = -Sxx + Syy - Szz, a23 = Syz + Szy;
    float a33 = -Sxx - Syy + Szz;
    float v00 = 1.f, v01 = 0.f, v02 = 0.f, v03 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v13 = 0.f;
    float v20 = 0.f, v21 = 0.f, v22 = 1.f, v23 = 0.f, v30 = 0.f, v31 = 0.f, v32 = 0.f, v33 = 1.f;
#pragma unroll
    for (int sweep = 0; sweep < MR_SWEEPS; ++sweep) {
        mr_rot(a00, a11, a01, a02, a12, a03, a13, v00, v01, v10, v11, v20, v21, v30, v31);
        mr_rot(a00, a22, a02, a01, a12, a03, a23, v00, v02, v10, v12, v20, v22, v30, v32);
        mr_rot(a00, a33, a03, a01, a13, a02, a23, v00, v03, v10, v13, v20, v23, v30, v33);
        mr_rot(a11, a22, a12, a01, a02, a13, a23, v01, v02, v11, v12, v21, v22, v31, v32);
        mr_rot(a11, a33, a13, a01, a03, a12, a23, v01, v03, v11, v13, v21, v23, v31, v33);
        mr_rot(a22, a33, a23, a02, a03, a12, a13, v02, v03, v12, v13, v22, v23, v32, v33);
    }
    // the column of the largest eigenvalue (the first of equal ones), by selects between named values: an index into the columns
    // would put them in scratch
    const bool b1 = a11 > a00;
    const float l1 = b1 ? a11 : a00;
    const bool b2 = a22 > l1;
    const float l2 = b2 ? a22 : l1;
    const bool b3 = a33 > l2;
    const float w = b3 ? v03 : b2 ? v02 : b1 ? v01 : v00, x = b3 ? v13 : b2 ? v12 : b1 ? v11 : v10;
    const float y = b3 ? v23 : b2 ? v22 : b1 ? v21 : v20, z = b3 ? v33 : b2 ? v32 : b1 ? v31 : v30;
    const float r = 1.f / sqrtf(w * w + x * x + y * y + z * z);             // (the columns stay orthonormal to rounding)
    return make_float4(w * r, x * r, y * r, z * r);
}

struct MrRot {
    float xx, xy, xz, yx, yy, yz, zx, zy, zz;
};

__host__ __device__ __forceinline__ MrRot mr_rotation(float4 q) {
    const float w = q.x, x = q.y, y = q.z, z = q.w;
    MrRot R;
    R.xx = 1.f - 2.f * (y * y + z * z);
    R.xy = 2.f * (x * y - w * z);
    R.xz = 2.f * (x * z + w * y);
    R.yx = 2.f * (x * y + w * z);
    R.yy = 1.f - 2.f * (x * x + z * z);
    R.yz = 2.f * (y * z - w * x);
    R.zx = 2.f * (x * z - w * y);
    R.zy = 2.f * (y * z + w * x);
    R.zz = 1.f - 2.f * (x * x + y * y);
    return R;
}

struct MrRec {
    float4 fit;             // (q, centroid)
    float4 quat;            // (w, x, y, z)
};

// (q, centroid) and the quaternion of one placement; (tbx, tby, tbz) = mean(target)
__host__ __device__ __forceinline__ MrRec mr_record(const MpLds& L, const int32_t* __restrict__ st, int S, int M, float tbx, float tby,
                                                    float tbz) {
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
    float Sxx = 0.f, Sxy = 0.f, Sxz = 0.f, Syx = 0.f, Syy = 0.f, Syz = 0.f, Szx = 0.f, Szy = 0.f, Szz = 0.f;
    for (int s = 0; s < S; ++s) {
        const int r0 = st[s], n = L.sl[s], m0 = L.so[s];
        for (int i = 0; i < n; ++i) {
            const float* x = L.xs + 3 * (r0 + i);
            const float* t = L.tg + 3 * (m0 + i);
            const float ux = x[0] - cx, uy = x[1] - cy, uz = x[2] - cz, tx = t[0] - tbx, ty = t[1] - tby, tz = t[2] - tbz;
            Sxx += tx * ux;
            Sxy += tx * uy;
            Sxz += tx * uz;
            Syx += ty * ux;
            Syy += ty * uy;
            Syz += ty * uz;
            Szx += tz * ux;
            Szy += tz * uy;
            Szz += tz * uz;
        }
    }
    const float4 qt = mr_quaternion(Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz);
    const MrRot R = mr_rotation(qt);
    float q = 0.f;
    for (int s = 0; s < S; ++s) {
        const int r0 = st[s], n = L.sl[s], m0 = L.so[s];
        for (int i = 0; i < n; ++i) {
            const float* x = L.xs + 3 * (r0 + i);
            const float* t = L.tg + 3 * (m0 + i);
            const float tx = t[0] - tbx, ty = t[1] - tby, tz = t[2] - tbz;
            const float ex = (x[0] - cx) - (R.xx * tx + R.xy * ty + R.xz * tz);
            const float ey = (x[1] - cy) - (R.yx * tx + R.yy * ty + R.yz * tz);
            const float ez = (x[2] - cz) - (R.zx * tx + R.zy * ty + R.zz * tz);
            q += ex * ex + ey * ey + ez * ez;
        }
    }
    return MrRec{make_float4(q, cx, cy, cz), qt};
}

__device__ inline void mr_target_mean(const MpLds& L, int M, float& tbx, float& tby, float& tbz) {
    tbx = tby = tbz = 0.f;
    for (int m = 0; m < M; ++m) {
        tbx += L.tg[3 * m];
        tby += L.tg[3 * m + 1];
        tbz += L.tg[3 * m + 2];
    }
    tbx /= (float)M;
    tby /= (float)M;
    tbz /= (float)M;
}

__device__ inline int mr_block_min(int v, int* slot) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = slot[0];
    for (int w = 1; w < MP_WAVES; ++w) r = min(r, slot[w]);
    return r;
}

// large-P path, first launch: one placement per thread, records to work[b, p, 0..1]
__global__ __launch_bounds__(MP_THREADS) void k_motif_rigid_records(const float* __restrict__ x0, int N, int P, int S, int M,
                                                                    const int32_t* __restrict__ seg_len,
                                                                    const int32_t* __restrict__ starts, const float* __restrict__ target,
                                                                    float4* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    const int b = blockIdx.y;
    const MpLds L = mp_carve(mp_smem, N, M, S, 0);          // (act / wcnt unused here)
    mp_stage(L, x0 + (size_t)b * 3 * N, target, seg_len, N, M, S);
    __syncthreads();
    float tbx, tby, tbz;
    mr_target_mean(L, M, tbx, tby, tbz);
    const int p = blockIdx.x * MP_THREADS + threadIdx.x;
    if (p < P) {
        const MrRec r = mr_record(L, starts + (size_t)p * S, S, M, tbx, tby, tbz);
        float4* o = work + 2 * ((size_t)b * P + p);
        o[0] = r.fit;
        o[1] = r.quat;
    }
}

template <bool SPILL>
__global__ __launch_bounds__(MP_THREADS) void k_motif_rigid(const float* __restrict__ x0, int N, int P, int S, int M,
                                                            const int32_t* __restrict__ seg_len, const int32_t* __restrict__ starts,
                                                            const float* __restrict__ target, const float* __restrict__ var_p,
                                                            const float4* __restrict__ work, float* __restrict__ logp,
                                                            float* __restrict__ grad, int32_t* __restrict__ best,
                                                            float* __restrict__ rmsd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const MpLds L = mp_carve(mp_smem, N, M, S, SPILL ? 0 : 2 * P);
    mp_stage(L, x0 + (size_t)b * 3 * N, target, seg_len, N, M, S);
    const float var = *var_p, two_var = 2.f * var;
    __syncthreads();
    float tbx, tby, tbz;
    mr_target_mean(L, M, tbx, tby, tbz);
    if (!SPILL)
        for (int p = tid; p < P; p += MP_THREADS) {
            const MrRec r = mr_record(L, starts + (size_t)p * S, S, M, tbx, tby, tbz);
            L.rec[2 * p] = r.fit;
            L.rec[2 * p + 1] = r.quat;
        }
    const float4* rec = SPILL ? work + 2 * (size_t)b * P : L.rec;
    __syncthreads();

    // score = -q / (2 var), in this one form wherever it is needed; logsumexp with the max taken first
    float mx = -INFINITY;
    for (int p = tid; p < P; p += MP_THREADS) mx = fmaxf(mx, -rec[2 * p].x / two_var);
    mx = mp_block_max(mx, L.red);
    float se = 0.f;
    for (int p = tid; p < P; p += MP_THREADS) se += expf(-rec[2 * p].x / two_var - mx);
    se = mp_block_sum(se, L.red);
    if (logp && blockIdx.x == 0 && tid == 0) logp[b] = mx + logf(se) - logf((float)P);

    // the lowest placement that reaches the max, and its RMSD
    if (best || rmsd) {
        int bp = P;
        for (int p = tid; p < P; p += MP_THREADS)
            if (p < bp && -rec[2 * p].x / two_var == mx) bp = p;
        bp = mr_block_min(bp, L.wcnt);
        if (bp >= P) bp = 0;                                  // (only a non-finite input gets here)
        if (blockIdx.x == 0 && tid == 0) {
            if (best) best[b] = bp;
            if (rmsd) rmsd[b] = sqrtf(rec[2 * bp].x / (float)M);
        }
        __syncthreads();                                      // (wcnt is used again below)
    }
    if (!grad) return;

    // the placements whose weight is not exactly 0, in ascending order: as k_motif_potential lists them
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int cap = mp_act_cap(P);
    int cnt = 0;
    for (int c0 = 0; c0 < P; c0 += MP_THREADS) {
        const int p = c0 + tid;
        const bool on = p < P && expf(-rec[2 * p].x / two_var - mx) != 0.f;
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

    // gather: lane = residue, wave = a contiguous quarter of the (listed) placements; R from the record's quaternion (wave-uniform)
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
            const float4 rp = rec[2 * p];
            const float e = expf(-rp.x / two_var - mx);       // bitwise the term of `se`
            if (e == 0.f) continue;                           // (wave-uniform)
            const int32_t* st = starts + (size_t)p * S;
            int m = -1;
            for (int s = 0; s < S; ++s) {
                const int d = n - st[s];
                if ((unsigned)d < (unsigned)L.sl[s]) m = L.so[s] + d;
            }
            if (m >= 0) {
                const MrRot R = mr_rotation(rec[2 * p + 1]);
                const float* t = L.tg + 3 * m;
                const float tx = t[0] - tbx, ty = t[1] - tby, tz = t[2] - tbz;
                bx += e * ((xn - rp.y) - (R.xx * tx + R.xy * ty + R.xz * tz));
                by += e * ((yn - rp.z) - (R.yx * tx + R.yy * ty + R.yz * tz));
                bz += e * ((zn - rp.w) - (R.zx * tx + R.zy * ty + R.zz * tz));
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

// ---- the group-wise form: genie_motif_potential_grouped ---------------------------------------------------------------------------
// A multi-motif problem: segment s belongs to group seg_group[s] (0..G-1); the segments of one group keep their relative pose, the
// groups move independently, so every group is superposed (or, align 0, translated) on its own.  For group g with M_g residues:
//   c^g_bp(m) = x0[b, r_p(m)] - mean_{m in g} x0[b, r_p(m)],   t^g(m) = target[m] - mean_{m in g} target[m]
//   e^g_bp(m) = c^g_bp(m) - R^g_bp t^g(m)   (R^g = I, or the proper rotation that minimises sum_{m in g} |e^g|^2: mr_quaternion)
//   q_bp = sum_g q^g_bp,  q^g_bp = sum_{m in g} |e^g_bp(m)|^2   (summed from the residuals, the groups added in group order)
//   score[b,p] = -q_bp / (2 var),   logp, w, best as above,   grad[b,n] = -sum_p w_bp [n in p] e^{g(n)}_bp(m_p(n)) / var
//   rmsd[b] = sqrt(q_{b,best} / M),   group_rmsd[b,g] = sqrt(q^g_{b,best} / M_g)
// (sum_{m in g} e^g = 0 because both sides are centred per group, so the translation form needs no mean term either.)  Placements stay
// joint: one softmax over p, the segments of all groups in file order.
//
// Layout as above.  The record of a placement is per group: (q^g, centroid of g) and, for the rigid fit, g's quaternion, G * rw float4
// (rw = 1 or 2), followed for all placements by the totals q_p, one float each.  They stay in LDS while they fit in MG_LDS_REC bytes
// and spill to `work` beyond.  The target is centred per group once, in LDS, when it is staged.  In the gather a lane's residue picks
// the group, so the record (and R) is read per lane; the weight stays wave-uniform.
constexpr size_t MG_LDS_REC = 96 * 1024;         // bytes of placement records kept in LDS; more spill to `work`

// float4 slots of one particle's records: P * G * rw of them, then the P totals padded to whole slots
__host__ __device__ inline size_t mg_slots(int P, int G, int rw) { return (size_t)P * G * rw + ((size_t)P + 3) / 4; }

// dynamic LDS: [rec: float4 x P_lds*G*rw] [qt: P_lds floats, padded] [xs: 3N] [tg: 3M] [gm: 3G] [part: WAVES*64*3] [red: 2*WAVES]
//              [sl, so, sg: 3S int] [gn: G int] [wcnt: WAVES int] [act: mp_act_cap(P) int]
size_t mg_lds_bytes(int N, int M, int S, int G, int P, int P_lds, int rw) {
    return mg_slots(P_lds, G, rw) * sizeof(float4) +
           sizeof(float) * (3 * (size_t)N + 3 * (size_t)M + 3 * (size_t)G + MP_WAVES * 64 * 3 + 2 * MP_WAVES) +
           sizeof(int) * (3 * (size_t)S + G + MP_WAVES + mp_act_cap(P));
}

struct MgLds {
    float4* rec;
    float *qt, *xs, *tg, *gm, *part, *red;
    int *sl, *so, *sg, *gn, *wcnt, *act;
};

__device__ inline MgLds mg_carve(unsigned char* base, int N, int M, int S, int G, int P_lds, int rw) {
    MgLds L;
    L.rec = reinterpret_cast<float4*>(base);
    L.qt = reinterpret_cast<float*>(L.rec + (size_t)P_lds * G * rw);
    L.xs = reinterpret_cast<float*>(L.rec + mg_slots(P_lds, G, rw));
    L.tg = L.xs + 3 * N;
    L.gm = L.tg + 3 * M;
    L.part = L.gm + 3 * G;
    L.red = L.part + MP_WAVES * 64 * 3;
    L.sl = reinterpret_cast<int*>(L.red + 2 * MP_WAVES);
    L.so = L.sl + S;
    L.sg = L.so + S;
    L.gn = L.sg + S;
    L.wcnt = L.gn + G;
    L.act = L.wcnt + MP_WAVES;
    return L;
}

// x0[b], the target and the segment table into LDS; then every group's target mean and size (one thread per group, its residues in
// motif order) and the target centred per group in place.  Ends with the block in step.  (seg_group is the caller's, validated where
// it is built; it is clamped all the same: it indexes LDS.)
__device__ inline void mg_stage(const MgLds& L, const float* __restrict__ x0b, const float* __restrict__ target,
                                const int32_t* __restrict__ seg_len, const int32_t* __restrict__ seg_group, int N, int M, int S, int G) {
    for (int i = threadIdx.x; i < 3 * N; i += MP_THREADS) L.xs[i] = x0b[i];
    for (int i = threadIdx.x; i < 3 * M; i += MP_THREADS) L.tg[i] = target[i];
    if (threadIdx.x == 0) {
        int off = 0;
        for (int s = 0; s < S; ++s) {
            const int n = seg_len[s];
            L.sl[s] = n;
            L.so[s] = off;
            L.sg[s] = min(max(seg_group[s], 0), G - 1);
            off += n;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < G) {
        const int g = threadIdx.x;
        float tx = 0.f, ty = 0.f, tz = 0.f;
        int cnt = 0;
        for (int s = 0; s < S; ++s) {
            if (L.sg[s] != g) continue;
            const int n = L.sl[s], m0 = L.so[s];
            for (int i = 0; i < n; ++i) {
                const float* t = L.tg + 3 * (m0 + i);
                tx += t[0];
                ty += t[1];
                tz += t[2];
            }
            cnt += n;
        }
        L.gm[3 * g] = tx / (float)cnt;
        L.gm[3 * g + 1] = ty / (float)cnt;
        L.gm[3 * g + 2] = tz / (float)cnt;
        L.gn[g] = cnt;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < M; m += MP_THREADS) {
        int g = 0;
        for (int s = 0; s < S; ++s)
            if ((unsigned)(m - L.so[s]) < (unsigned)L.sl[s]) g = L.sg[s];
        L.tg[3 * m] -= L.gm[3 * g];
        L.tg[3 * m + 1] -= L.gm[3 * g + 1];
        L.tg[3 * m + 2] -= L.gm[3 * g + 2];
    }
    __syncthreads();
}

// the G records of one placement to out[0 .. G*rw) (LDS or `work`); returns q_p.  L.tg is centred per group.
template <bool RIGID>
__device__ __forceinline__ float mg_record(const MgLds& L, const int32_t* __restrict__ st, int S, int G, float4* out) {
    float qp = 0.f;
    for (int g = 0; g < G; ++g) {
        const float ng = (float)L.gn[g];
        float cx = 0.f, cy = 0.f, cz = 0.f;
        for (int s = 0; s < S; ++s) {
            if (L.sg[s] != g) continue;
            const int r0 = st[s], n = L.sl[s];
            for (int i = 0; i < n; ++i) {
                const float* x = L.xs + 3 * (r0 + i);
                cx += x[0];
                cy += x[1];
                cz += x[2];
            }
        }
        cx /= ng;
        cy /= ng;
        cz /= ng;
        float q = 0.f;
        if (RIGID) {
            float Sxx = 0.f, Sxy = 0.f, Sxz = 0.f, Syx = 0.f, Syy = 0.f, Syz = 0.f, Szx = 0.f, Szy = 0.f, Szz = 0.f;
            for (int s = 0; s < S; ++s) {
                if (L.sg[s] != g) continue;
                const int r0 = st[s], n = L.sl[s], m0 = L.so[s];
                for (int i = 0; i < n; ++i) {
                    const float* x = L.xs + 3 * (r0 + i);
                    const float* t = L.tg + 3 * (m0 + i);
                    const float ux = x[0] - cx, uy = x[1] - cy, uz = x[2] - cz, tx = t[0], ty = t[1], tz = t[2];
                    Sxx += tx * ux;
                    Sxy += tx * uy;
                    Sxz += tx * uz;
                    Syx += ty * ux;
                    Syy += ty * uy;
                    Syz += ty * uz;
                    Szx += tz * ux;
                    Szy += tz * uy;
                    Szz += tz * uz;
                }
            }
            const float4 qt = mr_quaternion(Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz);
            const MrRot R = mr_rotation(qt);
            for (int s = 0; s < S; ++s) {
                if (L.sg[s] != g) continue;
                const int r0 = st[s], n = L.sl[s], m0 = L.so[s];
                for (int i = 0; i < n; ++i) {
                    const float* x = L.xs + 3 * (r0 + i);
                    const float* t = L.tg + 3 * (m0 + i);
                    const float tx = t[0], ty = t[1], tz = t[2];
                    const float ex = (x[0] - cx) - (R.xx * tx + R.xy * ty + R.xz * tz);
                    const float ey = (x[1] - cy) - (R.yx * tx + R.yy * ty + R.yz * tz);
                    const float ez = (x[2] - cz) - (R.zx * tx + R.zy * ty + R.zz * tz);
                    q += ex * ex + ey * ey + ez * ez;
                }
            }
            out[2 * g + 1] = qt;
        } else {
            for (int s = 0; s < S; ++s) {
                if (L.sg[s] != g) continue;
                const int r0 = st[s], n = L.sl[s], m0 = L.so[s];
                for (int i = 0; i < n; ++i) {
                    const float* x = L.xs + 3 * (r0 + i);
                    const float* t = L.tg + 3 * (m0 + i);
                    const float ex = (x[0] - cx) - t[0], ey = (x[1] - cy) - t[1], ez = (x[2] - cz) - t[2];
                    q += ex * ex + ey * ey + ez * ez;
                }
            }
        }
        out[(RIGID ? 2 : 1) * g] = make_float4(q, cx, cy, cz);
        qp += q;
    }
    return qp;
}

// large-P path, first launch: one placement per thread, records and totals to work[b]
template <bool RIGID>
__global__ __launch_bounds__(MP_THREADS) void k_motif_grouped_records(const float* __restrict__ x0, int N, int P, int S, int M, int G,
                                                                      const int32_t* __restrict__ seg_len,
                                                                      const int32_t* __restrict__ seg_group,
                                                                      const int32_t* __restrict__ starts, const float* __restrict__ target,
                                                                      float4* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    constexpr int RW = RIGID ? 2 : 1;
    const int b = blockIdx.y;
    const MgLds L = mg_carve(mp_smem, N, M, S, G, 0, RW);          // (act / wcnt unused here)
    mg_stage(L, x0 + (size_t)b * 3 * N, target, seg_len, seg_group, N, M, S, G);
    const int p = blockIdx.x * MP_THREADS + threadIdx.x;
    if (p < P) {
        float4* rec = work + (size_t)b * mg_slots(P, G, RW);
        reinterpret_cast<float*>(rec + (size_t)P * G * RW)[p] = mg_record<RIGID>(L, starts + (size_t)p * S, S, G, rec + (size_t)p * G * RW);
    }
}

template <bool SPILL, bool RIGID>
__global__ __launch_bounds__(MP_THREADS) void k_motif_grouped(const float* __restrict__ x0, int N, int P, int S, int M, int G,
                                                              const int32_t* __restrict__ seg_len, const int32_t* __restrict__ seg_group,
                                                              const int32_t* __restrict__ starts, const float* __restrict__ target,
                                                              const float* __restrict__ var_p, const float4* __restrict__ work,
                                                              float* __restrict__ logp, float* __restrict__ grad,
                                                              int32_t* __restrict__ best, float* __restrict__ rmsd,
                                                              float* __restrict__ group_rmsd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    constexpr int RW = RIGID ? 2 : 1;
    const int b = blockIdx.y, tid = threadIdx.x;
    const MgLds L = mg_carve(mp_smem, N, M, S, G, SPILL ? 0 : P, RW);
    const float var = *var_p, two_var = 2.f * var;
    mg_stage(L, x0 + (size_t)b * 3 * N, target, seg_len, seg_group, N, M, S, G);
    if (!SPILL)
        for (int p = tid; p < P; p += MP_THREADS) L.qt[p] = mg_record<RIGID>(L, starts + (size_t)p * S, S, G, L.rec + (size_t)p * G * RW);
    const float4* rec = SPILL ? work + (size_t)b * mg_slots(P, G, RW) : L.rec;
    const float* qt = SPILL ? reinterpret_cast<const float*>(rec + (size_t)P * G * RW) : L.qt;
    __syncthreads();

    // score = -q / (2 var), in this one form wherever it is needed; logsumexp with the max taken first
    float mx = -INFINITY;
    for (int p = tid; p < P; p += MP_THREADS) mx = fmaxf(mx, -qt[p] / two_var);
    mx = mp_block_max(mx, L.red);
    float se = 0.f;
    for (int p = tid; p < P; p += MP_THREADS) se += expf(-qt[p] / two_var - mx);
    se = mp_block_sum(se, L.red);
    if (logp && blockIdx.x == 0 && tid == 0) logp[b] = mx + logf(se) - logf((float)P);

    // the lowest placement that reaches the max, its RMSD and that of every group in it
    if (best || rmsd || group_rmsd) {
        int bp = P;
        for (int p = tid; p < P; p += MP_THREADS)
            if (p < bp && -qt[p] / two_var == mx) bp = p;
        bp = mr_block_min(bp, L.wcnt);
        if (bp >= P) bp = 0;                                  // (only a non-finite input gets here)
        if (blockIdx.x == 0) {
            if (tid == 0 && best) best[b] = bp;
            if (tid == 0 && rmsd) rmsd[b] = sqrtf(qt[bp] / (float)M);
            if (tid < G && group_rmsd) group_rmsd[(size_t)b * G + tid] = sqrtf(rec[((size_t)bp * G + tid) * RW].x / (float)L.gn[tid]);
        }
        __syncthreads();                                      // (wcnt is used again below)
    }
    if (!grad) return;

    // the placements whose weight is not exactly 0, in ascending order: as k_motif_potential lists them
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int cap = mp_act_cap(P);
    int cnt = 0;
    for (int c0 = 0; c0 < P; c0 += MP_THREADS) {
        const int p = c0 + tid;
        const bool on = p < P && expf(-qt[p] / two_var - mx) != 0.f;
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

    // gather: lane = residue, wave = a contiguous quarter of the (listed) placements; the residue's segment picks the group, and with
    // it the centroid and R of the record (per lane; the weight is wave-uniform)
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
            const float e = expf(-qt[p] / two_var - mx);      // bitwise the term of `se`
            if (e == 0.f) continue;                           // (wave-uniform)
            const int32_t* st = starts + (size_t)p * S;
            int m = -1, g = 0;
            for (int s = 0; s < S; ++s) {
                const int d = n - st[s];
                if ((unsigned)d < (unsigned)L.sl[s]) {
                    m = L.so[s] + d;
                    g = L.sg[s];
                }
            }
            if (m >= 0) {
                const float4* rg = rec + ((size_t)p * G + g) * RW;
                const float4 rp = rg[0];
                const float* t = L.tg + 3 * m;
                if (RIGID) {
                    const MrRot R = mr_rotation(rg[1]);
                    const float tx = t[0], ty = t[1], tz = t[2];
                    bx += e * ((xn - rp.y) - (R.xx * tx + R.xy * ty + R.xz * tz));
                    by += e * ((yn - rp.z) - (R.yx * tx + R.yy * ty + R.yz * tz));
                    bz += e * ((zn - rp.w) - (R.zx * tx + R.zy * ty + R.zz * tz));
                } else {
                    bx += e * ((xn - rp.y) - t[0]);
                    by += e * ((yn - rp.z) - t[1]);
                    bz += e * ((zn - rp.w) - t[2]);
                }
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
        float* gout = grad + ((size_t)b * N + n) * 3;
        gout[0] = gx * sc;
        gout[1] = gy * sc;
        gout[2] = gz * sc;
    }
}

template <bool RIGID>
int mg_launch(hipStream_t st, int B, int N, const float* x0, int P, int S, int M, int G, const int32_t* seg_len, const int32_t* seg_group,
              const int32_t* starts, const float* target, const float* var, float* logp, float* grad, int32_t* best, float* rmsd,
              float* group_rmsd, void* work, bool spill, size_t lds) {
    const dim3 grid(grad ? (N + MP_TILE - 1) / MP_TILE : 1, B);          // without a gradient there is nothing to tile
    if (spill) {
        if (lds > 64 * 1024) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_motif_grouped_records<RIGID>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_motif_grouped<true, RIGID>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        }
        float4* rec = static_cast<float4*>(work);
        hipLaunchKernelGGL(k_motif_grouped_records<RIGID>, dim3((P + MP_THREADS - 1) / MP_THREADS, B), dim3(MP_THREADS), lds, st, x0, N, P,
                           S, M, G, seg_len, seg_group, starts, target, rec);
        hipLaunchKernelGGL((k_motif_grouped<true, RIGID>), grid, dim3(MP_THREADS), lds, st, x0, N, P, S, M, G, seg_len, seg_group, starts,
                           target, var, (const float4*)rec, logp, grad, best, rmsd, group_rmsd);
    } else {
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_motif_grouped<false, RIGID>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((k_motif_grouped<false, RIGID>), grid, dim3(MP_THREADS), lds, st, x0, N, P, S, M, G, seg_len, seg_group, starts,
                           target, var, (const float4*)nullptr, logp, grad, best, rmsd, group_rmsd);
    }
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
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

size_t genie_motif_potential_rigid_work_bytes(int B, int P) {
    return (B >= 1 && P > MR_LDS_P) ? (size_t)B * (size_t)P * 2 * sizeof(float4) : 0;
}

int genie_motif_potential_rigid(genie_stream_t stream, int B, int N, const float* x0, int P, int S, int M, const int32_t* seg_len,
                                const int32_t* starts, const float* target, const float* var, float* logp_out, float* grad_out,
                                int32_t* best_out, float* rmsd_out, void* work, size_t work_bytes) {
    if (!x0 || !seg_len || !starts || !target || !var) return GENIE_E_ARG;
    if ((logp_out == nullptr) != (grad_out == nullptr) || (!logp_out && !best_out && !rmsd_out)) return GENIE_E_ARG;
    if (B < 1 || B > 65535 || N < 1 || P < 1 || S < 1 || M < 3 || M > N || S > M || (int64_t)P * S > INT32_MAX) return GENIE_E_ARG;
    const bool spill = P > MR_LDS_P;
    const size_t need = genie_motif_potential_rigid_work_bytes(B, P);
    if (spill && (!work || work_bytes < need || (reinterpret_cast<uintptr_t>(work) & 15))) return GENIE_E_ARG;
    const size_t lds = mp_lds_bytes(N, M, S, P, spill ? 0 : 2 * P);
    if (lds > MP_LDS_MAX) return GENIE_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grad_out ? (N + MP_TILE - 1) / MP_TILE : 1, B);          // without a gradient there is nothing to tile
    if (spill) {
        if (lds > 64 * 1024) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_motif_rigid_records), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_motif_rigid<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds);
        }
        float4* rec = static_cast<float4*>(work);
        hipLaunchKernelGGL(k_motif_rigid_records, dim3((P + MP_THREADS - 1) / MP_THREADS, B), dim3(MP_THREADS), lds, st, x0, N, P, S, M,
                           seg_len, starts, target, rec);
        hipLaunchKernelGGL(k_motif_rigid<true>, grid, dim3(MP_THREADS), lds, st, x0, N, P, S, M, seg_len, starts, target, var,
                           (const float4*)rec, logp_out, grad_out, best_out, rmsd_out);
    } else {
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_motif_rigid<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds);
        hipLaunchKernelGGL(k_motif_rigid<false>, grid, dim3(MP_THREADS), lds, st, x0, N, P, S, M, seg_len, starts, target, var,
                           (const float4*)nullptr, logp_out, grad_out, best_out, rmsd_out);
    }
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}

size_t genie_motif_potential_grouped_work_bytes(int B, int P, int G, int align) {
    if (B < 1 || P < 1 || G < 1 || G > GENIE_MOTIF_MAX_GROUPS || (align != 0 && align != 1)) return 0;
    const size_t bytes = mg_slots(P, G, align ? 2 : 1) * sizeof(float4);
    return bytes > MG_LDS_REC ? (size_t)B * bytes : 0;
}

int genie_motif_potential_grouped(genie_stream_t stream, int B, int N, const float* x0, int P, int S, int M, int G, const int32_t* seg_len,
                                  const int32_t* seg_group, const int32_t* starts, const float* target, const float* var, int align,
                                  float* logp_out, float* grad_out, int32_t* best_out, float* rmsd_out, float* group_rmsd_out, void* work,
                                  size_t work_bytes) {
    if (!x0 || !seg_len || !seg_group || !starts || !target || !var) return GENIE_E_ARG;
    if ((logp_out == nullptr) != (grad_out == nullptr) || (!logp_out && !best_out && !rmsd_out && !group_rmsd_out)) return GENIE_E_ARG;
    if (B < 1 || B > 65535 || N < 1 || P < 1 || S < 1 || M < 1 || M > N || S > M || (int64_t)P * S > INT32_MAX) return GENIE_E_ARG;
    if (G < 1 || G > GENIE_MOTIF_MAX_GROUPS || G > S || (align != 0 && align != 1)) return GENIE_E_ARG;
    if (align == 1 && M < 3 * G) return GENIE_E_ARG;          // (every group needs 3 residues: the caller checks seg_len itself)
    const int rw = align ? 2 : 1;
    const size_t need = genie_motif_potential_grouped_work_bytes(B, P, G, align);
    const bool spill = need > 0;
    if (spill && (!work || work_bytes < need || (reinterpret_cast<uintptr_t>(work) & 15))) return GENIE_E_ARG;
    const size_t lds = mg_lds_bytes(N, M, S, G, P, spill ? 0 : P, rw);
    if (lds > MP_LDS_MAX) return GENIE_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    return align ? mg_launch<true>(st, B, N, x0, P, S, M, G, seg_len, seg_group, starts, target, var, logp_out, grad_out, best_out, rmsd_out,
                                   group_rmsd_out, work, spill, lds)
                 : mg_launch<false>(st, B, N, x0, P, S, M, G, seg_len, seg_group, starts, target, var, logp_out, grad_out, best_out,
                                    rmsd_out, group_rmsd_out, work, spill, lds);
}
