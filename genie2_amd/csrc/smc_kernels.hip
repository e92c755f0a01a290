// Motif placement potential of twisted-diffusion / SMC sampling (include/genie_hip.h): the fork's motif twisting function,
// genie/sampler/unconditional_smc.py:303-345 (genie2_amd/smc.py:59-70 is its PyTorch restatement), with its gradient, in one pass
// instead of a Python loop over placements and an autograd walk back through it.  Three entries, four forms, one kernel skeleton.
//
// Placement p puts segment s at residues starts[p,s] .. starts[p,s] + seg_len[s] - 1; motif position m runs over the segments
// in order (what x0[:, mask] selects).  Every form has, for particle b, a residual e_bp(m) per placed residue and
//   q_bp = sum_m |e_bp(m)|^2,   score[b,p] = -q_bp / (2 var),   logp[b] = logsumexp_p score[b,p] - log P,   w_bp = softmax_p score[b,:]
//   grad[b,n] = -sum_p w_bp [n in p] (e_bp(m_p(n)) - mean_m e_bp(m)) / var
// and, where it reports a fit, best[b] = the lowest p with the largest score and rmsd[b] = sqrt(q_{b,best} / M).
//
// The skeleton (k_motif<Form, SPILL>): grid (ceil(N / 64), B), 256 threads.  Every work-group of particle b stages x0[b], the target
// and the segment table in LDS, writes the record of every placement (B * P * M is about 1e5, cheap to repeat per residue tile),
// reduces max and sum of exp over the scores in a fixed tree, picks the best placement (an integer min), lists the placements whose
// weight is not exactly 0 in ascending order (scores reach -1e5 with var about 1e-2, so late in the trajectory that is one or a few),
// then gathers the gradient of its 64 residues, one per lane: each wave walks a contiguous quarter of the listed placements in
// order, in partial sums of MP_CHUNK, and the four wave sums are added in wave order.  No atomics, no scatter: every output is
// written once, in a fixed order, so results are bitwise reproducible.  While a particle's records fit in LDS it is one launch; beyond
// that k_motif_records<Form> writes them to the caller's `work` first and the main kernel reads them from there (two launches).
// Without a gradient to write (a fit only), one work-group per particle does the scoring and the gather is skipped.  `starts` is
// trusted (the caller validates it once when it builds it); it only ever indexes LDS.
//
// A form supplies only what its mathematics changes: the record of a placement (its width in float4 slots, where q lives, how
// record() fills it), score(p), the residual() of a lane's residue in the gather, any staging of its own, and whether it reports a
// fit.  The forms, each stated where it is defined below:
//   Translate     genie_motif_potential          (score, centroid): 1 slot                          e = (c - target) + mean(target)
//   Rigid         genie_motif_potential_rigid    (q, centroid), quaternion: 2 slots                 e = c - R (target - mean(target))
//   Grouped<ROT>  genie_motif_potential_grouped  per group (q^g, centroid)[, quaternion]; totals q  e = c^g - [R^g] t^g, t^g centred in LDS
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/genie_hip.h"
#include "horn.h"

namespace {

constexpr int MP_THREADS = 256;
constexpr int MP_WAVES = MP_THREADS / 64;
constexpr int MP_TILE = 64;             // residues per work-group in the gather: one per lane
constexpr int MP_CHUNK = 64;            // placements per inner partial sum of the gather (two-level f32 summation)
constexpr size_t MP_LDS_MAX = 160 * 1024;
constexpr int MP_LDS_P = 2048;          // Translate: placement records (16 B each) kept in LDS; more spill to `work`
constexpr int MR_LDS_P = 1024;          // Rigid: placement records (32 B each) kept in LDS; more spill to `work`
constexpr size_t MG_LDS_REC = 96 * 1024;         // Grouped: bytes of placement records kept in LDS; more spill to `work`

// the active-placement list holds this many entries (P itself when there are fewer)
__host__ __device__ inline int mp_act_cap(int P) { return P < MP_LDS_P ? P : MP_LDS_P; }

// dynamic LDS: [rec: float4 x slots (0 when the records are in `work`)] [xs: 3N] [tg: 3M] [gm: 3G] [part: WAVES*64*3] [red: 2*WAVES]
//              [sl, so: 2S int] [sg: S int] [gn: G int] [wcnt: WAVES int] [act: mp_act_cap(P) int]
// gm (group target means), sg (segment -> group) and gn (group sizes) exist for the grouped forms only: G = 0 is a single body.
struct MpLds {
    float4* rec;
    float *xs, *tg, *gm, *part, *red;
    int *sl, *so, *sg, *gn, *wcnt, *act;
};

size_t mp_lds_bytes(int N, int M, int S, int G, int P, size_t slots) {
    return slots * sizeof(float4) + sizeof(float) * (3 * (size_t)N + 3 * (size_t)M + 3 * (size_t)G + MP_WAVES * 64 * 3 + 2 * MP_WAVES) +
           sizeof(int) * (2 * (size_t)S + (G ? (size_t)S + G : 0) + MP_WAVES + mp_act_cap(P));
}

__device__ inline MpLds mp_carve(unsigned char* base, int N, int M, int S, int G, size_t slots) {
    MpLds L;
    L.rec = reinterpret_cast<float4*>(base);
    L.xs = reinterpret_cast<float*>(L.rec + slots);
    L.tg = L.xs + 3 * N;
    L.gm = L.tg + 3 * M;
    L.part = L.gm + 3 * G;
    L.red = L.part + MP_WAVES * 64 * 3;
    L.sl = reinterpret_cast<int*>(L.red + 2 * MP_WAVES);
    L.so = L.sl + S;
    L.sg = L.so + S;
    L.gn = L.sg + (G ? S : 0);
    L.wcnt = L.gn + G;
    L.act = L.wcnt + MP_WAVES;
    return L;
}

// x0[b], the target and the segment table into LDS (segment offsets by one thread, in order).  (seg_group is the caller's,
// validated where it is built; it is clamped all the same: it indexes LDS.)
template <bool GROUPED>
__device__ inline void mp_stage(const MpLds& L, const float* __restrict__ x0b, const float* __restrict__ target,
                                const int32_t* __restrict__ seg_len, const int32_t* __restrict__ seg_group, int N, int M, int S, int G) {
    for (int i = threadIdx.x; i < 3 * N; i += MP_THREADS) L.xs[i] = x0b[i];
    for (int i = threadIdx.x; i < 3 * M; i += MP_THREADS) L.tg[i] = target[i];
    if (threadIdx.x == 0) {
        int off = 0;
        for (int s = 0; s < S; ++s) {
            const int n = seg_len[s];
            L.sl[s] = n;
            L.so[s] = off;
            if (GROUPED) L.sg[s] = min(max(seg_group[s], 0), G - 1);
            off += n;
        }
    }
}

// the sizes of one call, the same for every form (G = 0 for a single body)
struct MpDims {
    int N, P, S, M, G;
    float var, two_var;
};

struct MpVec {
    float x, y, z;
};

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

__device__ inline int mp_block_min(int v, int* slot) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = slot[0];
    for (int w = 1; w < MP_WAVES; ++w) r = min(r, slot[w]);
    return r;
}

// mean(target) over all M motif residues
__device__ inline MpVec mp_target_mean(const MpLds& L, int M) {
    float tx = 0.f, ty = 0.f, tz = 0.f;
    for (int m = 0; m < M; ++m) {
        tx += L.tg[3 * m];
        ty += L.tg[3 * m + 1];
        tz += L.tg[3 * m + 2];
    }
    return MpVec{tx / (float)M, ty / (float)M, tz / (float)M};
}

// ---- the rotation of a superposed fit: MrMat, mr_quaternion and mr_rotation are in horn.h
__host__ __device__ __forceinline__ MpVec mr_apply(const MrMat& R, float tx, float ty, float tz) {
    return MpVec{R.xx * tx + R.xy * ty + R.xz * tz, R.yx * tx + R.yy * ty + R.yz * tz, R.zx * tx + R.zy * ty + R.zz * tz};
}

// ---- one body of one placement: the loops over its placed residues ------------------------------------------------------------------
// A body is every segment (ALL) or the segments of group g.  SHIFT: the target is centred at use (t - tb); otherwise L.tg is taken
// as it stands (Translate's uncentred target, a group's target centred in LDS).

// the centroid of the body's n placed residues
template <bool ALL>
__host__ __device__ __forceinline__ MpVec mp_centroid(const MpLds& L, const int32_t* __restrict__ st, int S, int g, float n) {
    float cx = 0.f, cy = 0.f, cz = 0.f;
    for (int s = 0; s < S; ++s) {
        if (!ALL && L.sg[s] != g) continue;
        const int r0 = st[s], len = L.sl[s];
        for (int i = 0; i < len; ++i) {
            const float* x = L.xs + 3 * (r0 + i);
            cx += x[0];
            cy += x[1];
            cz += x[2];
        }
    }
    return MpVec{cx / n, cy / n, cz / n};
}

// S_ab = sum_m t_a(m) c_b(m), c = x - centroid
template <bool ALL, bool SHIFT>
__host__ __device__ __forceinline__ MrMat mp_correlation(const MpLds& L, const int32_t* __restrict__ st, int S, int g, MpVec c, MpVec tb) {
    MrMat C = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
        if (!ALL && L.sg[s] != g) continue;
        const int r0 = st[s], len = L.sl[s], m0 = L.so[s];
        for (int i = 0; i < len; ++i) {
            const float* x = L.xs + 3 * (r0 + i);
            const float* t = L.tg + 3 * (m0 + i);
            const float ux = x[0] - c.x, uy = x[1] - c.y, uz = x[2] - c.z;
            const float tx = SHIFT ? t[0] - tb.x : t[0], ty = SHIFT ? t[1] - tb.y : t[1], tz = SHIFT ? t[2] - tb.z : t[2];
            C.xx += tx * ux;
            C.xy += tx * uy;
            C.xz += tx * uz;
            C.yx += ty * ux;
            C.yy += ty * uy;
            C.yz += ty * uz;
            C.zx += tz * ux;
            C.zy += tz * uy;
            C.zz += tz * uz;
        }
    }
    return C;
}

struct MpFit {
    float4 fit;             // (q, centroid)
    float4 quat;            // (w, x, y, z) when ROT
};

// the fit of one body: centroid, then (ROT) the rotation from the correlation, then q = sum_m |(x - centroid) - R t|^2 (ROT) or
// |(x - centroid) - t|^2 (smc.py:66-68): always summed from the residuals, never as G_x + G_t - 2 lambda, which cancels to nothing
// exactly when the fit is good.  (The residual loop stays in this function: moved into one of its own, the compiler contracts the
// first Jacobi sweep next to it differently, and the last bits of the quaternion change.)
template <bool ALL, bool ROT, bool SHIFT>
__host__ __device__ __forceinline__ MpFit mp_fit(const MpLds& L, const int32_t* __restrict__ st, int S, int g, float n, MpVec tb) {
    const MpVec c = mp_centroid<ALL>(L, st, S, g, n);
    float4 qt = make_float4(1.f, 0.f, 0.f, 0.f);
    if (ROT) qt = mr_quaternion(mp_correlation<ALL, SHIFT>(L, st, S, g, c, tb));
    const MrMat R = mr_rotation(qt);
    float q = 0.f;
    for (int s = 0; s < S; ++s) {
        if (!ALL && L.sg[s] != g) continue;
        const int r0 = st[s], len = L.sl[s], m0 = L.so[s];
        for (int i = 0; i < len; ++i) {
            const float* x = L.xs + 3 * (r0 + i);
            const float* t = L.tg + 3 * (m0 + i);
            const float tx = SHIFT ? t[0] - tb.x : t[0], ty = SHIFT ? t[1] - tb.y : t[1], tz = SHIFT ? t[2] - tb.z : t[2];
            const float ex = (x[0] - c.x) - (ROT ? R.xx * tx + R.xy * ty + R.xz * tz : tx);
            const float ey = (x[1] - c.y) - (ROT ? R.yx * tx + R.yy * ty + R.yz * tz : ty);
            const float ez = (x[2] - c.z) - (ROT ? R.zx * tx + R.zy * ty + R.zz * tz : tz);
            q += ex * ex + ey * ey + ez * ez;
        }
    }
    return MpFit{make_float4(q, c.x, c.y, c.z), qt};
}

// ---- the forms -------------------------------------------------------------------------------------------------------------------
// Each: slots(P, G) float4 of records per particle; stage() after x0, target and segments are in LDS (it may end with a barrier of its
// own); record() writes placement p's record; score() of a written record; residual() of the residue at (xn) that placement p puts at
// motif position m, in a segment of group g (0 for a single body): the e of the gradient, its mean term included; HAS_FIT: best /
// rmsd (and q() for them).

// Translation only, the reference's own potential; the target may be uncentred:
//   c_bp(m) = x0[b, r_p(m)] - mean_m x0[b, r_p(m)],   e_bp(m) = c_bp(m) - target[m]
// mean_m e_bp(m) = mean_m c_bp(m) - mean_m target[m] = -mean(target) for every (b, p) because c is centred; it is taken in that
// exact form (zero for a centred target, and the entry stays right for one that is not).  The record holds the score itself.
struct Translate {
    static constexpr bool GROUPED = false, HAS_FIT = false;
    __host__ __device__ static size_t slots(int P, int) { return (size_t)P; }
    MpVec tb;

    __device__ __forceinline__ void stage(const MpLds& L, const MpDims& d) { tb = mp_target_mean(L, d.M); }
    __device__ __forceinline__ void record(const MpLds& L, const MpDims& d, const int32_t* __restrict__ st, float4* rec, int p) const {
        const MpFit r = mp_fit<true, false, false>(L, st, d.S, 0, (float)d.M, tb);
        rec[p] = make_float4(-r.fit.x / (2.f * d.var), r.fit.y, r.fit.z, r.fit.w);
    }
    __device__ __forceinline__ float score(const MpDims&, const float4* rec, int p) const { return rec[p].x; }
    __device__ __forceinline__ MpVec residual(const MpLds& L, const MpDims&, const float4* rec, int p, int m, int, MpVec xn) const {
        const float4 rp = rec[p];
        const float* t = L.tg + 3 * m;
        return MpVec{((xn.x - rp.y) - t[0]) + tb.x, ((xn.y - rp.z) - t[1]) + tb.y, ((xn.z - rp.w) - t[2]) + tb.z};
    }
};

// Superposed: every placement is compared to the motif in its best-fitting orientation.  With t_c = target - mean(target):
//   R_bp = argmin over proper rotations of sum_m |c_bp(m) - R t_c(m)|^2,   e_bp(m) = c_bp(m) - R_bp t_c(m)
// (the derivative through R vanishes at the optimum, and sum_m e = 0 because both sides are centred).  The record is (q, centroid)
// and the quaternion; the gather rebuilds R from it (wave-uniform).  score = -q / (2 var) in this one form wherever it is needed.
struct Rigid {
    static constexpr bool GROUPED = false, HAS_FIT = true;
    __host__ __device__ static size_t slots(int P, int) { return 2 * (size_t)P; }
    MpVec tb;

    __device__ __forceinline__ void stage(const MpLds& L, const MpDims& d) { tb = mp_target_mean(L, d.M); }
    __device__ __forceinline__ void record(const MpLds& L, const MpDims& d, const int32_t* __restrict__ st, float4* rec, int p) const {
        const MpFit r = mp_fit<true, true, true>(L, st, d.S, 0, (float)d.M, tb);
        rec[2 * p] = r.fit;
        rec[2 * p + 1] = r.quat;
    }
    __device__ __forceinline__ float q(const MpDims&, const float4* rec, int p) const { return rec[2 * p].x; }
    __device__ __forceinline__ float score(const MpDims& d, const float4* rec, int p) const { return -rec[2 * p].x / d.two_var; }
    __device__ __forceinline__ MpVec residual(const MpLds& L, const MpDims&, const float4* rec, int p, int m, int, MpVec xn) const {
        const float4 rp = rec[2 * p];
        const MrMat R = mr_rotation(rec[2 * p + 1]);
        const float* t = L.tg + 3 * m;
        const MpVec rt = mr_apply(R, t[0] - tb.x, t[1] - tb.y, t[2] - tb.z);
        return MpVec{(xn.x - rp.y) - rt.x, (xn.y - rp.z) - rt.y, (xn.z - rp.w) - rt.z};
    }
};

// Group-wise, a multi-motif problem: segment s belongs to group seg_group[s] (0..G-1); the segments of one group keep their relative
// pose, the groups move independently, so every group is superposed (ROT) or translated on its own.  For group g with M_g residues:
//   c^g_bp(m) = x0[b, r_p(m)] - mean_{m in g} x0[b, r_p(m)],   t^g(m) = target[m] - mean_{m in g} target[m]
//   e^g_bp(m) = c^g_bp(m) - R^g_bp t^g(m)   (R^g = I, or the proper rotation that minimises sum_{m in g} |e^g|^2)
//   q_bp = sum_g q^g_bp,  q^g_bp = sum_{m in g} |e^g_bp(m)|^2   (the groups added in group order),   e_bp(m) = e^{g(m)}_bp(m)
//   group_rmsd[b,g] = sqrt(q^g_{b,best} / M_g)
// (sum_{m in g} e^g = 0 because both sides are centred per group, so the translation form needs no mean term either.)  Placements stay
// joint: one softmax over p, the segments of all groups in file order.  The record of a placement is per group: (q^g, centroid of g)
// and, ROT, g's quaternion, G * RW float4, followed for all placements by the totals q_p, one float each, padded to whole slots.  The
// target is centred per group once, in LDS, when it is staged.  In the gather a lane's residue picks the group, so the record (and R)
// is read per lane; the weight stays wave-uniform.
template <bool ROT>
struct Grouped {
    static constexpr bool GROUPED = true, HAS_FIT = true;
    static constexpr int RW = ROT ? 2 : 1;
    __host__ __device__ static size_t slots(int P, int G) { return (size_t)P * G * RW + ((size_t)P + 3) / 4; }
    __device__ static const float* totals(const MpDims& d, const float4* rec) {
        return reinterpret_cast<const float*>(rec + (size_t)d.P * d.G * RW);
    }

    // every group's target mean and size (one thread per group, its residues in motif order), then the target centred per group in
    // place.  Ends with the block in step.
    __device__ __forceinline__ void stage(const MpLds& L, const MpDims& d) {
        if ((int)threadIdx.x < d.G) {
            const int g = threadIdx.x;
            float tx = 0.f, ty = 0.f, tz = 0.f;
            int cnt = 0;
            for (int s = 0; s < d.S; ++s) {
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
        for (int m = threadIdx.x; m < d.M; m += MP_THREADS) {
            int g = 0;
            for (int s = 0; s < d.S; ++s)
                if ((unsigned)(m - L.so[s]) < (unsigned)L.sl[s]) g = L.sg[s];
            L.tg[3 * m] -= L.gm[3 * g];
            L.tg[3 * m + 1] -= L.gm[3 * g + 1];
            L.tg[3 * m + 2] -= L.gm[3 * g + 2];
        }
        __syncthreads();
    }
    __device__ __forceinline__ void record(const MpLds& L, const MpDims& d, const int32_t* __restrict__ st, float4* rec, int p) const {
        float4* out = rec + (size_t)p * d.G * RW;
        float qp = 0.f;
        for (int g = 0; g < d.G; ++g) {
            const MpFit r = mp_fit<false, ROT, false>(L, st, d.S, g, (float)L.gn[g], MpVec{0.f, 0.f, 0.f});
            if (ROT) out[2 * g + 1] = r.quat;
            out[RW * g] = r.fit;
            qp += r.fit.x;
        }
        const_cast<float*>(totals(d, rec))[p] = qp;
    }
    __device__ __forceinline__ float q(const MpDims& d, const float4* rec, int p) const { return totals(d, rec)[p]; }
    __device__ __forceinline__ float score(const MpDims& d, const float4* rec, int p) const { return -totals(d, rec)[p] / d.two_var; }
    __device__ __forceinline__ float group_q(const MpDims& d, const float4* rec, int p, int g) const {
        return rec[((size_t)p * d.G + g) * RW].x;
    }
    __device__ __forceinline__ MpVec residual(const MpLds& L, const MpDims& d, const float4* rec, int p, int m, int g, MpVec xn) const {
        const float4* rg = rec + ((size_t)p * d.G + g) * RW;
        const float4 rp = rg[0];
        const float* t = L.tg + 3 * m;
        const MpVec rt = ROT ? mr_apply(mr_rotation(rg[1]), t[0], t[1], t[2]) : MpVec{t[0], t[1], t[2]};
        return MpVec{(xn.x - rp.y) - rt.x, (xn.y - rp.z) - rt.y, (xn.z - rp.w) - rt.z};
    }
};

// ---- the skeleton ----------------------------------------------------------------------------------------------------------------
// carve and stage: what both kernels begin with.  Ends with everything a record needs in LDS and visible.
template <class Form>
__device__ __forceinline__ void mp_begin(unsigned char* smem, size_t slots, const float* __restrict__ x0b, const float* __restrict__ target,
                                         const int32_t* __restrict__ seg_len, const int32_t* __restrict__ seg_group, const MpDims& d,
                                         MpLds& L, Form& f) {
    L = mp_carve(smem, d.N, d.M, d.S, d.G, slots);
    mp_stage<Form::GROUPED>(L, x0b, target, seg_len, seg_group, d.N, d.M, d.S, d.G);
    __syncthreads();
    f.stage(L, d);
}

// large-P path, first launch: one placement per thread, records to work[b]
template <class Form>
__global__ __launch_bounds__(MP_THREADS) void k_motif_records(const float* __restrict__ x0, int N, int P, int S, int M, int G,
                                                              const int32_t* __restrict__ seg_len, const int32_t* __restrict__ seg_group,
                                                              const int32_t* __restrict__ starts, const float* __restrict__ target,
                                                              const float* __restrict__ var_p, float4* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    const int b = blockIdx.y;
    const float var = *var_p;
    const MpDims d = {N, P, S, M, Form::GROUPED ? G : 0, var, 2.f * var};
    MpLds L;
    Form f;
    mp_begin(mp_smem, 0, x0 + (size_t)b * 3 * N, target, seg_len, seg_group, d, L, f);          // (act / wcnt unused here)
    const int p = blockIdx.x * MP_THREADS + threadIdx.x;
    if (p < P) f.record(L, d, starts + (size_t)p * S, work + (size_t)b * Form::slots(P, d.G), p);
}

template <class Form, bool SPILL>
__global__ __launch_bounds__(MP_THREADS) void k_motif(const float* __restrict__ x0, int N, int P, int S, int M, int G,
                                                      const int32_t* __restrict__ seg_len, const int32_t* __restrict__ seg_group,
                                                      const int32_t* __restrict__ starts, const float* __restrict__ target,
                                                      const float* __restrict__ var_p, const float4* __restrict__ work,
                                                      float* __restrict__ logp, float* __restrict__ grad, int32_t* __restrict__ best,
                                                      float* __restrict__ rmsd, float* __restrict__ group_rmsd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float var = *var_p;
    const MpDims d = {N, P, S, M, Form::GROUPED ? G : 0, var, 2.f * var};
    MpLds L;
    Form f;
    mp_begin(mp_smem, SPILL ? 0 : Form::slots(P, d.G), x0 + (size_t)b * 3 * N, target, seg_len, seg_group, d, L, f);
    if (!SPILL)
        for (int p = tid; p < P; p += MP_THREADS) f.record(L, d, starts + (size_t)p * S, L.rec, p);
    const float4* rec = SPILL ? work + (size_t)b * Form::slots(P, d.G) : L.rec;
    __syncthreads();

    // logsumexp with the max taken first: late in the trajectory scores reach -1e5 and the softmax is one-hot
    float mx = -INFINITY;
    for (int p = tid; p < P; p += MP_THREADS) mx = fmaxf(mx, f.score(d, rec, p));
    mx = mp_block_max(mx, L.red);
    float se = 0.f;
    for (int p = tid; p < P; p += MP_THREADS) se += expf(f.score(d, rec, p) - mx);
    se = mp_block_sum(se, L.red);
    if (logp && blockIdx.x == 0 && tid == 0) logp[b] = mx + logf(se) - logf((float)P);

    // the lowest placement that reaches the max, its RMSD and that of every group in it
    if constexpr (Form::HAS_FIT) {
        if (best || rmsd || group_rmsd) {
            int bp = P;
            for (int p = tid; p < P; p += MP_THREADS)
                if (p < bp && f.score(d, rec, p) == mx) bp = p;
            bp = mp_block_min(bp, L.wcnt);
            if (bp >= P) bp = 0;                                  // (only a non-finite input gets here)
            if (blockIdx.x == 0) {
                if (tid == 0 && best) best[b] = bp;
                if (tid == 0 && rmsd) rmsd[b] = sqrtf(f.q(d, rec, bp) / (float)M);
                if constexpr (Form::GROUPED)
                    if (tid < d.G && group_rmsd) group_rmsd[(size_t)b * d.G + tid] = sqrtf(f.group_q(d, rec, bp, tid) / (float)L.gn[tid]);
            }
            __syncthreads();                                      // (wcnt is used again below)
        }
    }
    if (!grad) return;                                            // a fit only: nothing to gather

    // the placements whose weight is not exactly 0, in ascending order (late in the trajectory that is one or a few): ballot +
    // prefix count per wave, per 256-placement chunk.  If there are more than the list holds, the gather walks every placement.
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int cap = mp_act_cap(P);
    int cnt = 0;
    for (int c0 = 0; c0 < P; c0 += MP_THREADS) {
        const int p = c0 + tid;
        const bool on = p < P && expf(f.score(d, rec, p) - mx) != 0.f;
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
    const MpVec xn = {live ? L.xs[3 * n] : 0.f, live ? L.xs[3 * n + 1] : 0.f, live ? L.xs[3 * n + 2] : 0.f};
    const int k0 = (int)((int64_t)K * w / MP_WAVES), k1 = (int)((int64_t)K * (w + 1) / MP_WAVES);
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int c0 = k0; c0 < k1; c0 += MP_CHUNK) {
        const int c1 = min(c0 + MP_CHUNK, k1);
        float bx = 0.f, by = 0.f, bz = 0.f;
        for (int k = c0; k < c1; ++k) {
            const int p = __builtin_amdgcn_readfirstlane(listed ? L.act[k] : k);
            const float e = expf(f.score(d, rec, p) - mx);    // bitwise the term of `se`
            if (e == 0.f) continue;                           // (wave-uniform)
            const int32_t* st = starts + (size_t)p * S;
            int m = -1, g = 0;
            for (int s = 0; s < S; ++s) {
                const int dn = n - st[s];
                if ((unsigned)dn < (unsigned)L.sl[s]) {
                    m = L.so[s] + dn;
                    if (Form::GROUPED) g = L.sg[s];
                }
            }
            if (m >= 0) {
                const MpVec r = f.residual(L, d, rec, p, m, g, xn);
                bx += e * r.x;
                by += e * r.y;
                bz += e * r.z;
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
        float* out = grad + ((size_t)b * N + n) * 3;
        out[0] = gx * sc;
        out[1] = gy * sc;
        out[2] = gz * sc;
    }
}

// the arguments of one call, as the entries take them (what a form lacks is 0 / NULL)
struct MpCall {
    int B, N;
    const float* x0;
    int P, S, M, G;
    const int32_t *seg_len, *seg_group, *starts;
    const float *target, *var;
    float *logp, *grad;
    int32_t* best;
    float *rmsd, *group_rmsd;
    void* work;
    size_t work_bytes;
};

// `need`: the form's *_work_bytes for this call; above 0 the records spill to `work` (checked here) and a first launch writes them
template <class Form>
int mp_launch(genie_stream_t stream, const MpCall& c, size_t need) {
    const bool spill = need > 0;
    if (spill && (!c.work || c.work_bytes < need || (reinterpret_cast<uintptr_t>(c.work) & 15))) return GENIE_E_ARG;
    const size_t lds = mp_lds_bytes(c.N, c.M, c.S, c.G, c.P, spill ? 0 : Form::slots(c.P, c.G));
    if (lds > MP_LDS_MAX) return GENIE_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(c.grad ? (c.N + MP_TILE - 1) / MP_TILE : 1, c.B);          // without a gradient there is nothing to tile
    auto main_kernel = spill ? k_motif<Form, true> : k_motif<Form, false>;
    if (lds > 64 * 1024) {
        if (spill)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_motif_records<Form>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(main_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    float4* rec = spill ? static_cast<float4*>(c.work) : nullptr;
    if (spill)
        hipLaunchKernelGGL(k_motif_records<Form>, dim3((c.P + MP_THREADS - 1) / MP_THREADS, c.B), dim3(MP_THREADS), lds, st, c.x0, c.N, c.P,
                           c.S, c.M, c.G, c.seg_len, c.seg_group, c.starts, c.target, c.var, rec);
    hipLaunchKernelGGL(main_kernel, grid, dim3(MP_THREADS), lds, st, c.x0, c.N, c.P, c.S, c.M, c.G, c.seg_len, c.seg_group, c.starts,
                       c.target, c.var, (const float4*)rec, c.logp, c.grad, c.best, c.rmsd, c.group_rmsd);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}

}  // namespace

size_t genie_motif_potential_work_bytes(int B, int P) {
    return (B >= 1 && P > MP_LDS_P) ? (size_t)B * Translate::slots(P, 0) * sizeof(float4) : 0;
}

int genie_motif_potential(genie_stream_t stream, int B, int N, const float* x0, int P, int S, int M, const int32_t* seg_len,
                          const int32_t* starts, const float* target, const float* var, float* logp_out, float* grad_out, void* work,
                          size_t work_bytes) {
    if (!x0 || !seg_len || !starts || !target || !var || !logp_out || !grad_out) return GENIE_E_ARG;
    if (B < 1 || B > 65535 || N < 1 || P < 1 || S < 1 || M < 1 || M > N || S > M || (int64_t)P * S > INT32_MAX) return GENIE_E_ARG;
    const MpCall c = {B, N, x0, P, S, M, 0, seg_len, nullptr, starts, target, var, logp_out, grad_out, nullptr, nullptr, nullptr, work,
                      work_bytes};
    return mp_launch<Translate>(stream, c, genie_motif_potential_work_bytes(B, P));
}

size_t genie_motif_potential_rigid_work_bytes(int B, int P) {
    return (B >= 1 && P > MR_LDS_P) ? (size_t)B * Rigid::slots(P, 0) * sizeof(float4) : 0;
}

int genie_motif_potential_rigid(genie_stream_t stream, int B, int N, const float* x0, int P, int S, int M, const int32_t* seg_len,
                                const int32_t* starts, const float* target, const float* var, float* logp_out, float* grad_out,
                                int32_t* best_out, float* rmsd_out, void* work, size_t work_bytes) {
    if (!x0 || !seg_len || !starts || !target || !var) return GENIE_E_ARG;
    if ((logp_out == nullptr) != (grad_out == nullptr) || (!logp_out && !best_out && !rmsd_out)) return GENIE_E_ARG;
    if (B < 1 || B > 65535 || N < 1 || P < 1 || S < 1 || M < 3 || M > N || S > M || (int64_t)P * S > INT32_MAX) return GENIE_E_ARG;
    const MpCall c = {B, N, x0, P, S, M, 0, seg_len, nullptr, starts, target, var, logp_out, grad_out, best_out, rmsd_out, nullptr, work,
                      work_bytes};
    return mp_launch<Rigid>(stream, c, genie_motif_potential_rigid_work_bytes(B, P));
}

size_t genie_motif_potential_grouped_work_bytes(int B, int P, int G, int align) {
    if (B < 1 || P < 1 || G < 1 || G > GENIE_MOTIF_MAX_GROUPS || (align != 0 && align != 1)) return 0;
    const size_t bytes = (align ? Grouped<true>::slots(P, G) : Grouped<false>::slots(P, G)) * sizeof(float4);
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
    const MpCall c = {B, N, x0, P, S, M, G, seg_len, seg_group, starts, target, var, logp_out, grad_out, best_out, rmsd_out, group_rmsd_out,
                      work, work_bytes};
    const size_t need = genie_motif_potential_grouped_work_bytes(B, P, G, align);
    return align ? mp_launch<Grouped<true>>(stream, c, need) : mp_launch<Grouped<false>>(stream, c, need);
}
