// Symmetry potential of twisted-diffusion / SMC sampling (include/genie_hip.h: genie_symmetry_potential): how far a chain is from
// repeating itself under one or two generators -- the n-fold of a cyclic oligomer or a closed toroid, the n-fold and the two-fold of a
// dihedral one, the screw of an open repeat -- with its gradient and a per-particle report, in one launch instead of a PyTorch
// callable with an SVD inside the sampling loop.  The reference has no counterpart.
//
// A generator g is a list of pairs (src_i, dst_i), given as the per-residue table partner[g][0][n] (the residue n maps to, as a
// source) and partner[g][1][n] (the residue that maps to n), -1 for none.  For particle b with coordinates x_n:
//   c_s = mean x[src],  c_d = mean x[dst],  p_i = x[src_i] - c_s,  q_i = x[dst_i] - c_d
//   R_g = argmin over proper rotations of sum_i |q_i - R p_i|^2      (Horn's quaternion of sum_i p_i q_i^T, horn.h)
//   E_g = sum_i |q_i - R_g p_i|^2                                    (summed from the residuals: near symmetry |q|^2 + |p|^2 - 2 lambda
//                                                                     has no digits left)
//   logp[b] = -sum_g w_g E_g / (2 var)
//   grad[b, dst_i] += -w_g (q_i - R_g p_i) / var,   grad[b, src_i] += w_g R_g^T (q_i - R_g p_i) / var
// (R_g held at its optimum: E does not move with R to first order, and the residuals sum to 0, so the centroids drop out.)
//
// k_symmetry: grid B, 256 threads: one work-group per particle stages x0[b] in LDS (12 N bytes) and makes three strided passes over
// the residues, both generators in each.  Pass 1 sums x[src] and x[dst] - x[src] (c_d = c_s + their mean: for a closed ring the two
// sets are the same and the difference of two separately rounded means would be noise) and counts the pairs; pass 2 sums the nine
// correlation entries; wave g then finds the quaternion of generator g (wave-uniform work, the two generators side by side); pass 3
// forms, per residue, the residual of its pair as a source and of its pair as a destination, adds the squares of the first to E_g
// and writes the residue's gradient.  A residue has at most one role of each kind per generator, so the gradient is a gather: no
// atomics, no scatter.  Every block sum is a butterfly inside each wave and the four wave results added in wave order, so two calls
// on the same inputs are bitwise equal.  Table entries index LDS: they are clamped into 0..N-1 (negative: none).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"
#include "horn.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int SYM_THREADS = 256;
constexpr int SYM_WAVES = SYM_THREADS / 64;
constexpr int SYM_G = GENIE_SYMMETRY_MAX_GENERATORS;
constexpr int SYM_SUMS = 9;             // the widest block sum, per generator: the correlation
constexpr size_t SYM_LDS_MAX = 160 * 1024;

struct SymVec {
    float x, y, z;
};

// dynamic LDS: [xs: 3N] [part: WAVES * G * SUMS] [quat: 4 G]
size_t sym_lds_bytes(int N) { return sizeof(float) * (3 * (size_t)N + SYM_WAVES * SYM_G * SYM_SUMS + 4 * SYM_G); }

__device__ inline SymVec sym_row(const float* xs, int i) { return {xs[3 * i], xs[3 * i + 1], xs[3 * i + 2]}; }

// entry n of a role's table: the partner clamped into 0..N-1, or -1 for none
__device__ inline int sym_partner(const int32_t* __restrict__ table, int n, int N) {
    const int p = table[n];
    return p < 0 ? -1 : min(p, N - 1);
}

// the block's sums of v[g][0..K-1], in a fixed tree: butterfly inside each wave, then the wave results in wave order.  Every thread
// gets the same bits.  (Two barriers: `part` is free again when it returns.)
template <int K>
__device__ inline void sym_block_sum(float (&v)[SYM_G][K], int G, float* part) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int g = 0; g < SYM_G; ++g)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (g >= G) continue;
            float s = v[g][k];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) part[(w * SYM_G + g) * SYM_SUMS + k] = s;
        }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < SYM_G; ++g)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (g >= G) continue;
            float s = part[g * SYM_SUMS + k];
            for (int u = 1; u < SYM_WAVES; ++u) s += part[(u * SYM_G + g) * SYM_SUMS + k];
            v[g][k] = s;
        }
    __syncthreads();
}

__global__ __launch_bounds__(SYM_THREADS) void k_symmetry(const float* __restrict__ x0, int N, int G, const int32_t* __restrict__ partner,
                                                          float w0, float w1, const float* __restrict__ var_p, float* __restrict__ logp,
                                                          float* __restrict__ grad, float* __restrict__ report) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sym_smem[];
    float* xs = reinterpret_cast<float*>(sym_smem);
    float* part = xs + 3 * (size_t)N;
    float* quat = part + SYM_WAVES * SYM_G * SYM_SUMS;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* x0b = x0 + (size_t)b * 3 * N;
    for (int i = tid; i < 3 * N; i += SYM_THREADS) xs[i] = x0b[i];
    __syncthreads();
    const float wg[SYM_G] = {w0, w1};

    // pass 1: sum x[src], sum (x[dst] - x[src]) and the number of pairs
    float s1[SYM_G][7];
    for (int g = 0; g < SYM_G; ++g)
        for (int k = 0; k < 7; ++k) s1[g][k] = 0.f;
#pragma unroll
    for (int g = 0; g < SYM_G; ++g) {
        if (g >= G) break;
        const int32_t* to = partner + (size_t)g * 2 * N;
        for (int n = tid; n < N; n += SYM_THREADS) {
            const int d = sym_partner(to, n, N);
            if (d < 0) continue;
            const SymVec a = sym_row(xs, n), c = sym_row(xs, d);
            s1[g][0] += a.x;
            s1[g][1] += a.y;
            s1[g][2] += a.z;
            s1[g][3] += c.x - a.x;
            s1[g][4] += c.y - a.y;
            s1[g][5] += c.z - a.z;
            s1[g][6] += 1.f;
        }
    }
    sym_block_sum<7>(s1, G, part);
    SymVec cs[SYM_G], cd[SYM_G], shift[SYM_G];
    float len[SYM_G];
#pragma unroll
    for (int g = 0; g < SYM_G; ++g) {
        len[g] = g < G ? s1[g][6] : 0.f;
        const float l = len[g] > 0.f ? len[g] : 1.f;                 // (divided, not scaled by 1 / l: equal points have their own mean)
        cs[g] = {s1[g][0] / l, s1[g][1] / l, s1[g][2] / l};
        shift[g] = {s1[g][3] / l, s1[g][4] / l, s1[g][5] / l};
        cd[g] = {cs[g].x + shift[g].x, cs[g].y + shift[g].y, cs[g].z + shift[g].z};
    }

    // pass 2: the correlation sum_i p_i q_i^T
    float s2[SYM_G][9];
    for (int g = 0; g < SYM_G; ++g)
        for (int k = 0; k < 9; ++k) s2[g][k] = 0.f;
#pragma unroll
    for (int g = 0; g < SYM_G; ++g) {
        if (g >= G) break;
        const int32_t* to = partner + (size_t)g * 2 * N;
        for (int n = tid; n < N; n += SYM_THREADS) {
            const int d = sym_partner(to, n, N);
            if (d < 0) continue;
            const SymVec a = sym_row(xs, n), c = sym_row(xs, d);
            const float px = a.x - cs[g].x, py = a.y - cs[g].y, pz = a.z - cs[g].z;
            const float qx = c.x - cd[g].x, qy = c.y - cd[g].y, qz = c.z - cd[g].z;
            s2[g][0] += px * qx;
            s2[g][1] += px * qy;
            s2[g][2] += px * qz;
            s2[g][3] += py * qx;
            s2[g][4] += py * qy;
            s2[g][5] += py * qz;
            s2[g][6] += pz * qx;
            s2[g][7] += pz * qy;
            s2[g][8] += pz * qz;
        }
    }
    sym_block_sum<9>(s2, G, part);

    // the rotations: wave g solves generator g
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (w < G) {
        float s[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = w == 0 ? s2[0][k] : s2[1][k];
        const float4 q = mr_quaternion(MrMat{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8]});
        if ((tid & 63) == 0) {
            quat[4 * w] = q.x;
            quat[4 * w + 1] = q.y;
            quat[4 * w + 2] = q.z;
            quat[4 * w + 3] = q.w;
        }
    }
    __syncthreads();
    float4 qt[SYM_G];
    MrMat R[SYM_G];
#pragma unroll
    for (int g = 0; g < SYM_G; ++g) {
        qt[g] = g < G ? make_float4(quat[4 * g], quat[4 * g + 1], quat[4 * g + 2], quat[4 * g + 3]) : make_float4(1.f, 0.f, 0.f, 0.f);
        R[g] = mr_rotation(qt[g]);
    }

    // pass 3: the residuals, E_g from a residue's pair as a source, the gradient from both of its roles
    const float sc = -1.f / (2.f * *var_p);
    float s3[SYM_G][1] = {{0.f}, {0.f}};
    for (int n = tid; n < N; n += SYM_THREADS) {
        const SymVec a = sym_row(xs, n);
        float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
        for (int g = 0; g < SYM_G; ++g) {
            if (g >= G) break;
            const int32_t* to = partner + (size_t)g * 2 * N;
            const MrMat& M = R[g];
            const int d = sym_partner(to, n, N), s = sym_partner(to + N, n, N);
            if (d >= 0) {                                           // n is a source: e = q - R p, dE / dx_n = -2 R^T e
                const SymVec c = sym_row(xs, d);
                const float px = a.x - cs[g].x, py = a.y - cs[g].y, pz = a.z - cs[g].z;
                const float ex = (c.x - cd[g].x) - (M.xx * px + M.xy * py + M.xz * pz);
                const float ey = (c.y - cd[g].y) - (M.yx * px + M.yy * py + M.yz * pz);
                const float ez = (c.z - cd[g].z) - (M.zx * px + M.zy * py + M.zz * pz);
                s3[g][0] += ex * ex + ey * ey + ez * ez;
                gx -= 2.f * wg[g] * (M.xx * ex + M.yx * ey + M.zx * ez);
                gy -= 2.f * wg[g] * (M.xy * ex + M.yy * ey + M.zy * ez);
                gz -= 2.f * wg[g] * (M.xz * ex + M.yz * ey + M.zz * ez);
            }
            if (s >= 0) {                                           // n is a destination: dE / dx_n = 2 e
                const SymVec c = sym_row(xs, s);
                const float px = c.x - cs[g].x, py = c.y - cs[g].y, pz = c.z - cs[g].z;
                gx += 2.f * wg[g] * ((a.x - cd[g].x) - (M.xx * px + M.xy * py + M.xz * pz));
                gy += 2.f * wg[g] * ((a.y - cd[g].y) - (M.yx * px + M.yy * py + M.yz * pz));
                gz += 2.f * wg[g] * ((a.z - cd[g].z) - (M.zx * px + M.zy * py + M.zz * pz));
            }
        }
        if (grad) {
            float* out = grad + ((size_t)b * N + n) * 3;
            out[0] = sc * gx + 0.f;                                 // (+ 0: a free residue's gradient is +0, not -0)
            out[1] = sc * gy + 0.f;
            out[2] = sc * gz + 0.f;
        }
    }
    sym_block_sum<1>(s3, G, part);
    if (tid != 0) return;

    float weighted = 0.f, total = 0.f, pairs = 0.f;
#pragma unroll
    for (int g = 0; g < SYM_G; ++g) {
        if (g >= G) break;
        weighted += wg[g] * s3[g][0];
        total += s3[g][0];
        pairs += len[g];
    }
    if (logp) logp[b] = sc * weighted;
    if (!report) return;
    float* r = report + (size_t)b * GENIE_SYMMETRY_REPORT;
    r[0] = weighted;
    r[1] = pairs > 0.f ? sqrtf(total / pairs) : 0.f;
#pragma unroll
    for (int g = 0; g < SYM_G; ++g) {
        float* o = r + 2 + 3 * g;
        if (g >= G || !(len[g] > 0.f)) {
            o[0] = o[1] = o[2] = 0.f;
            continue;
        }
        // angle = 2 atan2(|v|, |w|): no acos, whose slope is unbounded at the 0 and 180 degrees a two-fold sits at.  The axis u is
        // fixed by R, so u . (c_d - R c_s) = u . (c_d - c_s): the rise is taken in that form, without the rounding of R c_s.
        const float vx = qt[g].y, vy = qt[g].z, vz = qt[g].w, vn = sqrtf(vx * vx + vy * vy + vz * vz);
        o[0] = sqrtf(s3[g][0] / len[g]);
        o[1] = 2.f * atan2f(vn, fabsf(qt[g].x)) * 57.29577951308232f;
        o[2] = vn > 0.f ? fabsf(vx * shift[g].x + vy * shift[g].y + vz * shift[g].z) / vn
                        : sqrtf(shift[g].x * shift[g].x + shift[g].y * shift[g].y + shift[g].z * shift[g].z);
    }
}

int sym_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_symmetry_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

bool sym_bad(float v) { return !(v >= 0.f) || isinf(v); }          // negative, NaN or infinite

}  // namespace

size_t genie_symmetry_potential_work_bytes(int B, int N) {
    (void)B, (void)N;
    return 0;           // one work-group holds a particle from the first sum to the gradient: nothing passes through memory
}

int genie_symmetry_potential(genie_stream_t stream, int B, int N, const float* x0, int G, const int32_t* partner, float weight0,
                             float weight1, const float* var, float* logp_out, float* grad_out, float* report_out, void* work,
                             size_t work_bytes) {
    if (B < 1 || B > 65535) return sym_refuse("B outside 1..65535");
    if (N < 1) return sym_refuse("N below 1");
    if (!x0) return sym_refuse("x0 is NULL");
    if (G < 1 || G > SYM_G) return sym_refuse("G outside 1..2");
    if (!partner) return sym_refuse("partner is NULL");
    if (sym_bad(weight0)) return sym_refuse("weight0 negative or not finite");
    if (sym_bad(weight1)) return sym_refuse("weight1 negative or not finite");
    if (!var) return sym_refuse("var is NULL");
    if (!logp_out && !grad_out && !report_out) return sym_refuse("no output asked for (logp_out, grad_out and report_out are NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return sym_refuse("logp_out and grad_out are given together or both NULL");
    if (work_bytes < genie_symmetry_potential_work_bytes(B, N) || (work_bytes > 0 && !work))
        return sym_refuse("work is NULL with work_bytes above 0, or work_bytes below genie_symmetry_potential_work_bytes(B, N)");
    const size_t lds = sym_lds_bytes(N);
    if (lds > SYM_LDS_MAX) return sym_refuse("N too large: the staging of x0[b] does not fit in LDS");
    hipStream_t st = (hipStream_t)stream;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(k_symmetry), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return GENIE_E_HIP;
    hipLaunchKernelGGL(k_symmetry, dim3(B), dim3(SYM_THREADS), lds, st, x0, N, G, partner, weight0, G > 1 ? weight1 : 0.f, var, logp_out,
                       grad_out, report_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
