// Secondary-structure potential of twisted-diffusion / SMC sampling (include/genie_hip.h: genie_secstruct_potential): soft helix and
// extended content bounds and an optional per-residue blueprint, scored on C-alpha geometry alone, with their gradient, a per-particle
// report and a hard H / E / C assignment, in one launch instead of a PyTorch callable and an autograd walk back through it.  The
// reference has no differentiable counterpart: genie/sampler/secstruct.py writes a PDB and runs P-SEA on the host.
//
// For particle b with coordinates x_n, n = 0..N-1 (all N rows: the twisted sampler's batches are never ragged) there are W = N - 4
// windows; window i covers residues i..i+4 and has four features
//   d2 = |x_{i+2} - x_i|,  d3 = |x_{i+3} - x_i|,  d4 = |x_{i+4} - x_i|,
//   chi = ((b1 x b2) . b3) / (|b1| |b2| |b3|),   b_k = x_{i+k} - x_{i+k-1}
// and for class c in {H, E}, with the table's targets mu and tolerances sigma,
//   z_cf = (f - mu_cf) / sigma_cf,   u_c,i = 1/4 sum_f z_cf^2,   s_c,i = 1 / (1 + u_c,i),   n_c = sum_i s_c,i
//   E_c   = w_c [ (W f_c^min - n_c)_+^2 + (n_c - W f_c^max)_+^2 ]
//   E_tgt = w_T sum_{i targeted as c} u_c,i          (window i is targeted as c when target[i..i+4] all equal c)
//   logp[b] = -(E_H + E_E + E_tgt) / (2 var)
//   dE/dx = sum_i sum_f C_f,i df_i/dx,   C_f,i = sum_c A_c,i z_cf / (2 sigma_cf),
//   A_c,i = -2 w_c [ (n_c - W f_c^max)_+ - (W f_c^min - n_c)_+ ] s_c,i^2 + w_T [i targeted as c]
// A distance that is exactly 0 has direction 0; a window with any |b_k| = 0 has chi = 0 and no chi force: every output is finite.
//
// k_secstruct: grid B, 256 threads, one work-group per particle (everything is O(N)).  It stages x0[b] in LDS, computes the four
// features, the hard class and the target class of every window (one window per thread, strided) into LDS, reduces n_H, n_E and
// E_tgt in a fixed tree (butterfly inside each wave, then the waves in wave order), turns each window's features into its four
// coefficients C_f,i in place (the same thread owns the same windows), and then gathers: one residue per thread, strided, walks the
// at most 5 windows that contain it, the window that starts at it first, adding C_f,i df_i/dx_n and taking the union of their hard
// classes.  A second fixed tree adds the residue counts; thread 0 writes logp and the report.
// No atomics, no scatter, no work buffer: every output is written once, in a fixed order, so two calls on the same inputs are
// bitwise equal.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int SS_THREADS = 256;
constexpr int SS_WAVES = SS_THREADS / 64;
constexpr size_t SS_LDS_MAX = 160 * 1024;
constexpr int SS_HARD_H = 1, SS_HARD_E = 2;        // bits 0-1 of a window's flags: its hard classes; bits 2-3: its target class

struct SsParams {
    float mu[2][4], sigma[2][4];                    // [class H, E][d2, d3, d4, chi]
    float lo[2], hi[2], weight[2];                  // content bounds (fractions) and weights
    float target_weight;
    int W;
};

// dynamic LDS: [xs: 3N] [feat: 4W] [flags: W] [red: WAVES]
size_t ss_lds_bytes(int N) { return sizeof(float) * (3 * (size_t)N + 5 * ((size_t)N - 4) + SS_WAVES); }

__device__ inline float ss_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int ss_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum in a fixed tree: butterfly inside each wave, then the wave results in wave order (every thread gets the same bits)
__device__ inline float ss_block_sum(float v, float* red) {
    v = ss_wave_sum(v);
    __syncthreads();                                            // (red is free again)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < SS_WAVES; ++w) r += red[w];
    return r;
}

__device__ inline int ss_block_sum(int v, float* red) {
    v = ss_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = __int_as_float(v);
    __syncthreads();
    int r = __float_as_int(red[0]);
    for (int w = 1; w < SS_WAVES; ++w) r += __float_as_int(red[w]);
    return r;
}

struct SsVec {
    float x, y, z;
};

__device__ inline SsVec ss_sub(const float* a, const float* b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
__device__ inline SsVec ss_cross(SsVec a, SsVec b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline float ss_dot(SsVec a, SsVec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline float ss_len(SsVec a) { return sqrtf(ss_dot(a, a)); }

// chi of the window whose first residue is at p (p[0..11]: residues 0..3), 0 where a bond has length 0
__device__ inline float ss_chi(const float* p) {
    const SsVec b1 = ss_sub(p + 3, p), b2 = ss_sub(p + 6, p + 3), b3 = ss_sub(p + 9, p + 6);
    const float l = ss_len(b1) * ss_len(b2) * ss_len(b3);
    return l > 0.f ? ss_dot(ss_cross(b1, b2), b3) / l : 0.f;
}

// sum_f C_f df/dx_k of one window (p: its first residue, c: its four coefficients) for the residue at position k = 0..4 in it
__device__ inline SsVec ss_window_force(const float* p, const float* c, int k) {
    SsVec f = {0.f, 0.f, 0.f};
    // the distances: d_m = |p_m - p_0| pulls on residue m (+) and on residue 0 (-)
    for (int m = 2; m <= 4; ++m) {
        if (k != 0 && k != m) continue;
        const SsVec d = ss_sub(p + 3 * m, p);
        const float len = ss_len(d);
        const float g = len > 0.f ? (k == 0 ? -c[m - 2] : c[m - 2]) / len : 0.f;       // (coincident residues: no direction)
        f.x += g * d.x;
        f.y += g * d.y;
        f.z += g * d.z;
    }
    if (k == 4) return f;
    // chi = T / L, T = (b1 x b2) . b3, L = |b1| |b2| |b3|:  dchi/db_j = (dT/db_j) / L - chi b_j / |b_j|^2
    const SsVec b1 = ss_sub(p + 3, p), b2 = ss_sub(p + 6, p + 3), b3 = ss_sub(p + 9, p + 6);
    const float q1 = ss_dot(b1, b1), q2 = ss_dot(b2, b2), q3 = ss_dot(b3, b3);
    const float l = sqrtf(q1) * sqrtf(q2) * sqrtf(q3);
    if (!(l > 0.f)) return f;
    const float chi = ss_dot(ss_cross(b1, b2), b3) / l, il = 1.f / l;
    const SsVec t1 = ss_cross(b2, b3), t2 = ss_cross(b3, b1), t3 = ss_cross(b1, b2);
    const float r1 = chi / q1, r2 = chi / q2, r3 = chi / q3;
    const SsVec g1 = {t1.x * il - r1 * b1.x, t1.y * il - r1 * b1.y, t1.z * il - r1 * b1.z};
    const SsVec g2 = {t2.x * il - r2 * b2.x, t2.y * il - r2 * b2.y, t2.z * il - r2 * b2.z};
    const SsVec g3 = {t3.x * il - r3 * b3.x, t3.y * il - r3 * b3.y, t3.z * il - r3 * b3.z};
    SsVec g;
    if (k == 0) g = {-g1.x, -g1.y, -g1.z};
    else if (k == 1) g = {g1.x - g2.x, g1.y - g2.y, g1.z - g2.z};
    else if (k == 2) g = {g2.x - g3.x, g2.y - g3.y, g2.z - g3.z};
    else g = g3;
    f.x += c[3] * g.x;
    f.y += c[3] * g.y;
    f.z += c[3] * g.z;
    return f;
}

__device__ inline int ss_code(int8_t t) { return t == 1 ? 1 : (t == 2 ? 2 : 0); }

__global__ __launch_bounds__(SS_THREADS) void k_secstruct(const float* __restrict__ x0, int N, SsParams q,
                                                          const int8_t* __restrict__ target, const float* __restrict__ var_p,
                                                          float* __restrict__ logp, float* __restrict__ grad,
                                                          float* __restrict__ report, int8_t* __restrict__ assign) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ss_smem[];
    const int W = q.W;
    float* xs = reinterpret_cast<float*>(ss_smem);
    float* feat = xs + 3 * (size_t)N;                           // feat[4 i + f]: the features, later the coefficients C_f,i
    int* flags = reinterpret_cast<int*>(feat + 4 * (size_t)W);
    float* red = reinterpret_cast<float*>(flags + W);
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* x0b = x0 + (size_t)b * 3 * N;
    for (int i = tid; i < 3 * N; i += SS_THREADS) xs[i] = x0b[i];
    __syncthreads();

    // windows: features, soft scores, hard and target classes
    float sh = 0.f, se = 0.f, et = 0.f;
    for (int i = tid; i < W; i += SS_THREADS) {
        const float* p = xs + 3 * i;
        float f[4];
        f[0] = ss_len(ss_sub(p + 6, p));
        f[1] = ss_len(ss_sub(p + 9, p));
        f[2] = ss_len(ss_sub(p + 12, p));
        f[3] = ss_chi(p);
        float u[2];
        int flag = 0;
        for (int c = 0; c < 2; ++c) {
            float acc = 0.f;
            bool inside = true;
            for (int k = 0; k < 4; ++k) {
                const float z = (f[k] - q.mu[c][k]) / q.sigma[c][k];
                acc += z * z;
                inside = inside && fabsf(z) <= 1.f;
            }
            u[c] = 0.25f * acc;
            if (inside) flag |= c == 0 ? SS_HARD_H : SS_HARD_E;
        }
        sh += 1.f / (1.f + u[0]);
        se += 1.f / (1.f + u[1]);
        if (target) {
            const int t = ss_code(target[i]);
            bool same = t != 0;
            for (int k = 1; k < 5; ++k) same = same && ss_code(target[i + k]) == t;
            if (same) {
                flag |= t << 2;
                et += u[t - 1];
            }
        }
        for (int k = 0; k < 4; ++k) feat[4 * i + k] = f[k];
        flags[i] = flag;
    }
    const float n_h = ss_block_sum(sh, red), n_e = ss_block_sum(se, red), u_t = ss_block_sum(et, red);
    const float n_c[2] = {n_h, n_e};
    float under[2], over[2], a[2];
    for (int c = 0; c < 2; ++c) {
        under[c] = fmaxf((float)W * q.lo[c] - n_c[c], 0.f);
        over[c] = fmaxf(n_c[c] - (float)W * q.hi[c], 0.f);
        a[c] = 2.f * q.weight[c] * (over[c] - under[c]);
    }

    // the windows' coefficients, in place (each thread rewrites the windows it wrote)
    if (grad) {
        for (int i = tid; i < W; i += SS_THREADS) {
            float f[4], coef[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < 4; ++k) f[k] = feat[4 * i + k];
            const int t = flags[i] >> 2;
            for (int c = 0; c < 2; ++c) {
                float z[4], acc = 0.f;
                for (int k = 0; k < 4; ++k) {
                    z[k] = (f[k] - q.mu[c][k]) / q.sigma[c][k];
                    acc += z[k] * z[k];
                }
                const float s = 1.f / (1.f + 0.25f * acc);
                const float A = (t == c + 1 ? q.target_weight : 0.f) - a[c] * s * s;
                for (int k = 0; k < 4; ++k) coef[k] += A * z[k] / (2.f * q.sigma[c][k]);
            }
            for (int k = 0; k < 4; ++k) feat[4 * i + k] = coef[k];
        }
    }
    __syncthreads();

    // residues: gather the force and the hard class over the windows that contain them, the window starting at the residue first
    const float sc = grad ? -1.f / (2.f * *var_p) : 0.f;
    int res_h = 0, res_e = 0, missed = 0;
    for (int n = tid; n < N; n += SS_THREADS) {
        SsVec g = {0.f, 0.f, 0.f};
        int seen = 0;
        for (int k = 0; k < 5; ++k) {
            const int i = n - k;
            if (i < 0 || i >= W) continue;
            seen |= flags[i];
            if (grad) {
                const SsVec f = ss_window_force(xs + 3 * i, feat + 4 * i, k);
                g.x += f.x;
                g.y += f.y;
                g.z += f.z;
            }
        }
        const int cls = (seen & SS_HARD_H) ? 1 : ((seen & SS_HARD_E) ? 2 : 0);
        res_h += cls == 1;
        res_e += cls == 2;
        if (target) {
            const int t = ss_code(target[n]);
            missed += t != 0 && t != cls;
        }
        if (assign) assign[(size_t)b * N + n] = (int8_t)cls;
        if (grad) {
            float* out = grad + ((size_t)b * N + n) * 3;
            out[0] = sc * g.x;
            out[1] = sc * g.y;
            out[2] = sc * g.z;
        }
    }
    if (!logp && !report) return;                               // (uniform: kernel arguments)
    if (report) {
        res_h = ss_block_sum(res_h, red);
        res_e = ss_block_sum(res_e, red);
        missed = ss_block_sum(missed, red);
    }
    if (tid != 0) return;
    float e[2];
    for (int c = 0; c < 2; ++c) e[c] = q.weight[c] * (under[c] * under[c] + over[c] * over[c]);
    const float e_t = q.target_weight * u_t;
    if (logp) logp[b] = -((e[0] + e[1]) + e_t) / (2.f * *var_p);
    if (report) {
        float* r = report + (size_t)b * GENIE_SECSTRUCT_REPORT;
        r[0] = n_h / (float)W;
        r[1] = n_e / (float)W;
        r[2] = (float)res_h;
        r[3] = (float)res_e;
        r[4] = e[0];
        r[5] = e[1];
        r[6] = e_t;
        r[7] = (float)missed;
    }
}

int ss_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_secstruct_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

bool ss_bad(float v) { return !(v >= 0.f) || isinf(v); }           // negative, NaN or infinite

}  // namespace

int genie_secstruct_potential(genie_stream_t stream, int B, int N, const float* x0, const float* table, float helix_min, float helix_max,
                              float helix_weight, float extended_min, float extended_max, float extended_weight, const int8_t* target,
                              float target_weight, const float* var, float* logp_out, float* grad_out, float* report_out,
                              int8_t* assign_out) {
    if (B < 1 || B > 65535) return ss_refuse("B outside 1..65535");
    if (N < 5) return ss_refuse("N below 5 (a window covers five residues)");
    if (!x0) return ss_refuse("x0 is NULL");
    if (!var) return ss_refuse("var is NULL");
    if (!table) return ss_refuse("table is NULL");
    if (!logp_out && !grad_out && !report_out && !assign_out)
        return ss_refuse("no output asked for (logp_out, grad_out, report_out and assign_out are NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return ss_refuse("logp_out and grad_out are given together or both NULL");
    SsParams q;
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 4; ++k) {
            q.mu[c][k] = table[8 * c + k];
            q.sigma[c][k] = table[8 * c + 4 + k];
            if (!isfinite(q.mu[c][k])) return ss_refuse("a target mu of the table is not finite");
            if (!(q.sigma[c][k] > 0.f) || isinf(q.sigma[c][k])) return ss_refuse("a sigma of the table is not positive and finite");
        }
    if (ss_bad(helix_weight)) return ss_refuse("helix_weight negative or not finite");
    if (ss_bad(extended_weight)) return ss_refuse("extended_weight negative or not finite");
    if (ss_bad(target_weight)) return ss_refuse("target_weight negative or not finite");
    if (!(helix_min >= 0.f && helix_max <= 1.f && helix_min <= helix_max))
        return ss_refuse("helix_min, helix_max: needs 0 <= min <= max <= 1");
    if (!(extended_min >= 0.f && extended_max <= 1.f && extended_min <= extended_max))
        return ss_refuse("extended_min, extended_max: needs 0 <= min <= max <= 1");
    if (target_weight > 0.f && !target) return ss_refuse("target_weight > 0 with a NULL target");
    const size_t lds = ss_lds_bytes(N);
    if (lds > SS_LDS_MAX) return ss_refuse("N too large: the staging of x0[b] and its windows does not fit in LDS");
    q.lo[0] = helix_min, q.hi[0] = helix_max, q.weight[0] = helix_weight;
    q.lo[1] = extended_min, q.hi[1] = extended_max, q.weight[1] = extended_weight;
    q.target_weight = target_weight;
    q.W = N - 4;
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_secstruct), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_secstruct, dim3(B), dim3(SS_THREADS), lds, (hipStream_t)stream, x0, N, q, target, var, logp_out, grad_out,
                       report_out, assign_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
