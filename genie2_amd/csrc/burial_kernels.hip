// Burial potential of twisted-diffusion / SMC sampling (include/genie_hip.h: genie_burial_potential): the half-sphere exposure of
// every residue of a C-alpha chain -- the soft number of residues in the half sphere its virtual C-beta direction points into --
// kept in a per-residue range and, averaged over the chain, in a range of its own, with its gradient and a per-particle report, in
// three launches.  It is the one built-in potential that tells inside from outside.  The reference has no counterpart.
//
// For particle b with coordinates x_n, n = 0..N-1:
//   b_n = 2 x_n - x_{n-1} - x_{n+1} (0 at the two ends),  rho_n = sqrt(|b_n|^2 + eps^2),  u_n = b_n / rho_n
//   for |j - n| >= separation:  r = x_j - x_n,  q = |r|^2,  s = 1 / (1 + (q / radius^2)^3),  h = u_n . r,
//                               g = 1/2 (1 + h / sqrt(h^2 + width^2))
//   c_n = sum_j s g,  m = (1/N) sum_n c_n
//   E_res = sum_n w_n [(lo_n - c_n)_+^2 + (c_n - hi_n)_+^2],  E_mean = mean_weight [(mean_min - m)_+^2 + (m - mean_max)_+^2]
//   logp[b] = -(E_res + E_mean) / (2 var)
// With k_n = w_n [(c_n - hi_n)_+ - (lo_n - c_n)_+] + (mean_weight / N) [(m - mean_max)_+ - (mean_min - m)_+],
// f_nj = g ds/dr + s g' u_n (ds/dr = -6 (q / radius^2)^2 s^2 r / radius^2, g' = 1/2 width^2 / (h^2 + width^2)^(3/2)),
// a_n = sum_j s g' r and v_n = (a_n - u_n (u_n . a_n)) / rho_n (0 at the two ends):
//   grad[b,i] = -(1/var) [ sum_n k_n f_ni - k_i sum_j f_ij + 2 k_i v_i - k_{i-1} v_{i-1} - k_{i+1} v_{i+1} ]
//
// k_burial_count: grid (ceil(N / 64), B), 256 threads.  Every work-group stages x and forms u of the whole particle in LDS (24 N
// bytes) and handles 64 centres n, one per lane: each wave walks a contiguous quarter of the neighbours j (wave-uniform j: an LDS
// broadcast) in partial sums of BU_CHUNK, the four wave sums are added in wave order, c_n goes to `work`.
// k_burial_force (only with a gradient): the same grid.  x, u, rho and k of the whole particle are staged (32 N bytes): k needs m,
// which every work-group sums from the c_n in one fixed order.  Lane i walks the pairs again: as the centre it collects a_i and
// sum_j f_ij, as the neighbour of centre j it collects k_j f_ji (skipped, for the whole wave, where k_j = 0).  Wave 0 adds the four
// wave sums in wave order and stores P_i = sum_n k_n f_ni - k_i sum_j f_ij and k_i v_i (6 floats per residue).
// k_burial_finish: grid (ceil(N / 256), B), 256 threads, one residue per thread: the three-residue stencil over k v, the scale by
// -1/var, burial_out; work-group 0 of a particle reduces the c_n in a fixed order and writes logp and the report.
// No atomics, no scatter: every output is written once, in a fixed order, so two calls on the same inputs are bitwise equal.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int BU_THREADS = 256;
constexpr int BU_WAVES = BU_THREADS / 64;
constexpr int BU_TILE = 64;             // centres per work-group of the pair kernels: one per lane
constexpr int BU_CHUNK = 64;            // neighbours per inner partial sum (two-level f32 summation)
constexpr int BU_PART = 10;             // per-lane partials a wave of k_burial_force leaves in LDS: a xyz, D xyz, sum s g', G xyz
constexpr int BU_WORK = 7;              // floats of `work` per (particle, residue): c, P xyz, k v xyz
constexpr size_t BU_LDS_MAX = 64 * 1024;
constexpr float BU_P_FAR = 1e12f;       // q / radius^2 from which p^2 s^2 < 1e-48 is 0 in float32: the force is skipped, no inf * 0

struct BuParams {
    float inv_r2, width2, mean_min, mean_max, mean_weight;
    int separation;
    const float *lo, *hi, *w;           // [N] each, or all NULL
};

// dynamic LDS: k_burial_count [xs: 3N] [us: 3N] [part: THREADS]; k_burial_force [xs: 3N] [us: 3N] [rho: N] [ks: N] [part: PART * THREADS]
size_t bu_count_lds(int N) { return sizeof(float) * (6 * (size_t)N + BU_THREADS); }
size_t bu_force_lds(int N) { return sizeof(float) * (8 * (size_t)N + BU_PART * BU_THREADS); }

__device__ inline float bu_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int bu_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum of one value per thread of a 256-thread work-group, the same bits in every thread: butterfly, then the waves in wave order
__device__ inline float bu_block_sum(float v, float* red) {
    v = bu_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return r;
}

// m of a particle from its c_n, by a 256-thread work-group: thread t adds c_t, c_{t+256}, ... (the one order both kernels use)
__device__ inline float bu_mean(const float* __restrict__ c, int N, float* red) {
    float v = 0.f;
    for (int n = threadIdx.x; n < N; n += BU_THREADS) v += c[n];
    return bu_block_sum(v, red) / (float)N;
}

__device__ inline float bu_mean_k(const BuParams& q, float m, int N) {
    return q.mean_weight > 0.f ? (q.mean_weight / (float)N) * (fmaxf(m - q.mean_max, 0.f) - fmaxf(q.mean_min - m, 0.f)) : 0.f;
}

__device__ inline float bu_k(const BuParams& q, int n, float c, float mean_k) {
    if (!q.w) return mean_k;
    const float w = q.w[n];
    return w > 0.f ? w * (fmaxf(c - q.hi[n], 0.f) - fmaxf(q.lo[n] - c, 0.f)) + mean_k : mean_k;
}

// u_n into us and rho_n (returned) from the staged xs; the two ends have no direction
__device__ inline float bu_direction(const float* xs, float* us, int n, int N) {
    float bx = 0.f, by = 0.f, bz = 0.f;
    if (n >= 1 && n <= N - 2) {
        bx = 2.f * xs[3 * n] - xs[3 * n - 3] - xs[3 * n + 3];
        by = 2.f * xs[3 * n + 1] - xs[3 * n - 2] - xs[3 * n + 4];
        bz = 2.f * xs[3 * n + 2] - xs[3 * n - 1] - xs[3 * n + 5];
    }
    const float rho = sqrtf(bx * bx + by * by + bz * bz + GENIE_BURIAL_EPS * GENIE_BURIAL_EPS);
    us[3 * n] = bx / rho;
    us[3 * n + 1] = by / rho;
    us[3 * n + 2] = bz / rho;
    return rho;
}

// s from q = |r|^2; *dsc with ds/dr = *dsc r (0 from BU_P_FAR on)
__device__ inline float bu_switch(float q2, float inv_r2, float* dsc) {
    const float p = q2 * inv_r2, p2 = p * p;
    const float s = 1.f / (1.f + p2 * p);
    *dsc = p < BU_P_FAR ? -6.f * inv_r2 * p2 * s * s : 0.f;
    return s;
}

// g and g' of h = u . r
__device__ inline float bu_half(float h, float width2, float* gp) {
    const float it = 1.f / sqrtf(h * h + width2);
    *gp = 0.5f * width2 * it * it * it;
    return 0.5f + 0.5f * h * it;
}

__global__ __launch_bounds__(BU_THREADS) void k_burial_count(const float* __restrict__ x0, int N, BuParams q, float* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bu_smem[];
    float* xs = reinterpret_cast<float*>(bu_smem);
    float* us = xs + 3 * (size_t)N;
    float* part = us + 3 * (size_t)N;
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* xb = x0 + (size_t)b * N * 3;
    for (int i = tid; i < 3 * N; i += BU_THREADS) xs[i] = xb[i];
    __syncthreads();
    for (int n = tid; n < N; n += BU_THREADS) (void)bu_direction(xs, us, n, N);
    __syncthreads();

    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n = blockIdx.x * BU_TILE + lane;
    const bool live = n < N;
    const int nn = live ? n : 0;
    const float xn = xs[3 * nn], yn = xs[3 * nn + 1], zn = xs[3 * nn + 2];
    const float ux = us[3 * nn], uy = us[3 * nn + 1], uz = us[3 * nn + 2];
    float c = 0.f;
    const int j0 = (int)((int64_t)N * w / BU_WAVES), j1 = (int)((int64_t)N * (w + 1) / BU_WAVES);
    for (int c0 = j0; c0 < j1; c0 += BU_CHUNK) {
        const int c1 = min(c0 + BU_CHUNK, j1);
        float bc = 0.f;
        for (int j = c0; j < c1; ++j) {
            const float rx = xs[3 * j] - xn, ry = xs[3 * j + 1] - yn, rz = xs[3 * j + 2] - zn;
            float dsc, gp;
            const float s = bu_switch(rx * rx + ry * ry + rz * rz, q.inv_r2, &dsc);
            const float g = bu_half(ux * rx + uy * ry + uz * rz, q.width2, &gp);
            if (live && abs(j - n) >= q.separation) bc += s * g;
        }
        c += bc;
    }
    part[w * 64 + lane] = c;
    __syncthreads();
    if (w != 0 || !live) return;
    work[(size_t)b * N * BU_WORK + n] = ((part[lane] + part[64 + lane]) + part[128 + lane]) + part[192 + lane];
}

__global__ __launch_bounds__(BU_THREADS) void k_burial_force(const float* __restrict__ x0, int N, BuParams q, float* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bu_smem[];
    float* xs = reinterpret_cast<float*>(bu_smem);
    float* us = xs + 3 * (size_t)N;
    float* rhos = us + 3 * (size_t)N;
    float* ks = rhos + N;
    float* part = ks + N;
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* xb = x0 + (size_t)b * N * 3;
    float* wb = work + (size_t)b * N * BU_WORK;
    for (int i = tid; i < 3 * N; i += BU_THREADS) xs[i] = xb[i];
    const float mean_k = bu_mean_k(q, bu_mean(wb, N, part), N);         // (`part` is free until the walk; the barriers order the staging too)
    for (int n = tid; n < N; n += BU_THREADS) {
        rhos[n] = bu_direction(xs, us, n, N);
        ks[n] = bu_k(q, n, wb[n], mean_k);
    }
    __syncthreads();

    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int i = blockIdx.x * BU_TILE + lane;
    const bool live = i < N;
    const int ii = live ? i : 0;
    const float xi = xs[3 * ii], yi = xs[3 * ii + 1], zi = xs[3 * ii + 2];
    const float ux = us[3 * ii], uy = us[3 * ii + 1], uz = us[3 * ii + 2];
    float ax = 0.f, ay = 0.f, az = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, sg = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    const int j0 = (int)((int64_t)N * w / BU_WAVES), j1 = (int)((int64_t)N * (w + 1) / BU_WAVES);
    for (int c0 = j0; c0 < j1; c0 += BU_CHUNK) {
        const int c1 = min(c0 + BU_CHUNK, j1);
        float bax = 0.f, bay = 0.f, baz = 0.f, bdx = 0.f, bdy = 0.f, bdz = 0.f, bsg = 0.f, bgx = 0.f, bgy = 0.f, bgz = 0.f;
        for (int j = c0; j < c1; ++j) {
            const float rx = xs[3 * j] - xi, ry = xs[3 * j + 1] - yi, rz = xs[3 * j + 2] - zi;
            const bool on = live && abs(j - i) >= q.separation;
            float dsc, gp;
            const float s = bu_switch(rx * rx + ry * ry + rz * rz, q.inv_r2, &dsc);
            // i the centre, j its neighbour: a_i, and f_ij = g dsc r + s g' u_i as D + u_i sum s g'
            const float g = bu_half(ux * rx + uy * ry + uz * rz, q.width2, &gp);
            const float sgp = on ? s * gp : 0.f, gd = on ? g * dsc : 0.f;
            bax += sgp * rx;
            bay += sgp * ry;
            baz += sgp * rz;
            bsg += sgp;
            bdx += gd * rx;
            bdy += gd * ry;
            bdz += gd * rz;
            // j the centre, i its neighbour (r' = -r): k_j f_ji = k_j (-g_j dsc r + s g_j' u_j)
            const float kj = ks[j];                                     // (wave-uniform)
            if (kj != 0.f) {
                const float vx = us[3 * j], vy = us[3 * j + 1], vz = us[3 * j + 2];
                float gpj;
                const float gj = bu_half(-(vx * rx + vy * ry + vz * rz), q.width2, &gpj);
                const float c1j = on ? -kj * gj * dsc : 0.f, c2j = on ? kj * s * gpj : 0.f;
                bgx += c1j * rx + c2j * vx;
                bgy += c1j * ry + c2j * vy;
                bgz += c1j * rz + c2j * vz;
            }
        }
        ax += bax;
        ay += bay;
        az += baz;
        dx += bdx;
        dy += bdy;
        dz += bdz;
        sg += bsg;
        gx += bgx;
        gy += bgy;
        gz += bgz;
    }
    float* mine = part + w * 64 + lane;                                 // part[k][w][lane]
    mine[0 * BU_THREADS] = ax;
    mine[1 * BU_THREADS] = ay;
    mine[2 * BU_THREADS] = az;
    mine[3 * BU_THREADS] = dx;
    mine[4 * BU_THREADS] = dy;
    mine[5 * BU_THREADS] = dz;
    mine[6 * BU_THREADS] = sg;
    mine[7 * BU_THREADS] = gx;
    mine[8 * BU_THREADS] = gy;
    mine[9 * BU_THREADS] = gz;
    __syncthreads();
    if (w != 0 || !live) return;

    float v[BU_PART];
    for (int k = 0; k < BU_PART; ++k) {
        const float* p = part + k * BU_THREADS + lane;
        v[k] = ((p[0] + p[64]) + p[128]) + p[192];
    }
    const float ki = ks[i], rho = rhos[i];
    const float ua = ux * v[0] + uy * v[1] + uz * v[2];
    const bool inner = i >= 1 && i <= N - 2;                            // (an end's b is the constant 0: no pull)
    float* out = wb + (size_t)N + (size_t)i * 3;
    out[0] = v[7] - ki * (v[3] + ux * v[6]);
    out[1] = v[8] - ki * (v[4] + uy * v[6]);
    out[2] = v[9] - ki * (v[5] + uz * v[6]);
    out += 3 * (size_t)N;
    out[0] = inner ? ki * ((v[0] - ux * ua) / rho) : 0.f;
    out[1] = inner ? ki * ((v[1] - uy * ua) / rho) : 0.f;
    out[2] = inner ? ki * ((v[2] - uz * ua) / rho) : 0.f;
}

__global__ __launch_bounds__(BU_THREADS) void k_burial_finish(int N, BuParams q, const float* __restrict__ var_p,
                                                              const float* __restrict__ work, float* __restrict__ logp,
                                                              float* __restrict__ grad, float* __restrict__ report,
                                                              float* __restrict__ burial_out) {
    __shared__ float red[BU_WAVES], lows[BU_WAVES], highs[BU_WAVES], worst[BU_WAVES];
    __shared__ int bad[BU_WAVES];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* wb = work + (size_t)b * N * BU_WORK;
    const int i = blockIdx.x * BU_THREADS + tid;
    if (i < N) {
        if (burial_out) burial_out[(size_t)b * N + i] = wb[i];
        if (grad) {
            const float* P = wb + (size_t)N;
            const float* kv = wb + 4 * (size_t)N;
            const float sc = -1.f / *var_p;
            float* out = grad + ((size_t)b * N + i) * 3;
            for (int d = 0; d < 3; ++d) {
                const float before = i > 0 ? kv[3 * (i - 1) + d] : 0.f, after = i < N - 1 ? kv[3 * (i + 1) + d] : 0.f;
                out[d] = sc * (((P[3 * i + d] + 2.f * kv[3 * i + d]) - before) - after);
            }
        }
    }
    if (blockIdx.x != 0 || (!logp && !report)) return;                  // (uniform over the work-group)

    // the particle's sums, thread t taking residues t, t + 256, ...: butterfly over the lanes, then the waves in wave order
    const float m = bu_mean(wb, N, red);
    float cmin = INFINITY, cmax = -INFINITY, e = 0.f, vmax = 0.f;
    int nv = 0;
    for (int n = tid; n < N; n += BU_THREADS) {
        const float c = wb[n];
        cmin = fminf(cmin, c);
        cmax = fmaxf(cmax, c);
        const float w = q.w ? q.w[n] : 0.f;
        if (w > 0.f) {
            const float under = fmaxf(q.lo[n] - c, 0.f), over = fmaxf(c - q.hi[n], 0.f);
            e += w * (under * under + over * over);
            vmax = fmaxf(vmax, fmaxf(under, over));
            if (under > 0.f || over > 0.f) ++nv;
        }
    }
    const float e_res = bu_block_sum(e, red);
    for (int o = 32; o > 0; o >>= 1) {
        cmin = fminf(cmin, __shfl_xor(cmin, o, 64));
        cmax = fmaxf(cmax, __shfl_xor(cmax, o, 64));
        vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
    }
    nv = bu_wave_sum(nv);
    if ((tid & 63) == 0) {
        lows[tid >> 6] = cmin;
        highs[tid >> 6] = cmax;
        worst[tid >> 6] = vmax;
        bad[tid >> 6] = nv;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int o = 1; o < BU_WAVES; ++o) {
        cmin = fminf(cmin, lows[o]);
        cmax = fmaxf(cmax, highs[o]);
        vmax = fmaxf(vmax, worst[o]);
        nv += bad[o];
    }
    const float below = fmaxf(q.mean_min - m, 0.f), above = fmaxf(m - q.mean_max, 0.f);
    const float e_mean = q.mean_weight > 0.f ? q.mean_weight * (below * below + above * above) : 0.f;
    if (logp) logp[b] = -(e_res + e_mean) / (2.f * *var_p);
    if (report) {
        float* r = report + (size_t)b * GENIE_BURIAL_REPORT;
        r[0] = m;
        r[1] = cmin;
        r[2] = cmax;
        r[3] = (float)nv;
        r[4] = vmax;
        r[5] = e_res;
        r[6] = e_mean;
    }
}

int bu_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_burial_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

bool bu_bad(float v) { return !(v >= 0.f) || isinf(v); }           // negative, NaN or infinite

}  // namespace

size_t genie_burial_potential_work_bytes(int B, int N) {
    return (B >= 1 && B <= 65535 && N >= 1 && N <= GENIE_BURIAL_MAX_LENGTH) ? (size_t)B * N * BU_WORK * sizeof(float) : 0;
}

int genie_burial_potential(genie_stream_t stream, int B, int N, const float* x0, float radius, float width, int separation, const float* lo,
                           const float* hi, const float* w, float mean_min, float mean_max, float mean_weight, const float* var,
                           float* logp_out, float* grad_out, float* report_out, float* burial_out, void* work, size_t work_bytes) {
    if (B < 1 || B > 65535) return bu_refuse("B outside 1..65535");
    if (N < 1) return bu_refuse("N below 1");
    if (N > GENIE_BURIAL_MAX_LENGTH || bu_force_lds(N) > BU_LDS_MAX)
        return bu_refuse("N above GENIE_BURIAL_MAX_LENGTH (1728): the staging of the particle does not fit in LDS");
    if (!x0) return bu_refuse("x0 is NULL");
    if (!var) return bu_refuse("var is NULL");
    if (separation < 1) return bu_refuse("separation below 1");
    if (!(radius > 0.f) || isinf(radius)) return bu_refuse("radius not finite or not above 0");
    if (!(radius * radius > 0.f) || isinf(radius * radius) || isinf(1.f / (radius * radius)))
        return bu_refuse("radius: its square is no normal float");
    if (!(width > 0.f) || isinf(width) || !(width * width > 0.f) || isinf(width * width)) return bu_refuse("width not finite or not above 0");
    const int given = (lo != nullptr) + (hi != nullptr) + (w != nullptr);
    if (given != 0 && given != 3) return bu_refuse("lo, hi and w are given together or all NULL");
    if (bu_bad(mean_weight)) return bu_refuse("mean_weight negative or not finite");
    if (bu_bad(mean_min)) return bu_refuse("mean_min negative or not finite");
    if (!(mean_max >= 0.f)) return bu_refuse("mean_max negative or NaN");
    if (mean_max < mean_min) return bu_refuse("mean_max below mean_min");
    if (!logp_out && !grad_out && !report_out && !burial_out)
        return bu_refuse("no output asked for (logp_out, grad_out, report_out and burial_out are NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return bu_refuse("logp_out and grad_out are given together or both NULL");
    if (logp_out && given == 0 && !(mean_weight > 0.f))
        return bu_refuse("no term enabled (lo, hi, w NULL and mean_weight 0) and logp_out asked for");
    if (!work || work_bytes < genie_burial_potential_work_bytes(B, N))
        return bu_refuse("work is NULL or work_bytes below genie_burial_potential_work_bytes(B, N)");
    if (reinterpret_cast<uintptr_t>(work) & 3) return bu_refuse("work not 4-byte aligned");
    const BuParams q = {1.f / (radius * radius), width * width, mean_min, mean_max, mean_weight, separation, lo, hi, w};
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (N + BU_TILE - 1) / BU_TILE;
    float* slots = static_cast<float*>(work);
    hipLaunchKernelGGL(k_burial_count, dim3(tiles, B), dim3(BU_THREADS), bu_count_lds(N), st, x0, N, q, slots);
    if (grad_out) hipLaunchKernelGGL(k_burial_force, dim3(tiles, B), dim3(BU_THREADS), bu_force_lds(N), st, x0, N, q, slots);
    hipLaunchKernelGGL(k_burial_finish, dim3((N + BU_THREADS - 1) / BU_THREADS, B), dim3(BU_THREADS), 0, st, N, q, var,
                       (const float*)slots, logp_out, grad_out, report_out, burial_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
