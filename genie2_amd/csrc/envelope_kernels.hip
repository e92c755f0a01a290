// Envelope potential of twisted-diffusion / SMC sampling (include/genie_hip.h: genie_envelope_potential): a design is kept inside a
// given 3D shape -- M weighted points y_m -- and made to fill it, by a soft assignment in both directions between the particle's
// residues and the points, with its gradient and a per-particle report, in three launches.  The reference has no counterpart.
//
// For particle b with coordinates x_n and q_nm = |x_n - y_m|^2 (from coordinate differences):
//   s_n = -tau log sum_m exp(-q_nm / tau),  a_n = sqrt(max(s_n, 0) + eps^2),  h_n = (a_n - inside_distance)_+
//   t_m = -tau log sum_n exp(-q_nm / tau),  c_m = sqrt(max(t_m, 0) + eps^2),  g_m = (c_m - cover_distance)_+
//   E = inside_weight sum_n h_n^2 + cover_weight (N / sum v) sum_m v_m g_m^2,  logp[b] = -E / (2 var)
//   grad[b,n] = -(1/var) [ inside_weight (h_n / a_n) sum_m p_nm (x_n - y_m) + sum_m k_m r_nm (x_n - y_m) ]
//   p_nm = exp((s_n - q_nm) / tau),  r_nm = exp((t_m - q_nm) / tau),  k_m = cover_weight (N / sum v) v_m g_m / c_m
//
// k_envelope_soft_min: grid (ceil(N / 64) + ceil(M / 64), B), W = 16 waves (4 in a launch of GENIE_ENVELOPE_FILL work-groups or more,
// which fills the device without them; a wave's walk is a serial chain, so a small launch is latency-bound).  The two soft minima are
// one loop (ev_soft_min) with the roles swapped: a work-group of the first ceil(N / 64) owns 64 residues, one per lane, and walks
// the points; one of the others owns 64 points and walks the particle's residues.  The walked side is staged through LDS in chunks of GENIE_ENVELOPE_CHUNK rows (x, y,
// z padded to 16 bytes: one ds_read_b128 of a wave-uniform address, an LDS broadcast).  Each wave takes a contiguous W-th of a
// chunk twice: first for the smallest q, then for sum exp((min - q) / tau) -- one exponential per pair, none above 1, so a particle
// 300 A away underflows nothing.  A lane carries a (minimum, rescaled sum) pair, merged with that share's pair by two exponentials;
// the waves' pairs are merged in wave order.  Wave 0 stores s_n (or t_m and k_m) to `work`, a_n / c_m to distance_out /
// gap_out, and the tile's three sums (sum h^2 or sum v g^2, the count and the maximum of the positive hinges: a butterfly over the
// 64 lanes) to the tile's slot of `work`.
// k_envelope_gather (only with a gradient): grid (ceil(N / 64), B).  Lane n walks the points again, staged with t_m and k_m, and adds
// [ci_n p_nm + k_m r_nm] (x_n - y_m), ci_n = inside_weight h_n / a_n: the first exponential is skipped where ci_n = 0, the second
// where k_m = 0 (wave-uniform) -- most pairs once a design sits inside.  Sums per wave and chunk, then the waves in wave order.
// k_envelope_finish: grid (B), 256 threads: the tile slots are read into LDS and thread 0 adds them in tile order; logp and the
// report.
// No atomics, no scatter: every output is written once, in a fixed order, so two calls on the same inputs are bitwise equal.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int EV_THREADS = 1024;        // the most threads of a work-group: 16 waves share a tile's walk, which is a serial chain per wave
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr int EV_FEW = 256;             // threads of a work-group in a launch of GENIE_ENVELOPE_FILL work-groups or more: the device is full
constexpr int EV_TILE = 64;             // residues (or points) a work-group owns: one per lane
constexpr int EV_CHUNK = GENIE_ENVELOPE_CHUNK;      // rows of the walked side staged in LDS at a time
constexpr int EV_SLOT = 3;              // floats a tile leaves for the finishing step: the energy sum, the count, the maximum
constexpr float EV_LOG2E = 1.44269504088896340736f;

struct EvParams {
    float tau, c2;                      // c2 = log2(e) / tau: exp(z / tau) = exp2(z c2)
    float inside, inside_weight, cover, cover_weight;
};

__host__ __device__ inline int ev_tiles(int n) { return (n + EV_TILE - 1) / EV_TILE; }

// floats of `work` per particle: [s: N] [t: M] [k: M] [residue tiles: 3 each] [point tiles: 3 each]
__host__ __device__ inline size_t ev_work_floats(int N, int M) { return (size_t)N + 2 * (size_t)M + EV_SLOT * (size_t)(ev_tiles(N) + ev_tiles(M)); }

__device__ inline float ev_exp2(float z) { return __builtin_amdgcn_exp2f(z); }      // v_exp_f32: z <= 0 here, a denormal result may be 0

__device__ inline float ev_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline float ev_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// sum v of the envelope by a work-group, the same bits in every thread of every work-group: thread t adds v_t, v_{t+threads},
// ..., a butterfly over the lanes, then the waves in wave order; M without weights
__device__ inline float ev_weight_sum(const float* __restrict__ weights, int M, float* red) {
    if (!weights) return (float)M;
    float v = 0.f;
    for (int m = threadIdx.x; m < M; m += blockDim.x) v += weights[m];
    v = ev_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int o = 1; o < (int)(blockDim.x >> 6); ++o) r += red[o];
    __syncthreads();
    return r;
}

// (m, s) <- the pair of the union of (m, s) and (mb, sb): s = sum exp((m - q) / tau) over its rows, s = 0 for none
__device__ inline void ev_merge(float& m, float& s, float mb, float sb, float c2) {
    if (!(sb > 0.f)) return;
    if (!(s > 0.f)) {
        m = mb;
        s = sb;
        return;
    }
    const float mn = fminf(m, mb);
    s = s * ev_exp2((mn - m) * c2) + sb * ev_exp2((mn - mb) * c2);
    m = mn;
}

__device__ inline float ev_q(float ox, float oy, float oz, const float4& y) {
    const float dx = ox - y.x, dy = oy - y.y, dz = oz - y.z;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// -tau log sum_j exp(-|o - walked_j|^2 / tau) over the `count` rows of `walked` [count, 3] (global memory), o this lane's own point:
// every thread of the work-group calls it; the value is the lane's in every wave
__device__ inline float ev_soft_min(float ox, float oy, float oz, const float* __restrict__ walked, int count, const EvParams& p,
                                    float4* stage, float* pairs) {
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int threads = blockDim.x, waves = threads >> 6;
    float m = INFINITY, s = 0.f;
    for (int c0 = 0; c0 < count; c0 += EV_CHUNK) {
        const int len = min(EV_CHUNK, count - c0);
        __syncthreads();                                                // (the chunk before is read out)
        for (int i = tid; i < len; i += threads) {
            const float* r = walked + 3 * (size_t)(c0 + i);
            stage[i] = make_float4(r[0], r[1], r[2], 0.f);
        }
        __syncthreads();
        const int j0 = len * w / waves, j1 = len * (w + 1) / waves;
        if (j0 == j1) continue;
        float cm = INFINITY, cs = 0.f;
#pragma unroll 4
        for (int j = j0; j < j1; ++j) cm = fminf(cm, ev_q(ox, oy, oz, stage[j]));
#pragma unroll 4
        for (int j = j0; j < j1; ++j) cs += ev_exp2((cm - ev_q(ox, oy, oz, stage[j])) * p.c2);
        ev_merge(m, s, cm, cs, p.c2);
    }
    pairs[2 * (w * 64 + lane)] = m;
    pairs[2 * (w * 64 + lane) + 1] = s;
    __syncthreads();
    m = pairs[2 * lane];
    s = pairs[2 * lane + 1];
    for (int o = 1; o < waves; ++o) ev_merge(m, s, pairs[2 * (o * 64 + lane)], pairs[2 * (o * 64 + lane) + 1], p.c2);
    return m - p.tau * logf(s);
}

__global__ __launch_bounds__(EV_THREADS) void k_envelope_soft_min(const float* __restrict__ x0, int N, int M, const float* __restrict__ points,
                                                                  const float* __restrict__ weights, EvParams p, float* __restrict__ work,
                                                                  float* __restrict__ distance_out, float* __restrict__ gap_out) {
    __shared__ float4 stage[EV_CHUNK];
    __shared__ float pairs[2 * EV_THREADS];
    __shared__ float red[EV_WAVES];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int tiles_n = ev_tiles(N);
    const bool residues = (int)blockIdx.x < tiles_n;                    // (uniform over the work-group)
    const int tile = residues ? (int)blockIdx.x : (int)blockIdx.x - tiles_n;
    const float* xb = x0 + (size_t)b * N * 3;
    float* wb = work + (size_t)b * ev_work_floats(N, M);
    const float* own = residues ? xb : points;
    const int own_count = residues ? N : M;
    const int i = tile * EV_TILE + lane;
    const bool live = i < own_count;
    const int ii = live ? i : 0;
    const float ox = own[3 * (size_t)ii], oy = own[3 * (size_t)ii + 1], oz = own[3 * (size_t)ii + 2];
    const float sum_v = residues ? 0.f : ev_weight_sum(weights, M, red);
    const float sm = ev_soft_min(ox, oy, oz, residues ? points : xb, residues ? M : N, p, stage, pairs);
    if (tid >= 64) return;

    const float d = sqrtf(fmaxf(sm, 0.f) + GENIE_ENVELOPE_EPS * GENIE_ENVELOPE_EPS);
    const float hinge = live ? fmaxf(d - (residues ? p.inside : p.cover), 0.f) : 0.f;
    const float v = (!residues && weights && live) ? weights[i] : 1.f;
    const float e = ev_wave_sum(v * hinge * hinge);
    const float count = ev_wave_sum(hinge > 0.f ? 1.f : 0.f);
    const float worst = ev_wave_max(hinge);
    if (live) {
        if (residues) {
            wb[i] = sm;
            if (distance_out) distance_out[(size_t)b * N + i] = d;
        } else {
            wb[(size_t)N + i] = sm;
            wb[(size_t)N + M + i] = p.cover_weight > 0.f ? p.cover_weight * ((float)N / sum_v) * v * (hinge / d) : 0.f;
            if (gap_out) gap_out[(size_t)b * M + i] = d;
        }
    }
    if (lane == 0) {
        float* slot = wb + (size_t)N + 2 * (size_t)M + EV_SLOT * (size_t)blockIdx.x;
        slot[0] = e;
        slot[1] = count;
        slot[2] = worst;
    }
}

__global__ __launch_bounds__(EV_THREADS) void k_envelope_gather(const float* __restrict__ x0, int N, int M, const float* __restrict__ points,
                                                                EvParams p, const float* __restrict__ var_p, const float* __restrict__ work,
                                                                float* __restrict__ grad) {
    __shared__ float4 stage[EV_CHUNK];                                  // y_m and t_m
    __shared__ float coefs[EV_CHUNK];                                   // k_m
    __shared__ float part[3 * EV_THREADS];
    const int b = blockIdx.y, tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const float* xb = x0 + (size_t)b * N * 3;
    const float* wb = work + (size_t)b * ev_work_floats(N, M);
    const float* tm = wb + (size_t)N;
    const float* km = tm + (size_t)M;
    const int n = blockIdx.x * EV_TILE + lane;
    const bool live = n < N;
    const int nn = live ? n : 0;
    const float xn = xb[3 * (size_t)nn], yn = xb[3 * (size_t)nn + 1], zn = xb[3 * (size_t)nn + 2];
    const float sn = wb[nn];
    const float a = sqrtf(fmaxf(sn, 0.f) + GENIE_ENVELOPE_EPS * GENIE_ENVELOPE_EPS);
    const float ci = (live && p.inside_weight > 0.f) ? p.inside_weight * (fmaxf(a - p.inside, 0.f) / a) : 0.f;
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int c0 = 0; c0 < M; c0 += EV_CHUNK) {
        const int len = min(EV_CHUNK, M - c0);
        __syncthreads();
        for (int i = tid; i < len; i += (int)blockDim.x) {
            const float* r = points + 3 * (size_t)(c0 + i);
            stage[i] = make_float4(r[0], r[1], r[2], tm[c0 + i]);
            coefs[i] = km[c0 + i];
        }
        __syncthreads();
        const int waves = blockDim.x >> 6;
        const int j0 = len * w / waves, j1 = len * (w + 1) / waves;
        float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll 4
        for (int j = j0; j < j1; ++j) {
            const float4 y = stage[j];
            const float kj = coefs[j];                                  // (wave-uniform)
            const float dx = xn - y.x, dy = yn - y.y, dz = zn - y.z;
            const float q = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            float c = 0.f;
            if (ci != 0.f) c = ci * ev_exp2((sn - q) * p.c2);
            if (kj != 0.f) c += kj * ev_exp2((y.w - q) * p.c2);
            bx += c * dx;
            by += c * dy;
            bz += c * dz;
        }
        gx += bx;
        gy += by;
        gz += bz;
    }
    part[w * 64 + lane] = gx;
    part[EV_THREADS + w * 64 + lane] = gy;
    part[2 * EV_THREADS + w * 64 + lane] = gz;
    __syncthreads();
    if (w != 0 || !live) return;
    const float sc = -1.f / *var_p;
    float* out = grad + ((size_t)b * N + n) * 3;
    for (int d = 0; d < 3; ++d) {
        const float* q = part + d * EV_THREADS + lane;
        float v = q[0];
        for (int o = 1; o < (int)(blockDim.x >> 6); ++o) v += q[64 * o];
        out[d] = sc * v;
    }
}

__global__ __launch_bounds__(EV_THREADS) void k_envelope_finish(int N, int M, const float* __restrict__ weights, EvParams p,
                                                                const float* __restrict__ var_p, const float* __restrict__ work,
                                                                float* __restrict__ logp, float* __restrict__ report) {
    __shared__ float slots[EV_SLOT * (GENIE_ENVELOPE_MAX_LENGTH + GENIE_ENVELOPE_MAX_POINTS) / EV_TILE];
    __shared__ float red[EV_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int tiles_n = ev_tiles(N), tiles_m = ev_tiles(M);
    const float* sb = work + (size_t)b * ev_work_floats(N, M) + (size_t)N + 2 * (size_t)M;
    for (int i = tid; i < EV_SLOT * (tiles_n + tiles_m); i += (int)blockDim.x) slots[i] = sb[i];
    const float sum_v = ev_weight_sum(weights, M, red);
    __syncthreads();
    if (tid != 0) return;
    float e[2] = {0.f, 0.f}, count[2] = {0.f, 0.f}, worst[2] = {0.f, 0.f};
    for (int t = 0; t < tiles_n + tiles_m; ++t) {                       // in tile order
        const int side = t >= tiles_n;
        e[side] += slots[EV_SLOT * t];
        count[side] += slots[EV_SLOT * t + 1];
        worst[side] = fmaxf(worst[side], slots[EV_SLOT * t + 2]);
    }
    const float e_inside = p.inside_weight > 0.f ? p.inside_weight * e[0] : 0.f;
    const float e_cover = p.cover_weight > 0.f ? p.cover_weight * ((float)N / sum_v) * e[1] : 0.f;
    if (logp) logp[b] = -(e_inside + e_cover) / (2.f * *var_p);
    if (report) {
        float* r = report + (size_t)b * GENIE_ENVELOPE_REPORT;
        r[0] = count[0];
        r[1] = worst[0];
        r[2] = count[1];
        r[3] = worst[1];
        r[4] = e_inside;
        r[5] = e_cover;
    }
}

int ev_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_envelope_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

bool ev_sizes_ok(int B, int N, int M) {
    return B >= 1 && B <= 65535 && N >= 1 && N <= GENIE_ENVELOPE_MAX_LENGTH && M >= 1 && M <= GENIE_ENVELOPE_MAX_POINTS;
}

}  // namespace

size_t genie_envelope_potential_work_bytes(int B, int N, int M) {
    return ev_sizes_ok(B, N, M) ? (size_t)B * ev_work_floats(N, M) * sizeof(float) : 0;
}

int genie_envelope_potential(genie_stream_t stream, int B, int N, const float* x0, int M, const float* points, const float* weights,
                             float softness, float inside_distance, float inside_weight, float cover_distance, float cover_weight,
                             const float* var, float* logp_out, float* grad_out, float* report_out, float* distance_out, float* gap_out,
                             void* work, size_t work_bytes) {
    if (B < 1 || B > 65535) return ev_refuse("B outside 1..65535");
    if (N < 1 || N > GENIE_ENVELOPE_MAX_LENGTH) return ev_refuse("N outside 1..GENIE_ENVELOPE_MAX_LENGTH (4096)");
    if (M < 1 || M > GENIE_ENVELOPE_MAX_POINTS) return ev_refuse("M outside 1..GENIE_ENVELOPE_MAX_POINTS (16384)");
    if (!x0) return ev_refuse("x0 is NULL");
    if (!points) return ev_refuse("points is NULL");
    if (!var) return ev_refuse("var is NULL");
    if (!(softness > 0.f) || isinf(softness) || isinf(EV_LOG2E / softness)) return ev_refuse("softness (tau) not finite or not above 0");
    if (!(inside_distance > GENIE_ENVELOPE_EPS) || isinf(inside_distance))
        return ev_refuse("inside_distance not finite or not above GENIE_ENVELOPE_EPS (0.1)");
    if (!(cover_distance > GENIE_ENVELOPE_EPS) || isinf(cover_distance))
        return ev_refuse("cover_distance not finite or not above GENIE_ENVELOPE_EPS (0.1)");
    if (!(inside_weight >= 0.f) || isinf(inside_weight)) return ev_refuse("inside_weight negative or not finite");
    if (!(cover_weight >= 0.f) || isinf(cover_weight)) return ev_refuse("cover_weight negative or not finite");
    if (inside_weight == 0.f && cover_weight == 0.f) return ev_refuse("no term enabled (inside_weight and cover_weight are 0)");
    if (!logp_out && !grad_out && !report_out && !distance_out && !gap_out)
        return ev_refuse("no output asked for (logp_out, grad_out, report_out, distance_out and gap_out are NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return ev_refuse("logp_out and grad_out are given together or both NULL");
    if (!work || work_bytes < genie_envelope_potential_work_bytes(B, N, M))
        return ev_refuse("work is NULL or work_bytes below genie_envelope_potential_work_bytes(B, N, M)");
    if (reinterpret_cast<uintptr_t>(work) & 3) return ev_refuse("work not 4-byte aligned");
    const EvParams p = {softness, EV_LOG2E / softness, inside_distance, inside_weight, cover_distance, cover_weight};
    hipStream_t st = (hipStream_t)stream;
    float* slots = static_cast<float*>(work);
    // (64-bit counts: B tiles stays below 2^25)
    const int64_t groups = (int64_t)B * (ev_tiles(N) + ev_tiles(M)), gather_groups = (int64_t)B * ev_tiles(N);
    const dim3 threads(groups >= GENIE_ENVELOPE_FILL ? EV_FEW : EV_THREADS), gather_threads(gather_groups >= GENIE_ENVELOPE_FILL ? EV_FEW : EV_THREADS);
    hipLaunchKernelGGL(k_envelope_soft_min, dim3(ev_tiles(N) + ev_tiles(M), B), threads, 0, st, x0, N, M, points, weights, p, slots,
                       distance_out, gap_out);
    if (grad_out)
        hipLaunchKernelGGL(k_envelope_gather, dim3(ev_tiles(N), B), gather_threads, 0, st, x0, N, M, points, p, var, (const float*)slots,
                           grad_out);
    if (logp_out || report_out)
        hipLaunchKernelGGL(k_envelope_finish, dim3(B), dim3(EV_FEW), 0, st, N, M, weights, p, var, (const float*)slots, logp_out,
                           report_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
