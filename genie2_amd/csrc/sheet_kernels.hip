// Sheet potential of twisted-diffusion / SMC sampling (include/genie_hip.h: genie_sheet_potential): soft bounds on the antiparallel and
// the parallel strand-pairing content and an optional ladder of listed rungs, scored on C-alpha distances alone, with their gradient,
// a per-particle report and every residue's partner, in two launches instead of a PyTorch callable and an autograd walk back through
// it.  The reference has no counterpart; the secondary-structure potential (csrc/secstruct_kernels.hip) scores local geometry only.
//
// For particle b with coordinates x_n, n = 0..N-1 (all N rows: the twisted sampler's batches are never ragged), class c in {A, P} and
// a rung (i, j), 1 <= i < j <= N-2, j - i >= sep_c, with D[p, q] = |x_p - x_q|:
//   A: d0 = D[i, j], d1 = D[i-1, j+1], d2 = D[i+1, j-1]          P: d0 = D[i, j], d1 = D[i-1, j-1], d2 = D[i+1, j+1]
//   z_f = (d_f - mu_c) / sigma_c,   u = 1/3 sum_f z_f^2,   s = 1 / (1 + u)^2,   n_c = sum_rungs s
//   E_c = w_c [ (N f_c^min - n_c)_+^2 + (n_c - N f_c^max)_+^2 ],   E_lad = w_L sum_terms coef (D[p, q] - mu)^2
//   logp[b] = -(E_A + E_P + E_lad) / (2 var)
//   grad[b] = -(a_A G_A + a_P G_P + w_L G_lad) / (2 var),   G_c = d n_c / d x,   a_c = 2 w_c [ (n_c - N f_c^max)_+ - (N f_c^min - n_c)_+ ]
// A distance that is exactly 0 has direction 0, so every output is finite for finite inputs.
//
// k_sheet: grid (ceil(N / 64), B), 256 threads.  Every work-group of particle b stages x0[b] in LDS (12 N bytes) and handles its 64
// residues, one per lane, which keeps its rows n-2..n+2 in registers; each wave walks a contiguous quarter of the partners m
// (wave-uniform m: the rows m-2..m+2 are LDS broadcasts, kept as a sliding window) in partial sums of SHT_CHUNK.  The walk is centred
// on distances, not on rungs: with p = min(n, m), q = max(n, m), D[p, q] is the d0 of rung (p, q), the d1 of (p+1, q-1) and the d2
// of (p-1, q+1) in class A, and the d0 of (p, q), the d1 of (p+1, q+1) and the d2 of (p-1, q-1) in class P; all six share the z of
// D[p, q] inside their class, so the lane recomputes the six u from nine distances (the antidiagonal D[p+k, q-k] and the diagonal
// D[p+k, q+k], k = -2..2) and adds the force along x_n - x_m.  No lane writes another lane's residue.  Soft counts and formed-rung
// counts are taken where n is the rung's lower centre (n < m), the best partner from both sides (u is summed in an order that does
// not depend on the side, so both ends see the same bits).  The four wave results are combined in wave order; wave 0 then gathers
// the lane's ladder terms from the per-residue table (partners ascending, energies and missed rungs from the entries with partner >
// residue), writes the three unscaled gradient fields G_A, G_P, G_lad and the partners, and reduces the tile's sums by butterfly
// into the tile's 8 slots of `work`.
// k_sheet_finish: grid (ceil(N / 64), B), 64 threads: every thread adds the tiles in tile order (the same bits everywhere), forms
// a_A and a_P and writes its residue's gradient; thread 0 of tile 0 writes logp and the report.
// No atomics, no scatter: every output is written once, in a fixed order, so two calls on the same inputs are bitwise equal.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int SHT_THREADS = 256;
constexpr int SHT_WAVES = SHT_THREADS / 64;
constexpr int SHT_TILE = 64;            // residues per work-group: one per lane
constexpr int SHT_CHUNK = 64;           // partners per inner partial sum (two-level f32 summation)
constexpr int SHT_PART = 14;            // per-lane partials a wave leaves in LDS: G_A, G_P (3 each), n_A, n_P, formed A, P, best s, m A, P
constexpr int SHT_SLOTS = 8;            // 4-byte slots of `work` per (particle, tile), the SHT_* below
constexpr int SHT_FIELDS = 9;           // floats of `work` per residue: G_A, G_P, G_lad
constexpr size_t SHT_LDS_MAX = 160 * 1024;
constexpr int SHT_PARTNER_MASK = GENIE_SHEET_PARALLEL - 1;
enum { SHT_N_A, SHT_N_P, SHT_FORMED_A, SHT_FORMED_P, SHT_PAIRED, SHT_E_LAD, SHT_MISSED, SHT_UNUSED };

struct ShtParams {
    float mu[2], inv_sigma[2];          // [class A, P]
    int sep[2];
    float lo[2], hi[2], weight[2];      // content bounds (rungs per residue) and weights
    float ladder_weight;
    int L2;
};

// dynamic LDS: [xs: 3N] [part: SHT_PART * WAVES * 64]
size_t sht_lds_bytes(int N) { return sizeof(float) * (3 * (size_t)N + SHT_PART * SHT_WAVES * 64); }

__device__ inline float sht_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int sht_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct ShtVec {
    float x, y, z;
};

__device__ inline ShtVec sht_row(const float* xs, int i, int N) {           // row i of the particle, clamped into 0..N-1
    const float* p = xs + 3 * min(max(i, 0), N - 1);
    return {p[0], p[1], p[2]};
}

__device__ inline float sht_dist(ShtVec a, ShtVec b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return sqrtf(dx * dx + dy * dy + dz * dz);
}

// u of a rung from the squared z of its three distances, centre first: summed so that swapping the two outer ones changes no bit
__device__ inline float sht_u(float centre, float a, float b) { return ((a + b) + centre) * (1.f / 3.f); }

// whether the rung (i, j) of class c, given with its three z, is formed: all |z| <= 1
__device__ inline bool sht_inside(float z0, float z1, float z2) { return fabsf(z0) <= 1.f && fabsf(z1) <= 1.f && fabsf(z2) <= 1.f; }

__global__ __launch_bounds__(SHT_THREADS) void k_sheet(const float* __restrict__ x0, int N, ShtParams q,
                                                       const int32_t* __restrict__ lad_offset, const int32_t* __restrict__ lad_partner,
                                                       const float* __restrict__ lad_mu, const float* __restrict__ lad_coef,
                                                       float* __restrict__ fields, float* __restrict__ slots, int32_t* __restrict__ pairs,
                                                       int walk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sht_smem[];
    float* xs = reinterpret_cast<float*>(sht_smem);
    float* part = xs + 3 * (size_t)N;
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* x0b = x0 + (size_t)b * 3 * N;
    for (int i = tid; i < 3 * N; i += SHT_THREADS) xs[i] = x0b[i];
    __syncthreads();

    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n = blockIdx.x * SHT_TILE + lane;
    const bool live = n < N;
    ShtVec rn[5];                                                   // rows n-2..n+2
    for (int k = 0; k < 5; ++k) rn[k] = sht_row(xs, n + k - 2, N);

    float g[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, cnt[2] = {0.f, 0.f}, best_s[2] = {0.f, 0.f};
    int formed[2] = {0, 0}, best_m[2] = {-1, -1};
    if (walk) {
        const int m0 = (int)((int64_t)N * w / SHT_WAVES), m1 = (int)((int64_t)N * (w + 1) / SHT_WAVES);
        ShtVec rm[5];                                               // rows m-2..m+2 (wave-uniform)
        for (int k = 0; k < 4; ++k) rm[k + 1] = sht_row(xs, m0 + k - 2, N);
        for (int c0 = m0; c0 < m1; c0 += SHT_CHUNK) {
            const int c1 = min(c0 + SHT_CHUNK, m1);
            float cg[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, cc[2] = {0.f, 0.f};
            for (int m = c0; m < c1; ++m) {
                for (int k = 0; k < 4; ++k) rm[k] = rm[k + 1];
                rm[4] = sht_row(xs, m + 2, N);
                const bool low = n < m;                             // the lane holds the lower residue of the pair
                const int p = low ? n : m, r = low ? m : n, gap = r - p;
                // squared z of the antidiagonal D[p+k, q-k] and of the diagonal D[p+k, q+k], k = -2..2, in both classes' own scale
                float za[5], zp[5];
                for (int k = 0; k < 5; ++k) {
                    const float da = sht_dist(rn[low ? k : 4 - k], rm[low ? 4 - k : k]);
                    za[k] = (da - q.mu[0]) * q.inv_sigma[0];
                    if (k == 2) {
                        zp[k] = (da - q.mu[1]) * q.inv_sigma[1];
                    } else {
                        zp[k] = (sht_dist(rn[k], rm[k]) - q.mu[1]) * q.inv_sigma[1];
                    }
                }
                float qa[5], qp[5];
                for (int k = 0; k < 5; ++k) {
                    qa[k] = za[k] * za[k];
                    qp[k] = zp[k] * zp[k];
                }
                // the rungs that hold D[p, q]: (p, q), (p+1, q-1), (p-1, q+1) in A; (p, q), (p+1, q+1), (p-1, q-1) in P
                const bool inner = live && p >= 1 && r <= N - 2;
                const bool ea0 = inner && gap >= q.sep[0];
                const bool ea1 = live && gap - 2 >= q.sep[0];                                    // (p+1 >= 1 and q-1 <= N-2 always)
                const bool ea2 = live && p >= 2 && r <= N - 3 && gap + 2 >= q.sep[0];
                const bool ep0 = inner && gap >= q.sep[1];
                const bool ep1 = live && r <= N - 3 && gap >= q.sep[1];
                const bool ep2 = live && p >= 2 && gap >= q.sep[1];
                const float ta0 = 1.f / (1.f + sht_u(qa[2], qa[1], qa[3]));
                const float ta1 = 1.f / (1.f + sht_u(qa[3], qa[2], qa[4]));
                const float ta2 = 1.f / (1.f + sht_u(qa[1], qa[0], qa[2]));
                const float tp0 = 1.f / (1.f + sht_u(qp[2], qp[1], qp[3]));
                const float tp1 = 1.f / (1.f + sht_u(qp[3], qp[2], qp[4]));
                const float tp2 = 1.f / (1.f + sht_u(qp[1], qp[0], qp[2]));
                // d n_c / d D[p, q] = sum_rungs (-2 / (1 + u)^3) (2 z / (3 sigma_c))
                const float ka = (ea0 ? ta0 * ta0 * ta0 : 0.f) + (ea1 ? ta1 * ta1 * ta1 : 0.f) + (ea2 ? ta2 * ta2 * ta2 : 0.f);
                const float kp = (ep0 ? tp0 * tp0 * tp0 : 0.f) + (ep1 ? tp1 * tp1 * tp1 : 0.f) + (ep2 ? tp2 * tp2 * tp2 : 0.f);
                const float dx = rn[2].x - rm[2].x, dy = rn[2].y - rm[2].y, dz = rn[2].z - rm[2].z;
                const float d = sqrtf(dx * dx + dy * dy + dz * dz);
                const float inv = d > 0.f ? (-4.f / 3.f) / d : 0.f;  // (coincident residues: no direction)
                const float fa = inv * ka * za[2] * q.inv_sigma[0], fp = inv * kp * zp[2] * q.inv_sigma[1];
                cg[0][0] += fa * dx;
                cg[0][1] += fa * dy;
                cg[0][2] += fa * dz;
                cg[1][0] += fp * dx;
                cg[1][1] += fp * dy;
                cg[1][2] += fp * dz;
                // the rung (p, q) itself: its score where the lane is its lower centre, its partner from both sides
                const float sa = ta0 * ta0, sp = tp0 * tp0;
                if (ea0) {
                    if (low) cc[0] += sa;
                    if (sht_inside(za[2], za[1], za[3])) {
                        formed[0] += low;
                        if (sa > best_s[0]) best_s[0] = sa, best_m[0] = m;
                    }
                }
                if (ep0) {
                    if (low) cc[1] += sp;
                    if (sht_inside(zp[2], zp[1], zp[3])) {
                        formed[1] += low;
                        if (sp > best_s[1]) best_s[1] = sp, best_m[1] = m;
                    }
                }
            }
            for (int c = 0; c < 2; ++c) {
                g[c][0] += cg[c][0];
                g[c][1] += cg[c][1];
                g[c][2] += cg[c][2];
                cnt[c] += cc[c];
            }
        }
    }
    float* mine = part + w * 64 + lane;                             // part[k][w][lane]
    constexpr int ST = SHT_WAVES * 64;
    for (int c = 0; c < 2; ++c) {
        for (int k = 0; k < 3; ++k) mine[(3 * c + k) * ST] = g[c][k];
        mine[(6 + c) * ST] = cnt[c];
        mine[(8 + c) * ST] = __int_as_float(formed[c]);
        mine[(10 + c) * ST] = best_s[c];
        mine[(12 + c) * ST] = __int_as_float(best_m[c]);
    }
    __syncthreads();
    if (w != 0) return;

    for (int v = 1; v < SHT_WAVES; ++v) {                           // waves in wave order: partners ascending, so ties keep the lowest
        const float* o = part + v * 64 + lane;
        for (int c = 0; c < 2; ++c) {
            for (int k = 0; k < 3; ++k) g[c][k] += o[(3 * c + k) * ST];
            cnt[c] += o[(6 + c) * ST];
            formed[c] += __float_as_int(o[(8 + c) * ST]);
            const float s = o[(10 + c) * ST];
            if (s > best_s[c]) best_s[c] = s, best_m[c] = __float_as_int(o[(12 + c) * ST]);
        }
    }

    // the lane's ladder terms, partners ascending.  (The table is the caller's, validated where it is built; offsets and partners
    // are clamped all the same: they index the table and LDS.)
    float lx = 0.f, ly = 0.f, lz = 0.f, el = 0.f;
    int missed = 0;
    if (live && q.L2 > 0) {
        const int k0 = min(max(lad_offset[n], 0), q.L2), k1 = min(max(lad_offset[n + 1], k0), q.L2);
        for (int k = k0; k < k1; ++k) {
            const int word = lad_partner[k];
            const int p = min(max(word & SHT_PARTNER_MASK, 0), N - 1);
            const ShtVec o = sht_row(xs, p, N);
            const float dx = rn[2].x - o.x, dy = rn[2].y - o.y, dz = rn[2].z - o.z;
            const float d = sqrtf(dx * dx + dy * dy + dz * dz);
            const float dev = d - lad_mu[k], coef = lad_coef[k];
            const float f = d > 0.f ? 2.f * coef * dev / d : 0.f;
            lx += f * dx;
            ly += f * dy;
            lz += f * dz;
            if (p > n) {
                el += coef * dev * dev;
                if (word & GENIE_SHEET_RUNG) {                      // the d0 of a listed rung (n, p): is it formed in its class?
                    const int c = (word & GENIE_SHEET_PARALLEL) ? 1 : 0;
                    const float d1 = sht_dist(rn[1], sht_row(xs, c ? p - 1 : p + 1, N));
                    const float d2 = sht_dist(rn[3], sht_row(xs, c ? p + 1 : p - 1, N));
                    const float mu = q.mu[c], is = q.inv_sigma[c];
                    missed += !sht_inside((d - mu) * is, (d1 - mu) * is, (d2 - mu) * is);
                }
            }
        }
    }

    if (live) {
        if (fields) {
            float* out = fields + ((size_t)b * N + n) * SHT_FIELDS;
            for (int c = 0; c < 2; ++c)
                for (int k = 0; k < 3; ++k) out[3 * c + k] = g[c][k];
            out[6] = lx;
            out[7] = ly;
            out[8] = lz;
        }
        if (pairs) {
            pairs[((size_t)b * N + n) * 2] = best_m[0];
            pairs[((size_t)b * N + n) * 2 + 1] = best_m[1];
        }
    }

    // the tile's share of the particle's sums (lanes past N hold 0)
    const float na = sht_wave_sum(cnt[0]), np = sht_wave_sum(cnt[1]);
    const int fa = sht_wave_sum(formed[0]), fp = sht_wave_sum(formed[1]);
    const int paired = sht_wave_sum((int)(best_m[0] >= 0 || best_m[1] >= 0));
    el = sht_wave_sum(el);
    missed = sht_wave_sum(missed);
    if (lane == 0) {
        float* slot = slots + ((size_t)b * gridDim.x + blockIdx.x) * SHT_SLOTS;
        slot[SHT_N_A] = na;
        slot[SHT_N_P] = np;
        slot[SHT_FORMED_A] = __int_as_float(fa);
        slot[SHT_FORMED_P] = __int_as_float(fp);
        slot[SHT_PAIRED] = __int_as_float(paired);
        slot[SHT_E_LAD] = el;
        slot[SHT_MISSED] = __int_as_float(missed);
        slot[SHT_UNUSED] = 0.f;
    }
}

__global__ __launch_bounds__(64) void k_sheet_finish(int N, int tiles, ShtParams q, const float* __restrict__ var_p,
                                                     const float* __restrict__ fields, const float* __restrict__ slots,
                                                     float* __restrict__ logp, float* __restrict__ grad, float* __restrict__ report) {
    const int b = blockIdx.y, n = blockIdx.x * SHT_TILE + threadIdx.x;
    const float* slot = slots + (size_t)b * tiles * SHT_SLOTS;
    float nc[2] = {0.f, 0.f}, el = 0.f;
    int fa = 0, fp = 0, paired = 0, missed = 0;
    for (int t = 0; t < tiles; ++t, slot += SHT_SLOTS) {            // tile order, the same in every thread
        nc[0] += slot[SHT_N_A];
        nc[1] += slot[SHT_N_P];
        fa += __float_as_int(slot[SHT_FORMED_A]);
        fp += __float_as_int(slot[SHT_FORMED_P]);
        paired += __float_as_int(slot[SHT_PAIRED]);
        el += slot[SHT_E_LAD];
        missed += __float_as_int(slot[SHT_MISSED]);
    }
    float e[2], a[2];
    for (int c = 0; c < 2; ++c) {
        const float under = fmaxf((float)N * q.lo[c] - nc[c], 0.f), over = fmaxf(nc[c] - (float)N * q.hi[c], 0.f);
        e[c] = q.weight[c] * (under * under + over * over);
        a[c] = 2.f * q.weight[c] * (over - under);
    }
    const float e_lad = q.ladder_weight * el;
    if (grad && n < N) {
        const float sc = -1.f / (2.f * *var_p);
        const float* f = fields + ((size_t)b * N + n) * SHT_FIELDS;
        float* out = grad + ((size_t)b * N + n) * 3;
        for (int k = 0; k < 3; ++k) out[k] = sc * ((a[0] * f[k] + a[1] * f[3 + k]) + q.ladder_weight * f[6 + k]);
    }
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (logp) logp[b] = -((e[0] + e[1]) + e_lad) / (2.f * *var_p);
    if (report) {
        float* r = report + (size_t)b * GENIE_SHEET_REPORT;
        r[0] = nc[0] / (float)N;
        r[1] = nc[1] / (float)N;
        r[2] = (float)fa;
        r[3] = (float)fp;
        r[4] = (float)paired;
        r[5] = e[0];
        r[6] = e[1];
        r[7] = e_lad;
        r[8] = (float)missed;
    }
}

int sht_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_sheet_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

bool sht_bad(float v) { return !(v >= 0.f) || isinf(v); }          // negative, NaN or infinite

size_t sht_field_bytes(int B, int N) { return (size_t)B * (size_t)N * SHT_FIELDS * sizeof(float); }

}  // namespace

size_t genie_sheet_potential_work_bytes(int B, int N) {
    return (B >= 1 && N >= 1) ? sht_field_bytes(B, N) + (size_t)B * (((size_t)N + SHT_TILE - 1) / SHT_TILE) * SHT_SLOTS * sizeof(float) : 0;
}

int genie_sheet_potential(genie_stream_t stream, int B, int N, const float* x0, float mu_antiparallel, float sigma_antiparallel,
                          float mu_parallel, float sigma_parallel, int separation_antiparallel, int separation_parallel,
                          float antiparallel_min, float antiparallel_max, float antiparallel_weight, float parallel_min,
                          float parallel_max, float parallel_weight, int L2, const int32_t* lad_offset, const int32_t* lad_partner,
                          const float* lad_mu, const float* lad_coef, float ladder_weight, const float* var, float* logp_out,
                          float* grad_out, float* report_out, int32_t* pairs_out, void* work, size_t work_bytes) {
    if (B < 1 || B > 65535) return sht_refuse("B outside 1..65535");
    if (N < 1) return sht_refuse("N below 1");
    if (!x0) return sht_refuse("x0 is NULL");
    if (!var) return sht_refuse("var is NULL");
    if (!logp_out && !grad_out && !report_out && !pairs_out)
        return sht_refuse("no output asked for (logp_out, grad_out, report_out and pairs_out are NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return sht_refuse("logp_out and grad_out are given together or both NULL");
    if (separation_antiparallel < 3) return sht_refuse("separation_antiparallel below 3");
    if (separation_parallel < 3) return sht_refuse("separation_parallel below 3");
    if (!isfinite(mu_antiparallel)) return sht_refuse("mu_antiparallel is not finite");
    if (!isfinite(mu_parallel)) return sht_refuse("mu_parallel is not finite");
    if (!(sigma_antiparallel > 0.f) || isinf(sigma_antiparallel)) return sht_refuse("sigma_antiparallel is not positive and finite");
    if (!(sigma_parallel > 0.f) || isinf(sigma_parallel)) return sht_refuse("sigma_parallel is not positive and finite");
    if (sht_bad(antiparallel_weight)) return sht_refuse("antiparallel_weight negative or not finite");
    if (sht_bad(parallel_weight)) return sht_refuse("parallel_weight negative or not finite");
    if (sht_bad(ladder_weight)) return sht_refuse("ladder_weight negative or not finite");
    if (sht_bad(antiparallel_min) || !(antiparallel_min <= antiparallel_max))
        return sht_refuse("antiparallel_min, antiparallel_max: needs 0 <= min <= max with min finite (max may be inf)");
    if (sht_bad(parallel_min) || !(parallel_min <= parallel_max))
        return sht_refuse("parallel_min, parallel_max: needs 0 <= min <= max with min finite (max may be inf)");
    if (L2 < 0 || (L2 & 1)) return sht_refuse("L2 negative or odd (every ladder term is listed at both of its residues)");
    if (L2 > 0 && (!lad_offset || !lad_partner || !lad_mu || !lad_coef))
        return sht_refuse("L2 > 0 with a NULL ladder table (lad_offset, lad_partner, lad_mu, lad_coef)");
    if (!work || work_bytes < genie_sheet_potential_work_bytes(B, N))
        return sht_refuse("work is NULL or work_bytes below genie_sheet_potential_work_bytes(B, N)");
    if (reinterpret_cast<uintptr_t>(work) & 3) return sht_refuse("work not 4-byte aligned");
    const size_t lds = sht_lds_bytes(N);
    if (lds > SHT_LDS_MAX) return sht_refuse("N too large: the staging of x0[b] does not fit in LDS");
    ShtParams q;
    q.mu[0] = mu_antiparallel, q.inv_sigma[0] = 1.f / sigma_antiparallel, q.sep[0] = separation_antiparallel;
    q.mu[1] = mu_parallel, q.inv_sigma[1] = 1.f / sigma_parallel, q.sep[1] = separation_parallel;
    q.lo[0] = antiparallel_min, q.hi[0] = antiparallel_max, q.weight[0] = antiparallel_weight;
    q.lo[1] = parallel_min, q.hi[1] = parallel_max, q.weight[1] = parallel_weight;
    q.ladder_weight = ladder_weight;
    q.L2 = L2;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (N + SHT_TILE - 1) / SHT_TILE;
    // the report's contents and counts and the partners need the walk even at weight 0
    const int walk = (report_out || pairs_out || antiparallel_weight > 0.f || parallel_weight > 0.f) ? 1 : 0;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(k_sheet), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return GENIE_E_HIP;
    float* fields = static_cast<float*>(work);
    float* slots = fields + (size_t)B * N * SHT_FIELDS;
    hipLaunchKernelGGL(k_sheet, dim3(tiles, B), dim3(SHT_THREADS), lds, st, x0, N, q, lad_offset, lad_partner, lad_mu, lad_coef,
                       grad_out ? fields : nullptr, slots, pairs_out, walk);
    if (logp_out || report_out)
        hipLaunchKernelGGL(k_sheet_finish, dim3(tiles, B), dim3(64), 0, st, N, tiles, q, var, (const float*)fields, (const float*)slots,
                           logp_out, grad_out, report_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
