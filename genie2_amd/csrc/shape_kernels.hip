// Shape potential of twisted-diffusion / SMC sampling (include/genie_hip.h: genie_shape_potential): a radius-of-gyration cap, a
// C-alpha clash term over all residue pairs and the caller's pairwise distance restraints, with their gradient and a per-particle
// report, in two launches instead of a PyTorch callable and an autograd walk back through it.  The reference has no counterpart: its
// one twisting function is the motif potential (csrc/smc_kernels.hip).
//
// For particle b with coordinates x_n, n = 0..N-1 (all N rows: the twisted sampler's batches are never ragged):
//   m = mean_n x_n,  c_n = x_n - m,  rog = sqrt(sum_n |c_n|^2 / N)
//   E_rog   = rog_weight   * max(0, rog - rog_max)^2
//   E_clash = clash_weight * sum_{i<j, j-i >= clash_separation} max(0, clash_distance - d_ij)^2,   d_ij = |x_i - x_j|
//   E_rst   = sum_r w_r (max(0, lo_r - d_r)^2 + max(0, d_r - hi_r)^2),   d_r = |x_{i_r} - x_{j_r}|
//   logp[b] = -(E_rog + E_clash + E_rst) / (2 var)
//   grad[b,n] = -(1/var) [ rog_weight (rog - rog_max)_+ c_n / (N rog) - clash_weight sum_{j eligible} (clash_distance - d_nj)_+ u_nj
//                          + sum_{r containing n} w_r ((d_r - hi_r)_+ - (lo_r - d_r)_+) u_{n,partner} ],   u_nj = (x_n - x_j) / d_nj
// with u = 0 where d is exactly 0 and the rog term 0 where rog is exactly 0, so every output is finite for finite inputs.
//
// k_shape: grid (ceil(N / 64), B), 256 threads.  Every work-group of particle b stages x0[b] in LDS (12 N bytes) and recomputes the
// centroid and sum |c|^2 (O(N), strided per thread, then a fixed tree: bitwise the same in every work-group), then handles its 64
// residues, one per lane: each wave walks a contiguous quarter of the partners j (wave-uniform j: an LDS broadcast) in partial sums of
// SH_CHUNK, and the four wave sums are added in wave order.  A pair's energy, count and distance are taken at its lower residue
// (j > n), its force at both.  Wave 0 then gathers the lane's restraints from the per-residue table (partners ascending, energies and
// counts from the entries with partner > residue), writes the gradient, and reduces the tile's energies, counts, minimum and largest
// violation over its lanes by butterfly into the tile's 8 slots of `work`.
// k_shape_finish: one thread per particle adds the tiles in tile order and writes logp and the report.
// No atomics, no scatter: every output is written once, in a fixed order, so two calls on the same inputs are bitwise equal.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_WAVES = SH_THREADS / 64;
constexpr int SH_TILE = 64;             // residues per work-group: one per lane
constexpr int SH_CHUNK = 64;            // partners per inner partial sum (two-level f32 summation)
constexpr int SH_PART = 6;              // per-lane partials a wave leaves in LDS: force x, y, z, energy, count, minimum
constexpr int SH_SLOTS = 8;             // 4-byte slots of `work` per (particle, tile), the SH_* below
constexpr size_t SH_LDS_MAX = 160 * 1024;
enum { SH_E_CLASH, SH_N_CLASH, SH_MIN, SH_E_RST, SH_N_VIOL, SH_MAX_VIOL, SH_ROG, SH_UNUSED };

struct ShParams {
    float rog_max, rog_weight, clash_distance, clash_weight;
    int clash_separation, R2;
};

// dynamic LDS: [xs: 3N] [part: SH_PART * WAVES * 64] [red: WAVES]
size_t sh_lds_bytes(int N) { return sizeof(float) * (3 * (size_t)N + SH_PART * SH_WAVES * 64 + SH_WAVES); }

__device__ inline float sh_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int sh_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum in a fixed tree: butterfly inside each wave, then the wave results in wave order (every thread gets the same bits)
__device__ inline float sh_block_sum(float v, float* red) {
    v = sh_wave_sum(v);
    __syncthreads();                                            // (red is free again)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < SH_WAVES; ++w) r += red[w];
    return r;
}

__global__ __launch_bounds__(SH_THREADS) void k_shape(const float* __restrict__ x0, int N, ShParams q,
                                                      const int32_t* __restrict__ rst_offset, const int32_t* __restrict__ rst_partner,
                                                      const float* __restrict__ rst_lo, const float* __restrict__ rst_hi,
                                                      const float* __restrict__ rst_weight, const float* __restrict__ var_p,
                                                      float* __restrict__ grad, float* __restrict__ work, int pairs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sh_smem[];
    float* xs = reinterpret_cast<float*>(sh_smem);
    float* part = xs + 3 * (size_t)N;
    float* red = part + SH_PART * SH_WAVES * 64;
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* x0b = x0 + (size_t)b * 3 * N;
    for (int i = tid; i < 3 * N; i += SH_THREADS) xs[i] = x0b[i];
    __syncthreads();

    // centroid and radius of gyration
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int n = tid; n < N; n += SH_THREADS) {
        sx += xs[3 * n];
        sy += xs[3 * n + 1];
        sz += xs[3 * n + 2];
    }
    const float mx = sh_block_sum(sx, red) / (float)N, my = sh_block_sum(sy, red) / (float)N, mz = sh_block_sum(sz, red) / (float)N;
    float ss = 0.f;
    for (int n = tid; n < N; n += SH_THREADS) {
        const float cx = xs[3 * n] - mx, cy = xs[3 * n + 1] - my, cz = xs[3 * n + 2] - mz;
        ss += cx * cx + cy * cy + cz * cz;
    }
    const float rog = sqrtf(sh_block_sum(ss, red) / (float)N);

    // pairs: lane = residue n, wave = a contiguous quarter of the partners j
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n = blockIdx.x * SH_TILE + lane;
    const bool live = n < N;
    const float xn = live ? xs[3 * n] : 0.f, yn = live ? xs[3 * n + 1] : 0.f, zn = live ? xs[3 * n + 2] : 0.f;
    float ax = 0.f, ay = 0.f, az = 0.f, ae = 0.f, amin = INFINITY;
    int acnt = 0;
    if (pairs) {
        const int j0 = (int)((int64_t)N * w / SH_WAVES), j1 = (int)((int64_t)N * (w + 1) / SH_WAVES);
        for (int c0 = j0; c0 < j1; c0 += SH_CHUNK) {
            const int c1 = min(c0 + SH_CHUNK, j1);
            float bx = 0.f, by = 0.f, bz = 0.f, be = 0.f;
            for (int j = c0; j < c1; ++j) {
                const float dx = xn - xs[3 * j], dy = yn - xs[3 * j + 1], dz = zn - xs[3 * j + 2];
                const float d = sqrtf(dx * dx + dy * dy + dz * dz);
                const int gap = j - n;
                const bool eligible = live && (gap >= q.clash_separation || -gap >= q.clash_separation);
                const float t = q.clash_distance - d;
                if (eligible && t > 0.f) {
                    const float g = d > 0.f ? t / d : 0.f;          // (coincident residues: no direction)
                    bx += g * dx;
                    by += g * dy;
                    bz += g * dz;
                    if (gap > 0) {
                        be += t * t;
                        ++acnt;
                    }
                }
                if (eligible && gap > 0) amin = fminf(amin, d);
            }
            ax += bx;
            ay += by;
            az += bz;
            ae += be;
        }
    }
    float* mine = part + w * 64 + lane;                             // part[k][w][lane]
    mine[0 * SH_WAVES * 64] = ax;
    mine[1 * SH_WAVES * 64] = ay;
    mine[2 * SH_WAVES * 64] = az;
    mine[3 * SH_WAVES * 64] = ae;
    mine[4 * SH_WAVES * 64] = __int_as_float(acnt);
    mine[5 * SH_WAVES * 64] = amin;
    __syncthreads();
    if (w != 0) return;

    float fx = part[lane], fy = part[SH_WAVES * 64 + lane], fz = part[2 * SH_WAVES * 64 + lane], ec = part[3 * SH_WAVES * 64 + lane];
    int nc = __float_as_int(part[4 * SH_WAVES * 64 + lane]);
    float dmin = part[5 * SH_WAVES * 64 + lane];
    for (int v = 1; v < SH_WAVES; ++v) {
        const float* o = part + v * 64 + lane;
        fx += o[0];
        fy += o[SH_WAVES * 64];
        fz += o[2 * SH_WAVES * 64];
        ec += o[3 * SH_WAVES * 64];
        nc += __float_as_int(o[4 * SH_WAVES * 64]);
        dmin = fminf(dmin, o[5 * SH_WAVES * 64]);
    }

    // the lane's restraints, partners ascending.  (The table is the caller's, validated where it is built; offsets and partners
    // are clamped all the same: they index the table and LDS.)
    float rx = 0.f, ry = 0.f, rz = 0.f, er = 0.f, vmax = 0.f;
    int nv = 0;
    if (live && q.R2 > 0) {
        const int k0 = min(max(rst_offset[n], 0), q.R2), k1 = min(max(rst_offset[n + 1], k0), q.R2);
        for (int k = k0; k < k1; ++k) {
            const int p = min(max(rst_partner[k], 0), N - 1);
            const float dx = xn - xs[3 * p], dy = yn - xs[3 * p + 1], dz = zn - xs[3 * p + 2];
            const float d = sqrtf(dx * dx + dy * dy + dz * dz);
            const float under = fmaxf(rst_lo[k] - d, 0.f), over = fmaxf(d - rst_hi[k], 0.f), wt = rst_weight[k];
            const float g = d > 0.f ? wt * (over - under) / d : 0.f;
            rx += g * dx;
            ry += g * dy;
            rz += g * dz;
            if (p > n) {
                er += wt * (under * under + over * over);
                const float excess = fmaxf(under, over);
                if (excess > 0.f) {
                    ++nv;
                    vmax = fmaxf(vmax, excess);
                }
            }
        }
    }

    if (grad && live) {
        const float over = fmaxf(rog - q.rog_max, 0.f);
        const float kr = rog > 0.f ? q.rog_weight * over / ((float)N * rog) : 0.f;
        const float sc = -1.f / *var_p;
        float* out = grad + ((size_t)b * N + n) * 3;
        out[0] = sc * ((kr * (xn - mx) - q.clash_weight * fx) + rx);
        out[1] = sc * ((kr * (yn - my) - q.clash_weight * fy) + ry);
        out[2] = sc * ((kr * (zn - mz) - q.clash_weight * fz) + rz);
    }

    // the tile's share of the particle's sums (lanes past N hold 0 / +inf)
    ec = sh_wave_sum(ec);
    nc = sh_wave_sum(nc);
    er = sh_wave_sum(er);
    nv = sh_wave_sum(nv);
    for (int o = 32; o > 0; o >>= 1) {
        dmin = fminf(dmin, __shfl_xor(dmin, o, 64));
        vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
    }
    if (lane == 0) {
        float* slot = work + ((size_t)b * gridDim.x + blockIdx.x) * SH_SLOTS;
        slot[SH_E_CLASH] = ec;
        slot[SH_N_CLASH] = __int_as_float(nc);
        slot[SH_MIN] = dmin;
        slot[SH_E_RST] = er;
        slot[SH_N_VIOL] = __int_as_float(nv);
        slot[SH_MAX_VIOL] = vmax;
        slot[SH_ROG] = rog;
        slot[SH_UNUSED] = 0.f;
    }
}

__global__ __launch_bounds__(64) void k_shape_finish(int B, int tiles, ShParams q, const float* __restrict__ var_p,
                                                     const float* __restrict__ work, float* __restrict__ logp, float* __restrict__ report) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float* slot = work + (size_t)b * tiles * SH_SLOTS;
    const float rog = slot[SH_ROG];
    float ec = 0.f, er = 0.f, dmin = INFINITY, vmax = 0.f;
    int nc = 0, nv = 0;
    for (int t = 0; t < tiles; ++t, slot += SH_SLOTS) {
        ec += slot[SH_E_CLASH];
        nc += __float_as_int(slot[SH_N_CLASH]);
        dmin = fminf(dmin, slot[SH_MIN]);
        er += slot[SH_E_RST];
        nv += __float_as_int(slot[SH_N_VIOL]);
        vmax = fmaxf(vmax, slot[SH_MAX_VIOL]);
    }
    const float over = fmaxf(rog - q.rog_max, 0.f);
    const float e_rog = q.rog_weight * over * over, e_clash = q.clash_weight * ec;
    if (logp) logp[b] = -((e_rog + e_clash) + er) / (2.f * *var_p);
    if (report) {
        float* r = report + (size_t)b * GENIE_SHAPE_REPORT;
        r[0] = rog;
        r[1] = dmin;
        r[2] = (float)nc;
        r[3] = e_rog;
        r[4] = e_clash;
        r[5] = er;
        r[6] = (float)nv;
        r[7] = vmax;
    }
}

int sh_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_shape_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

bool sh_bad(float v) { return !(v >= 0.f) || isinf(v); }           // negative, NaN or infinite

}  // namespace

size_t genie_shape_potential_work_bytes(int B, int N) {
    return (B >= 1 && N >= 1) ? (size_t)B * (((size_t)N + SH_TILE - 1) / SH_TILE) * SH_SLOTS * sizeof(float) : 0;
}

int genie_shape_potential(genie_stream_t stream, int B, int N, const float* x0, float rog_max, float rog_weight, float clash_distance,
                          int clash_separation, float clash_weight, int R2, const int32_t* rst_offset, const int32_t* rst_partner,
                          const float* rst_lo, const float* rst_hi, const float* rst_weight, const float* var, float* logp_out,
                          float* grad_out, float* report_out, void* work, size_t work_bytes) {
    if (B < 1 || B > 65535) return sh_refuse("B outside 1..65535");
    if (N < 1) return sh_refuse("N below 1");
    if (!x0) return sh_refuse("x0 is NULL");
    if (!var) return sh_refuse("var is NULL");
    if (!logp_out && !grad_out && !report_out) return sh_refuse("no output asked for (logp_out, grad_out and report_out are NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return sh_refuse("logp_out and grad_out are given together or both NULL");
    if (clash_separation < 1) return sh_refuse("clash_separation below 1");
    if (sh_bad(rog_max)) return sh_refuse("rog_max negative or not finite");
    if (sh_bad(rog_weight)) return sh_refuse("rog_weight negative or not finite");
    if (sh_bad(clash_distance)) return sh_refuse("clash_distance negative or not finite");
    if (sh_bad(clash_weight)) return sh_refuse("clash_weight negative or not finite");
    if (R2 < 0 || (R2 & 1)) return sh_refuse("R2 negative or odd (every restraint is listed at both of its residues)");
    if (R2 > 0 && (!rst_offset || !rst_partner || !rst_lo || !rst_hi || !rst_weight))
        return sh_refuse("R2 > 0 with a NULL restraint table (rst_offset, rst_partner, rst_lo, rst_hi, rst_weight)");
    if (!work || work_bytes < genie_shape_potential_work_bytes(B, N))
        return sh_refuse("work is NULL or work_bytes below genie_shape_potential_work_bytes(B, N)");
    if (reinterpret_cast<uintptr_t>(work) & 3) return sh_refuse("work not 4-byte aligned");
    const size_t lds = sh_lds_bytes(N);
    if (lds > SH_LDS_MAX) return sh_refuse("N too large: the staging of x0[b] does not fit in LDS");
    const ShParams q = {rog_max, rog_weight, clash_distance, clash_weight, clash_separation, R2};
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (N + SH_TILE - 1) / SH_TILE;
    const int pairs = (report_out || clash_weight > 0.f) ? 1 : 0;    // the report's minimum and count need the walk even at weight 0
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_shape), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    float* slots = static_cast<float*>(work);
    hipLaunchKernelGGL(k_shape, dim3(tiles, B), dim3(SH_THREADS), lds, st, x0, N, q, rst_offset, rst_partner, rst_lo, rst_hi, rst_weight,
                       var, grad_out, slots, pairs);
    hipLaunchKernelGGL(k_shape_finish, dim3((B + 63) / 64), dim3(64), 0, st, B, tiles, q, var, (const float*)slots, logp_out, report_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
