// Context potential of twisted-diffusion / SMC sampling (include/genie_hip.h: genie_context_potential): a binding partner, given as
// C-alpha coordinates in the motif file's frame, that follows each particle's own placement of the motif.  For every particle the
// motif's anchors t_k are superposed on the design residues idx[k] that hold them; the fitted rigid motion places the context; the
// placed context is scored against the rest of the design with the binder potential's clash and contact terms; and the gradient is
// the exact gradient of that function, the part that flows through the fitted rotation included.  Three launches.
//
// For particle b with coordinates x_n, anchors a_k = x_idx[k] (k = 0..A-1), motif coordinates t_k and context y_c (c = 0..C-1):
//   abar = mean a_k, tbar = mean t_k, S = sum_k (t_k - tbar)(a_k - abar)^T, (q, lam0) the top eigenpair of Horn's K(S), R = R(q)
//   y'_c = R (y_c - tbar) + abar
//   pairs: n not an anchor, every c: d = |x_n - y'_c|, then E_clash, C, E_contact and logp exactly as in binder_kernels.hip
// With p_nc the pair's force on x_n in units of d(-E/2)/dx (clash_weight (clash_distance - d)_+ (x_n - y'_c) / d, plus
// 6 k / contact_distance^2 r^4 s^2 (x_n - y'_c)), P = sum_nc p_nc and M = sum_nc p_nc (y'_c - abar)^T:
//   grad[b,n]      = (1/var) sum_c p_nc                                                      n not an anchor
//   grad[b,idx[k]] = (1/var) ( -P / A + D^T (t_k - tbar) ),  D = mr_fit_adjoint(eigenpairs, G_R),  G_R = -M R   (horn.h)
// (the reaction on the placed context is h_c = -sum_n p_nc; sum_c h_c = -P reaches the anchors through the centroid, and
// sum_c h_c (y_c - tbar)^T = G_R = d(-E/2)/dR through the rotation; (y_c - tbar)^T = (y'_c - abar)^T R, so the moments are taken
// against the staged coordinates.)
//
// k_context_fit: grid B, one wave per particle.  Marks the residue-to-anchor map (-1: not an anchor), checks the anchor row (an
// index outside 0..N-1 or given twice sets the particle's flag), accumulates abar, tbar and S with lanes striding over the anchors
// and a butterfly, runs mr_eigen, and leaves R, abar, tbar, the four eigenpairs, anchor_rmsd and the flag in `work`; writes pose_out.
// k_context: grid (ceil(N / 64), B), 256 threads.  Every work-group stages w_c = R (y_c - tbar) = y'_c - abar in LDS (12 C bytes,
// transformed while staging) and handles its 64 design residues, one per lane, as x_n - abar; anchors sit out.  Each wave walks a
// contiguous quarter of the context in partial sums of CX_CHUNK; beside the binder kernel's sums every lane keeps the 2 x 9 moments
// p (y'_c - abar)^T of the two terms.  The four wave sums are added in wave order; wave 0 stores the unscaled forces and reduces the
// tile's sums, counts, minimum and 2 x (3 + 9) moment sums by butterfly into the tile's slots.
// k_context_finish: the same grid with 64 threads.  Every work-group adds the tiles in tile order, forms the contact coefficient k,
// P, M, G_R and the adjoint D (the same bits in every work-group); tile 0 writes logp and the report; lane n writes its direct
// gradient, or its anchor share if n is an anchor.  A flagged particle gets logp 0, a gradient of 0 and a report of 0.
// No atomics, no scatter: every output is written once, in a fixed order, so two calls on the same inputs are bitwise equal.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"
#include "horn.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int CX_THREADS = 256;
constexpr int CX_WAVES = CX_THREADS / 64;
constexpr int CX_TILE = 64;             // design residues per work-group: one per lane
constexpr int CX_CHUNK = 64;            // context atoms per inner partial sum (two-level f32 summation)
constexpr int CX_PART = 11;             // per-lane partials a wave leaves in LDS: F xyz, G xyz, clash energy, C, contacts, clashes, min d^2
constexpr int CX_MOM = 18;              // per-wave moment sums: clash p w^T (9), contact p w^T (9)
constexpr int CX_SLOTS = 32;            // 4-byte slots of `work` per (particle, tile), the CX_* below
constexpr int CX_FORCE = 6;             // floats of `work` per (particle, residue): F xyz, G xyz
constexpr int CX_FIT = 40;              // floats of `work` per particle for the fit, the CF_* below
constexpr size_t CX_LDS_MAX = 160 * 1024;
constexpr float CX_R2_FAR = 1e12f;      // r^2 from which r^4 s^2 < 1e-48 is 0 in float32: the force is skipped, no inf * 0
enum { CX_E_CLASH, CX_C, CX_N_CONTACT, CX_N_CLASH, CX_MIN2, CX_N_INTERFACE, CX_P_CLASH, CX_M_CLASH = CX_P_CLASH + 3, CX_P_CONTACT = CX_M_CLASH + 9,
       CX_M_CONTACT = CX_P_CONTACT + 3, CX_USED = CX_M_CONTACT + 9 };
enum { CF_R = 0, CF_ABAR = 9, CF_TBAR = 12, CF_Q = 15, CF_V1 = 19, CF_V2 = 23, CF_V3 = 27, CF_LAM = 31, CF_RMSD = 35, CF_FLAG = 36 };
static_assert(CX_USED <= CX_SLOTS && CF_FLAG < CX_FIT, "slot layout");

struct CxParams {
    float clash_distance, clash_weight, contact_distance, contacts_min, contacts_max, contacts_weight;
    int A, C;
};

// dynamic LDS of k_context: [ws: 3C] [part: CX_PART * WAVES * 64] [mom: CX_MOM * WAVES]
size_t cx_lds_bytes(int C) { return sizeof(float) * (3 * (size_t)C + CX_PART * CX_WAVES * 64 + CX_MOM * CX_WAVES); }

// floats of `work` per particle: [fit: CX_FIT] [anchor map: N] [tile slots: tiles * CX_SLOTS] [forces: N * CX_FORCE]
__host__ __device__ inline size_t cx_stride(int N) {
    const size_t tiles = ((size_t)N + CX_TILE - 1) / CX_TILE;
    return CX_FIT + (size_t)N + tiles * CX_SLOTS + (size_t)N * CX_FORCE;
}

__device__ inline float cx_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int cx_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// s(d) and r^4 s^2 from d^2 (r = d / contact_distance); the latter 0 from CX_R2_FAR on
__device__ inline float cx_switch(float d2, float inv_cd2, float* g) {
    const float r2 = d2 * inv_cd2, r4 = r2 * r2;
    const float s = 1.f / (1.f + r4 * r2);
    *g = r2 < CX_R2_FAR ? r4 * s * s : 0.f;
    return s;
}

__device__ inline void cx_store4(float* p, float4 v) {
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
    p[3] = v.w;
}

__device__ inline float4 cx_load4(const float* p) { return make_float4(p[0], p[1], p[2], p[3]); }

__global__ __launch_bounds__(64) void k_context_fit(const float* __restrict__ x0, int N, int A, const int32_t* __restrict__ anchor_index,
                                                    const float* __restrict__ anchor_xyz, float* __restrict__ work, float* __restrict__ pose) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float* wb = work + (size_t)b * cx_stride(N);
    int* map = reinterpret_cast<int*>(wb + CX_FIT);
    const int32_t* idx = anchor_index + (size_t)b * A;
    const float* xb = x0 + (size_t)b * N * 3;
    for (int n = lane; n < N; n += 64) map[n] = -1;
    __syncthreads();
    // the anchor row: an index outside 0..N-1 is clamped for the reads below and flags the particle
    int bad = 0;
    float ax = 0.f, ay = 0.f, az = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
    for (int k = lane; k < A; k += 64) {
        int i = idx[k];
        if (i < 0 || i >= N) {
            bad = 1;
            i = min(max(i, 0), N - 1);
        } else {
            map[i] = k;
        }
        ax += xb[3 * i];
        ay += xb[3 * i + 1];
        az += xb[3 * i + 2];
        tx += anchor_xyz[3 * k];
        ty += anchor_xyz[3 * k + 1];
        tz += anchor_xyz[3 * k + 2];
    }
    __syncthreads();
    // an index given twice: one of the two anchors does not find itself in the map
    for (int k = lane; k < A; k += 64) {
        const int i = idx[k];
        if (i >= 0 && i < N && map[i] != k) bad = 1;
    }
    bad = cx_wave_sum(bad) > 0 ? 1 : 0;
    const float inv = 1.f / (float)A;
    ax = cx_wave_sum(ax) * inv;
    ay = cx_wave_sum(ay) * inv;
    az = cx_wave_sum(az) * inv;
    tx = cx_wave_sum(tx) * inv;
    ty = cx_wave_sum(ty) * inv;
    tz = cx_wave_sum(tz) * inv;
    MrMat S = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = lane; k < A; k += 64) {
        const int i = min(max(idx[k], 0), N - 1);
        const float cx = xb[3 * i] - ax, cy = xb[3 * i + 1] - ay, cz = xb[3 * i + 2] - az;
        const float ux = anchor_xyz[3 * k] - tx, uy = anchor_xyz[3 * k + 1] - ty, uz = anchor_xyz[3 * k + 2] - tz;
        S.xx += ux * cx;
        S.xy += ux * cy;
        S.xz += ux * cz;
        S.yx += uy * cx;
        S.yy += uy * cy;
        S.yz += uy * cz;
        S.zx += uz * cx;
        S.zy += uz * cy;
        S.zz += uz * cz;
    }
    S.xx = cx_wave_sum(S.xx);
    S.xy = cx_wave_sum(S.xy);
    S.xz = cx_wave_sum(S.xz);
    S.yx = cx_wave_sum(S.yx);
    S.yy = cx_wave_sum(S.yy);
    S.yz = cx_wave_sum(S.yz);
    S.zx = cx_wave_sum(S.zx);
    S.zy = cx_wave_sum(S.zy);
    S.zz = cx_wave_sum(S.zz);
    const MrEigen e = mr_eigen(S);
    const MrMat R = mr_rotation(e.q);
    float ss = 0.f;
    for (int k = lane; k < A; k += 64) {
        const int i = min(max(idx[k], 0), N - 1);
        const float cx = xb[3 * i] - ax, cy = xb[3 * i + 1] - ay, cz = xb[3 * i + 2] - az;
        const float ux = anchor_xyz[3 * k] - tx, uy = anchor_xyz[3 * k + 1] - ty, uz = anchor_xyz[3 * k + 2] - tz;
        const float rx = R.xx * ux + R.xy * uy + R.xz * uz - cx, ry = R.yx * ux + R.yy * uy + R.yz * uz - cy;
        const float rz = R.zx * ux + R.zy * uy + R.zz * uz - cz;
        ss += rx * rx + ry * ry + rz * rz;
    }
    ss = cx_wave_sum(ss);
    if (lane != 0) return;
    const float r[9] = {R.xx, R.xy, R.xz, R.yx, R.yy, R.yz, R.zx, R.zy, R.zz};
    for (int k = 0; k < 9; ++k) wb[CF_R + k] = r[k];
    wb[CF_ABAR] = ax;
    wb[CF_ABAR + 1] = ay;
    wb[CF_ABAR + 2] = az;
    wb[CF_TBAR] = tx;
    wb[CF_TBAR + 1] = ty;
    wb[CF_TBAR + 2] = tz;
    cx_store4(wb + CF_Q, e.q);
    cx_store4(wb + CF_V1, e.v1);
    cx_store4(wb + CF_V2, e.v2);
    cx_store4(wb + CF_V3, e.v3);
    cx_store4(wb + CF_LAM, make_float4(e.lam0, e.lam1, e.lam2, e.lam3));
    wb[CF_RMSD] = sqrtf(ss * inv);
    wb[CF_FLAG] = __int_as_float(bad);
    for (int k = CF_FLAG + 1; k < CX_FIT; ++k) wb[k] = 0.f;
    if (pose) {
        float* p = pose + (size_t)b * 12;
        for (int k = 0; k < 9; ++k) p[k] = bad ? (k % 4 == 0 ? 1.f : 0.f) : r[k];
        p[9] = bad ? 0.f : ax - (R.xx * tx + R.xy * ty + R.xz * tz);
        p[10] = bad ? 0.f : ay - (R.yx * tx + R.yy * ty + R.yz * tz);
        p[11] = bad ? 0.f : az - (R.zx * tx + R.zy * ty + R.zz * tz);
    }
}

__global__ __launch_bounds__(CX_THREADS) void k_context(const float* __restrict__ x0, int N, CxParams q, const float* __restrict__ context,
                                                        float* __restrict__ work, int pairs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cx_smem[];
    float* ws = reinterpret_cast<float*>(cx_smem);
    float* part = ws + 3 * (size_t)q.C;
    float* mom = part + CX_PART * CX_WAVES * 64;
    const int b = blockIdx.y, tid = threadIdx.x;
    float* wb = work + (size_t)b * cx_stride(N);
    const int* map = reinterpret_cast<const int*>(wb + CX_FIT);
    {
        const float* R = wb + CF_R;
        const float tx = wb[CF_TBAR], ty = wb[CF_TBAR + 1], tz = wb[CF_TBAR + 2];
        for (int c = tid; c < q.C; c += CX_THREADS) {
            const float ux = context[3 * c] - tx, uy = context[3 * c + 1] - ty, uz = context[3 * c + 2] - tz;
            ws[3 * c] = R[0] * ux + R[1] * uy + R[2] * uz;
            ws[3 * c + 1] = R[3] * ux + R[4] * uy + R[5] * uz;
            ws[3 * c + 2] = R[6] * ux + R[7] * uy + R[8] * uz;
        }
    }
    __syncthreads();

    // pairs: lane = design residue n (anchors sit out), wave = a contiguous quarter of the context
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n = blockIdx.x * CX_TILE + lane;
    const bool inside = n < N;
    const bool live = inside && map[n] < 0;
    const float* xp = x0 + ((size_t)b * N + (inside ? n : 0)) * 3;
    const float xn = live ? xp[0] - wb[CF_ABAR] : 0.f, yn = live ? xp[1] - wb[CF_ABAR + 1] : 0.f, zn = live ? xp[2] - wb[CF_ABAR + 2] : 0.f;
    const float inv_cd2 = 1.f / (q.contact_distance * q.contact_distance), cd2 = q.contact_distance * q.contact_distance;
    const float cl2 = q.clash_distance * q.clash_distance;
    float fx = 0.f, fy = 0.f, fz = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, ae = 0.f, ac = 0.f, amin = INFINITY;
    float mc[9], mg[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) mc[k] = mg[k] = 0.f;
    int ncon = 0, ncl = 0;
    if (pairs && live) {
        const int m0 = (int)((int64_t)q.C * w / CX_WAVES), m1 = (int)((int64_t)q.C * (w + 1) / CX_WAVES);
        for (int c0 = m0; c0 < m1; c0 += CX_CHUNK) {
            const int c1 = min(c0 + CX_CHUNK, m1);
            float bfx = 0.f, bfy = 0.f, bfz = 0.f, bgx = 0.f, bgy = 0.f, bgz = 0.f, be = 0.f, bc = 0.f;
            float bm[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) bm[k] = 0.f;
            for (int m = c0; m < c1; ++m) {
                const float wx = ws[3 * m], wy = ws[3 * m + 1], wz = ws[3 * m + 2];
                const float dx = xn - wx, dy = yn - wy, dz = zn - wz;
                const float d2 = dx * dx + dy * dy + dz * dz;
                float g;
                bc += cx_switch(d2, inv_cd2, &g);
                const float px = g * dx, py = g * dy, pz = g * dz;
                bgx += px;
                bgy += py;
                bgz += pz;
                bm[0] += px * wx;
                bm[1] += px * wy;
                bm[2] += px * wz;
                bm[3] += py * wx;
                bm[4] += py * wy;
                bm[5] += py * wz;
                bm[6] += pz * wx;
                bm[7] += pz * wy;
                bm[8] += pz * wz;
                if (d2 < cd2) ++ncon;
                if (d2 < cl2) {
                    const float d = sqrtf(d2), t = q.clash_distance - d;
                    const float u = d > 0.f ? t / d : 0.f;              // (coincident atoms: no direction)
                    const float ux = u * dx, uy = u * dy, uz = u * dz;
                    bfx += ux;
                    bfy += uy;
                    bfz += uz;
                    mc[0] += ux * wx;
                    mc[1] += ux * wy;
                    mc[2] += ux * wz;
                    mc[3] += uy * wx;
                    mc[4] += uy * wy;
                    mc[5] += uy * wz;
                    mc[6] += uz * wx;
                    mc[7] += uz * wy;
                    mc[8] += uz * wz;
                    be += t * t;
                    ++ncl;
                }
                amin = fminf(amin, d2);
            }
            fx += bfx;
            fy += bfy;
            fz += bfz;
            gx += bgx;
            gy += bgy;
            gz += bgz;
            ae += be;
            ac += bc;
#pragma unroll
            for (int k = 0; k < 9; ++k) mg[k] += bm[k];
        }
    }
    float* mine = part + w * 64 + lane;                                 // part[k][w][lane]
    mine[0 * CX_WAVES * 64] = fx;
    mine[1 * CX_WAVES * 64] = fy;
    mine[2 * CX_WAVES * 64] = fz;
    mine[3 * CX_WAVES * 64] = gx;
    mine[4 * CX_WAVES * 64] = gy;
    mine[5 * CX_WAVES * 64] = gz;
    mine[6 * CX_WAVES * 64] = ae;
    mine[7 * CX_WAVES * 64] = ac;
    mine[8 * CX_WAVES * 64] = __int_as_float(ncon);
    mine[9 * CX_WAVES * 64] = __int_as_float(ncl);
    mine[10 * CX_WAVES * 64] = amin;
    // the wave's moments over its lanes (lanes that sit out hold 0)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float sc = cx_wave_sum(mc[k]), sg = cx_wave_sum(mg[k]);
        if (lane == 0) {
            mom[w * CX_MOM + k] = sc;
            mom[w * CX_MOM + 9 + k] = sg;
        }
    }
    __syncthreads();
    if (w != 0) return;

    float v[CX_PART - 3];
    for (int k = 0; k < CX_PART - 3; ++k) v[k] = part[k * CX_WAVES * 64 + lane];
    int nc = __float_as_int(part[8 * CX_WAVES * 64 + lane]), nl = __float_as_int(part[9 * CX_WAVES * 64 + lane]);
    float dmin = part[10 * CX_WAVES * 64 + lane];
    for (int o = 1; o < CX_WAVES; ++o) {
        const float* p = part + o * 64 + lane;
        for (int k = 0; k < CX_PART - 3; ++k) v[k] += p[k * CX_WAVES * 64];
        nc += __float_as_int(p[8 * CX_WAVES * 64]);
        nl += __float_as_int(p[9 * CX_WAVES * 64]);
        dmin = fminf(dmin, p[10 * CX_WAVES * 64]);
    }
    const size_t tiles = gridDim.x;
    if (inside) {
        float* f = wb + CX_FIT + (size_t)N + tiles * CX_SLOTS + (size_t)n * CX_FORCE;
        for (int k = 0; k < CX_FORCE; ++k) f[k] = v[k];
    }

    // the tile's share of the particle's sums (lanes that sit out hold 0 / +inf)
    float* slot = wb + CX_FIT + (size_t)N + (size_t)blockIdx.x * CX_SLOTS;
    const float ec = cx_wave_sum(v[6]), cs = cx_wave_sum(v[7]);
    const int ni = cx_wave_sum(nc > 0 ? 1 : 0);
    nc = cx_wave_sum(nc);
    nl = cx_wave_sum(nl);
    for (int o = 32; o > 0; o >>= 1) dmin = fminf(dmin, __shfl_xor(dmin, o, 64));
    float ps[6];
    for (int k = 0; k < 6; ++k) ps[k] = cx_wave_sum(v[k]);
    if (lane < CX_MOM) {                                                // lane k: moment k, the waves in wave order
        float s = mom[lane];
        for (int o = 1; o < CX_WAVES; ++o) s += mom[o * CX_MOM + lane];
        slot[(lane < 9 ? CX_M_CLASH : CX_M_CONTACT - 9) + lane] = s;
    }
    if (lane == 0) {
        slot[CX_E_CLASH] = ec;
        slot[CX_C] = cs;
        slot[CX_N_CONTACT] = __int_as_float(nc);
        slot[CX_N_CLASH] = __int_as_float(nl);
        slot[CX_MIN2] = dmin;
        slot[CX_N_INTERFACE] = __int_as_float(ni);
        for (int k = 0; k < 3; ++k) {
            slot[CX_P_CLASH + k] = ps[k];
            slot[CX_P_CONTACT + k] = ps[3 + k];
        }
        for (int k = CX_USED; k < CX_SLOTS; ++k) slot[k] = 0.f;
    }
}

__global__ __launch_bounds__(64) void k_context_finish(int N, CxParams q, const float* __restrict__ anchor_xyz, const float* __restrict__ var_p,
                                                       const float* __restrict__ work, float* __restrict__ logp, float* __restrict__ grad,
                                                       float* __restrict__ report) {
    const int b = blockIdx.y, lane = threadIdx.x, tiles = gridDim.x;
    const float* wb = work + (size_t)b * cx_stride(N);
    const int* map = reinterpret_cast<const int*>(wb + CX_FIT);
    const float* slots = wb + CX_FIT + (size_t)N;
    const int bad = __float_as_int(wb[CF_FLAG]);

    // the particle's sums, tiles in tile order (the same bits in every work-group)
    float ec = 0.f, cs = 0.f, dmin = INFINITY;
    int nc = 0, nl = 0, ni = 0;
    float pc[3] = {0.f, 0.f, 0.f}, pg[3] = {0.f, 0.f, 0.f}, mc[9], mg[9];
    for (int k = 0; k < 9; ++k) mc[k] = mg[k] = 0.f;
    for (int t = 0; t < tiles; ++t) {
        const float* slot = slots + (size_t)t * CX_SLOTS;
        ec += slot[CX_E_CLASH];
        cs += slot[CX_C];
        nc += __float_as_int(slot[CX_N_CONTACT]);
        nl += __float_as_int(slot[CX_N_CLASH]);
        dmin = fminf(dmin, slot[CX_MIN2]);
        ni += __float_as_int(slot[CX_N_INTERFACE]);
        for (int k = 0; k < 3; ++k) {
            pc[k] += slot[CX_P_CLASH + k];
            pg[k] += slot[CX_P_CONTACT + k];
        }
        for (int k = 0; k < 9; ++k) {
            mc[k] += slot[CX_M_CLASH + k];
            mg[k] += slot[CX_M_CONTACT + k];
        }
    }
    const float below = fmaxf(q.contacts_min - cs, 0.f), above = fmaxf(cs - q.contacts_max, 0.f);

    if (blockIdx.x == 0 && lane == 0) {
        const float e_clash = q.clash_weight * ec, e_contact = q.contacts_weight * (below * below + above * above);
        if (logp) logp[b] = bad ? 0.f : -(e_clash + e_contact) / (2.f * *var_p);
        if (report) {
            float* r = report + (size_t)b * GENIE_CONTEXT_REPORT;
            r[0] = bad ? 0.f : cs;
            r[1] = bad ? 0.f : (float)nc;
            r[2] = bad ? 0.f : (float)ni;
            r[3] = bad ? 0.f : sqrtf(dmin);
            r[4] = bad ? 0.f : (float)nl;
            r[5] = bad ? 0.f : wb[CF_RMSD];
            r[6] = bad ? 0.f : e_clash;
            r[7] = bad ? 0.f : e_contact;
        }
    }

    const int n = blockIdx.x * CX_TILE + lane;
    if (!grad || n >= N) return;
    float* out = grad + ((size_t)b * N + n) * 3;
    if (bad) {
        out[0] = out[1] = out[2] = 0.f;
        return;
    }
    const float inv_cd2 = 1.f / (q.contact_distance * q.contact_distance);
    const float k = q.contacts_weight * (above - below), six_k = 6.f * inv_cd2 * k, sc = 1.f / *var_p;
    const int a = map[n];
    if (a < 0) {
        const float* f = slots + (size_t)tiles * CX_SLOTS + (size_t)n * CX_FORCE;
        out[0] = sc * (q.clash_weight * f[0] + six_k * f[3]);
        out[1] = sc * (q.clash_weight * f[1] + six_k * f[4]);
        out[2] = sc * (q.clash_weight * f[2] + six_k * f[5]);
        return;
    }
    // an anchor: the reaction on the placed context, through the centroid and through the rotation
    float P[3], M[9];
    for (int i = 0; i < 3; ++i) P[i] = q.clash_weight * pc[i] + six_k * pg[i];
    for (int i = 0; i < 9; ++i) M[i] = q.clash_weight * mc[i] + six_k * mg[i];
    const float* R = wb + CF_R;
    MrMat G;                                                            // G_R = -M R
    G.xx = -(M[0] * R[0] + M[1] * R[3] + M[2] * R[6]);
    G.xy = -(M[0] * R[1] + M[1] * R[4] + M[2] * R[7]);
    G.xz = -(M[0] * R[2] + M[1] * R[5] + M[2] * R[8]);
    G.yx = -(M[3] * R[0] + M[4] * R[3] + M[5] * R[6]);
    G.yy = -(M[3] * R[1] + M[4] * R[4] + M[5] * R[7]);
    G.yz = -(M[3] * R[2] + M[4] * R[5] + M[5] * R[8]);
    G.zx = -(M[6] * R[0] + M[7] * R[3] + M[8] * R[6]);
    G.zy = -(M[6] * R[1] + M[7] * R[4] + M[8] * R[7]);
    G.zz = -(M[6] * R[2] + M[7] * R[5] + M[8] * R[8]);
    MrEigen e;
    e.q = cx_load4(wb + CF_Q);
    e.v1 = cx_load4(wb + CF_V1);
    e.v2 = cx_load4(wb + CF_V2);
    e.v3 = cx_load4(wb + CF_V3);
    e.lam0 = wb[CF_LAM];
    e.lam1 = wb[CF_LAM + 1];
    e.lam2 = wb[CF_LAM + 2];
    e.lam3 = wb[CF_LAM + 3];
    const MrMat D = mr_fit_adjoint(e, G);
    const float ux = anchor_xyz[3 * a] - wb[CF_TBAR], uy = anchor_xyz[3 * a + 1] - wb[CF_TBAR + 1], uz = anchor_xyz[3 * a + 2] - wb[CF_TBAR + 2];
    const float inv_a = 1.f / (float)q.A;
    out[0] = sc * (D.xx * ux + D.yx * uy + D.zx * uz - P[0] * inv_a);
    out[1] = sc * (D.xy * ux + D.yy * uy + D.zy * uz - P[1] * inv_a);
    out[2] = sc * (D.xz * ux + D.yz * uy + D.zz * uz - P[2] * inv_a);
}

int cx_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_context_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

bool cx_bad(float v) { return !(v >= 0.f) || isinf(v); }           // negative, NaN or infinite

}  // namespace

size_t genie_context_potential_work_bytes(int B, int N) { return (B >= 1 && N >= 1) ? (size_t)B * cx_stride(N) * sizeof(float) : 0; }

int genie_context_potential(genie_stream_t stream, int B, int N, const float* x0, int A, const int32_t* anchor_index, const float* anchor_xyz,
                            int C, const float* context, float clash_distance, float clash_weight, float contact_distance, float contacts_min,
                            float contacts_max, float contacts_weight, const float* var, float* logp_out, float* grad_out, float* report_out,
                            float* pose_out, void* work, size_t work_bytes) {
    if (B < 1 || B > 65535) return cx_refuse("B outside 1..65535");
    if (N < 1) return cx_refuse("N below 1");
    if (A < 3 || A > N) return cx_refuse("A outside 3..N");
    if (C < 1) return cx_refuse("C below 1");
    if (!x0) return cx_refuse("x0 is NULL");
    if (!anchor_index) return cx_refuse("anchor_index is NULL");
    if (!anchor_xyz) return cx_refuse("anchor_xyz is NULL");
    if (!context) return cx_refuse("context is NULL");
    if (!var) return cx_refuse("var is NULL");
    if (!logp_out && !grad_out && !report_out && !pose_out)
        return cx_refuse("no output asked for (logp_out, grad_out, report_out and pose_out are NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return cx_refuse("logp_out and grad_out are given together or both NULL");
    if (cx_bad(clash_distance)) return cx_refuse("clash_distance negative or not finite");
    if (cx_bad(clash_weight)) return cx_refuse("clash_weight negative or not finite");
    if (cx_bad(contact_distance)) return cx_refuse("contact_distance negative or not finite");
    if (!(contact_distance * contact_distance > 0.f) || isinf(1.f / (contact_distance * contact_distance)))
        return cx_refuse("contact_distance is 0 (or its square is no normal float)");
    if (cx_bad(contacts_min)) return cx_refuse("contacts_min negative or not finite");
    if (!(contacts_max >= 0.f)) return cx_refuse("contacts_max negative or NaN");
    if (contacts_max < contacts_min) return cx_refuse("contacts_max below contacts_min");
    if (cx_bad(contacts_weight)) return cx_refuse("contacts_weight negative or not finite");
    if (!work || work_bytes < genie_context_potential_work_bytes(B, N))
        return cx_refuse("work is NULL or work_bytes below genie_context_potential_work_bytes(B, N)");
    if (reinterpret_cast<uintptr_t>(work) & 3) return cx_refuse("work not 4-byte aligned");
    if (C > GENIE_CONTEXT_MAX_ATOMS) return cx_refuse("C too large: the staging of the context does not fit in LDS");
    const size_t lds = cx_lds_bytes(C);
    if (lds > CX_LDS_MAX) return cx_refuse("C too large: the staging of the context does not fit in LDS");
    const CxParams q = {clash_distance, clash_weight, contact_distance, contacts_min, contacts_max, contacts_weight, A, C};
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (N + CX_TILE - 1) / CX_TILE;
    float* slots = static_cast<float*>(work);
    hipLaunchKernelGGL(k_context_fit, dim3(B), dim3(64), 0, st, x0, N, A, anchor_index, anchor_xyz, slots, pose_out);
    if (logp_out || report_out) {
        // the report's counts and minimum need the walk even at weight 0
        const int pairs = (report_out || clash_weight > 0.f || contacts_weight > 0.f) ? 1 : 0;
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_context), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_context, dim3(tiles, B), dim3(CX_THREADS), lds, st, x0, N, q, context, slots, pairs);
        hipLaunchKernelGGL(k_context_finish, dim3(tiles, B), dim3(64), 0, st, N, q, anchor_xyz, var, (const float*)slots, logp_out, grad_out,
                           report_out);
    }
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
