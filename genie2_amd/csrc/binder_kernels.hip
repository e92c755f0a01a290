// Binder potential of twisted-diffusion / SMC sampling (include/genie_hip.h: genie_binder_potential): how a design sits against a
// fixed target given as C-alpha coordinates -- a clash term over all design-target pairs, a soft count of contacts kept in a range,
// and a minimum of soft contacts on each listed hotspot -- with its gradient and a per-particle report, in two launches.  It is the
// one built-in potential that looks at something that is not being sampled.  The reference has no counterpart.
//
// For particle b with coordinates x_n, n = 0..N-1, and the target y_m, m = 0..M-1, hot[h] the H hotspot indices:
//   d_nm = |x_n - y_m|,  r = d / contact_distance,  s(d) = 1 / (1 + r^6)       (from d^2: no square root)
//   E_clash   = clash_weight    * sum_{n,m} max(0, clash_distance - d_nm)^2
//   C         = sum_{n,m} s(d_nm)
//   E_contact = contacts_weight * ( max(0, contacts_min - C)^2 + max(0, C - contacts_max)^2 )
//   c_h       = sum_n s(d_{n,hot[h]})
//   E_hot     = hotspot_weight  * sum_h max(0, hotspot_contacts - c_h)^2
//   logp[b]   = -(E_clash + E_contact + E_hot) / (2 var)
// With F_n = sum_m (clash_distance - d_nm)_+ (x_n - y_m) / d_nm (0 where d is exactly 0), G_n = sum_m r^4 s^2 (x_n - y_m)
// (ds/dx_n = -6 r^4 s^2 (x_n - y_m) / contact_distance^2), A_n = sum_h (hotspot_contacts - c_h)_+ r^4 s^2 (x_n - y_hot[h]) and
// k = contacts_weight ((C - contacts_max)_+ - (contacts_min - C)_+):
//   grad[b,n] = (1/var) [ clash_weight F_n + 6 / contact_distance^2 (k G_n - hotspot_weight A_n) ]
//
// k_binder: grid (ceil(N / 64), B), 256 threads.  Every work-group stages the target in LDS (12 M bytes) and handles its 64 design
// residues, one per lane, read straight from x0: each wave walks a contiguous quarter of the target (wave-uniform m: an LDS
// broadcast) in partial sums of BD_CHUNK, and the four wave sums are added in wave order.  The waves then share the hotspots (h = w,
// w + 4, ...): the tile's c_h and the number of its residues in contact with the hotspot, by butterfly over the lanes, into the
// tile's hotspot slots of `work`.  Wave 0 stores F_n and G_n unscaled (6 floats per residue) and reduces the tile's sums, counts and
// minimum by butterfly into the tile's 8 slots.
// k_binder_finish: the same grid with 64 threads.  Every work-group adds the tiles of its particle in tile order (C and the c_h are
// global to the particle, so the three hinge coefficients exist only now), lane h taking hotspot h; tile 0 writes logp, the report
// and hotspot_out; every lane scales its residue's F_n and G_n and adds the at most 64 hotspot pairs, hotspots ascending.
// No atomics, no scatter: every output is written once, in a fixed order, so two calls on the same inputs are bitwise equal.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/genie_hip.h"

void set_handle_free_error(const char* msg);           // genie_api.hip: the text of genie_last_error(NULL)

namespace {

constexpr int BD_THREADS = 256;
constexpr int BD_WAVES = BD_THREADS / 64;
constexpr int BD_TILE = 64;             // design residues per work-group: one per lane
constexpr int BD_CHUNK = 64;            // target residues per inner partial sum (two-level f32 summation)
constexpr int BD_PART = 11;             // per-lane partials a wave leaves in LDS: F xyz, G xyz, clash energy, C, contacts, clashes, min d^2
constexpr int BD_SLOTS = 8;             // 4-byte slots of `work` per (particle, tile), the BD_* below
constexpr int BD_FORCE = 6;             // floats of `work` per (particle, residue): F xyz, G xyz
constexpr size_t BD_LDS_MAX = 160 * 1024;
constexpr float BD_R2_FAR = 1e12f;      // r^2 from which r^4 s^2 < 1e-48 is 0 in float32: the force is skipped, no inf * 0
enum { BD_E_CLASH, BD_C, BD_N_CONTACT, BD_N_CLASH, BD_MIN2, BD_N_INTERFACE, BD_UNUSED0, BD_UNUSED1 };

struct BdParams {
    float clash_distance, clash_weight, contact_distance, contacts_min, contacts_max, contacts_weight, hotspot_contacts, hotspot_weight;
    int M, H;
};

// dynamic LDS of k_binder: [ys: 3M] [part: BD_PART * WAVES * 64]
size_t bd_lds_bytes(int M) { return sizeof(float) * (3 * (size_t)M + BD_PART * BD_WAVES * 64); }

// floats of `work` per particle: [tile slots: tiles * BD_SLOTS] [hotspot slots: tiles * 2H] [forces: N * BD_FORCE]
__host__ __device__ inline size_t bd_stride(int N, int H) {
    const size_t tiles = ((size_t)N + BD_TILE - 1) / BD_TILE;
    return tiles * (BD_SLOTS + 2 * (size_t)H) + (size_t)N * BD_FORCE;
}

__device__ inline float bd_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int bd_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// s(d) and r^4 s^2 from d^2 (r = d / contact_distance); the latter 0 from BD_R2_FAR on
__device__ inline float bd_switch(float d2, float inv_cd2, float* g) {
    const float r2 = d2 * inv_cd2, r4 = r2 * r2;
    const float s = 1.f / (1.f + r4 * r2);
    *g = r2 < BD_R2_FAR ? r4 * s * s : 0.f;
    return s;
}

__global__ __launch_bounds__(BD_THREADS) void k_binder(const float* __restrict__ x0, int N, BdParams q, const float* __restrict__ target,
                                                       const int32_t* __restrict__ hotspot, float* __restrict__ work, int pairs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bd_smem[];
    float* ys = reinterpret_cast<float*>(bd_smem);
    float* part = ys + 3 * (size_t)q.M;
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < 3 * q.M; i += BD_THREADS) ys[i] = target[i];
    __syncthreads();

    // pairs: lane = design residue n, wave = a contiguous quarter of the target
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n = blockIdx.x * BD_TILE + lane;
    const bool live = n < N;
    const float* xp = x0 + ((size_t)b * N + (live ? n : 0)) * 3;
    const float xn = live ? xp[0] : 0.f, yn = live ? xp[1] : 0.f, zn = live ? xp[2] : 0.f;
    const float inv_cd2 = 1.f / (q.contact_distance * q.contact_distance), cd2 = q.contact_distance * q.contact_distance;
    const float cl2 = q.clash_distance * q.clash_distance;
    float fx = 0.f, fy = 0.f, fz = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, ae = 0.f, ac = 0.f, amin = INFINITY;
    int ncon = 0, ncl = 0;
    if (pairs && live) {
        const int m0 = (int)((int64_t)q.M * w / BD_WAVES), m1 = (int)((int64_t)q.M * (w + 1) / BD_WAVES);
        for (int c0 = m0; c0 < m1; c0 += BD_CHUNK) {
            const int c1 = min(c0 + BD_CHUNK, m1);
            float bfx = 0.f, bfy = 0.f, bfz = 0.f, bgx = 0.f, bgy = 0.f, bgz = 0.f, be = 0.f, bc = 0.f;
            for (int m = c0; m < c1; ++m) {
                const float dx = xn - ys[3 * m], dy = yn - ys[3 * m + 1], dz = zn - ys[3 * m + 2];
                const float d2 = dx * dx + dy * dy + dz * dz;
                float g;
                bc += bd_switch(d2, inv_cd2, &g);
                bgx += g * dx;
                bgy += g * dy;
                bgz += g * dz;
                if (d2 < cd2) ++ncon;
                if (d2 < cl2) {
                    const float d = sqrtf(d2), t = q.clash_distance - d;
                    const float u = d > 0.f ? t / d : 0.f;              // (coincident atoms: no direction)
                    bfx += u * dx;
                    bfy += u * dy;
                    bfz += u * dz;
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
        }
    }
    float* mine = part + w * 64 + lane;                                 // part[k][w][lane]
    mine[0 * BD_WAVES * 64] = fx;
    mine[1 * BD_WAVES * 64] = fy;
    mine[2 * BD_WAVES * 64] = fz;
    mine[3 * BD_WAVES * 64] = gx;
    mine[4 * BD_WAVES * 64] = gy;
    mine[5 * BD_WAVES * 64] = gz;
    mine[6 * BD_WAVES * 64] = ae;
    mine[7 * BD_WAVES * 64] = ac;
    mine[8 * BD_WAVES * 64] = __int_as_float(ncon);
    mine[9 * BD_WAVES * 64] = __int_as_float(ncl);
    mine[10 * BD_WAVES * 64] = amin;

    // hotspots, shared by the waves: the tile's soft contacts and its residues in contact.  (The list is the caller's, validated
    // where it is built; an index is clamped all the same: it indexes LDS.)
    float* wb = work + (size_t)b * bd_stride(N, q.H);
    float* hslot = wb + (size_t)gridDim.x * BD_SLOTS + (size_t)blockIdx.x * 2 * q.H;
    for (int h = w; h < q.H; h += BD_WAVES) {
        const int m = min(max(hotspot[h], 0), q.M - 1);
        const float dx = xn - ys[3 * m], dy = yn - ys[3 * m + 1], dz = zn - ys[3 * m + 2];
        const float d2 = dx * dx + dy * dy + dz * dz;
        float g;
        const float s = bd_switch(d2, inv_cd2, &g);
        const float c = bd_wave_sum(live ? s : 0.f);
        const int k = bd_wave_sum(live && d2 < cd2 ? 1 : 0);
        if (lane == 0) {
            hslot[2 * h] = c;
            hslot[2 * h + 1] = __int_as_float(k);
        }
    }
    __syncthreads();
    if (w != 0) return;

    float v[BD_PART - 3];
    for (int k = 0; k < BD_PART - 3; ++k) v[k] = part[k * BD_WAVES * 64 + lane];
    int nc = __float_as_int(part[8 * BD_WAVES * 64 + lane]), nl = __float_as_int(part[9 * BD_WAVES * 64 + lane]);
    float dmin = part[10 * BD_WAVES * 64 + lane];
    for (int o = 1; o < BD_WAVES; ++o) {
        const float* p = part + o * 64 + lane;
        for (int k = 0; k < BD_PART - 3; ++k) v[k] += p[k * BD_WAVES * 64];
        nc += __float_as_int(p[8 * BD_WAVES * 64]);
        nl += __float_as_int(p[9 * BD_WAVES * 64]);
        dmin = fminf(dmin, p[10 * BD_WAVES * 64]);
    }
    if (live) {
        float* f = wb + (size_t)gridDim.x * (BD_SLOTS + 2 * (size_t)q.H) + (size_t)n * BD_FORCE;
        for (int k = 0; k < BD_FORCE; ++k) f[k] = v[k];
    }

    // the tile's share of the particle's sums (lanes past N hold 0 / +inf)
    const float ec = bd_wave_sum(v[6]), cs = bd_wave_sum(v[7]);
    const int ni = bd_wave_sum(nc > 0 ? 1 : 0);
    nc = bd_wave_sum(nc);
    nl = bd_wave_sum(nl);
    for (int o = 32; o > 0; o >>= 1) dmin = fminf(dmin, __shfl_xor(dmin, o, 64));
    if (lane == 0) {
        float* slot = wb + (size_t)blockIdx.x * BD_SLOTS;
        slot[BD_E_CLASH] = ec;
        slot[BD_C] = cs;
        slot[BD_N_CONTACT] = __int_as_float(nc);
        slot[BD_N_CLASH] = __int_as_float(nl);
        slot[BD_MIN2] = dmin;
        slot[BD_N_INTERFACE] = __int_as_float(ni);
        slot[BD_UNUSED0] = 0.f;
        slot[BD_UNUSED1] = 0.f;
    }
}

__global__ __launch_bounds__(64) void k_binder_finish(const float* __restrict__ x0, int N, BdParams q, const float* __restrict__ target,
                                                      const int32_t* __restrict__ hotspot, const float* __restrict__ var_p,
                                                      const float* __restrict__ work, float* __restrict__ logp, float* __restrict__ grad,
                                                      float* __restrict__ report, float* __restrict__ hotspot_out) {
    __shared__ float hy[3 * GENIE_BINDER_MAX_HOTSPOTS], hu[GENIE_BINDER_MAX_HOTSPOTS];
    const int b = blockIdx.y, lane = threadIdx.x, tiles = gridDim.x;
    const float* wb = work + (size_t)b * bd_stride(N, q.H);

    // the particle's sums, tiles in tile order (the same bits in every work-group)
    float ec = 0.f, cs = 0.f, dmin = INFINITY;
    int nc = 0, nl = 0, ni = 0;
    for (int t = 0; t < tiles; ++t) {
        const float* slot = wb + (size_t)t * BD_SLOTS;
        ec += slot[BD_E_CLASH];
        cs += slot[BD_C];
        nc += __float_as_int(slot[BD_N_CONTACT]);
        nl += __float_as_int(slot[BD_N_CLASH]);
        dmin = fminf(dmin, slot[BD_MIN2]);
        ni += __float_as_int(slot[BD_N_INTERFACE]);
    }
    // lane h: hotspot h
    float ch = 0.f, under = 0.f;
    int touched = 0;
    if (lane < q.H) {
        const float* hs = wb + (size_t)tiles * BD_SLOTS + 2 * lane;
        for (int t = 0; t < tiles; ++t, hs += 2 * q.H) {
            ch += hs[0];
            touched += __float_as_int(hs[1]);
        }
        under = fmaxf(q.hotspot_contacts - ch, 0.f);
        const int m = min(max(hotspot[lane], 0), q.M - 1);
        hy[3 * lane] = target[3 * m];
        hy[3 * lane + 1] = target[3 * m + 1];
        hy[3 * lane + 2] = target[3 * m + 2];
        hu[lane] = under;
    }
    __syncthreads();
    const float below = fmaxf(q.contacts_min - cs, 0.f), above = fmaxf(cs - q.contacts_max, 0.f);

    if (blockIdx.x == 0) {
        const float eh = q.hotspot_weight * bd_wave_sum(under * under);
        const int nh = bd_wave_sum(touched > 0 ? 1 : 0);
        if (hotspot_out && lane < q.H) hotspot_out[(size_t)b * q.H + lane] = ch;
        if (lane == 0) {
            const float e_clash = q.clash_weight * ec, e_contact = q.contacts_weight * (below * below + above * above);
            if (logp) logp[b] = -((e_clash + e_contact) + eh) / (2.f * *var_p);
            if (report) {
                float* r = report + (size_t)b * GENIE_BINDER_REPORT;
                r[0] = cs;
                r[1] = (float)nc;
                r[2] = (float)ni;
                r[3] = sqrtf(dmin);
                r[4] = (float)nl;
                r[5] = (float)nh;
                r[6] = e_clash;
                r[7] = e_contact;
                r[8] = eh;
            }
        }
    }

    const int n = blockIdx.x * BD_TILE + lane;
    if (!grad || n >= N) return;
    const float* xp = x0 + ((size_t)b * N + n) * 3;
    const float xn = xp[0], yn = xp[1], zn = xp[2];
    const float inv_cd2 = 1.f / (q.contact_distance * q.contact_distance);
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int h = 0; h < q.H; ++h) {
        const float dx = xn - hy[3 * h], dy = yn - hy[3 * h + 1], dz = zn - hy[3 * h + 2];
        float g;
        (void)bd_switch(dx * dx + dy * dy + dz * dz, inv_cd2, &g);
        g *= hu[h];
        ax += g * dx;
        ay += g * dy;
        az += g * dz;
    }
    const float* f = wb + (size_t)tiles * (BD_SLOTS + 2 * (size_t)q.H) + (size_t)n * BD_FORCE;
    const float k = q.contacts_weight * (above - below), six = 6.f * inv_cd2, sc = 1.f / *var_p;
    float* out = grad + ((size_t)b * N + n) * 3;
    out[0] = sc * (q.clash_weight * f[0] + six * (k * f[3] - q.hotspot_weight * ax));
    out[1] = sc * (q.clash_weight * f[1] + six * (k * f[4] - q.hotspot_weight * ay));
    out[2] = sc * (q.clash_weight * f[2] + six * (k * f[5] - q.hotspot_weight * az));
}

int bd_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "genie_binder_potential: %s", why);
    set_handle_free_error(msg);
    return GENIE_E_ARG;
}

bool bd_bad(float v) { return !(v >= 0.f) || isinf(v); }           // negative, NaN or infinite

}  // namespace

size_t genie_binder_potential_work_bytes(int B, int N, int H) {
    return (B >= 1 && N >= 1 && H >= 0 && H <= GENIE_BINDER_MAX_HOTSPOTS) ? (size_t)B * bd_stride(N, H) * sizeof(float) : 0;
}

int genie_binder_potential(genie_stream_t stream, int B, int N, const float* x0, int M, const float* target, int H, const int32_t* hotspot,
                           float clash_distance, float clash_weight, float contact_distance, float contacts_min, float contacts_max,
                           float contacts_weight, float hotspot_contacts, float hotspot_weight, const float* var, float* logp_out,
                           float* grad_out, float* report_out, float* hotspot_out, void* work, size_t work_bytes) {
    if (B < 1 || B > 65535) return bd_refuse("B outside 1..65535");
    if (N < 1) return bd_refuse("N below 1");
    if (M < 1) return bd_refuse("M below 1");
    if (!x0) return bd_refuse("x0 is NULL");
    if (!target) return bd_refuse("target is NULL");
    if (!var) return bd_refuse("var is NULL");
    if (H < 0 || H > GENIE_BINDER_MAX_HOTSPOTS) return bd_refuse("H outside 0..GENIE_BINDER_MAX_HOTSPOTS (64)");
    if (H > 0 && !hotspot) return bd_refuse("H > 0 with a NULL hotspot list");
    if (hotspot_out && H == 0) return bd_refuse("hotspot_out given with H = 0");
    if (!logp_out && !grad_out && !report_out && !hotspot_out)
        return bd_refuse("no output asked for (logp_out, grad_out, report_out and hotspot_out are NULL)");
    if ((logp_out == nullptr) != (grad_out == nullptr)) return bd_refuse("logp_out and grad_out are given together or both NULL");
    if (bd_bad(clash_distance)) return bd_refuse("clash_distance negative or not finite");
    if (bd_bad(clash_weight)) return bd_refuse("clash_weight negative or not finite");
    if (bd_bad(contact_distance)) return bd_refuse("contact_distance negative or not finite");
    if (!(contact_distance * contact_distance > 0.f) || isinf(1.f / (contact_distance * contact_distance)))
        return bd_refuse("contact_distance is 0 (or its square is no normal float)");
    if (bd_bad(contacts_min)) return bd_refuse("contacts_min negative or not finite");
    if (!(contacts_max >= 0.f)) return bd_refuse("contacts_max negative or NaN");
    if (contacts_max < contacts_min) return bd_refuse("contacts_max below contacts_min");
    if (bd_bad(contacts_weight)) return bd_refuse("contacts_weight negative or not finite");
    if (bd_bad(hotspot_contacts)) return bd_refuse("hotspot_contacts negative or not finite");
    if (bd_bad(hotspot_weight)) return bd_refuse("hotspot_weight negative or not finite");
    if (!work || work_bytes < genie_binder_potential_work_bytes(B, N, H))
        return bd_refuse("work is NULL or work_bytes below genie_binder_potential_work_bytes(B, N, H)");
    if (reinterpret_cast<uintptr_t>(work) & 3) return bd_refuse("work not 4-byte aligned");
    const size_t lds = bd_lds_bytes(M);
    if (lds > BD_LDS_MAX) return bd_refuse("M too large: the staging of the target does not fit in LDS");
    const BdParams q = {clash_distance, clash_weight, contact_distance, contacts_min, contacts_max, contacts_weight, hotspot_contacts,
                        hotspot_weight, M, H};
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (N + BD_TILE - 1) / BD_TILE;
    // the report's counts and minimum need the walk even at weight 0
    const int pairs = (report_out || clash_weight > 0.f || contacts_weight > 0.f) ? 1 : 0;
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_binder), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    float* slots = static_cast<float*>(work);
    hipLaunchKernelGGL(k_binder, dim3(tiles, B), dim3(BD_THREADS), lds, st, x0, N, q, target, hotspot, slots, pairs);
    hipLaunchKernelGGL(k_binder_finish, dim3(tiles, B), dim3(64), 0, st, x0, N, q, target, hotspot, var, (const float*)slots, logp_out,
                       grad_out, report_out, hotspot_out);
    return hipGetLastError() == hipSuccess ? GENIE_OK : GENIE_E_HIP;
}
