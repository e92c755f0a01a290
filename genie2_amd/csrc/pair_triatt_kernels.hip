// Triangular attention of the pair stack (genie/model/modules/triangular_attention.py:30-144 on
// primitives.py:163-281; Algorithms 13 / 14 of the AlphaFold 2 supplement), eval mode:
//
//   x = LayerNorm(p);  tb[b,q,k,h] = x[b,q,k,:] . W_b[h,:]
//   a[b,i,h,q,k] = (x[b,i,q] Wq_h) . (x[b,i,k] Wk_h) / sqrt(c) + 1e9 (mask[b,i,k] - 1) + tb[b,q,k,h]
//   o = softmax_k(a) (x[b,i,k] Wv_h);   p[b,i,q,:] += W_o (o * sigmoid(W_g x[b,i,q] + b_g)) + b_o
//
// The ending node is the same on p with its i / j axes swapped: p is transposed into a p-sized scratch (the triangle
// multiplication's x buffer, idle here), the module runs on the copy with row-contiguous access throughout, and the
// result is transposed back (one element is a 512-byte channel vector, so both copies are coalesced as they stand).
//
// Structure of one module (launch_triatt):
//   k_triatt_ln (bias pass)   LayerNorm + the H bias dot products of every pair, plain f32 FMAs -> tb [B,H,N,NPK]
//   per slab of S attention rows (b, i)  -- S N pair rows, sized so that the slab's q|k|v|g (2 KiB per pair) stays cache resident:
//     k_triatt_ln             LayerNorm of the slab -> xn
//     k_gemm_rows[_hx]        xn [S N,128] x [512,128]^T -> q|k|v|g   (split-f16 in hx mode, f32 MFMA in f32 mode)
//     k_triatt_core           flash-style attention per (row, head), gate applied, result written over q
//     k_gemm_rows[_hx]        gated o x W_o^T + b_o + p -> p   (residual add in place)
// The logits [B,N,H,N,N] exist only as 32 x 32 accumulator tiles.
//
// k_triatt_core: one work-group = (attention row, head, 128 queries); each of its 4 waves owns 32 queries.
//   S^T = K Q^T: the MFMA's A operand is a 32-key tile from LDS, B the wave's Q fragments (registers, loaded once), so a lane
//   holds ONE query column and 16 of the tile's 32 keys in its accumulator registers: the running max / sum of the online
//   softmax are per-lane scalars and one cross-half shuffle per tile completes them.  P^T (those same registers) is directly
//   the B operand of O^T = V^T P^T ("D^T chaining", hx.h), with V^T read from LDS in the matching key order.
//   hx mode: Q, K, V and P are split in f16 halves (hx.h) and each product is three f16 MFMAs: Q / K / V with load-time
//   scales from their weights' Cauchy-Schwarz bounds (genie_api.hip), P (in [0, 1]) with 2^14.  f32 mode: v_mfma_f32_32x32x2_f32.
//   Scaling, bias, max, exp and sum are f32 VALU work in both.
//   LDS: K tile 32 x (C + 4) f32, V^T tile C x 36 f32, 32 mask floats: 9.3 KiB at C = 32.  Registers: S^T, P and O^T tiles
//   (16 each) + Q fragments (16 in hx mode at C = 32).
//   Masked keys (padded residues, tile tail beyond N) are excluded outright -- in the reference exp(-1e9 - max) underflows to
//   exactly 0 in a valid row; what padded rows receive is free (the layer ends with p *= mask) and stays finite.
// No atomics; every reduction has a fixed order: results are bitwise reproducible.
#include <algorithm>
#include "hx.h"

#define TA_LDV 36            // V^T tile: keys + 4 pad
#define TA_SP 16384.0f       // scale of the probabilities' f16 split

// LayerNorm of pair rows row0 .. row0 + nrows - 1 of X [B N N][128] (16 lanes per row, 8 channels each) and, per row,
//   xn != NULL: the normalised row -> xn[local row][128]
//   tb != NULL: its H bias values   -> tb[((b H + h) N + q) NPK + k],  row = (b N + q) N + k
__global__ __launch_bounds__(256) void k_triatt_ln(const float* __restrict__ X, size_t row0, int nrows, int N,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   const float* __restrict__ wb, int H, float* __restrict__ xn,
                                                   float* __restrict__ tb, int NPK) {
    const int tid = threadIdx.x, sub = tid & 15;
    const int lrow = blockIdx.x * 16 + (tid >> 4);
    const bool ok = lrow < nrows;
    const size_t row = row0 + (size_t)(ok ? lrow : nrows - 1);      // idle lanes shadow the last row: shuffles stay uniform
    const float* x = X + row * 128 + sub * 8;
    const float4 a = *reinterpret_cast<const float4*>(x), b = *reinterpret_cast<const float4*>(x + 4);
    float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.0f / 128.0f);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] -= mean; ss += v[e] * v[e]; }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) ss += __shfl_xor(ss, o);
    const float rstd = 1.0f / sqrtf(ss * (1.0f / 128.0f) + GENIE_LN_EPS);
    const float4 g0 = *reinterpret_cast<const float4*>(gamma + sub * 8), g1 = *reinterpret_cast<const float4*>(gamma + sub * 8 + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(beta + sub * 8), b1 = *reinterpret_cast<const float4*>(beta + sub * 8 + 4);
    const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = v[e] * rstd * gg[e] + bb[e];
    if (xn && ok) {
        float* o = xn + (size_t)lrow * 128 + sub * 8;
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    if (tb) {
        const size_t nn = (size_t)N * N;
        const size_t bi = row / nn, rem = row - bi * nn;
        const size_t q = rem / N, k = rem - q * N;
        for (int h = 0; h < H; ++h) {
            const float* w = wb + h * 128 + sub * 8;
            const float4 w0 = *reinterpret_cast<const float4*>(w), w1 = *reinterpret_cast<const float4*>(w + 4);
            float d = v[0] * w0.x;
            d = fmaf(v[1], w0.y, d); d = fmaf(v[2], w0.z, d); d = fmaf(v[3], w0.w, d);
            d = fmaf(v[4], w1.x, d); d = fmaf(v[5], w1.y, d); d = fmaf(v[6], w1.z, d); d = fmaf(v[7], w1.w, d);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) d += __shfl_xor(d, o);
            if (ok && sub == 0) tb[((bi * H + h) * N + q) * NPK + k] = d;
        }
    }
}

// out[b,i,j,:] = in[b,j,i,:]   ([B,N,N,128] f32; one thread per float4)
__global__ __launch_bounds__(256) void k_triatt_transpose(const float* __restrict__ in, float* __restrict__ out, int N, size_t n4) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n4) return;
    const size_t c4 = t & 31, pr = t >> 5;
    const size_t nn = (size_t)N * N;
    const size_t b = pr / nn, rem = pr - b * nn;
    const size_t i = rem / N, j = rem - i * N;
    *reinterpret_cast<float4*>(out + pr * 128 + c4 * 4) = *reinterpret_cast<const float4*>(in + ((b * N + j) * N + i) * 128 + c4 * 4);
}

struct TriAttCoreP {
    float* qkvg;             // [slab pair rows][512]: q | k | v | g, head h at columns h C .. of each; gated o replaces q
    const float* tb;         // [B][H][N][NPK]
    const float* rmaskf;     // [B][N]
    int ar0;                 // first attention row (b N + i) of the slab
    int N, NPK, H;
    float cqk;               // 1 / sqrt(C) (hx: / (sq sk))
    float sq, sk, sv, cpv;   // hx operand scales, 1 / (TA_SP sv)
};

template <int C, bool HX>
__global__ __launch_bounds__(256) void k_triatt_core(const TriAttCoreP P) {
    constexpr int LDK = C + 4, F = C / 4, NCK = C / 16, NKB = C / 8;
    __shared__ __attribute__((aligned(16))) float sK[32 * LDK];
    __shared__ __attribute__((aligned(16))) float sVt[C * TA_LDV];
    __shared__ __attribute__((aligned(16))) float sM[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, li = lane & 31;
    const int N = P.N, h = blockIdx.y;
    const int ar = P.ar0 + blockIdx.z, b = ar / N;
    float* base = P.qkvg + (size_t)blockIdx.z * N * 512 + h * C;
    const int q0 = blockIdx.x * 128 + wave * 32;
    const bool wave_on = q0 < N;                 // (wave-uniform; idle waves still stage tiles and meet every barrier)
    const int q = q0 + li;
    const bool q_ok = q < N;
    const float* qrow = base + (size_t)(q_ok ? q : 0) * 512;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // Q fragments, once
    h8 qh[NCK], ql[NCK];
    float4 qf[NKB];
    if constexpr (HX) {
#pragma unroll
        for (int ck = 0; ck < NCK; ++ck) {
            const float4 a = q_ok ? *reinterpret_cast<const float4*>(qrow + 16 * ck + 8 * hh) : z4;
            const float4 c = q_ok ? *reinterpret_cast<const float4*>(qrow + 16 * ck + 8 * hh + 4) : z4;
            const float x[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
            hx_split8(x, P.sq, qh[ck], ql[ck]);
        }
    } else {
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) qf[kb] = q_ok ? *reinterpret_cast<const float4*>(qrow + 8 * kb + 4 * hh) : z4;
    }

    // staging role: one float4 of K and of V per thread and tile
    const bool st_on = tid < 32 * F;
    const int skey = tid / F, sc4 = (tid % F) * 4;
    const int nt = (N + 31) / 32;
    auto ld_tile = [&](int t, float4& kr, float4& vr, float& mr) {
        const int key = 32 * t + skey;
        const bool ok = st_on && key < N;
        const float* r = base + (size_t)(ok ? key : 0) * 512 + sc4;
        kr = ok ? *reinterpret_cast<const float4*>(r + 128) : z4;
        vr = ok ? *reinterpret_cast<const float4*>(r + 256) : z4;
        mr = (tid < 32 && 32 * t + tid < N) ? P.rmaskf[(size_t)b * N + 32 * t + tid] : 0.f;
    };
    float4 kr, vr;
    float mr;
    ld_tile(0, kr, vr, mr);

    const float* tbrow = P.tb + (((size_t)b * P.H + h) * N + (q_ok ? q : 0)) * P.NPK;
    f32x16 o = zero16();
    float m_run = -1e30f, l_run = 0.f;

    for (int t = 0; t < nt; ++t) {
        __syncthreads();                         // the previous tile's readers are done
        if (st_on) {
            *reinterpret_cast<float4*>(&sK[skey * LDK + sc4]) = kr;
            sVt[(sc4 + 0) * TA_LDV + skey] = vr.x; sVt[(sc4 + 1) * TA_LDV + skey] = vr.y;
            sVt[(sc4 + 2) * TA_LDV + skey] = vr.z; sVt[(sc4 + 3) * TA_LDV + skey] = vr.w;
        }
        if (tid < 32) sM[tid] = mr;
        __syncthreads();
        if (t + 1 < nt) ld_tile(t + 1, kr, vr, mr);     // in flight under this tile's arithmetic
        if (!wave_on) continue;
        const int k0 = 32 * t;

        // bias of this lane's 16 (key, q) pairs: keys k0 + 8 j + 4 hh + e
        float4 tb4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k0 + 8 * j + 4 * hh;
            tb4[j] = (q_ok && kk < P.NPK) ? *reinterpret_cast<const float4*>(tbrow + kk) : z4;
        }

        // S^T = K Q^T
        f32x16 s = zero16();
        if constexpr (HX) {
#pragma unroll
            for (int ck = 0; ck < NCK; ++ck) {
                const float* kp = &sK[li * LDK + 16 * ck + 8 * hh];
                const float4 a = *reinterpret_cast<const float4*>(kp), c = *reinterpret_cast<const float4*>(kp + 4);
                const float x[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
                h8 kh, kl;
                hx_split8(x, P.sk, kh, kl);
                MFH3(kh, kl, qh[ck], ql[ck], s);
            }
        } else {
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) s = mfma_8k(lfrag(sK, LDK, 0, kb, lane), qf[kb], s);
        }

        // online softmax, f32
        float pr[16];
        bool kv[16];
        float mx = -1e30f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 mk = *reinterpret_cast<const float4*>(&sM[8 * j + 4 * hh]);
            const float me[4] = {mk.x, mk.y, mk.z, mk.w}, te[4] = {tb4[j].x, tb4[j].y, tb4[j].z, tb4[j].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * j + e;
                kv[r] = me[e] != 0.f;
                pr[r] = fmaf(s[r], P.cqk, te[e]);
                mx = kv[r] ? fmaxf(mx, pr[r]) : mx;
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __expf(m_run - m_new);
        m_run = m_new;
        float lsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pr[r] = kv[r] ? __expf(pr[r] - m_new) : 0.f;
            lsum += pr[r];
        }
        l_run = fmaf(l_run, alpha, lsum);
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= alpha;

        // O^T += V^T P^T
        const int ch = li < C ? li : C - 1;
        const bool ch_ok = li < C;
        if constexpr (HX) {
#pragma unroll
            for (int ck = 0; ck < 2; ++ck) {
                const float* vp = &sVt[ch * TA_LDV + 16 * ck + 4 * hh];
                const float4 a = ch_ok ? *reinterpret_cast<const float4*>(vp) : z4;
                const float4 c = ch_ok ? *reinterpret_cast<const float4*>(vp + 8) : z4;
                const float x[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
                h8 vh, vl, ph, pl;
                hx_split8(x, P.sv, vh, vl);
                const float y[8] = {pr[8 * ck], pr[8 * ck + 1], pr[8 * ck + 2], pr[8 * ck + 3],
                                    pr[8 * ck + 4], pr[8 * ck + 5], pr[8 * ck + 6], pr[8 * ck + 7]};
                hx_split8(y, TA_SP, ph, pl);
                MFH3(vh, vl, ph, pl, o);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 a = ch_ok ? *reinterpret_cast<const float4*>(&sVt[ch * TA_LDV + 8 * j + 4 * hh]) : z4;
                o = mfma_8k(a, make_float4(pr[4 * j], pr[4 * j + 1], pr[4 * j + 2], pr[4 * j + 3]), o);
            }
        }
    }
    if (!wave_on) return;
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = (l_tot > 0.f ? 1.0f / l_tot : 0.f) * (HX ? P.cpv : 1.0f);
    if (!q_ok) return;
    // gate and store over q: channels acc_row(r) = 8 j + 4 hh + e, e = 0..3 contiguous
    float* orow = base + (size_t)q * 512;
#pragma unroll
    for (int j = 0; j < C / 8; ++j) {
        const int c0 = 8 * j + 4 * hh;
        const float4 g = *reinterpret_cast<const float4*>(orow + 384 + c0);
        float4 r;
        r.x = o[4 * j] * inv * sigmoidf_(g.x);
        r.y = o[4 * j + 1] * inv * sigmoidf_(g.y);
        r.z = o[4 * j + 2] * inv * sigmoidf_(g.z);
        r.w = o[4 * j + 3] * inv * sigmoidf_(g.w);
        *reinterpret_cast<float4*>(orow + c0) = r;
    }
}

// attention rows per slab: q|k|v|g of a slab is at most 32 MiB (+ one row), and never more than half of the tensor, so that
// slab + normalised copy + bias stay below one module's q, k, v, g even at the smallest sizes (workspace cap)
static int triatt_slab(int B, int N) { return std::max(1, std::min(16384 / N, B * N / 2)); }

int triatt_npk(int N) { return (N + 3) & ~3; }
void triatt_ws_floats(const genie_dims_t& d, int B, int N, size_t* tb, size_t* xn, size_t* qkvg) {
    const size_t rows = (size_t)triatt_slab(B, N) * N;
    *tb = (size_t)B * d.n_head_tri * N * triatt_npk(N);
    *xn = rows * 128;
    *qkvg = rows * 512;
}

void launch_triatt(genie_ctx* h, hipStream_t st, const TriAttW& w, bool starting) {
    const genie_dims_t& d = h->d;
    const int B = h->B, N = h->N, H = d.n_head_tri, C = d.c_hidden_tri_att, NPK = triatt_npk(N);
    const size_t P = (size_t)B * N * N, n4 = P * 32;
    float* X = h->p;
    if (!starting) {
        ProfScope ps(h, st, KC_TRIATT_TRANSPOSE);
        hipLaunchKernelGGL(k_triatt_transpose, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, h->p, h->xcm, N, n4);
        X = h->xcm;
    }
    {
        ProfScope ps(h, st, KC_TRIATT_PROJ);
        hipLaunchKernelGGL(k_triatt_ln, dim3((unsigned)((P + 15) / 16)), dim3(256), 0, st, X, (size_t)0, (int)P, N, w.ln_g, w.ln_b, w.wb, H,
                           (float*)nullptr, h->ta_tb, NPK);
    }
    const int S = triatt_slab(B, N);
    TriAttCoreP cp;
    cp.qkvg = h->ta_qkvg; cp.tb = h->ta_tb; cp.rmaskf = h->rmaskf; cp.N = N; cp.NPK = NPK; cp.H = H;
    const float rs = 1.0f / sqrtf((float)C);
    cp.cqk = h->hx ? rs / (w.sq * w.sk) : rs;
    cp.sq = w.sq; cp.sk = w.sk; cp.sv = w.sv; cp.cpv = 1.0f / (TA_SP * w.sv);
    for (int ar0 = 0; ar0 < B * N; ar0 += S) {
        const int ns = std::min(S, B * N - ar0), rows = ns * N;
        float* Xs = X + (size_t)ar0 * N * 128;
        {
            ProfScope ps(h, st, KC_TRIATT_PROJ);
            hipLaunchKernelGGL(k_triatt_ln, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, Xs, (size_t)0, rows, N, w.ln_g, w.ln_b,
                               w.wb, H, h->ta_xn, (float*)nullptr, NPK);
        }
        launch_gemm_rows(h, st, h->ta_xn, 128, rows, 128, w.proj_w, 512, w.proj_b, nullptr, 0, nullptr, 0, h->ta_qkvg, 512, KC_TRIATT_PROJ);
        {
            ProfScope ps(h, st, KC_TRIATT_CORE);
            cp.ar0 = ar0;
            const dim3 grid((N + 127) / 128, H, ns);
            if (C == 32) {
                if (h->hx) hipLaunchKernelGGL((k_triatt_core<32, true>), grid, dim3(256), 0, st, cp);
                else hipLaunchKernelGGL((k_triatt_core<32, false>), grid, dim3(256), 0, st, cp);
            } else {
                if (h->hx) hipLaunchKernelGGL((k_triatt_core<16, true>), grid, dim3(256), 0, st, cp);
                else hipLaunchKernelGGL((k_triatt_core<16, false>), grid, dim3(256), 0, st, cp);
            }
        }
        launch_gemm_rows(h, st, h->ta_qkvg, 512, rows, 128, w.out_w, 128, w.out_b, Xs, 128, nullptr, 0, Xs, 128, KC_TRIATT_PROJ);
    }
    if (!starting) {
        ProfScope ps(h, st, KC_TRIATT_TRANSPOSE);
        hipLaunchKernelGGL(k_triatt_transpose, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, h->xcm, h->p, N, n4);
    }
}
