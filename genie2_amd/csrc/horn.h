// The rotation of a superposed fit, shared by the motif potentials (smc_kernels.hip) and the symmetry potential
// (symmetry_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

constexpr int MR_SWEEPS = 6;            // cyclic Jacobi sweeps of the 4x4 (quadratic convergence: 4 reach float32 on these matrices)

// R = argmin over proper rotations of sum_m |c(m) - R t(m)|^2 for centred c and t is Horn's quaternion: the eigenvector of the
// largest eigenvalue of the symmetric 4x4 matrix built from the correlation sum_m t c^T, found by MR_SWEEPS cyclic Jacobi sweeps in
// float32 with the matrix and the eigenvectors in named registers (a quaternion is always a proper rotation: a mirror image does not
// fit).  A collinear selection has a double largest eigenvalue: Jacobi still returns one unit eigenvector of it, the score is the
// same for all of them.  (Plain arithmetic, __host__ too: it can be run on the CPU against a float64 fit.)
struct MrMat {
    float xx, xy, xz, yx, yy, yz, zx, zy, zz;
};

// one Jacobi rotation in the (p, q) plane: a_pq -> 0.  (a1p, a1q), (a2p, a2q): the two other rows' entries in columns p and q;
// v*p, v*q: columns p and q of the eigenvector matrix.
__host__ __device__ __forceinline__ void mr_mix(float& x, float& y, float s, float tau) {
    const float g = x, h = y;
    x = g - s * (h + tau * g);
    y = h + s * (g - tau * h);
}

__host__ __device__ __forceinline__ void mr_rot(float& app, float& aqq, float& apq, float& a1p, float& a1q, float& a2p, float& a2q,
                                                float& v0p, float& v0q, float& v1p, float& v1q, float& v2p, float& v2q, float& v3p,
                                                float& v3q) {
    const float th = (aqq - app) / (2.f * apq);
    float t = copysignf(1.f, th) / (fabsf(th) + sqrtf(th * th + 1.f));      // (th = +-inf gives 0)
    t = apq == 0.f ? 0.f : t;                                               // (and th = 0/0 is never used)
    const float c = 1.f / sqrtf(t * t + 1.f), s = t * c, tau = s / (1.f + c), h = t * apq;
    app -= h;
    aqq += h;
    apq = 0.f;
    mr_mix(a1p, a1q, s, tau);
    mr_mix(a2p, a2q, s, tau);
    mr_mix(v0p, v0q, s, tau);
    mr_mix(v1p, v1q, s, tau);
    mr_mix(v2p, v2q, s, tau);
    mr_mix(v3p, v3q, s, tau);
}

// Horn (1987): the unit quaternion (w, x, y, z) of the proper rotation R that maximises sum_m (R t(m)) . c(m), from S_ab = sum_m t_a c_b
__host__ __device__ __forceinline__ float4 mr_quaternion(const MrMat& S) {
    float a00 = S.xx + S.yy + S.zz, a01 = S.yz - S.zy, a02 = S.zx - S.xz, a03 = S.xy - S.yx;
    float a11 = S.xx - S.yy - S.zz, a12 = S.xy + S.yx, a13 = S.zx + S.xz;
    float a22 = -S.xx + S.yy - S.zz, a23 = S.yz + S.zy;
    float a33 = -S.xx - S.yy + S.zz;
    float v00 = 1.f, v01 = 0.f, v02 = 0.f, v03 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v13 = 0.f;
    float v20 = 0.f, v21 = 0.f, v22 = 1.f, v23 = 0.f, v30 = 0.f, v31 = 0.f, v32 = 0.f, v33 = 1.f;
#pragma unroll
    for (int sweep = 0; sweep < MR_SWEEPS; ++sweep) {
        mr_rot(a00, a11, a01, a02, a12, a03, a13, v00, v01, v10, v11, v20, v21, v30, v31);
        mr_rot(a00, a22, a02, a01, a12, a03, a23, v00, v02, v10, v12, v20, v22, v30, v32);
        mr_rot(a00, a33, a03, a01, a13, a02, a23, v00, v03, v10, v13, v20, v23, v30, v33);
        mr_rot(a11, a22, a12, a01, a02, a13, a23, v01, v02, v11, v12, v21, v22, v31, v32);
        mr_rot(a11, a33, a13, a01, a03, a12, a23, v01, v03, v11, v13, v21, v23, v31, v33);
        mr_rot(a22, a33, a23, a02, a03, a12, a13, v02, v03, v12, v13, v22, v23, v32, v33);
    }
    // the column of the largest eigenvalue (the first of equal ones), by selects between named values: an index into the columns
    // would put them in scratch
    const bool b1 = a11 > a00;
    const float l1 = b1 ? a11 : a00;
    const bool b2 = a22 > l1;
    const float l2 = b2 ? a22 : l1;
    const bool b3 = a33 > l2;
    const float w = b3 ? v03 : b2 ? v02 : b1 ? v01 : v00, x = b3 ? v13 : b2 ? v12 : b1 ? v11 : v10;
    const float y = b3 ? v23 : b2 ? v22 : b1 ? v21 : v20, z = b3 ? v33 : b2 ? v32 : b1 ? v31 : v30;
    const float r = 1.f / sqrtf(w * w + x * x + y * y + z * z);             // (the columns stay orthonormal to rounding)
    return make_float4(w * r, x * r, y * r, z * r);
}

// mr_quaternion's sibling for a caller that differentiates through the fit (context_kernels.hip): the same sweeps and the same choice
// of the largest eigenvalue, but all four eigenpairs are kept -- q and lam0 as mr_quaternion finds them, the three others in the
// column order the sweeps leave (the chosen column's place is taken by column 0), every vector normalised.
struct MrEigen {
    float4 q, v1, v2, v3;
    float lam0, lam1, lam2, lam3;
};

__host__ __device__ __forceinline__ float4 mr_unit(float w, float x, float y, float z) {
    const float r = 1.f / sqrtf(w * w + x * x + y * y + z * z);
    return make_float4(w * r, x * r, y * r, z * r);
}

__host__ __device__ __forceinline__ MrEigen mr_eigen(const MrMat& S) {
    float a00 = S.xx + S.yy + S.zz, a01 = S.yz - S.zy, a02 = S.zx - S.xz, a03 = S.xy - S.yx;
    float a11 = S.xx - S.yy - S.zz, a12 = S.xy + S.yx, a13 = S.zx + S.xz;
    float a22 = -S.xx + S.yy - S.zz, a23 = S.yz + S.zy;
    float a33 = -S.xx - S.yy + S.zz;
    float v00 = 1.f, v01 = 0.f, v02 = 0.f, v03 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v13 = 0.f;
    float v20 = 0.f, v21 = 0.f, v22 = 1.f, v23 = 0.f, v30 = 0.f, v31 = 0.f, v32 = 0.f, v33 = 1.f;
#pragma unroll
    for (int sweep = 0; sweep < MR_SWEEPS; ++sweep) {
        mr_rot(a00, a11, a01, a02, a12, a03, a13, v00, v01, v10, v11, v20, v21, v30, v31);
        mr_rot(a00, a22, a02, a01, a12, a03, a23, v00, v02, v10, v12, v20, v22, v30, v32);
        mr_rot(a00, a33, a03, a01, a13, a02, a23, v00, v03, v10, v13, v20, v23, v30, v33);
        mr_rot(a11, a22, a12, a01, a02, a13, a23, v01, v02, v11, v12, v21, v22, v31, v32);
        mr_rot(a11, a33, a13, a01, a03, a12, a23, v01, v03, v11, v13, v21, v23, v31, v33);
        mr_rot(a22, a33, a23, a02, a03, a12, a13, v02, v03, v12, v13, v22, v23, v32, v33);
    }
    const bool b1 = a11 > a00;
    const float l1 = b1 ? a11 : a00;
    const bool b2 = a22 > l1;
    const float l2 = b2 ? a22 : l1;
    const bool b3 = a33 > l2;
    // the chosen column is 3 if b3, else 2 if b2, else 1 if b1, else 0; columns 1..3 keep their place unless chosen
    const bool c1 = b1 && !b2 && !b3, c2 = b2 && !b3, c3 = b3;
    MrEigen e;
    e.lam0 = b3 ? a33 : l2;
    e.q = mr_unit(b3 ? v03 : b2 ? v02 : b1 ? v01 : v00, b3 ? v13 : b2 ? v12 : b1 ? v11 : v10, b3 ? v23 : b2 ? v22 : b1 ? v21 : v20,
                  b3 ? v33 : b2 ? v32 : b1 ? v31 : v30);
    e.lam1 = c1 ? a00 : a11;
    e.v1 = mr_unit(c1 ? v00 : v01, c1 ? v10 : v11, c1 ? v20 : v21, c1 ? v30 : v31);
    e.lam2 = c2 ? a00 : a22;
    e.v2 = mr_unit(c2 ? v00 : v02, c2 ? v10 : v12, c2 ? v20 : v22, c2 ? v30 : v32);
    e.lam3 = c3 ? a00 : a33;
    e.v3 = mr_unit(c3 ? v00 : v03, c3 ? v10 : v13, c3 ? v20 : v23, c3 ? v30 : v33);
    return e;
}

// The adjoint of the fit: for a scalar E of R = mr_rotation(q) with G = dE/dR (G.xy = dE/dR_xy), dE/dS of the correlation S that
// mr_eigen was given.  g = dR/dq : G with its component along q removed; first-order perturbation of the top eigenvector,
// dq = sum_i v_i (v_i . dK q) / (lam0 - lam_i), gives dE/dK_ij = z_i q_j with z = sum_i v_i (v_i . g) / (lam0 - lam_i); K is linear
// in S.  An eigenpair whose gap lam0 - lam_i is not above MR_GAP_FLOOR * lam0 contributes 0: there the rotation is not a
// differentiable function of S (two equally good fits), and float32 does not resolve a smaller gap.  Finite for finite inputs.
constexpr float MR_GAP_FLOOR = 1e-6f;

__host__ __device__ __forceinline__ float mr_share(float4 v, float lam0, float lam, float gw, float gx, float gy, float gz) {
    const float gap = lam0 - lam;
    return gap > MR_GAP_FLOOR * lam0 ? (v.x * gw + v.y * gx + v.z * gy + v.w * gz) / gap : 0.f;
}

__host__ __device__ __forceinline__ MrMat mr_fit_adjoint(const MrEigen& e, const MrMat& G) {
    const float w = e.q.x, x = e.q.y, y = e.q.z, z = e.q.w;
    float gw = 2.f * (-z * G.xy + y * G.xz + z * G.yx - x * G.yz - y * G.zx + x * G.zy);
    float gx = 2.f * (y * G.xy + z * G.xz + y * G.yx - 2.f * x * G.yy - w * G.yz + z * G.zx + w * G.zy - 2.f * x * G.zz);
    float gy = 2.f * (-2.f * y * G.xx + x * G.xy + w * G.xz + x * G.yx + z * G.yz - w * G.zx + z * G.zy - 2.f * y * G.zz);
    float gz = 2.f * (-2.f * z * G.xx - w * G.xy + x * G.xz + w * G.yx - 2.f * z * G.yy + y * G.yz + x * G.zx + y * G.zy);
    const float along = w * gw + x * gx + y * gy + z * gz;
    gw -= along * w;
    gx -= along * x;
    gy -= along * y;
    gz -= along * z;
    const float s1 = mr_share(e.v1, e.lam0, e.lam1, gw, gx, gy, gz), s2 = mr_share(e.v2, e.lam0, e.lam2, gw, gx, gy, gz);
    const float s3 = mr_share(e.v3, e.lam0, e.lam3, gw, gx, gy, gz);
    const float z0 = s1 * e.v1.x + s2 * e.v2.x + s3 * e.v3.x, z1 = s1 * e.v1.y + s2 * e.v2.y + s3 * e.v3.y;
    const float z2 = s1 * e.v1.z + s2 * e.v2.z + s3 * e.v3.z, z3 = s1 * e.v1.w + s2 * e.v2.w + s3 * e.v3.w;
    // dE/dK_ij = z_i q_j; K_01 = K_10 = S.yz - S.zy, K_02 = S.zx - S.xz, K_03 = S.xy - S.yx, K_12 = S.xy + S.yx, K_13 = S.zx + S.xz,
    // K_23 = S.yz + S.zy, and the diagonal as in mr_eigen
    const float m00 = z0 * w, m11 = z1 * x, m22 = z2 * y, m33 = z3 * z;
    const float m01 = z0 * x + z1 * w, m02 = z0 * y + z2 * w, m03 = z0 * z + z3 * w;
    const float m12 = z1 * y + z2 * x, m13 = z1 * z + z3 * x, m23 = z2 * z + z3 * y;
    MrMat D;
    D.xx = m00 + m11 - m22 - m33;
    D.yy = m00 - m11 + m22 - m33;
    D.zz = m00 - m11 - m22 + m33;
    D.xy = m03 + m12;
    D.yx = m12 - m03;
    D.yz = m01 + m23;
    D.zy = m23 - m01;
    D.zx = m02 + m13;
    D.xz = m13 - m02;
    return D;
}

__host__ __device__ __forceinline__ MrMat mr_rotation(float4 q) {
    const float w = q.x, x = q.y, y = q.z, z = q.w;
    MrMat R;
    R.xx = 1.f - 2.f * (y * y + z * z);
    R.xy = 2.f * (x * y - w * z);
    R.xz = 2.f * (x * z + w * y);
    R.yx = 2.f * (x * y + w * z);
    R.yy = 1.f - 2.f * (x * x + z * z);
    R.yz = 2.f * (y * z - w * x);
    R.zx = 2.f * (x * z - w * y);
    R.zy = 2.f * (y * z + w * x);
    R.zz = 1.f - 2.f * (x * x + y * y);
    return R;
}
