// Stand-alone check of csrc/horn.h's mr_eigen and mr_fit_adjoint on the host (they are plain arithmetic, __host__ too), against a
// float64 cyclic Jacobi written here.  tests/test_context_host.py compiles this file for the host alone with the address and
// undefined-behaviour sanitizers and runs it; it exits 0 when every check holds and prints the worst error / bound of each.
//
// Inputs: correlations S = sum_k t_k c_k^T of A random centred points t and c = Q t + noise for a random rotation Q, with the
// relative gap (lam0 - lam1) / lam0 of Horn's matrix at least 0.05 (others are drawn again).
// Bounds, with eps = 2^-24 and |K| the Frobenius norm of Horn's 4x4: 6 sweeps of 6 rotations perturb K by at most 36 eps |K| (each
// rotation is an orthogonal similarity applied in float32), so an eigenvalue is within 36 eps |K| of the float64 one and, by
// first-order perturbation, a unit eigenvector within 36 eps |K| / gap of it, gap the distance to the nearest other eigenvalue.  The
// adjoint is compared with a central difference of G : R(q(S)) in float64 (step 1e-5 |K|): its entries are sums of
// (v_i . g) / (lam0 - lam_i), so the relative error of a float32 entry is bounded by the eigenvector bound plus the eigenvalue
// bound over the gap, 4 x 36 eps |K| / gap3 in all with gap3 the smallest of the three gaps to lam0 (q, v_i, lam0 and lam_i each err),
// of the largest entry; the central difference adds at most 1e-6 of it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "../genie2_amd/csrc/horn.h"

namespace {

struct Rng {
    unsigned long long s;
    double uniform() {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return ((s >> 11) + 0.5) / 9007199254740992.0;
    }
    double normal() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }
};

void horn(const double S[3][3], double K[4][4]) {
    const double xx = S[0][0], xy = S[0][1], xz = S[0][2], yx = S[1][0], yy = S[1][1], yz = S[1][2], zx = S[2][0], zy = S[2][1], zz = S[2][2];
    const double k[4][4] = {{xx + yy + zz, yz - zy, zx - xz, xy - yx}, {yz - zy, xx - yy - zz, xy + yx, zx + xz},
                            {zx - xz, xy + yx, -xx + yy - zz, yz + zy}, {xy - yx, zx + xz, yz + zy, -xx - yy + zz}};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) K[i][j] = k[i][j];
}

// float64 cyclic Jacobi: eigenvalues descending in lam, eigenvectors in the columns of V
void jacobi(const double K[4][4], double lam[4], double V[4][4]) {
    double a[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            a[i][j] = K[i][j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 30; ++sweep)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                if (a[p][q] == 0.0) continue;
                const double th = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double x = a[k][p], y = a[k][q];
                    a[k][p] = c * x - s * y;
                    a[k][q] = s * x + c * y;
                }
                for (int k = 0; k < 4; ++k) {
                    const double x = a[p][k], y = a[q][k];
                    a[p][k] = c * x - s * y;
                    a[q][k] = s * x + c * y;
                }
                for (int k = 0; k < 4; ++k) {
                    const double x = V[k][p], y = V[k][q];
                    V[k][p] = c * x - s * y;
                    V[k][q] = s * x + c * y;
                }
            }
    int order[4] = {0, 1, 2, 3};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (a[order[j]][order[j]] > a[order[i]][order[i]]) {
                const int t = order[i];
                order[i] = order[j];
                order[j] = t;
            }
    double W[4][4];
    for (int i = 0; i < 4; ++i) {
        lam[i] = a[order[i]][order[i]];
        for (int k = 0; k < 4; ++k) W[k][i] = V[k][order[i]];
    }
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) V[k][i] = W[k][i];
}

void rotation(const double q[4], double R[3][3]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double r[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                            {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                            {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = r[i][j];
}

// G : R(q(S)) in float64
double energy(const double S[3][3], const double G[3][3]) {
    double K[4][4], lam[4], V[4][4], q[4], R[3][3], e = 0.0;
    horn(S, K);
    jacobi(K, lam, V);
    for (int k = 0; k < 4; ++k) q[k] = V[k][0];
    rotation(q, R);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) e += G[i][j] * R[i][j];
    return e;
}

double dot4(float4 a, const double V[4][4], int col) { return a.x * V[0][col] + a.y * V[1][col] + a.z * V[2][col] + a.w * V[3][col]; }

double dot4(float4 a, float4 b) { return (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z + (double)a.w * b.w; }

}  // namespace

int main() {
    const double eps = std::ldexp(1.0, -24);
    Rng rng = {20240607ULL};
    double worst_lam = 0.0, worst_q = 0.0, worst_orth = 0.0, worst_adj = 0.0;
    int done = 0, failed = 0;
    while (done < 200) {
        const int A = 3 + (int)(rng.uniform() * 20);
        double q0[4], Q[3][3], S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, G[3][3], n = 0.0;
        for (double& v : q0) {
            v = rng.normal();
            n += v * v;
        }
        for (double& v : q0) v /= std::sqrt(n);
        rotation(q0, Q);
        const double scale = std::pow(10.0, 2.0 * rng.uniform() - 0.5), noise = scale * rng.uniform();
        for (int k = 0; k < A; ++k) {
            double t[3], c[3];
            for (double& v : t) v = scale * rng.normal();
            for (int i = 0; i < 3; ++i) c[i] = Q[i][0] * t[0] + Q[i][1] * t[1] + Q[i][2] * t[2] + noise * rng.normal();
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) S[i][j] += t[i] * c[j];
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                S[i][j] = (double)(float)S[i][j];                       // both sides see the same float32 S
                G[i][j] = rng.normal();
            }
        double K[4][4], lam[4], V[4][4], normK = 0.0;
        horn(S, K);
        jacobi(K, lam, V);
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) normK += K[i][j] * K[i][j];
        normK = std::sqrt(normK);
        if (!(lam[0] > 0.0) || (lam[0] - lam[1]) / lam[0] < 0.05) continue;
        ++done;
        const MrMat Sf = {(float)S[0][0], (float)S[0][1], (float)S[0][2], (float)S[1][0], (float)S[1][1], (float)S[1][2],
                          (float)S[2][0], (float)S[2][1], (float)S[2][2]};
        const MrEigen e = mr_eigen(Sf);
        const float4 qq = mr_quaternion(Sf);
        if (qq.x != e.q.x || qq.y != e.q.y || qq.z != e.q.z || qq.w != e.q.w) {
            std::printf("case %d: mr_eigen's q is not mr_quaternion's\n", done);
            ++failed;
        }
        // eigenvalues: the float32 set against the float64 set, both sorted descending
        double got[4] = {e.lam0, e.lam1, e.lam2, e.lam3};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (got[j] > got[i]) {
                    const double t = got[i];
                    got[i] = got[j];
                    got[j] = t;
                }
        const double bound = 36.0 * eps * normK;
        for (int i = 0; i < 4; ++i) worst_lam = std::fmax(worst_lam, std::fabs(got[i] - lam[i]) / bound);
        worst_lam = std::fmax(worst_lam, std::fabs(e.lam0 - lam[0]) / bound);
        // the top eigenvector, up to sign
        const double sign = dot4(e.q, V, 0) < 0 ? -1.0 : 1.0, qf[4] = {e.q.x, e.q.y, e.q.z, e.q.w};
        double err_q = 0.0;
        for (int k = 0; k < 4; ++k) err_q += (qf[k] - sign * V[k][0]) * (qf[k] - sign * V[k][0]);
        err_q = std::sqrt(err_q);
        worst_q = std::fmax(worst_q, err_q / (bound / (lam[0] - lam[1])));
        // orthonormal to rounding (16 eps: four products and their sum, twice)
        const float4 vs[4] = {e.q, e.v1, e.v2, e.v3};
        for (int i = 0; i < 4; ++i)
            for (int j = i; j < 4; ++j) worst_orth = std::fmax(worst_orth, std::fabs(dot4(vs[i], vs[j]) - (i == j ? 1.0 : 0.0)) / (36.0 * eps));
        // the adjoint against a central difference in float64
        const MrMat Gf = {(float)G[0][0], (float)G[0][1], (float)G[0][2], (float)G[1][0], (float)G[1][1], (float)G[1][2],
                          (float)G[2][0], (float)G[2][1], (float)G[2][2]};
        double Gd[3][3] = {{Gf.xx, Gf.xy, Gf.xz}, {Gf.yx, Gf.yy, Gf.yz}, {Gf.zx, Gf.zy, Gf.zz}};
        const MrMat D = mr_fit_adjoint(e, Gf);
        const double Dg[3][3] = {{D.xx, D.xy, D.xz}, {D.yx, D.yy, D.yz}, {D.zx, D.zy, D.zz}};
        double fd[3][3], big = 0.0, diff = 0.0;
        const double h = 1e-5 * normK;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double Sp[3][3], Sm[3][3];
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) Sp[a][b] = Sm[a][b] = S[a][b];
                Sp[i][j] += h;
                Sm[i][j] -= h;
                fd[i][j] = (energy(Sp, Gd) - energy(Sm, Gd)) / (2.0 * h);
                big = std::fmax(big, std::fabs(fd[i][j]));
            }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) diff = std::fmax(diff, std::fabs(Dg[i][j] - fd[i][j]));
        const double gap3 = lam[0] - lam[1];
        worst_adj = std::fmax(worst_adj, diff / (big * (4.0 * bound / gap3 + 1e-6)));
    }
    std::printf("eigenvalues error / bound %.3f\nquaternion error / bound %.3f\northonormality error / bound %.3f\nadjoint error / bound %.3f\n",
                worst_lam, worst_q, worst_orth, worst_adj);
    if (!(worst_lam <= 1.0) || !(worst_q <= 1.0) || !(worst_orth <= 1.0) || !(worst_adj <= 1.0)) ++failed;
    // a degenerate fit stays finite: S = 0 (all points at one place) and a collinear selection (a double largest eigenvalue)
    const MrMat zero = {0, 0, 0, 0, 0, 0, 0, 0, 0}, line = {2.f, 0, 0, 0, 0, 0, 0, 0, 0}, ones = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    for (const MrMat& S : {zero, line}) {
        const MrMat D = mr_fit_adjoint(mr_eigen(S), ones);
        const float d[9] = {D.xx, D.xy, D.xz, D.yx, D.yy, D.yz, D.zx, D.zy, D.zz};
        for (float v : d)
            if (!std::isfinite(v)) {
                std::printf("a degenerate fit gave a non-finite adjoint\n");
                ++failed;
                break;
            }
    }
    std::printf(failed ? "FAILED\n" : "OK\n");
    return failed ? 1 : 0;
}
