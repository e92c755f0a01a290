"""What the symmetry potential's tests share (tests/test_symmetry_host.py, test_symmetry_gpu.py, tools/symmetry_potential_time.py): the
layouts and their generators written out independently of the package, a float64 torch oracle built on an SVD Kabsch fit (with the
determinant fix) and autograd through it, the header's analytic gradient written out with loops, and a float32 restatement of the
kind a user would put into the sampling loop.  Nothing here calls the library."""
import math

import torch

from _motif import walk

REPORT = ('e_symmetry', 'symmetry_rmsd', 'rmsd_0', 'angle_0', 'rise_0', 'rmsd_1', 'angle_1', 'rise_1')

# (B, N, symbol, unit length, linker, offset): the shapes of the parity tests
CASES = [(3, 6, 'C2', 3, 0, 0), (3, 12, 'D2', 3, 0, 0), (3, 9, 'R2', 4, 1, 0), (3, 63, 'C3', 21, 0, 0), (3, 64, 'C4', 16, 0, 0),
         (3, 65, 'C3', 21, 0, 1), (3, 129, 'D2', 31, 1, 2), (3, 256, 'C4', 64, 0, 0), (3, 256, 'D2', 60, 4, 2), (3, 300, 'R5', 50, 10, 5),
         (1, 1512, 'C6', 252, 0, 0)]


def case_id(case):
    B, N, sym, m, linker, offset = case
    return 'N%d-%s-m%d-l%d-o%d' % (N, sym, m, linker, offset)


def walks(B, N):
    """B random walks of C-alpha spacing, seeds 100 N + {0, 1, ...}: float32 [B, N, 3]."""
    return torch.cat([walk(1, N, 100 * N + k) for k in range(B)])


def generators(sym, m, N, linker=0, offset=0):
    """The generators of a layout as [(src, dst), ...] index lists, from the statement in include/genie_hip.h."""
    kind, n = sym[0], int(sym[1:])
    units = 2 * n if kind == 'D' else n
    assert offset + units * m + (units - 1) * linker <= N
    start = [offset + k * (m + linker) for k in range(units)]
    if kind == 'C':
        maps = [{k: (k + 1) % n for k in range(n)}]
    elif kind == 'R':
        maps = [{k: k + 1 for k in range(n - 1)}]
    else:
        g0 = {k: (k + 1) % n for k in range(n)}
        g0.update({n + k: n + (k - 1) % n for k in range(n)})
        g1 = {k: n + k for k in range(n)}
        g1.update({n + k: k for k in range(n)})
        maps = [g0, g1]
    return [([start[k] + a for k in mp for a in range(m)], [start[j] + a for j in mp.values() for a in range(m)]) for mp in maps]


def is_swap(gen):
    """A generator that is its own inverse (a two-fold): its correlation is symmetric, its angle exactly 180 or 0."""
    to = dict(zip(*gen))
    return all(to.get(d) == s for s, d in to.items())


def kabsch(p, q):
    """The proper rotation R [.., 3, 3] that minimises sum_i |q_i - R p_i|^2 for centred p, q [.., L, 3]: SVD of sum_i p_i q_i^T,
    with the determinant fix."""
    u, _, vt = torch.linalg.svd(p.transpose(-1, -2) @ q)
    v, ut = vt.transpose(-1, -2), u.transpose(-1, -2)
    d = torch.sign(torch.linalg.det(v @ ut))
    fix = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=-1))
    return v @ fix @ ut


def fit(x, gen, detach=False):
    """One generator on x [B, N, 3]: (E [B], R [B, 3, 3], c_s, c_d [B, 3], p, q [B, L, 3])."""
    src, dst = (torch.as_tensor(v, device=x.device) for v in gen)
    a, b = x[:, src], x[:, dst]
    cs, cd = a.mean(dim=1), b.mean(dim=1)
    p, q = a - cs[:, None], b - cd[:, None]
    R = kabsch(p.detach(), q.detach()) if detach else kabsch(p, q)
    e = q - p @ R.transpose(-1, -2)
    return (e ** 2).sum(dim=(1, 2)), R, cs, cd, p, q


def energy(x, gens, weights=None, detach=False):
    """sum_g w_g E_g [B]."""
    weights = [1.0] * len(gens) if weights is None else weights
    total = 0
    for w, gen in zip(weights, gens):
        total = total + w * fit(x, gen, detach)[0]
    return total


def horn_gap(p, q):
    """The gap between the two largest eigenvalues of Horn's 4x4 matrix of sum_i p_i q_i^T, relative to its spectral radius: [B]."""
    S = p.transpose(-1, -2) @ q
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (S[:, i, j] for i in range(3) for j in range(3))
    rows = [[xx + yy + zz, yz - zy, zx - xz, xy - yx], [yz - zy, xx - yy - zz, xy + yx, zx + xz],
            [zx - xz, xy + yx, -xx + yy - zz, yz + zy], [xy - yx, zx + xz, yz + zy, -xx - yy + zz]]
    ev = torch.linalg.eigvalsh(torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2))
    return (ev[:, 3] - ev[:, 2]) / ev.abs().amax(dim=1).clamp(min=1e-300)


def rotation_report(R, cs, cd):
    """(angle in degrees in [0, 180], rise) of a rotation R [B, 3, 3] that carries c_s to c_d: the angle from the antisymmetric part
    and the trace with atan2, the axis as the top eigenvector of the symmetric part (cos I + (1 - cos) u u^T), the rise
    |u . (c_d - R c_s)|, or |c_d - R c_s| when the angle is 0."""
    skew = 0.5 * torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], dim=-1)
    cos = 0.5 * (R.diagonal(dim1=-2, dim2=-1).sum(dim=-1) - 1.0)
    angle = torch.atan2(skew.norm(dim=-1), cos)
    u = torch.linalg.eigh(0.5 * (R + R.transpose(-1, -2)))[1][:, :, 2]
    t = cd - (R @ cs[:, :, None])[:, :, 0]
    rise = torch.where(angle > 1e-12, (u * t).sum(dim=-1).abs(), t.norm(dim=-1))
    return angle * (180.0 / math.pi), rise


def describe(x, gens, weights=None, detach=True):
    """The report fields of x [B, N, 3] (in x's precision) plus 'E' [B, G], 'L' [G], 'gap' [B, G] and 'norm' [B, G] (sum |p|^2)."""
    weights = [1.0] * len(gens) if weights is None else weights
    out = {k: torch.zeros(x.shape[0], dtype=x.dtype, device=x.device) for k in REPORT}
    E, gap, norm = [], [], []
    for g, gen in enumerate(gens):
        e, R, cs, cd, p, q = fit(x, gen, detach)
        angle, rise = rotation_report(R, cs, cd)
        out['rmsd_%d' % g], out['angle_%d' % g], out['rise_%d' % g] = (e / len(gen[0])).sqrt(), angle, rise
        out['e_symmetry'] = out['e_symmetry'] + weights[g] * e
        E.append(e)
        gap.append(horn_gap(p, q))
        norm.append((p ** 2).sum(dim=(1, 2)))
    out['symmetry_rmsd'] = (sum(E) / sum(len(gen[0]) for gen in gens)).sqrt()
    out.update(E=torch.stack(E, dim=1), L=[len(gen[0]) for gen in gens], gap=torch.stack(gap, dim=1), norm=torch.stack(norm, dim=1))
    return out


def reference(x, gens, var, weights=None, weight=1.0, grad=True):
    """The float64 oracle on x [B, N, 3]: 'logp' [B], 'grad' [B, N, 3] (autograd through the SVD fit; left out with grad=False, for
    inputs whose fit is degenerate) and the fields of describe."""
    y = x.detach().double().requires_grad_(grad)
    lp = -weight * energy(y, gens, weights) / (2.0 * var)
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in describe(y.detach(), gens, [weight * w for w in weights or [1.0] * len(gens)]).items()}
    out['logp'] = lp.detach()
    if grad:
        out['grad'], = torch.autograd.grad(lp.sum(), y)
    return out


def analytic_gradient(x, gens, var, weights=None, weight=1.0):
    """d logp / d x by the header's formula, written out with loops over particles, generators and pairs: R held at its optimum,
    dE / dx[dst_i] += 2 (q_i - R p_i), dE / dx[src_i] += -2 R^T (q_i - R p_i)."""
    x = x.detach().double()
    weights = [1.0] * len(gens) if weights is None else weights
    out = torch.zeros_like(x)
    for b in range(x.shape[0]):
        for w, (src, dst) in zip(weights, gens):
            _, R, _, _, p, q = fit(x[b:b + 1], (src, dst))
            for i in range(len(src)):
                e = q[0, i] - R[0] @ p[0, i]
                out[b, dst[i]] += 2.0 * w * e
                out[b, src[i]] += -2.0 * w * (R[0].T @ e)
    return -weight * out / (2.0 * var)


def logp32(x, gens, var, weights=None, weight=1.0):
    """The float32 restatement: log p of x [B, N, 3] in x's own precision and on its device, differentiable in x with the rotation
    of the SVD fit held fixed (what the header's gradient is)."""
    return -weight * energy(x, gens, weights, detach=True) / (2.0 * var)


def restatement32(x, gens, var, weights=None, weight=1.0):
    """{'logp', 'grad', the report fields} of the float32 restatement on x."""
    y = x.detach().float().requires_grad_(True)
    lp = logp32(y, gens, var, weights, weight)
    g, = torch.autograd.grad(lp.sum(), y)
    out = {k: v for k, v in describe(y.detach(), gens, [weight * w for w in weights or [1.0] * len(gens)]).items() if k in REPORT}
    out.update(logp=lp.detach(), grad=g)
    return out


def on_device(gens, device):
    """The generators' index lists as tensors on `device`, made once: what a caller of logp32 inside a loop holds."""
    return [(torch.as_tensor(src, device=device), torch.as_tensor(dst, device=device)) for src, dst in gens]


def twisting_function(gens, abar, tausq=1.0, weights=None, weight=1.0):
    """The float32 restatement as a TwistedSampler twisting function."""
    from genie2_amd.smc import xstart_variance
    gens = on_device(gens, abar.device)
    return lambda x0, step: logp32(x0, gens, xstart_variance(abar[step], tausq).to(torch.float32), weights, weight)


# ---- exact assemblies -------------------------------------------------------------------------------------------------------------

def axis_rotation(axis, degrees):
    """The rotation by `degrees` about `axis`, float64 [3, 3] (Rodrigues)."""
    u = torch.as_tensor(axis, dtype=torch.float64)
    u = u / u.norm()
    K = torch.tensor([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]], dtype=torch.float64)
    t = math.radians(degrees)
    return torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def assembly(unit, motions):
    """The units motions[k](unit) one after another: [len(motions) * m, 3].  A motion is (R [3, 3], t [3]) applied as R x + t."""
    return torch.cat([unit @ R.T + t for R, t in motions])


def repeated(R, t, n):
    """The motions identity, M, M^2, ..., M^(n-1) of M = (R, t)."""
    out = [(torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))]
    for _ in range(n - 1):
        Rk, tk = out[-1]
        out.append((R @ Rk, R @ tk + t))
    return out


def exact_unit(m, seed, centre=(9.0, 4.0, -3.0)):
    """A random-walk unit away from the origin (so that it does not sit on a symmetry axis through it): float64 [m, 3]."""
    return walk(1, m, seed)[0].double() + torch.tensor(centre, dtype=torch.float64)


def exact_cyclic(n, m, seed=1):
    return assembly(exact_unit(m, seed), repeated(axis_rotation((0.0, 0.0, 1.0), 360.0 / n), torch.zeros(3, dtype=torch.float64), n))


def exact_dihedral(n, m, seed=2):
    ring = repeated(axis_rotation((0.0, 0.0, 1.0), 360.0 / n), torch.zeros(3, dtype=torch.float64), n)
    flip = axis_rotation((1.0, 0.0, 0.0), 180.0)
    return assembly(exact_unit(m, seed), ring + [(flip @ R, flip @ t) for R, t in ring])


def exact_repeat(n, m, twist, rise, seed=3, axis=(1.0, 2.0, -0.5), through=(3.0, -2.0, 1.0)):
    """n units along one screw: a rotation by `twist` degrees about `axis` through the point `through`, and `rise` Angstrom along it."""
    R = axis_rotation(axis, twist)
    u = torch.tensor(axis, dtype=torch.float64)
    u = u / u.norm()
    c = torch.tensor(through, dtype=torch.float64)
    return assembly(exact_unit(m, seed), repeated(R, c - R @ c + rise * u, n))
