"""What the fold potential's test files share (tests/test_fold_host.py, test_fold_gpu.py, tools/fold_potential_time.py): the
definition of genie_fold_potential (include/genie_hip.h) restated in plain torch, independently of the library -- `eigh` on Horn's
4x4 matrix, every (particle, reference) pair with its 11 seeds side by side in one batch, every seed's LAST score kept with the
gradient under that seed's last fit held fixed (no autograd through the iterations) -- which runs in float64 as the oracle and in
float32 as the restatement a user would write; the rule that marks a pair ill-posed; the inputs and the case list.  Nothing here
calls the library."""
import math

import torch

import _similarity as S

REPORT = ('tm_nearest', 'nearest', 'tm_lowest_wanted', 'n_fold_violations', 'e_fold')
COUNTS = ('nearest', 'n_fold_violations')
SEEDS = S.SEEDS

# (B, N, R): the parity shapes of test_fold_gpu.py
CASES = [(3, 4, 1), (3, 5, 3), (3, 63, 5), (3, 64, 4), (3, 65, 5), (2, 129, 9), (2, 256, 3), (2, 257, 3), (1, 1706, 1), (8, 40, 300)]
TEMPLATE, AVOID = (0.6, math.inf), (0.0, 0.5)         # the bounds a template and an avoided fold get
BAND = (0.5, 0.6)                                       # the one row of a single-reference case: both hinges can be active
MARGIN = 1e-4                                           # no n_r within MARGIN N of an active bound; a tie of seeds within MARGIN in TM
GAP = 1e-4                                              # 7.8's rule: a Horn gap below this fraction of the spectral radius


def case_id(case):
    return 'B%d-N%d-R%d' % tuple(case)


def ascend_last(P, Q, n_iter):
    """The ascents of M pairs at once, P moving onto Q, both [M, N, 3].  Returns, in P's dtype, per seed: n [M, 11] (sum_n g_n of
    the last iteration), dn [M, 11, N, 3] (d n / d P with that iteration's fit held fixed: -(2 / d0^2) g_n^2 R^T e_n) and gap [M, 11]
    (the smallest relative gap between the two largest Horn eigenvalues over the seed's fits)."""
    M, N, _ = P.shape
    d0sq = S.d0(N) ** 2
    W = torch.zeros(SEEDS, N, dtype=P.dtype, device=P.device)
    for s, (start, length) in enumerate(S.windows(N)):
        W[s, start:start + length] = 1
    W = W[None].expand(M, SEEDS, N)
    gap = None
    for it in range(n_iter):
        sw = W.sum(-1, keepdim=True)
        sw = torch.where(sw > 0, sw, torch.ones_like(sw))
        Pc = P[:, None] - (W @ P / sw)[:, :, None]                   # [M, 11, N, 3]: about the weighted centroid of every seed
        Qc = Q[:, None] - (W @ Q / sw)[:, :, None]
        ev, vec = torch.linalg.eigh(S.horn_matrix(torch.einsum('msl,msli,mslj->msij', W, Pc, Qc)))
        g = (ev[..., 3] - ev[..., 2]) / ev.abs().amax(dim=-1).clamp(min=1e-30)
        gap = g if gap is None else torch.minimum(gap, g)
        Rm = S.quaternion_rotation(vec[..., :, 3])
        e = Pc @ Rm.transpose(-1, -2) - Qc                           # rows R (x_n - c_p) - (y_n - c_q)
        t = 1 / (1 + (e ** 2).sum(-1) / d0sq)
        W = t * t
    return t.sum(-1), -(2 / d0sq) * W[..., None] * (e @ Rm), gap


def hinges(n, N, bounds, upper=True):
    """(below, above) [B, R] of the soft counts n [B, R] under bounds [R, 3]; `upper=False` leaves the upper hinge out altogether
    (what hi = inf must equal)."""
    lo, hi = bounds[:, 0].to(n), bounds[:, 1].to(n)
    below = torch.clamp(N * lo - n, min=0)
    if not upper:
        return below, torch.zeros_like(n)
    finite = torch.isfinite(hi)
    above = torch.where(finite, torch.clamp(n - N * torch.where(finite, hi, torch.zeros_like(hi)), min=0), torch.zeros_like(n))
    return below, above


def evaluate(x, ref, bounds, var, n_iter=16, dtype=torch.float64, upper=True, chunk=512):
    """The definition on x [B, N, 3], ref [R, N, 3], bounds [R, 3] (lo, hi, weight) in `dtype` on the CPU: 'logp' [B], 'grad'
    [B, N, 3], 'tm', 'n', 'below', 'above' [B, R], 'seed' [B, R] int64, the REPORT fields [B], and for the ill-posed rule 'n_seeds'
    [B, R, 11], 'gap' [B, R] (the winning seed's), 'ill' [B, R] bool (filled by `mark_ill_posed`)."""
    x, ref = x.detach().to(dtype).cpu(), ref.detach().to(dtype).cpu()
    bounds = torch.as_tensor(bounds, dtype=torch.float64)
    B, N, R = x.shape[0], x.shape[1], ref.shape[0]
    bi, ri = torch.meshgrid(torch.arange(B), torch.arange(R), indexing='ij')
    bi, ri = bi.reshape(-1), ri.reshape(-1)
    parts = [ascend_last(x[bi[c:c + chunk]], ref[ri[c:c + chunk]], n_iter) for c in range(0, B * R, chunk)]
    n_seeds, dn_seeds, gaps = (torch.cat([p[k] for p in parts]) for k in range(3))
    seed = n_seeds.argmax(dim=1)                                    # (argmax: the first of equal ones, the lowest seed)
    pick = torch.arange(B * R)
    n, dn, gap = n_seeds[pick, seed].reshape(B, R), dn_seeds[pick, seed].reshape(B, R, N, 3), gaps[pick, seed].reshape(B, R)
    below, above = hinges(n, N, bounds, upper)
    w = bounds[:, 2].to(dtype)
    energy = (w * (below ** 2 + above ** 2)).sum(dim=1)
    k = w * (above - below)
    tm = n / N
    wanted = bounds[:, 0] > 0
    out = {'logp': -energy / (2 * var), 'grad': -(k[:, :, None, None] * dn).sum(dim=1) / var, 'tm': tm, 'n': n, 'below': below,
           'above': above, 'seed': seed.reshape(B, R), 'n_seeds': n_seeds.reshape(B, R, SEEDS), 'dn_seeds': dn_seeds.reshape(B, R, SEEDS, N, 3),
           'gap': gap, 'k': k, 'tm_nearest': tm.amax(dim=1), 'nearest': tm.argmax(dim=1),
           'tm_lowest_wanted': tm[:, wanted].amin(dim=1) if bool(wanted.any()) else torch.zeros(B, dtype=dtype),
           'n_fold_violations': ((below > 0) | (above > 0)).sum(dim=1), 'e_fold': energy}
    return out


def reference(x, ref, bounds, var, n_iter=16, upper=True):
    """The float64 oracle, with 'ill' [B, R]: the pairs whose gradient the definition does not pin down (`mark_ill_posed`)."""
    out = evaluate(x, ref, bounds, float(var), n_iter, torch.float64, upper)
    out['ill'] = mark_ill_posed(out, float(var))
    return out


def restatement32(x, ref, bounds, var, n_iter=16, upper=True):
    """The same code in float32."""
    return evaluate(x, ref, bounds, float(var), n_iter, torch.float32, upper)


def mark_ill_posed(out, var):
    """[B, R] bool from a float64 `evaluate`: a pair is ill-posed if another seed's score is within MARGIN (in TM) of the winner's
    while the gradient under its fit, weighted as the pair enters the particle's gradient, differs from the winner's by more than the
    gradient bar (1e-5 of the largest entry of the particle's gradient), or if a Horn gap of its winning ascent is below GAP."""
    n_seeds, dn, seed, k = out['n_seeds'], out['dn_seeds'], out['seed'], out['k']
    B, R, _, N, _ = dn.shape
    win_n = torch.gather(n_seeds, 2, seed[..., None])                # [B, R, 1]
    win_dn = torch.gather(dn, 2, seed[..., None, None, None].expand(B, R, 1, N, 3))
    close = ((win_n - n_seeds) <= MARGIN * N) & (torch.arange(SEEDS)[None, None] != seed[..., None])
    differ = (k.abs()[..., None] / var) * (dn - win_dn).abs().amax(dim=(3, 4))          # [B, R, 11]
    bar = 1e-5 * out['grad'].abs().amax(dim=(1, 2))[:, None, None]
    return (close & (differ > bar)).any(dim=2) | (out['gap'] < GAP)


def left_out(ref):
    """[B] bool: the particles left out of the log p and gradient comparison -- one of their pairs with an active hinge is ill-posed."""
    return (ref['ill'] & ((ref['below'] > 0) | (ref['above'] > 0))).any(dim=1)


def logp(x, ref, bounds, var, n_iter=16):
    """log p [B] in x's dtype on its device, differentiable in x by autograd: the winning fits come from an ascent that is not
    recorded, and the soft counts are formed again under them, so the derivative is the definition's (fits held fixed)."""
    B, N, R = x.shape[0], x.shape[1], ref.shape[0]
    ref, bounds = ref.to(x), torch.as_tensor(bounds).to(x)
    d0sq = S.d0(N) ** 2
    P, Q = x[:, None].expand(B, R, N, 3).reshape(B * R, N, 3), ref[None].expand(B, R, N, 3).reshape(B * R, N, 3)
    with torch.no_grad():
        Pd = P.detach()
        W = torch.zeros(SEEDS, N, dtype=x.dtype, device=x.device)
        for s, (start, length) in enumerate(S.windows(N)):
            W[s, start:start + length] = 1
        W = W[None].expand(B * R, SEEDS, N)
        for it in range(n_iter):
            sw = W.sum(-1, keepdim=True)
            sw = torch.where(sw > 0, sw, torch.ones_like(sw))
            cp, cq = W @ Pd / sw, W @ Q / sw
            Pc, Qc = Pd[:, None] - cp[:, :, None], Q[:, None] - cq[:, :, None]
            _, vec = torch.linalg.eigh(S.horn_matrix(torch.einsum('msl,msli,mslj->msij', W, Pc, Qc)))
            Rm = S.quaternion_rotation(vec[..., :, 3])
            t = 1 / (1 + ((Pc @ Rm.transpose(-1, -2) - Qc) ** 2).sum(-1) / d0sq)
            W = t * t
        seed = t.sum(-1).argmax(dim=1)
        pick = torch.arange(B * R, device=x.device)
        Rw, cpw, cqw = Rm[pick, seed], cp[pick, seed], cq[pick, seed]
    e = (P - cpw[:, None]) @ Rw.transpose(-1, -2) - (Q - cqw[:, None])
    n = (1 / (1 + (e ** 2).sum(-1) / d0sq)).sum(-1).reshape(B, R)
    below, above = hinges(n, N, bounds)
    return -(bounds[:, 2] * (below ** 2 + above ** 2)).sum(dim=1) / (2 * var)


def twisting_function(ref, bounds, abar, n_iter=16, tausq=1.0):
    """The float32 restatement as a TwistedSampler `twisting_function`, with FoldPotential's variance."""
    from genie2_amd.smc import xstart_variance

    def twist(x0, step):
        return logp(x0.float(), ref, bounds, xstart_variance(abar[step], tausq).to(torch.float32), n_iter)
    return twist


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def walk(N, seed):
    """One centred 3.8 A walk [N, 3], float32."""
    w = S.walk(1, N, seed)[0]
    return w - w.mean(dim=0, keepdim=True)


def designs(B, N, base=0):
    """B centred walks of seeds 100 N + base + k: [B, N, 3] float32."""
    return torch.stack([walk(N, 100 * N + base + k) for k in range(B)])


def references(x, R, base=0):
    """R references for the designs x [B, N, 3]: reference r is a moved copy of design r mod B with S.NOISE[r mod 6] Angstrom of noise
    per coordinate (0.2 to 4.5: TM from about 0.99 down), except every third one (r mod 3 == 2), an unrelated walk (TM about 0.1 to
    0.3): [R, N, 3] float32."""
    B, N = x.shape[0], x.shape[1]
    out = []
    for r in range(R):
        seed = 100 * N + base + 1000 + r
        out.append(walk(N, seed) + torch.tensor([3.0, -2.0, 1.0]) if r % 3 == 2 else S.moved(x[r % B], seed, S.NOISE[r % len(S.NOISE)]))
    return torch.stack(out)


def bounds_of(R, weight=1.0):
    """[R, 3] float64 rows (lo, hi, weight): TEMPLATE for reference 0, AVOID for the others; a single reference gets BAND.  (One
    template per case: a template is far from every design but its own, and far pairs are where seeds tie -- DESIGN.md 7.9.)"""
    rows = [list(BAND if R == 1 else TEMPLATE if r == 0 else AVOID) + [weight] for r in range(R)]
    return torch.tensor(rows, dtype=torch.float64)


# the seed offset of a case whose first choice the oracle turned down (check_inputs or the 5 % cap), found on the CPU
BASE = {(3, 63, 5): 140, (3, 64, 4): 50, (3, 65, 5): 10, (2, 129, 9): 30, (2, 256, 3): 10, (2, 257, 3): 10, (8, 40, 300): 30}


def check_inputs(ref, case):
    """The oracle's own conditions on an input (ref: `reference` of it): no n_r within MARGIN N of an active bound -- a bound is
    active when its hinge can be: lo > 0, hi finite -- and both an active lower and an active upper hinge on some particle (a case of
    one particle and one reference can hold one hinge only: one of the two).  Otherwise: take other seeds."""
    B, N, R = case
    bounds = bounds_of(R)
    lo, hi = N * bounds[:, 0], N * bounds[:, 1]
    d_lo = torch.where(lo > 0, (ref['n'] - lo).abs(), torch.full_like(ref['n'], math.inf))
    d_hi = torch.where(torch.isfinite(hi), (ref['n'] - torch.where(torch.isfinite(hi), hi, torch.zeros_like(hi))).abs(),
                       torch.full_like(ref['n'], math.inf))
    m = float(torch.minimum(d_lo, d_hi).min())
    assert m >= MARGIN * N, 'an n_r of this input is %.1e N from a bound: take other seeds' % (m / N)
    lower, upper = bool((ref['below'] > 0).any()), bool((ref['above'] > 0).any())
    assert (lower and upper) if B * R > 1 else (lower or upper), 'this input lacks an active hinge (lower %s, upper %s)' % (lower, upper)


def inputs(case):
    """(x [B, N, 3], ref [R, N, 3], bounds [R, 3]) of a case."""
    B, N, R = case
    base = BASE.get(tuple(case), 0)
    x = designs(B, N, base)
    return x, references(x, R, base), bounds_of(R)
