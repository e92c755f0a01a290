"""What the diversity potential's test files share (tests/test_diversity_host.py, test_diversity_gpu.py,
tools/diversity_potential_time.py): the definition of genie_diversity_potential (include/genie_hip.h) restated in plain torch,
independently of the library, on top of tests/_fold.py's `ascend_last` -- every cross-system pair i < j scored once with x_i moving,
its seeds side by side in one batch, the winning seed's LAST score given to both members, the moving-side gradient to x_i and the
reference-side gradient to x_j, each under that seed's last fit held fixed -- which runs in float64 as the oracle and in float32 as
the restatement a user would write; an autograd log p with the other particles detached, for use as a TwistedSampler
`twisting_function`; DESIGN.md 7.9's ill-posed rule for both sides of a pair; the inputs and the case list.  Nothing here calls the
library."""
import torch

import _fold as Fd
import _similarity as S

REPORT = ('tm_nearest_design', 'nearest_design', 'tm_mean_design', 'n_similar', 'e_diversity')
COUNTS = ('nearest_design', 'n_similar')
SEEDS = S.SEEDS

# (S, K, N): the parity shapes of test_diversity_gpu.py -- S systems of K particles of N residues
CASES = [(2, 1, 4), (3, 1, 5), (2, 2, 63), (3, 2, 64), (2, 3, 65), (4, 2, 129), (2, 2, 256), (3, 1, 257), (2, 1, 1706), (8, 8, 40), (2, 64, 24)]
TM_MAX = 0.5
MARGIN, GAP = Fd.MARGIN, Fd.GAP                         # no n_ij within MARGIN N of the bound; a tie of seeds within MARGIN in TM; 7.8's gap
SIGMA = (0.05, 0.1, 0.15, 0.2)                          # the noise of particle b, in units of d0(N): SIGMA[b % 4]


def case_id(case):
    return 'S%d-K%d-N%d' % tuple(case)


def pair_index(B, K):
    """(i, j) int64 [M] each: the scored pairs of a batch of B in systems of K -- i < j, i // K != j // K -- in the order i, then j."""
    i, j = torch.triu_indices(B, B, offset=1)
    keep = (i // K) != (j // K)
    return i[keep], j[keep]


def rotations_last(P, Q, n_iter):
    """The rotation of every seed's last fit, [M, 11, 3, 3] in P's dtype: `Fd.ascend_last`'s loop once more, keeping what it does not
    return.  (Its `dn` is -(2 / d0^2) g^2 e R as rows; the reference side needs +(2 / d0^2) g^2 e = -dn R^T.)"""
    M, N, _ = P.shape
    d0sq = S.d0(N) ** 2
    W = torch.zeros(SEEDS, N, dtype=P.dtype, device=P.device)
    for s, (start, length) in enumerate(S.windows(N)):
        W[s, start:start + length] = 1
    W = W[None].expand(M, SEEDS, N)
    for it in range(n_iter):
        sw = W.sum(-1, keepdim=True)
        sw = torch.where(sw > 0, sw, torch.ones_like(sw))
        Pc = P[:, None] - (W @ P / sw)[:, :, None]
        Qc = Q[:, None] - (W @ Q / sw)[:, :, None]
        _, vec = torch.linalg.eigh(S.horn_matrix(torch.einsum('msl,msli,mslj->msij', W, Pc, Qc)))
        Rm = S.quaternion_rotation(vec[..., :, 3])
        t = 1 / (1 + ((Pc @ Rm.transpose(-1, -2) - Qc) ** 2).sum(-1) / d0sq)
        W = t * t
    return Rm


def score_pairs(P, Q, n_iter):
    """M pairs, P moving onto Q, both [M, N, 3]: per seed n [M, 11], dp [M, 11, N, 3] (d n / d P, the fit held fixed), dq likewise
    (d n / d Q) and gap [M, 11] (`Fd.ascend_last`'s)."""
    n, dp, gap = Fd.ascend_last(P, Q, n_iter)
    return n, dp, -(dp @ rotations_last(P, Q, n_iter).transpose(-1, -2)), gap


def evaluate(x, K, var, tm_max=TM_MAX, weight=1.0, n_iter=16, dtype=torch.float64, chunk=256):
    """The definition on x [B, N, 3] as systems of K, in `dtype` on the CPU: 'logp' [B], 'grad' [B, N, 3]; [B, B], symmetric, 0 where
    nothing is scored: 'tm', 'n', 'a' (the hinge), 'scored' (bool), 'seed' (int64, -1), 'gap'; the REPORT fields [B]; 'margin' (the
    smallest |n_ij - N tm_max| over the scored pairs; inf without one); and, for the ill-posed rule, 'pairs' (i, j), 'n_seeds'
    [M, 11], 'dp_seeds', 'dq_seeds' [M, 11, N, 3], 'gap_seeds' [M, 11]."""
    x = x.detach().to(dtype).cpu()
    B, N = x.shape[0], x.shape[1]
    if B % K:
        raise ValueError('B = %d is no multiple of K = %d' % (B, K))
    i, j = pair_index(B, K)
    M = len(i)
    zero = lambda *shape: torch.zeros(*shape, dtype=dtype)      # noqa: E731
    n, seed, gap, grad = zero(B, B), torch.full((B, B), -1, dtype=torch.int64), torch.full((B, B), float('inf'), dtype=dtype), zero(B, N, 3)
    scored = torch.zeros(B, B, dtype=torch.bool)
    out = {'pairs': (i, j)}
    if M:
        parts = [score_pairs(x[i[c:c + chunk]], x[j[c:c + chunk]], n_iter) for c in range(0, M, chunk)]
        n_seeds, dp_seeds, dq_seeds, gap_seeds = (torch.cat([p[k] for p in parts]) for k in range(4))
        win = n_seeds.argmax(dim=1)                                 # (argmax: the first of equal ones, the lowest seed)
        pick = torch.arange(M)
        n_pair, dp, dq = n_seeds[pick, win], dp_seeds[pick, win], dq_seeds[pick, win]
        for a, b in ((i, j), (j, i)):
            n[a, b], seed[a, b], gap[a, b], scored[a, b] = n_pair, win, gap_seeds[pick, win], True
        hinge = torch.clamp(n_pair - N * tm_max, min=0)
        # d logp_b / d x_b = -(weight / (K var)) sum_j a_bj d n_bj / d x_b: the moving side of (i, j) is x_i's, the reference side x_j's
        grad.index_add_(0, i, -(weight / (K * var)) * hinge[:, None, None] * dp)
        grad.index_add_(0, j, -(weight / (K * var)) * hinge[:, None, None] * dq)
        out.update(n_seeds=n_seeds, dp_seeds=dp_seeds, dq_seeds=dq_seeds, gap_seeds=gap_seeds, win=win)
    a = torch.where(scored, torch.clamp(n - N * tm_max, min=0), zero(B, B))
    energy = (weight / K) * (a ** 2).sum(dim=1)
    tm = n / N
    count = scored.sum(dim=1)
    some = count > 0
    neg = torch.where(scored, tm, torch.full_like(tm, -1.0))
    out.update({'logp': -energy / (2 * var), 'grad': grad, 'tm': tm, 'n': n, 'a': a, 'scored': scored, 'seed': seed, 'gap': gap,
                'margin': float((n - N * tm_max).abs()[scored].min()) if M else float('inf'),
                'tm_nearest_design': torch.where(some, neg.amax(dim=1), zero(B)),
                'nearest_design': torch.where(some, neg.argmax(dim=1), torch.full((B,), -1)),
                'tm_mean_design': tm.sum(dim=1) / count.clamp(min=1), 'n_similar': (a > 0).sum(dim=1), 'e_diversity': energy})
    return out


def reference(x, K, var, tm_max=TM_MAX, weight=1.0, n_iter=16):
    """The float64 oracle, with 'ill' [B, B]: entry [b, j] says that the definition does not pin down what pair {b, j} gives to
    particle b's gradient (`mark_ill_posed`)."""
    out = evaluate(x, K, float(var), tm_max, weight, n_iter, torch.float64)
    out['ill'] = mark_ill_posed(out, K, float(var), weight)
    return out


def restatement32(x, K, var, tm_max=TM_MAX, weight=1.0, n_iter=16):
    """The same code in float32."""
    return evaluate(x, K, float(var), tm_max, weight, n_iter, torch.float32)


def mark_ill_posed(out, K, var, weight=1.0):
    """[B, B] bool from a float64 `evaluate`, DESIGN.md 7.9's rule on each side of a pair: [b, j] is ill-posed if another seed's score
    is within MARGIN (in TM) of the winner's while the gradient it would give particle b, weighted as the pair enters that gradient,
    differs from the winner's by more than the gradient bar (1e-5 of the largest entry of particle b's gradient), or if a Horn gap of
    the pair's winning ascent is below GAP."""
    B = out['n'].shape[0]
    ill = torch.zeros(B, B, dtype=torch.bool)
    i, j = out['pairs']
    if not len(i):
        return ill
    n_seeds, win = out['n_seeds'], out['win']
    M, _, N, _ = out['dp_seeds'].shape
    pick = torch.arange(M)
    win_n = n_seeds[pick, win][:, None]
    close = ((win_n - n_seeds) <= MARGIN * N) & (torch.arange(SEEDS)[None] != win[:, None])
    low_gap = out['gap_seeds'][pick, win] < GAP
    k = (weight / (K * var)) * out['a'][i, j]
    bar = 1e-5 * out['grad'].abs().amax(dim=(1, 2))
    for side, who, other in (('dp_seeds', i, j), ('dq_seeds', j, i)):
        d = out[side]
        differ = k[:, None] * (d - d[pick, win][:, None]).abs().amax(dim=(2, 3))         # [M, 11]
        ill[who, other] = (close & (differ > bar[who][:, None])).any(dim=1) | low_gap
    return ill


def left_out(ref):
    """[B] bool: the particles left out of the log p and gradient comparison -- one of their pairs with an active hinge is ill-posed."""
    return (ref['ill'] & (ref['a'] > 0)).any(dim=1)


def logp(x, K, var, tm_max=TM_MAX, weight=1.0, n_iter=16):
    """log p [B] in x's dtype on its device, differentiable in x by autograd with the definition's derivative: the winning fits come
    from an ascent that is not recorded; n_bj is then formed again under the pair's fit with x_b live and its partner detached, once
    for each member, so that autograd.grad(logp.sum(), x)[b] is d logp_b / d x_b and nothing else."""
    B, N = x.shape[0], x.shape[1]
    i, j = pair_index(B, K)
    i, j = i.to(x.device), j.to(x.device)
    if not len(i):
        return (x * 0).sum(dim=(1, 2))
    d0sq = S.d0(N) ** 2
    with torch.no_grad():
        P, Q = x.detach()[i], x.detach()[j]
        M = P.shape[0]
        W = torch.zeros(SEEDS, N, dtype=x.dtype, device=x.device)
        for s, (start, length) in enumerate(S.windows(N)):
            W[s, start:start + length] = 1
        W = W[None].expand(M, SEEDS, N)
        for it in range(n_iter):
            sw = W.sum(-1, keepdim=True)
            sw = torch.where(sw > 0, sw, torch.ones_like(sw))
            cp, cq = W @ P / sw, W @ Q / sw
            Pc, Qc = P[:, None] - cp[:, :, None], Q[:, None] - cq[:, :, None]
            _, vec = torch.linalg.eigh(S.horn_matrix(torch.einsum('msl,msli,mslj->msij', W, Pc, Qc)))
            Rm = S.quaternion_rotation(vec[..., :, 3])
            t = 1 / (1 + ((Pc @ Rm.transpose(-1, -2) - Qc) ** 2).sum(-1) / d0sq)
            W = t * t
        win = t.sum(-1).argmax(dim=1)
        pick = torch.arange(M, device=x.device)
        Rw, cpw, cqw = Rm[pick, win], cp[pick, win], cq[pick, win]

    def count(p, q):
        e = (p - cpw[:, None]) @ Rw.transpose(-1, -2) - (q - cqw[:, None])
        return (1 / (1 + (e ** 2).sum(-1) / d0sq)).sum(-1)

    a_i = torch.clamp(count(x[i], x.detach()[j]) - N * tm_max, min=0) ** 2           # particle i's own view of the pair: x_i live
    a_j = torch.clamp(count(x.detach()[i], x[j]) - N * tm_max, min=0) ** 2           # ... and particle j's: x_j live
    energy = torch.zeros(B, dtype=x.dtype, device=x.device).index_add(0, i, a_i).index_add(0, j, a_j) * (weight / K)
    return -energy / (2 * var)


def twisting_function(K, abar, tm_max=TM_MAX, weight=1.0, n_iter=16, tausq=1.0):
    """The float32 restatement as a TwistedSampler `twisting_function`, with DiversityPotential's variance."""
    from genie2_amd.smc import xstart_variance

    def twist(x0, step):
        return logp(x0.float(), K, xstart_variance(abar[step], tausq).to(torch.float32), tm_max, weight, n_iter)
    return twist


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

# the seed offset of a case whose first choice the oracle turned down (check_inputs), found on the CPU
BASE = {}


def inputs(case):
    """x [S K, N, 3] float32 of a case: particle b is a moved copy of one 3.8 A walk w0 with SIGMA[b % 4] d0(N) Angstrom of noise per
    coordinate (TM 0.88 to 0.99 to each other), except every third one (b % 3 == 2), an unrelated walk (TM 0.1 to 0.4 to all)."""
    Sy, K, N = case
    base = 100 * N + BASE.get(tuple(case), 0)
    w0 = Fd.walk(N, base)
    return torch.stack([Fd.walk(N, base + 1000 + b) + torch.tensor([3.0, -2.0, 1.0]) if b % 3 == 2
                        else S.moved(w0, base + 1 + b, SIGMA[b % 4] * S.d0(N)) for b in range(Sy * K)])


def check_inputs(ref, case):
    """The oracle's own conditions on an input (ref: `reference` of it): no n_ij within MARGIN N of the bound, an active and an idle
    pair wherever the case has more than one pair, at most 5 % of the particles left out.  Otherwise: take other seeds (BASE)."""
    Sy, K, N = case
    assert ref['margin'] >= MARGIN * N, 'an n_ij of this input is %.1e N from the bound: take other seeds' % (ref['margin'] / N)
    act = ref['a'][ref['scored']] > 0
    if len(ref['pairs'][0]) > 1:
        assert bool(act.any()) and bool((~act).any()), 'this input lacks an active or an idle pair (%d of %d active)' % (int(act.sum()) // 2, len(act) // 2)
    out = int(left_out(ref).sum())
    assert out <= 0.05 * Sy * K, '%d of %d particles are ill-posed: take other seeds' % (out, Sy * K)
