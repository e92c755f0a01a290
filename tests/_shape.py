"""What the shape potential's test files share (tests/test_shape_host.py, test_shape_gpu.py): two restatements of
genie_shape_potential (include/genie_hip.h) in plain torch that never call the library -- `reference` in float64 on the CPU with the
gradient from autograd (the oracle), and the same code in float32 (`restatement32`: the measure of what float32 arithmetic costs on an
input, the timing reference of tools/shape_potential_time.py and the torch `twisting_function` of the end-to-end tests) -- the
header's analytic gradient written out with loops, the margins of the discontinuous report fields, and the inputs of the cases.

A configuration is a dict: rog_max, rog_weight, clash_distance, clash_separation, clash_weight (floats / int; a weight of 0 switches
the term off) and restraints, a list of (i, j, lo, hi, weight)."""
import math

import torch

REPORT = ('rog', 'min_distance', 'n_clash', 'e_rog', 'e_clash', 'e_restraint', 'n_violated', 'max_violation')
COUNTS = ('n_clash', 'n_violated')


def config(rog_max=0.0, rog_weight=0.0, clash_distance=0.0, clash_separation=2, clash_weight=0.0, restraints=()):
    return dict(rog_max=float(rog_max), rog_weight=float(rog_weight), clash_distance=float(clash_distance),
                clash_separation=int(clash_separation), clash_weight=float(clash_weight), restraints=[tuple(r) for r in restraints])


def _norm(diff):
    """|diff| over the last axis, with value 0 and gradient 0 where it is exactly 0 (the kernel's zero-distance rule)."""
    sq = (diff ** 2).sum(dim=-1)
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def _restraint_tensors(cfg, x):
    r = cfg['restraints']
    idx = lambda k: torch.tensor([int(e[k]) for e in r], dtype=torch.long, device=x.device)          # noqa: E731
    val = lambda k: torch.tensor([float(e[k]) for e in r], dtype=x.dtype, device=x.device)           # noqa: E731
    return idx(0), idx(1), val(2), val(3), val(4)


def terms(x, cfg):
    """Everything the entry reports of x [B, N, 3], in x's dtype and on its device, differentiable: the REPORT fields [B] each, and
    'energy' = e_rog + e_clash + e_restraint."""
    B, N, _ = x.shape
    zero = torch.zeros(B, dtype=x.dtype, device=x.device)
    c = x - x.mean(dim=1, keepdim=True)
    s = (c ** 2).sum(dim=(1, 2)) / N
    pos = s > 0
    rog = torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), zero)
    out = {'rog': rog, 'e_rog': cfg['rog_weight'] * torch.clamp(rog - cfg['rog_max'], min=0) ** 2}
    i, j = torch.triu_indices(N, N, offset=cfg['clash_separation'], device=x.device)                 # i < j, j - i >= separation
    if len(i):
        d = _norm(x[:, i] - x[:, j])                                                                 # [B, pairs]
        out['min_distance'] = d.min(dim=1).values
        out['n_clash'] = (d < cfg['clash_distance']).sum(dim=1)
        out['e_clash'] = cfg['clash_weight'] * (torch.clamp(cfg['clash_distance'] - d, min=0) ** 2).sum(dim=1)
    else:
        out.update(min_distance=zero + math.inf, n_clash=torch.zeros(B, dtype=torch.long, device=x.device), e_clash=zero)
    if cfg['restraints']:
        ri, rj, lo, hi, w = _restraint_tensors(cfg, x)
        d = _norm(x[:, ri] - x[:, rj])                                                               # [B, R]
        under, over = torch.clamp(lo - d, min=0), torch.clamp(d - hi, min=0)
        out['e_restraint'] = (w * (under ** 2 + over ** 2)).sum(dim=1)
        excess = torch.maximum(under, over)
        out['n_violated'] = (excess > 0).sum(dim=1)
        out['max_violation'] = excess.max(dim=1).values
    else:
        out.update(e_restraint=zero, n_violated=torch.zeros(B, dtype=torch.long, device=x.device), max_violation=zero)
    out['energy'] = out['e_rog'] + out['e_clash'] + out['e_restraint']
    return out


def logp(x, cfg, var):
    return -terms(x, cfg)['energy'] / (2 * var)


def _evaluate(x, cfg, var):
    x = x.detach().clone().requires_grad_(True)
    t = terms(x, cfg)
    lp = -t['energy'] / (2 * var)
    grad, = torch.autograd.grad(lp.sum(), x)
    out = {k: t[k].detach() for k in REPORT}
    out.update(logp=lp.detach(), grad=grad)
    return out


def reference(x, cfg, var):
    """The float64 oracle on the CPU: 'logp' [B], 'grad' [B, N, 3] (autograd) and the REPORT fields."""
    return _evaluate(x.detach().double().cpu(), cfg, float(var))


def restatement32(x, cfg, var):
    """The same code in float32, on x's device."""
    return _evaluate(x.detach().float(), cfg, float(var))


def twisting_function(cfg, abar, tausq=1.0):
    """The float32 restatement as a TwistedSampler `twisting_function`, with ShapePotential's variance."""
    from genie2_amd.smc import xstart_variance

    def twist(x0, step):
        return logp(x0.float(), cfg, xstart_variance(abar[step], tausq).to(torch.float32))
    return twist


def analytic_gradient(x, cfg, var):
    """The gradient as include/genie_hip.h states it, written out with loops in float64 (small N only)."""
    x = x.detach().double()
    B, N, _ = x.shape
    g = torch.zeros_like(x)
    for b in range(B):
        c = x[b] - x[b].mean(dim=0, keepdim=True)
        rog = float(torch.sqrt((c ** 2).sum() / N))
        if rog > 0:
            g[b] += cfg['rog_weight'] * max(rog - cfg['rog_max'], 0.0) * c / (N * rog)
        for n in range(N):
            for j in range(N):
                if abs(n - j) >= cfg['clash_separation']:
                    d = float((x[b, n] - x[b, j]).norm())
                    if d > 0:
                        g[b, n] -= cfg['clash_weight'] * max(cfg['clash_distance'] - d, 0.0) * (x[b, n] - x[b, j]) / d
        for i, j, lo, hi, w in cfg['restraints']:
            d = float((x[b, i] - x[b, j]).norm())
            if d > 0:
                f = w * (max(d - hi, 0.0) - max(lo - d, 0.0)) * (x[b, i] - x[b, j]) / d
                g[b, i] += f
                g[b, j] -= f
    return -g / var


def margins(x, cfg):
    """How far the discontinuous report fields are from flipping, in Angstrom, in float64: the smallest |d - clash_distance| over the
    eligible pairs, |d_r - lo_r| (lo > 0) and |d_r - hi_r| (hi finite) over the restraints, and |rog - rog_max|."""
    x = x.detach().double().cpu()
    N = x.shape[1]
    t = terms(x, cfg)
    m = float((t['rog'] - cfg['rog_max']).abs().min())
    i, j = torch.triu_indices(N, N, offset=cfg['clash_separation'])
    if len(i):
        m = min(m, float((_norm(x[:, i] - x[:, j]) - cfg['clash_distance']).abs().min()))
    if cfg['restraints']:
        ri, rj, lo, hi, _ = _restraint_tensors(cfg, x)
        d = _norm(x[:, ri] - x[:, rj])
        if bool((lo > 0).any()):
            m = min(m, float((d - lo)[:, lo > 0].abs().min()))
        if bool(torch.isfinite(hi).any()):
            m = min(m, float((d - hi)[:, torch.isfinite(hi)].abs().min()))
    return m


def random_restraints(x, count, seed):
    """Up to `count` restraints on distinct random pairs of x [B, N, 3], their bounds set from particle 0's distance d: a third
    (0.5 d, 1.5 d) (satisfied there), a third (1.3 d, 2 d) (a lower violation), a third (0, 0.7 d) with every fourth upper bound of the
    first kind infinite; weights in 0.5..2."""
    N = x.shape[1]
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
    g = torch.Generator().manual_seed(seed)
    pick = torch.randperm(len(pairs), generator=g)[:count].tolist()
    weights = (0.5 + 1.5 * torch.rand(len(pick), generator=g)).tolist()
    out = []
    for k, (p, w) in enumerate(zip(pick, weights)):
        i, j = pairs[p]
        d = float((x[0, i].double() - x[0, j].double()).norm())
        lo, hi = ((0.5 * d, math.inf if k % 4 == 0 else 1.5 * d), (1.3 * d, 2.0 * d), (0.0, 0.7 * d))[k % 3]
        if k % 2:
            i, j = j, i                                              # (either order is accepted)
        out.append((i, j, round(lo, 3), round(hi, 3), round(w, 3)))
    return out


def walk_config(x, restraints=40, seed=0, clash_distance=4.0):
    """All three terms on the walks x: rog_max 0.6 of particle 0's radius of gyration, clashes below `clash_distance` from two
    residues apart, `restraints` random restraints (fewer where there are fewer pairs)."""
    rog = float(terms(x.double(), config())['rog'][0])
    return config(rog_max=round(0.6 * rog, 3), rog_weight=1.0, clash_distance=clash_distance, clash_separation=2, clash_weight=1.0,
                  restraints=random_restraints(x, restraints, seed))


def only(cfg, term):
    """cfg with one term left on: 'rog', 'clash' or 'restraints'."""
    out = dict(cfg)
    if term != 'rog':
        out['rog_weight'] = 0.0
    if term != 'clash':
        out['clash_weight'] = 0.0
    if term != 'restraints':
        out['restraints'] = []
    return out


def potential(cfg, n_res, abar, **kw):
    """The ShapePotential of a configuration (rog and clash always given: a weight of 0 is how cfg switches a term off)."""
    from genie2_amd.smc import ShapePotential
    return ShapePotential(n_res, abar, rog_max=cfg['rog_max'], rog_weight=cfg['rog_weight'], clash_distance=cfg['clash_distance'],
                          clash_separation=cfg['clash_separation'], clash_weight=cfg['clash_weight'],
                          restraints=cfg['restraints'] or None, device='cuda', **kw)
