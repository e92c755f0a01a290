"""What the burial potential's test files share (tests/test_burial_host.py, test_burial_gpu.py): two restatements of
genie_burial_potential (include/genie_hip.h) in plain torch that never call the library -- `reference` in float64 on the CPU with the
gradient from autograd (the oracle), and the same code in float32 (`restatement32`: the measure of what float32 arithmetic costs on an
input, the timing reference of tools/burial_potential_time.py and the torch `twisting_function` of the end-to-end tests) -- the
header's analytic gradient written out with loops, the margins of the discontinuous report fields, and the inputs of the cases.

A configuration is a dict: radius, width (floats), separation (int), targets, a list of (i, lo, hi, weight) with distinct residues,
and mean_min, mean_max, mean_weight (floats; a weight of 0 switches the term off)."""
import math

import torch

REPORT = ('burial_mean', 'burial_min', 'burial_max', 'n_burial_violated', 'max_burial_violation', 'e_burial_target', 'e_burial_mean')
COUNTS = ('n_burial_violated',)
EPS = 0.1               # GENIE_BURIAL_EPS

# (B, N, seed): the parity shapes of test_burial_gpu.py on _motif.walk(B, N, seed).  The seeds were picked on the CPU with the oracle
# alone: `inputs` asserts that no targeted c_n is within 1e-4 of one of its bounds.
CASES = [(3, 1, 1), (3, 2, 2), (3, 3, 3), (3, 4, 4), (3, 63, 63), (3, 64, 64), (3, 65, 65), (3, 129, 129), (3, 300, 300), (1, 1512, 1512)]


def case_id(case):
    return 'B%d-N%d' % tuple(case[:2])


def config(radius=10.0, width=2.0, separation=3, targets=(), mean_min=0.0, mean_max=math.inf, mean_weight=0.0):
    return dict(radius=float(radius), width=float(width), separation=int(separation),
                targets=[(int(t[0]), float(t[1]), float(t[2]), float(t[3]) if len(t) > 3 else 1.0) for t in targets],
                mean_min=float(mean_min), mean_max=float(mean_max), mean_weight=float(mean_weight))


def table(cfg, N, dtype=torch.float64, device='cpu'):
    """The per-residue table (lo, hi, w) [N] each of a configuration: w = 0 where a residue has no target."""
    lo, hi, w = torch.zeros(N, dtype=dtype), torch.full((N,), math.inf, dtype=dtype), torch.zeros(N, dtype=dtype)
    for i, a, b, weight in cfg['targets']:
        lo[i], hi[i], w[i] = a, b, weight
    return lo.to(device), hi.to(device), w.to(device)


def directions(x):
    """(u [B, N, 3], rho [B, N]) of x [B, N, 3]: the virtual C-beta direction, 0 at the two ends."""
    b = torch.zeros_like(x)
    if x.shape[1] >= 3:
        b = torch.cat([b[:, :1], 2 * x[:, 1:-1] - x[:, :-2] - x[:, 2:], b[:, -1:]], dim=1)
    rho = torch.sqrt((b ** 2).sum(dim=-1) + EPS ** 2)
    return b / rho[..., None], rho


def counts(x, cfg):
    """c [B, N]: the soft half-sphere count of every residue, differentiable in x."""
    N = x.shape[1]
    u, _ = directions(x)
    r = x[:, None, :, :] - x[:, :, None, :]                                     # [B, n, j] = x_j - x_n
    q = (r ** 2).sum(dim=-1)
    s = 1.0 / (1.0 + (q / cfg['radius'] ** 2) ** 3)
    h = (u[:, :, None, :] * r).sum(dim=-1)
    g = 0.5 * (1.0 + h / torch.sqrt(h ** 2 + cfg['width'] ** 2))
    idx = torch.arange(N, device=x.device)
    pair = ((idx[:, None] - idx[None, :]).abs() >= cfg['separation']).to(x.dtype)
    return (s * g * pair[None]).sum(dim=-1)


def terms(x, cfg):
    """Everything the entry reports of x [B, N, 3], in x's dtype and on its device, differentiable: the REPORT fields [B] each,
    'burial' [B, N] (the c_n) and 'energy' = e_burial_target + e_burial_mean."""
    B, N, _ = x.shape
    c = counts(x, cfg)
    m = c.mean(dim=1)
    lo, hi, w = table(cfg, N, x.dtype, x.device)
    under, over = torch.clamp(lo - c, min=0), torch.clamp(c - hi, min=0)
    excess = torch.where(w > 0, torch.maximum(under, over), torch.zeros_like(c))
    out = {'burial': c, 'burial_mean': m, 'burial_min': c.min(dim=1).values, 'burial_max': c.max(dim=1).values,
           'n_burial_violated': (excess > 0).sum(dim=1), 'max_burial_violation': excess.max(dim=1).values,
           'e_burial_target': (w * (under ** 2 + over ** 2)).sum(dim=1)}
    upper = torch.clamp(m - cfg['mean_max'], min=0) ** 2 if math.isfinite(cfg['mean_max']) else torch.zeros_like(m)
    out['e_burial_mean'] = cfg['mean_weight'] * (torch.clamp(cfg['mean_min'] - m, min=0) ** 2 + upper)
    out['energy'] = out['e_burial_target'] + out['e_burial_mean']
    return out


def logp(x, cfg, var):
    return -terms(x, cfg)['energy'] / (2 * var)


def _evaluate(x, cfg, var):
    x = x.detach().clone().requires_grad_(True)
    t = terms(x, cfg)
    lp = -t['energy'] / (2 * var)
    grad, = torch.autograd.grad(lp.sum(), x)
    out = {k: t[k].detach() for k in REPORT + ('burial',)}
    out.update(logp=lp.detach(), grad=grad)
    return out


def reference(x, cfg, var):
    """The float64 oracle on the CPU: 'logp' [B], 'grad' [B, N, 3] (autograd), the REPORT fields and 'burial' [B, N]."""
    return _evaluate(x.detach().double().cpu(), cfg, float(var))


def restatement32(x, cfg, var):
    """The same code in float32, on x's device."""
    return _evaluate(x.detach().float(), cfg, float(var))


def twisting_function(cfg, abar, tausq=1.0):
    """The float32 restatement as a TwistedSampler `twisting_function`, with BurialPotential's variance."""
    from genie2_amd.smc import xstart_variance

    def twist(x0, step):
        return logp(x0.float(), cfg, xstart_variance(abar[step], tausq).to(torch.float32))
    return twist


def analytic_gradient(x, cfg, var):
    """The gradient as include/genie_hip.h states it, written out with loops in float64 (small N only)."""
    x = x.detach().double()
    B, N, _ = x.shape
    R2, W2, sep = cfg['radius'] ** 2, cfg['width'] ** 2, cfg['separation']
    lo, hi, w = table(cfg, N)
    out = torch.zeros_like(x)
    for b in range(B):
        u, rho = directions(x[b:b + 1])
        u, rho = u[0], rho[0]
        c = torch.zeros(N, dtype=torch.float64)
        f = torch.zeros(N, N, 3, dtype=torch.float64)                           # f[n, j]
        a = torch.zeros(N, 3, dtype=torch.float64)
        for n in range(N):
            for j in range(N):
                if abs(j - n) < sep:
                    continue
                r = x[b, j] - x[b, n]
                q = float(r @ r)
                s = 1.0 / (1.0 + (q / R2) ** 3)
                h = float(u[n] @ r)
                g = 0.5 * (1.0 + h / math.sqrt(h * h + W2))
                gp = 0.5 * W2 / (h * h + W2) ** 1.5
                c[n] += s * g
                f[n, j] = g * (-6.0 * (q / R2) ** 2 * s * s / R2) * r + s * gp * u[n]
                a[n] += s * gp * r
        m = float(c.mean())
        mean_k = cfg['mean_weight'] / N * (max(m - cfg['mean_max'], 0.0) - max(cfg['mean_min'] - m, 0.0))
        k = [float(w[n]) * (max(float(c[n]) - float(hi[n]), 0.0) - max(float(lo[n]) - float(c[n]), 0.0)) + mean_k for n in range(N)]
        v = torch.zeros(N, 3, dtype=torch.float64)
        for n in range(1, N - 1):
            v[n] = (a[n] - u[n] * float(u[n] @ a[n])) / rho[n]
        for i in range(N):
            t = torch.zeros(3, dtype=torch.float64)
            for n in range(N):
                t += k[n] * f[n, i]
            t -= k[i] * f[i].sum(dim=0)
            t += 2 * k[i] * v[i]
            if i >= 1:
                t -= k[i - 1] * v[i - 1]
            if i + 1 < N:
                t -= k[i + 1] * v[i + 1]
            out[b, i] = -t / var
    return out


def margins(x, cfg):
    """How far the discontinuous report field (n_burial_violated) is from flipping, in float64: the smallest |c_n - lo_n| and
    |c_n - hi_n| over the targeted residues (w_n > 0) with a finite, positive bound; inf when there is none."""
    x = x.detach().double().cpu()
    c = counts(x, cfg)
    lo, hi, w = table(cfg, x.shape[1])
    m = math.inf
    for bound in (lo, hi):
        use = (w > 0) & torch.isfinite(bound) & (bound > 0)
        if bool(use.any()):
            m = min(m, float((c - bound)[:, use].abs().min()))
    return m


def walk_config(x, seed=0, **kw):
    """Both terms on the walks x [B, N, 3]: targets on about a third of the residues (at least one), their bounds set from particle
    0's own c_n so that a third are satisfied there ((0.5 c, 1.5 c), every other one without an upper bound), a third too exposed
    ((1.3 c + 0.5, 2 c + 1)) and a third too buried ((0, 0.7 c)), weights in 0.5..2; the mean held in (1.2 m + 0.25, 2 m + 1) of
    particle 0's own m, so that the mean term acts on it."""
    N = x.shape[1]
    base = config(**kw)
    c = counts(x[:1].double(), base)[0]
    g = torch.Generator().manual_seed(seed)
    pick = torch.randperm(N, generator=g)[:max(1, N // 3)].tolist()
    weights = (0.5 + 1.5 * torch.rand(len(pick), generator=g)).tolist()
    targets = []
    for k, (n, w) in enumerate(zip(pick, weights)):
        v = float(c[n])
        lo, hi = ((0.5 * v, math.inf if k % 2 == 0 else 1.5 * v), (1.3 * v + 0.5, 2.0 * v + 1.0), (0.0, 0.7 * v))[(k + 1) % 3]
        targets.append((n, round(lo, 3), round(hi, 3), round(w, 3)))
    m = float(c.mean())
    return config(**dict(kw, targets=sorted(targets), mean_min=round(1.2 * m + 0.25, 3), mean_max=round(2.0 * m + 1.0, 3), mean_weight=1.0))


def only(cfg, term):
    """cfg with one term left on: 'target' or 'mean'."""
    out = dict(cfg)
    if term != 'target':
        out['targets'] = []
    if term != 'mean':
        out['mean_weight'] = 0.0
    return out


def inputs(case, **kw):
    """(x [B, N, 3] float32, cfg) of a case, both terms on, checked: no targeted c_n within 1e-4 of a bound."""
    from _motif import walk
    B, N, seed = case
    x = walk(B, N, seed)
    cfg = walk_config(x, seed, **kw)
    m = margins(x, cfg)
    assert m >= 1e-4, 'a targeted residue of this input is %.1e from a bound: take another seed' % m
    return x, cfg


def potential(cfg, n_res, abar, **kw):
    """The BurialPotential of a configuration (the mean always given: a weight of 0 is how cfg switches that term off)."""
    from genie2_amd.smc import BurialPotential
    return BurialPotential(n_res, abar, targets=cfg['targets'] or None, mean=(cfg['mean_min'], cfg['mean_max']),
                           mean_weight=cfg['mean_weight'], radius=cfg['radius'], width=cfg['width'], separation=cfg['separation'],
                           device='cuda', **kw)
