"""What the sheet potential's test files share (tests/test_sheet_host.py, test_sheet_gpu.py): two restatements of
genie_sheet_potential (include/genie_hip.h) in plain torch that never call the library -- `reference` in float64 on the CPU with the
gradient from autograd (the oracle), and the same code in float32 (`restatement32`: the measure of what float32 arithmetic costs on an
input, the timing reference of tools/sheet_potential_time.py and the torch `twisting_function` of the end-to-end tests) -- the margins
of the discontinuous report fields, and the inputs of the cases.

A configuration is a dict: table (mu_A, sigma_A, mu_P, sigma_P), separation (sep_A, sep_P), antiparallel and parallel ((min, max) in
rungs per residue, max may be inf), antiparallel_weight, parallel_weight, ladder (a list of `(i, j, len, 'A'|'P'[, weight])` entries as
load_ladder returns them, or None) and ladder_weight; a weight of 0 switches a term off."""
import math

import torch

from _secstruct import _rotation, _unit, ideal_extended, ideal_helix  # noqa: F401

REPORT = ('antiparallel_content', 'parallel_content', 'n_antiparallel', 'n_parallel', 'n_paired', 'e_antiparallel', 'e_parallel',
          'e_ladder', 'n_ladder_missed')
COUNTS = ('n_antiparallel', 'n_parallel', 'n_paired', 'n_ladder_missed')
TABLE = (5.0, 0.6, 4.8, 0.5)
SEPARATION = (3, 5)
CLASSES = ('antiparallel', 'parallel')


def config(antiparallel=(0.0, math.inf), antiparallel_weight=0.0, parallel=(0.0, math.inf), parallel_weight=0.0, ladder=None,
           ladder_weight=0.0, table=TABLE, separation=SEPARATION):
    return dict(antiparallel=(float(antiparallel[0]), float(antiparallel[1])), antiparallel_weight=float(antiparallel_weight),
                parallel=(float(parallel[0]), float(parallel[1])), parallel_weight=float(parallel_weight),
                ladder=None if ladder is None else [tuple(e) for e in ladder], ladder_weight=float(ladder_weight),
                table=tuple(float(v) for v in table), separation=(int(separation[0]), int(separation[1])))


def rungs(ladder):
    """Ladder entries (i, j, len, class[, weight]) -> [(i, j, class index, weight)] with i < j: A pairs i + k with j - k, P pairs
    i + k with j + k, k = 0..len-1."""
    out = []
    for e in ladder or []:
        i, j, n, cls = int(e[0]), int(e[1]), int(e[2]), e[3]
        w = float(e[4]) if len(e) > 4 else 1.0
        for k in range(n):
            a, b = i + k, (j - k if cls == 'A' else j + k)
            out.append((min(a, b), max(a, b), 'AP'.index(cls), w))
    return out


def _norm(diff):
    """|diff| over the last axis, with value 0 and gradient 0 where it is exactly 0 (the kernel's zero-distance rule)."""
    sq = (diff ** 2).sum(dim=-1)
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def zscores(x, cfg):
    """[B, N, 3] -> [B, 2, M, M, 3], M = max(N - 2, 0): (d_f - mu_c) / sigma_c of the pair of interior residues (i + 1, j + 1) in the
    classes A, P, for the distances d0, d1, d2 (every ordered pair: the caller masks)."""
    N = x.shape[1]
    M = max(N - 2, 0)
    D = _norm(x[:, :, None, :] - x[:, None, :, :])
    d0 = D[:, 1:1 + M, 1:1 + M]
    a = torch.stack([d0, D[:, 0:M, 2:2 + M], D[:, 2:2 + M, 0:M]], dim=-1)
    p = torch.stack([d0, D[:, 0:M, 0:M], D[:, 2:2 + M, 2:2 + M]], dim=-1)
    mu_a, sg_a, mu_p, sg_p = cfg['table']
    return torch.stack([(a - mu_a) / sg_a, (p - mu_p) / sg_p], dim=1)


def eligible(N, cfg, device=None):
    """bool [2, M, M]: j - i >= sep_c."""
    k = torch.arange(max(N - 2, 0), device=device)
    gap = k[None, :] - k[:, None]
    return torch.stack([gap >= cfg['separation'][0], gap >= cfg['separation'][1]])


def terms(x, cfg):
    """Everything the entry reports of x [B, N, 3], in x's dtype and on its device, differentiable where it is continuous: the REPORT
    fields [B] each, 'pairs' [B, N, 2] (int32, -1: none), 's' [B, 2, M, M] (the scores, 0 where not eligible), 'formed' (bool, the
    same shape), 'n' [B, 2] and 'energy' = e_antiparallel + e_parallel + e_ladder."""
    B, N, _ = x.shape
    M = max(N - 2, 0)
    z = zscores(x, cfg)
    u = (z ** 2).sum(dim=-1) / 3.0                                                              # [B, 2, M, M]
    ok = eligible(N, cfg, x.device)[None]
    s = torch.where(ok, 1.0 / (1.0 + u) ** 2, torch.zeros_like(u))
    n = s.sum(dim=(2, 3))                                                                       # [B, 2]
    out = {'s': s, 'n': n, 'antiparallel_content': n[:, 0] / N, 'parallel_content': n[:, 1] / N}
    for c, name in enumerate(CLASSES):
        lo, hi = cfg[name]
        out['e_' + name] = cfg[name + '_weight'] * (torch.clamp(N * lo - n[:, c], min=0) ** 2 + torch.clamp(n[:, c] - N * hi, min=0) ** 2)
    inside = (z.detach().abs() <= 1).all(dim=-1)
    formed = ok & inside
    out['formed'] = formed
    out['n_antiparallel'], out['n_parallel'] = formed[:, 0].sum(dim=(1, 2)), formed[:, 1].sum(dim=(1, 2))
    # a residue's partner: over the formed rungs it is the i or the j of, the one with the highest score
    both = formed | formed.transpose(2, 3)
    score = torch.where(both, (s + s.transpose(2, 3)).detach(), -torch.ones_like(s))
    pairs = torch.full((B, N, 2), -1, dtype=torch.int32, device=x.device)
    if M > 0:
        best = score.argmax(dim=3)                                                              # [B, 2, M]
        found = both.any(dim=3)
        pairs[:, 1:1 + M] = torch.where(found, best + 1, -torch.ones_like(best)).to(torch.int32).transpose(1, 2)
    out['pairs'] = pairs
    out['n_paired'] = (pairs >= 0).any(dim=2).sum(dim=1)
    listed = rungs(cfg['ladder'])
    if listed:
        i = torch.tensor([r[0] - 1 for r in listed], device=x.device)
        j = torch.tensor([r[1] - 1 for r in listed], device=x.device)
        c = torch.tensor([r[2] for r in listed], device=x.device)
        w = torch.tensor([r[3] for r in listed], dtype=x.dtype, device=x.device)
        out['e_ladder'] = cfg['ladder_weight'] * (w[None] * u[:, c, i, j]).sum(dim=1)
        out['n_ladder_missed'] = (~inside[:, c, i, j]).sum(dim=1)
    else:
        out['e_ladder'] = torch.zeros(B, dtype=x.dtype, device=x.device)
        out['n_ladder_missed'] = torch.zeros(B, dtype=torch.long, device=x.device)
    out['energy'] = out['e_antiparallel'] + out['e_parallel'] + out['e_ladder']
    return out


def logp(x, cfg, var):
    return -terms(x, cfg)['energy'] / (2 * var)


def _evaluate(x, cfg, var):
    x = x.detach().clone().requires_grad_(True)
    t = terms(x, cfg)
    lp = -t['energy'] / (2 * var)
    grad = torch.autograd.grad(lp.sum(), x, allow_unused=True)[0] if lp.requires_grad else None
    out = {k: t[k].detach() for k in REPORT + ('pairs', 'n', 'formed')}
    out.update(logp=lp.detach(), grad=torch.zeros_like(x) if grad is None else grad)
    return out


def reference(x, cfg, var, device='cpu'):
    """The float64 oracle on the CPU: 'logp' [B], 'grad' [B, N, 3] (autograd), the REPORT fields, 'pairs', 'n' and 'formed'.  (The
    same float64 torch code on another `device` for a chain on which the CPU would take several seconds.)"""
    return _evaluate(x.detach().double().to(device), cfg, float(var))


def restatement32(x, cfg, var):
    """The same code in float32, on x's device."""
    return _evaluate(x.detach().float(), cfg, float(var))


def twisting_function(cfg, abar, tausq=1.0):
    """The float32 restatement as a TwistedSampler `twisting_function`, with SheetPotential's variance."""
    from genie2_amd.smc import xstart_variance

    def twist(x0, step):
        return logp(x0.float(), cfg, xstart_variance(abar[step], tausq).to(torch.float32))
    return twist


def margins(x, cfg):
    """How far the discontinuous or kinked quantities are from flipping, in float64: (the smallest | |z| - 1 | over the eligible and
    the listed rungs, the smallest |n_c - N f_c^{min,max}| over both classes and the bounds that can bind (a maximum of inf and a
    minimum of 0 cannot: a count is never negative), the smallest gap between the two highest scores among one residue's formed rungs
    of one class); inf where there is nothing to flip."""
    x = x.detach().double().cpu()
    B, N, _ = x.shape
    z = zscores(x, cfg)
    t = terms(x, cfg)
    ok = eligible(N, cfg)[None, :, :, :, None].expand_as(z).clone()
    for i, j, c, _ in rungs(cfg['ladder']):
        ok[:, c, i - 1, j - 1] = True
    box = float((z.abs() - 1).abs()[ok].min()) if bool(ok.any()) else math.inf
    binding = [(c, f) for c, name in enumerate(CLASSES) for f in cfg[name] if math.isfinite(f) and f > 0]
    hinge = min([float((t['n'][:, c] - N * f).abs().min()) for c, f in binding], default=math.inf)
    both = t['formed'] | t['formed'].transpose(2, 3)
    score = torch.where(both, t['s'] + t['s'].transpose(2, 3), torch.full_like(t['s'], -math.inf))
    tie = math.inf
    if score.shape[-1] >= 2:
        top = score.topk(2, dim=3).values
        two = torch.isfinite(top[..., 1])
        if bool(two.any()):
            tie = float((top[..., 0] - top[..., 1])[two].min())
    return box, hinge, tie


def analytic_gradient(x, cfg, var):
    """d logp / d x of x [B, N, 3] in float64, written out with loops from the formulas of include/genie_hip.h:
    ds/du = -2 / (1 + u)^3, du/dd_f = 2 z_f / (3 sigma_c), a distance of exactly 0 has direction 0."""
    x = x.detach().double().cpu()
    B, N, _ = x.shape
    t = terms(x, cfg)
    grad = torch.zeros_like(x)
    extra = {}
    for i, j, c, w in rungs(cfg['ladder']):
        extra[(i, j, c)] = extra.get((i, j, c), 0.0) + cfg['ladder_weight'] * w
    for b in range(B):
        for c, name in enumerate(CLASSES):
            mu, sigma = cfg['table'][2 * c], cfg['table'][2 * c + 1]
            lo, hi = cfg[name]
            n_c = float(t['n'][b, c])
            a = 2.0 * cfg[name + '_weight'] * (max(n_c - N * hi, 0.0) - max(N * lo - n_c, 0.0))      # dE_c / dn_c
            for i in range(1, N - 1):
                for j in range(i + 3, N - 1):
                    on = j - i >= cfg['separation'][c]
                    k = extra.get((i, j, c), 0.0)
                    if not on and k == 0.0:
                        continue
                    ends = [(i, j), (i - 1, j + 1), (i + 1, j - 1)] if c == 0 else [(i, j), (i - 1, j - 1), (i + 1, j + 1)]
                    diffs = [x[b, p] - x[b, q] for p, q in ends]
                    d = [float(v.norm()) for v in diffs]
                    zf = [(v - mu) / sigma for v in d]
                    u = sum(v * v for v in zf) / 3.0
                    de_du = (a * -2.0 / (1.0 + u) ** 3 if on else 0.0) + k
                    for (p, q), v, dist, zv in zip(ends, diffs, d, zf):
                        if dist > 0:
                            f = de_du * 2.0 * zv / (3.0 * sigma) * v / dist
                            grad[b, p] += f
                            grad[b, q] -= f
    return -grad / (2.0 * var)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def strand(n, reverse=False, offset=0.0):
    """An ideal flat pleated strand of C-alphas [n, 3], float64: 3.3 A rise along x, pleated by +-0.94 A in z (3.8 A bonds), at
    y = offset; `reverse` runs it from its far end back (the pleat stays where it is in space)."""
    k = torch.arange(n, dtype=torch.float64)
    xyz = torch.stack([3.3 * k, torch.full_like(k, offset), 0.94 * (1 - 2 * (k % 2))], dim=-1)
    return xyz.flip(0) if reverse else xyz


def ideal_sheet(n_strands, n=8, parallel=False, spacing=4.8):
    """n_strands ideal strands of n residues side by side, `spacing` apart, as one chain without loops [n_strands n, 3], float64:
    neighbours run in opposite directions, or all in the same with `parallel` (the chain then jumps back: the bonds between strands are
    not 3.8 A, which no term looks at)."""
    return torch.cat([strand(n, reverse=(not parallel) and s % 2 == 1, offset=spacing * s) for s in range(n_strands)])


def walk64(n, g):
    steps = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), dim=0)


def _loop(a, b, n, g):
    """n residues between the points a and b (exclusive): evenly spaced on the segment, bowed out by a sine of a random direction."""
    t = (torch.arange(1, n + 1, dtype=torch.float64) / (n + 1))[:, None]
    return a + t * (b - a) + 2.5 * torch.sin(math.pi * t) * _unit(g)


def sheet_chain(B, N, seed, jitter=0.15):
    """C-alpha chains [B, N, 3], float32: blocks of four kinds in rotation -- a three-stranded antiparallel sheet (7-residue strands,
    3-residue loops), a two-stranded parallel sheet (7-residue strands, a 6-residue crossover), an ideal helix of 10, a 3.8 A random
    walk of 8 -- each in a random orientation, joined with 3.8 A bonds, with Gaussian jitter of `jitter` A on every coordinate, cut to
    N.  Particle b starts the rotation at kind b % 4."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(B, N, 3, dtype=torch.float64)
    for b in range(B):
        rows, k = [], 0
        while sum(len(r) for r in rows) < N:
            kind = (b + k) % 4
            if kind == 0:
                st = [strand(7, reverse=s == 1, offset=4.8 * s) for s in range(3)]
                seg = torch.cat([st[0], _loop(st[0][-1], st[1][0], 3, g), st[1], _loop(st[1][-1], st[2][0], 3, g), st[2]])
            elif kind == 1:
                st = [strand(7, offset=4.8 * s) for s in range(2)]
                seg = torch.cat([st[0], _loop(st[0][-1], st[1][0], 6, g) + torch.tensor([0.0, 0.0, 5.0]), st[1]])
            elif kind == 2:
                seg = ideal_helix(10)
            else:
                seg = walk64(8, g)
            seg = (seg - seg[0]) @ _rotation(g).T
            start = torch.zeros(3, dtype=torch.float64) if not rows else rows[-1][-1] + 3.8 * _unit(g)
            rows.append(seg + start)
            k += 1
        out[b] = torch.cat(rows)[:N]
    out = out + jitter * torch.randn(B, N, 3, generator=g, dtype=torch.float64)
    return out.float()


def stray_ladder(N):
    """Ladder entries that do not follow sheet_chain's blocks, for N >= 6: one antiparallel and, from N = 12 on, one parallel ladder,
    with unequal weights; every centre lies in 1..N-2 and every rung spans at least 3 residues."""
    if N < 12:
        return [(1, N - 2, 1, 'A', 0.7)]
    n = min(4, (N - 4) // 4)
    return [(1, N - 2, n, 'A', 0.7), (2, N // 2 + 1, n, 'P')]


def chain_config(x, table=TABLE, separation=SEPARATION):
    """All three terms on the chains x: an antiparallel minimum above every particle's soft content, a parallel maximum at half of
    the smallest particle's (one class under its minimum, the other over its maximum), and stray_ladder(N) where N can hold one.
    Where the smallest parallel count is below 0.01 rungs (short chains: few or no parallel rungs), half of it would sit within
    float32 rounding of the count, and the maximum is 0.5 instead, which no particle reaches."""
    N = x.shape[1]
    t = terms(x.double(), config(table=table, separation=separation))
    ladder = stray_ladder(N) if N >= 6 else None
    p_min = float(t['parallel_content'].min())
    return config(antiparallel=(round(1.3 * float(t['antiparallel_content'].max()) + 0.05, 3), math.inf), antiparallel_weight=1.0,
                  parallel=(0.0, round(0.5 * p_min, 4) if N * p_min >= 0.01 else 0.5), parallel_weight=1.5,
                  ladder=ladder, ladder_weight=0.0 if ladder is None else 0.05, table=table, separation=separation)


def only(cfg, term):
    """cfg with one term left on: 'antiparallel', 'parallel' or 'ladder'."""
    out = dict(cfg)
    if term != 'antiparallel':
        out['antiparallel_weight'] = 0.0
    if term != 'parallel':
        out['parallel_weight'] = 0.0
    if term != 'ladder':
        out['ladder'], out['ladder_weight'] = None, 0.0
    return out


def potential(cfg, n_res, abar, **kw):
    """The SheetPotential of a configuration (both content terms always given: a weight of 0 is how cfg switches one off)."""
    from genie2_amd.smc import SheetPotential
    return SheetPotential(n_res, abar, antiparallel=cfg['antiparallel'], antiparallel_weight=cfg['antiparallel_weight'],
                          parallel=cfg['parallel'], parallel_weight=cfg['parallel_weight'], ladder=cfg['ladder'],
                          ladder_weight=cfg['ladder_weight'], table=cfg['table'], separation=cfg['separation'], device='cuda', **kw)
