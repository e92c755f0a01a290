"""What the secondary-structure potential's test files share (tests/test_secstruct_host.py, test_secstruct_gpu.py): two restatements
of genie_secstruct_potential (include/genie_hip.h) in plain torch that never call the library -- `reference` in float64 on the CPU with
the gradient from autograd (the oracle), and the same code in float32 (`restatement32`: the measure of what float32 arithmetic costs on
an input, the timing reference of tools/secstruct_potential_time.py and the torch `twisting_function` of the end-to-end tests) -- the
margins of the discontinuous report fields, and the inputs of the cases.

A configuration is a dict: table (16 floats: H mu, H sigma, E mu, E sigma over d2, d3, d4, chi), helix and extended ((min, max)
fractions), helix_weight, extended_weight, target (a string over `HE-`, or None) and target_weight; a weight of 0 switches a term off."""
import math

import torch

REPORT = ('helix_content', 'extended_content', 'n_helix', 'n_extended', 'e_helix', 'e_extended', 'e_target', 'n_target_missed')
COUNTS = ('n_helix', 'n_extended', 'n_target_missed')
TABLE = (5.5, 5.3, 6.4, 0.77, 0.5, 0.5, 0.6, 0.25, 6.7, 9.9, 12.4, -0.12, 0.6, 0.9, 1.1, 0.45)
CODES = {'-': 0, 'H': 1, 'E': 2}


def config(helix=(0.0, 1.0), helix_weight=0.0, extended=(0.0, 1.0), extended_weight=0.0, target=None, target_weight=0.0, table=TABLE):
    return dict(helix=(float(helix[0]), float(helix[1])), helix_weight=float(helix_weight),
                extended=(float(extended[0]), float(extended[1])), extended_weight=float(extended_weight), target=target,
                target_weight=float(target_weight), table=tuple(float(v) for v in table))


def _norm(diff):
    """|diff| over the last axis, with value 0 and gradient 0 where it is exactly 0 (the kernel's zero-distance rule)."""
    sq = (diff ** 2).sum(dim=-1)
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def features(x):
    """[B, N, 3] -> [B, W, 4]: d2, d3, d4 and the chirality of every window, chi = 0 (and no gradient) where a bond has length 0."""
    W = x.shape[1] - 4
    p = [x[:, k:k + W] for k in range(5)]
    b1, b2, b3 = p[1] - p[0], p[2] - p[1], p[3] - p[2]
    triple = (torch.linalg.cross(b1, b2, dim=-1) * b3).sum(dim=-1)
    length = _norm(b1) * _norm(b2) * _norm(b3)
    ok = length > 0
    chi = torch.where(ok, triple / torch.where(ok, length, torch.ones_like(length)), torch.zeros_like(length))
    return torch.stack([_norm(p[2] - p[0]), _norm(p[3] - p[0]), _norm(p[4] - p[0]), chi], dim=-1)


def zscores(x, cfg):
    """[B, N, 3] -> [B, W, 2, 4]: (f - mu_cf) / sigma_cf for the classes H, E."""
    t = torch.tensor(cfg['table'], dtype=x.dtype, device=x.device).view(2, 2, 4)               # [class, mu / sigma, feature]
    return (features(x)[:, :, None, :] - t[None, None, :, 0]) / t[None, None, :, 1]


def target_windows(target, N):
    """[W] codes: 1 / 2 where the window's five residues are all H / all E, else 0."""
    if target is None:
        return torch.zeros(N - 4, dtype=torch.long)
    return torch.tensor([CODES[target[i]] if target[i:i + 5] == target[i] * 5 else 0 for i in range(N - 4)], dtype=torch.long)


def terms(x, cfg):
    """Everything the entry reports of x [B, N, 3], in x's dtype and on its device, differentiable where it is continuous: the
    REPORT fields [B] each, 'assign' [B, N] (0 C, 1 H, 2 E), 'u' [B, W, 2], 'n' [B, 2] and 'energy' = e_helix + e_extended + e_target."""
    B, N, _ = x.shape
    W = N - 4
    z = zscores(x, cfg)
    u = 0.25 * (z ** 2).sum(dim=-1)                                                             # [B, W, 2]
    n = (1.0 / (1.0 + u)).sum(dim=1)                                                            # [B, 2]
    out = {'u': u, 'n': n, 'helix_content': n[:, 0] / W, 'extended_content': n[:, 1] / W}
    for c, name in enumerate(('helix', 'extended')):
        lo, hi = cfg[name]
        out['e_' + name] = cfg[name + '_weight'] * (torch.clamp(W * lo - n[:, c], min=0) ** 2 + torch.clamp(n[:, c] - W * hi, min=0) ** 2)
    tw = target_windows(cfg['target'], N).to(x.device)
    picked = torch.where(tw == 1, u[:, :, 0], torch.where(tw == 2, u[:, :, 1], torch.zeros_like(u[:, :, 0])))
    out['e_target'] = cfg['target_weight'] * picked.sum(dim=1)
    # the hard assignment: a window is of class c when all four |z| <= 1; a residue is H if any window containing it is, else E
    hard = (z.detach().abs() <= 1).all(dim=-1)                                                  # [B, W, 2]
    res = torch.zeros(B, N, 2, dtype=torch.bool, device=x.device)
    for k in range(5):
        res[:, k:k + W] |= hard
    assign = torch.where(res[:, :, 0], 1, torch.where(res[:, :, 1], 2, 0)).to(torch.int8)
    out['assign'] = assign
    out['n_helix'], out['n_extended'] = (assign == 1).sum(dim=1), (assign == 2).sum(dim=1)
    if cfg['target'] is None:
        out['n_target_missed'] = torch.zeros(B, dtype=torch.long, device=x.device)
    else:
        t = torch.tensor([CODES[c] for c in cfg['target']], dtype=torch.int8, device=x.device)
        out['n_target_missed'] = ((t[None] != 0) & (assign != t[None])).sum(dim=1)
    out['energy'] = out['e_helix'] + out['e_extended'] + out['e_target']
    return out


def logp(x, cfg, var):
    return -terms(x, cfg)['energy'] / (2 * var)


def _evaluate(x, cfg, var):
    x = x.detach().clone().requires_grad_(True)
    t = terms(x, cfg)
    lp = -t['energy'] / (2 * var)
    grad, = torch.autograd.grad(lp.sum(), x, allow_unused=True)
    out = {k: t[k].detach() for k in REPORT + ('assign', 'u', 'n')}
    out.update(logp=lp.detach(), grad=torch.zeros_like(x) if grad is None else grad)
    return out


def reference(x, cfg, var):
    """The float64 oracle on the CPU: 'logp' [B], 'grad' [B, N, 3] (autograd), the REPORT fields, 'assign', 'u' and 'n'."""
    return _evaluate(x.detach().double().cpu(), cfg, float(var))


def restatement32(x, cfg, var):
    """The same code in float32, on x's device."""
    return _evaluate(x.detach().float(), cfg, float(var))


def twisting_function(cfg, abar, tausq=1.0):
    """The float32 restatement as a TwistedSampler `twisting_function`, with SecStructPotential's variance."""
    from genie2_amd.smc import xstart_variance

    def twist(x0, step):
        return logp(x0.float(), cfg, xstart_variance(abar[step], tausq).to(torch.float32))
    return twist


def margins(x, cfg):
    """How far the discontinuous or kinked quantities are from flipping, in float64: (the smallest | |z| - 1 | over all windows,
    classes and features, the smallest |n_c - W f_c^{min,max}| over both classes and both bounds)."""
    x = x.detach().double().cpu()
    W = x.shape[1] - 4
    z = zscores(x, cfg)
    n = terms(x, cfg)['n']
    hinge = min(float((n[:, c] - W * f).abs().min()) for c, name in enumerate(('helix', 'extended')) for f in cfg[name])
    return float((z.abs() - 1).abs().min()), hinge


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def ideal_helix(n, handed=1.0):
    """An ideal alpha-helix of C-alphas [n, 3], float64: radius 2.3 A, rise 1.5 A, 100 degrees per residue; handed = -1 mirrors it."""
    k = torch.arange(n, dtype=torch.float64)
    a = math.radians(100.0) * k
    return torch.stack([2.3 * torch.cos(a), handed * 2.3 * torch.sin(a), 1.5 * k], dim=-1)


def ideal_extended(n):
    """An ideal extended segment [n, 3], float64: radius 0.95 A, rise 3.3 A, -165 degrees per residue."""
    k = torch.arange(n, dtype=torch.float64)
    a = math.radians(-165.0) * k
    return torch.stack([0.95 * torch.cos(a), 0.95 * torch.sin(a), 3.3 * k], dim=-1)


def _unit(g):
    v = torch.randn(3, generator=g, dtype=torch.float64)
    return v / v.norm()


def _rotation(g):
    """A proper rotation (determinant +1: a helix keeps its hand)."""
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))[None]
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def mixed_chain(B, N, seed, jitter=0.15):
    """C-alpha chains [B, N, 3], float32: segments of three kinds in rotation -- an ideal right-handed helix, an ideal extended
    segment, a random 3.8 A walk -- each in a random orientation, joined with 3.8 A bonds, with Gaussian jitter of `jitter` A on every
    coordinate.  The first three segments have 8 residues (so N >= 24 holds all three kinds), later ones 8..14; particle b starts
    the rotation at kind b % 3."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(B, N, 3, dtype=torch.float64)
    for b in range(B):
        rows, k = [], 0
        while sum(len(r) for r in rows) < N:
            n = 8 if k < 3 else 8 + int(torch.randint(0, 7, (1,), generator=g))
            kind = (b + k) % 3
            if kind == 0:
                seg = ideal_helix(n)
            elif kind == 1:
                seg = ideal_extended(n)
            else:
                steps = torch.randn(n, 3, generator=g, dtype=torch.float64)
                seg = torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), dim=0)
            seg = (seg - seg[0]) @ _rotation(g).T
            start = torch.zeros(3, dtype=torch.float64) if not rows else rows[-1][-1] + 3.8 * _unit(g)
            rows.append(seg + start)
            k += 1
        out[b] = torch.cat(rows)[:N]
    out = out + jitter * torch.randn(B, N, 3, generator=g, dtype=torch.float64)
    return out.float()


def blueprint(N):
    """A target of length N that does not follow mixed_chain's segments: runs of 7 H, 2 free, 7 E, 3 free, cut to N."""
    unit = 'HHHHHHH--EEEEEEE---'
    return (unit * (N // len(unit) + 1))[:N]


def chain_config(x, table=TABLE):
    """All three terms on the chains x: a helix minimum above every particle's soft helix content, an extended maximum below every
    particle's soft extended content (one class under its minimum, the other over its maximum), and blueprint(N)."""
    t = terms(x.double(), config(table=table))
    return config(helix=(round(min(1.0, 1.3 * float(t['helix_content'].max()) + 0.05), 3), 1.0), helix_weight=1.0,
                  extended=(0.0, round(0.5 * float(t['extended_content'].min()), 3)), extended_weight=1.5,
                  target=blueprint(x.shape[1]), target_weight=0.5, table=table)


def only(cfg, term):
    """cfg with one term left on: 'helix', 'extended' or 'target'."""
    out = dict(cfg)
    if term != 'helix':
        out['helix_weight'] = 0.0
    if term != 'extended':
        out['extended_weight'] = 0.0
    if term != 'target':
        out['target'], out['target_weight'] = None, 0.0
    return out


def potential(cfg, n_res, abar, **kw):
    """The SecStructPotential of a configuration (both content terms always given: a weight of 0 is how cfg switches one off)."""
    from genie2_amd.smc import SecStructPotential
    return SecStructPotential(n_res, abar, helix=cfg['helix'], helix_weight=cfg['helix_weight'], extended=cfg['extended'],
                              extended_weight=cfg['extended_weight'], target=cfg['target'], target_weight=cfg['target_weight'],
                              table=cfg['table'], device='cuda', **kw)
