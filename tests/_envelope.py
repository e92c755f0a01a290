"""What the envelope potential's test files share (tests/test_envelope_host.py, test_envelope_gpu.py): two restatements of
genie_envelope_potential (include/genie_hip.h) in plain torch that never call the library -- `reference` in float64 on the CPU with the
gradient from autograd (the oracle), and the same code in float32 (`restatement32`: the measure of what float32 arithmetic costs on an
input, the timing reference of tools/envelope_potential_time.py and the torch `twisting_function` of the end-to-end tests) -- the
header's analytic gradient written out with loops, the margins of the discontinuous report fields, and the inputs of the cases.

A configuration is a dict: 'raw' [M, 3] float64, the points as given; 'points' [M, 3] float64, the points as EnvelopePotential places
them (weighted centroid at the origin, rounded to float32: what the kernel reads); 'weights' [M] float64 or None; tau, inside,
inside_weight, cover, cover_weight (floats; a weight of 0 switches its term off)."""
import torch

REPORT = ('n_outside', 'max_outside', 'n_uncovered', 'max_uncovered', 'e_envelope_inside', 'e_envelope_cover')
COUNTS = ('n_outside', 'n_uncovered')
EPS = 0.1               # GENIE_ENVELOPE_EPS
CHUNK = 1024            # GENIE_ENVELOPE_CHUNK
FILL = 2048             # GENIE_ENVELOPE_FILL: work-groups of a launch from which it runs 4 waves per work-group instead of 16

# (B, N, seed, solid, spacing, M, weighted): the parity shapes of test_envelope_gpu.py on _motif.walk(B, N, seed) with the centroid
# removed.  The envelope is the first M lattice points of the solid (all of them where M is its whole count), weights 1 unless
# `weighted` (then uniform in 0.5..1.5 from the seed).  The first five are the ones the feature was specified with, the last five sit
# around the launch-size threshold of the entry; the seeds of all but the first five were picked on the CPU with the oracle alone:
# `inputs` asserts that no a_n is within 1e-4 of inside_distance and no c_m within 1e-4 of cover_distance.
CASES = [(3, 64, 64, 'ellipsoid:12,12,12', 3.0, 257, False), (3, 65, 65, 'ellipsoid:25,8,8', 3.0, 253, False),
         (3, 129, 129, 'ellipsoid:20,15,10', 2.5, 773, False), (2, 300, 300, 'ellipsoid:30,20,15', 3.0, 1375, False),
         (1, 1512, 5, 'sphere:40', 4.0, 4169, False),
         (3, 1, 1, 'sphere:24', 3.0, 1, False), (3, 2, 2, 'sphere:24', 3.0, 3, False), (3, 63, 63, 'sphere:24', 3.0, 64, False),
         (2, 70, 1023, 'sphere:24', 3.0, CHUNK - 1, False), (2, 70, 1024, 'sphere:24', 3.0, CHUNK, False),
         (2, 70, 1025, 'sphere:24', 3.0, CHUNK + 1, False),
         (1, CHUNK - 1, 1023, 'ellipsoid:12,12,12', 3.0, 257, False), (1, CHUNK, 1024, 'ellipsoid:12,12,12', 3.0, 257, False),
         (1, CHUNK + 1, 1025, 'ellipsoid:12,12,12', 3.0, 257, False),
         (3, 129, 7, 'ellipsoid:20,15,10', 2.5, 773, True),
         # either side of GENIE_ENVELOPE_FILL: B (1 + 1) work-groups of the soft minima, B of the gather; and a launch above it that
         # walks two chunks with 4 waves
         (FILL // 2 - 1, 2, 1023, 'sphere:24', 3.0, 3, False), (FILL // 2, 2, 1024, 'sphere:24', 3.0, 3, False),
         (FILL - 1, 2, 2047, 'sphere:24', 3.0, 3, False), (FILL, 2, 2048, 'sphere:24', 3.0, 3, False),
         (108, 70, 108, 'sphere:24', 3.0, CHUNK + 1, False)]


def case_id(case):
    return 'B%d-N%d-M%d%s' % (case[0], case[1], case[5], '-weighted' if case[6] else '')


def placed(points, weights=None, center=True):
    """The points as EnvelopePotential places them: the weighted centroid removed in float64, then rounded to float32."""
    y = torch.as_tensor(points).double()
    if center:
        u = torch.ones(len(y), dtype=torch.float64) if weights is None else torch.as_tensor(weights).double()
        y = y - (u[:, None] * y).sum(dim=0, keepdim=True) / u.sum()
    return y.float().double()


def config(points, weights=None, tau=4.0, inside=3.0, inside_weight=1.0, cover=5.0, cover_weight=1.0, center=True):
    raw = torch.as_tensor(points).double()
    w = None if weights is None else torch.as_tensor(weights).float().double()        # (the kernel reads float32 weights)
    return dict(raw=raw, points=placed(raw, w, center), weights=w, tau=float(tau), inside=float(inside), inside_weight=float(inside_weight),
                cover=float(cover), cover_weight=float(cover_weight), center=bool(center))


def cfg_key(cfg):
    return repr(sorted((k, v if not torch.is_tensor(v) else (tuple(v.shape), float(v.sum()), float((v ** 2).sum()))) for k, v in cfg.items()))


def soft_distances(x, cfg):
    """(a [B, N], c [B, M]) of x [B, N, 3], in x's dtype and on its device, differentiable in x."""
    y = cfg['points'].to(dtype=x.dtype, device=x.device)
    q = ((x[:, :, None, :] - y[None, None, :, :]) ** 2).sum(dim=-1)                 # [B, N, M], from the differences
    s = -cfg['tau'] * torch.logsumexp(-q / cfg['tau'], dim=2)
    t = -cfg['tau'] * torch.logsumexp(-q / cfg['tau'], dim=1)
    return torch.sqrt(torch.clamp(s, min=0) + EPS ** 2), torch.sqrt(torch.clamp(t, min=0) + EPS ** 2)


def terms(x, cfg):
    """Everything the entry reports of x [B, N, 3], in x's dtype and on its device, differentiable: the REPORT fields [B] each,
    'distance' [B, N] (the a_n), 'gap' [B, M] (the c_m) and 'energy' = e_envelope_inside + e_envelope_cover."""
    N = x.shape[1]
    a, c = soft_distances(x, cfg)
    M = c.shape[1]
    v = torch.ones(M, dtype=x.dtype, device=x.device) if cfg['weights'] is None else cfg['weights'].to(dtype=x.dtype, device=x.device)
    h, g = torch.clamp(a - cfg['inside'], min=0), torch.clamp(c - cfg['cover'], min=0)
    out = {'distance': a, 'gap': c, 'n_outside': (h > 0).sum(dim=1), 'max_outside': h.max(dim=1).values,
           'n_uncovered': (g > 0).sum(dim=1), 'max_uncovered': g.max(dim=1).values,
           'e_envelope_inside': cfg['inside_weight'] * (h ** 2).sum(dim=1),
           'e_envelope_cover': cfg['cover_weight'] * (N / v.sum()) * (v[None] * g ** 2).sum(dim=1)}
    out['energy'] = out['e_envelope_inside'] + out['e_envelope_cover']
    return out


def logp(x, cfg, var):
    return -terms(x, cfg)['energy'] / (2 * var)


def _evaluate(x, cfg, var):
    x = x.detach().clone().requires_grad_(True)
    t = terms(x, cfg)
    lp = -t['energy'] / (2 * var)
    grad, = torch.autograd.grad(lp.sum(), x)
    out = {k: t[k].detach() for k in REPORT + ('distance', 'gap')}
    out.update(logp=lp.detach(), grad=grad)
    return out


def reference(x, cfg, var):
    """The float64 oracle on the CPU: 'logp' [B], 'grad' [B, N, 3] (autograd), the REPORT fields, 'distance' [B, N] and 'gap' [B, M]."""
    return _evaluate(x.detach().double().cpu(), cfg, float(var))


def restatement32(x, cfg, var):
    """The same code in float32, on x's device."""
    return _evaluate(x.detach().float(), cfg, float(var))


def twisting_function(cfg, abar, tausq=1.0):
    """The float32 restatement as a TwistedSampler `twisting_function`, with EnvelopePotential's variance."""
    from genie2_amd.smc import xstart_variance

    def twist(x0, step):
        return logp(x0.float(), cfg, xstart_variance(abar[step], tausq).to(torch.float32))
    return twist


def loop_gradient(x, cfg, var):
    """The gradient as include/genie_hip.h states it, written out with loops in float64 (small N and M only)."""
    import math
    x = x.detach().double()
    y = cfg['points']
    B, N, _ = x.shape
    M = len(y)
    v = [1.0] * M if cfg['weights'] is None else cfg['weights'].tolist()
    tau, scale = cfg['tau'], N / sum(v)
    out = torch.zeros_like(x)
    for b in range(B):
        q = [[float(((x[b, n] - y[m]) ** 2).sum()) for m in range(M)] for n in range(N)]
        s, t = [], []
        for n in range(N):
            lo = min(q[n])
            s.append(lo - tau * math.log(sum(math.exp((lo - q[n][m]) / tau) for m in range(M))))
        for m in range(M):
            lo = min(q[n][m] for n in range(N))
            t.append(lo - tau * math.log(sum(math.exp((lo - q[n][m]) / tau) for n in range(N))))
        a = [math.sqrt(max(v_, 0.0) + EPS ** 2) for v_ in s]
        c = [math.sqrt(max(v_, 0.0) + EPS ** 2) for v_ in t]
        h = [max(0.0, v_ - cfg['inside']) for v_ in a]
        g = [max(0.0, v_ - cfg['cover']) for v_ in c]
        for n in range(N):
            acc = torch.zeros(3, dtype=torch.float64)
            for m in range(M):
                d = x[b, n] - y[m]
                acc += cfg['inside_weight'] * (h[n] / a[n]) * math.exp((s[n] - q[n][m]) / tau) * d
                acc += cfg['cover_weight'] * scale * v[m] * (g[m] / c[m]) * math.exp((t[m] - q[n][m]) / tau) * d
            out[b, n] = -acc / var
    return out


def margins(x, cfg):
    """How far the discontinuous report fields (n_outside, n_uncovered) are from flipping, in float64: the smallest |a_n -
    inside_distance| and |c_m - cover_distance|."""
    a, c = soft_distances(x.detach().double().cpu(), cfg)
    return min(float((a - cfg['inside']).abs().min()), float((c - cfg['cover']).abs().min()))


def centred_walk(B, N, seed):
    from _motif import walk
    x = walk(B, N, seed)
    return x - x.mean(dim=1, keepdim=True)


def case_config(case, **kw):
    from genie2_amd.smc import envelope_shape_points
    _, _, seed, solid, spacing, M, weighted = case
    pts = envelope_shape_points(solid, spacing)
    assert len(pts) >= M, (solid, spacing, len(pts), M)
    weights = 0.5 + torch.rand(M, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) if weighted else None
    return config(pts[:M], weights, **kw)


def inputs(case, **kw):
    """(x [B, N, 3] float32, cfg) of a case, both terms on, checked: no a_n within 1e-4 of inside_distance, no c_m within 1e-4 of
    cover_distance."""
    x, cfg = centred_walk(*case[:3]), case_config(case, **kw)
    m = margins(x, cfg)
    assert m >= 1e-4, 'a soft distance of this input is %.1e from its bound: take another seed' % m
    return x, cfg


def potential(cfg, n_res, abar, **kw):
    """The EnvelopePotential of a configuration, from the points as given."""
    from genie2_amd.smc import EnvelopePotential
    return EnvelopePotential(n_res, abar, cfg['raw'], weights=cfg['weights'], inside_distance=cfg['inside'], inside_weight=cfg['inside_weight'],
                             cover_distance=cfg['cover'], cover_weight=cfg['cover_weight'], softness=cfg['tau'], center=cfg['center'],
                             device='cuda', **kw)
