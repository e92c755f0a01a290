"""What the motif potential's test files share (tests/test_motif_potential.py, test_motif_rigid.py, test_motif_groups.py and the
float64 oracles tests/_motif_rigid.py, _motif_groups.py): the 6E6R inputs, chain-like coordinates, the MotifPotential runners and the
checks against an oracle's dict, with their bounds: logp within 1e-5 max(1, |logp|); gradient within 1e-5 of the particle's largest
gradient entry (+ `grad_floor`)."""
import os

import numpy as np
import torch

MOTIF = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'motif_problem_6E6R.pdb')


def segments_6e6r():
    from genie2_amd.sample_unconditional_motif import load_motif_segments
    return [torch.tensor(s, dtype=torch.float32) for s in load_motif_segments(MOTIF)]


def walk(B, N, seed, step=3.8):
    """Chain-like coordinates: a random walk of C-alpha spacing."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, N, 3, generator=g)
    return torch.cumsum(step * v / v.norm(dim=-1, keepdim=True), dim=1)


def all_starts(n_res, lens, max_offsets=10 ** 6, seed=0):
    from genie2_amd.smc import get_all_motif_locations, placement_starts
    return placement_starts(get_all_motif_locations(n_res, lens, max_offsets, np.random.RandomState(seed)))


def top_two_gap(score):
    """Relative gap between the two largest scores of every row [B, P >= 2]."""
    top = torch.topk(score, 2, dim=1).values
    return (top[:, 0] - top[:, 1]) / top[:, 0].abs()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _abar(T=1000):
    from genie2_amd import pack
    return pack.schedule_tensors(T)['alphas_cumprod'].cuda()


def _var500(abar):
    from genie2_amd.smc import xstart_variance
    return float(xstart_variance(abar[500], 0.012).to(torch.float32))      # the f32 value the kernel reads


def _fix_var(pot, v):
    pot.variance = lambda step, v=v: torch.tensor([v], dtype=torch.float32, device='cuda')
    return float(np.float32(v))


def _run(pot, x0, step=500):
    x = x0.cuda().requires_grad_(True)
    lp = pot(x, step)
    g, = torch.autograd.grad(lp.sum(), x)
    return lp.detach(), g


def _check(logp, grad, ref, what, grad_floor=0.0):
    lp, g = logp.double().cpu(), grad.double().cpu()
    tol = 1e-5 * ref['logp'].abs().clamp(min=1.0)
    print(what, 'logp error / bound', ((lp - ref['logp']).abs() / tol).tolist())
    for b in range(g.shape[0]):
        d = float((g[b] - ref['grad'][b]).abs().max())
        bound = 1e-5 * (float(ref['grad'][b].abs().max()) + grad_floor)
        print(what, 'particle %d: gradient error %.3e, bound %.3e' % (b, d, bound))
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), what
    assert bool(((lp - ref['logp']).abs() <= tol).all()), (what, lp, ref['logp'])
    for b in range(g.shape[0]):
        d = float((g[b] - ref['grad'][b]).abs().max())
        assert d <= 1e-5 * (float(ref['grad'][b].abs().max()) + grad_floor), (what, b, d)


def _pot(segs, n_res, abar, P=10 ** 6, seed=0, **kw):
    from genie2_amd.smc import MotifPotential
    return MotifPotential(segs, n_res, abar, max_offsets=P, rng=np.random.RandomState(seed), device='cuda', **kw)


def _lds_cap(work_bytes):
    """The largest P whose records stay in LDS (work_bytes(P) == 0), by bisection on the host function."""
    lo, hi = 1, 20000
    assert work_bytes(lo) == 0 and work_bytes(hi) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if work_bytes(mid) == 0:
            lo = mid
        else:
            hi = mid
    return lo


def _tiny_model(base_weights, T=12):
    from genie.config import Config
    from genie2_amd.diffusion import Genie
    cfg = Config()
    cfg.diffusion['n_timestep'] = T
    model = Genie(cfg)
    model.model.load_state_dict(base_weights)
    return model.eval().to('cuda:0')


def _ca_coordinates(path):
    ca = [line for line in open(path) if line.startswith('ATOM') and line[13:15].strip() == 'CA']
    return np.array([[float(line[30:38]), float(line[38:46]), float(line[46:54])] for line in ca])
