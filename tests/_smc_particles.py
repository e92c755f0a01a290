"""What the particle-system tests share (tests/test_smc_particles_host.py, test_smc_particles_gpu.py): the input recipe of the
kernel-level cases, a float64 oracle of genie_smc_reweight -- genie2_amd/smc.py's weight update, ESS, systematic resampling and
renormalisation, restated per system -- the same lines in float32 as the sampler runs them today (the error bar of the GPU test),
and a raw ctypes call of the entry for the refusals."""
import ctypes as C
import math
import types

import torch

# (S, K, N, sigma, seed).  Even systems keep their particles (ESS / K 0.78-0.95), odd ones resample (0.13-0.42): every case with two
# systems or more takes both branches in one call.
CASES = [(1, 1, 2, 0.2, 0), (1, 2, 2, 0.2, 0), (3, 5, 40, 0.2, 0), (2, 64, 40, 0.2, 1), (4, 8, 257, 0.02, 0)]
ESS_FRACTION = 0.5


def make_inputs(S, K, N, sigma, seed):
    """The inputs of one case, float32 on the CPU, from a generator seeded with `seed`."""
    g = torch.Generator().manual_seed(seed)
    B, f64 = S * K, torch.float64
    spread = torch.tensor([0.1 if s % 2 == 0 else 1.5 for s in range(S)], dtype=f64).repeat_interleave(K)
    mean_un = torch.cumsum(3.0 * torch.randn(B, N, 3, generator=g, dtype=f64), dim=1)
    a = torch.rand(B, generator=g, dtype=f64) * spread
    mean_tw = mean_un + 0.25 * sigma * a[:, None, None] * torch.randn(B, N, 3, generator=g, dtype=f64)
    x_new = mean_tw + 0.6 * sigma * torch.randn(B, N, 3, generator=g, dtype=f64)
    log_prob = torch.randn(B, generator=g, dtype=f64) * spread
    log_proposal = 0.3 * torch.randn(B, generator=g, dtype=f64)
    log_w_acc = 0.3 * torch.randn(B, generator=g, dtype=f64)
    u = torch.rand(S, generator=g, dtype=f64) / K
    out = dict(x_new=x_new, mean_tw=mean_tw, mean_un=mean_un, sigma=torch.tensor([sigma], dtype=f64), log_prob=log_prob, u=u,
               log_proposal=log_proposal, log_w_acc=log_w_acc)
    return {k: v.to(torch.float32) for k, v in out.items()}


def _log_density_sum(x, mean, sigma):
    return torch.distributions.normal.Normal(loc=mean, scale=sigma).log_prob(x).sum(dim=(1, 2))


def oracle(S, K, inp, ess_fraction=ESS_FRACTION):
    """float64, per system, from the float32 inputs: dict of log_w [S K], ess [S], resampled [S] bool, index [S K] (batch indices,
    identity where a system stays), log_w_acc and log_proposal [S K] after the call, cumsum [S, K] and points [S, K]."""
    d = {k: v.double() for k, v in inp.items()}
    sigma = d['sigma'].reshape(())
    log_rev = _log_density_sum(d['x_new'], d['mean_un'], sigma)
    log_tw = _log_density_sum(d['x_new'], d['mean_tw'], sigma)
    log_w = (log_rev + d['log_prob'] - log_tw) - d['log_proposal'] + d['log_w_acc']
    out = dict(log_w=log_w, ess=torch.zeros(S, dtype=torch.float64), resampled=torch.zeros(S, dtype=torch.bool),
               index=torch.arange(S * K), log_w_acc=torch.zeros(S * K, dtype=torch.float64), cumsum=torch.zeros(S, K, dtype=torch.float64),
               points=torch.zeros(S, K, dtype=torch.float64))
    for s in range(S):
        lw = log_w[s * K:(s + 1) * K]
        shifted = lw - lw.max()
        log_norm = shifted - torch.logsumexp(shifted, dim=0)                 # normalize_log_weights
        w = torch.exp(log_norm)
        out['ess'][s] = w.sum() ** 2 / (w ** 2).sum()                          # compute_ess
        sm = torch.softmax(lw, dim=0)
        out['cumsum'][s] = torch.cumsum(sm / sm.sum(), dim=0)
        out['points'][s] = d['u'][s] + torch.arange(K, dtype=torch.float64) / K
        if bool(out['ess'][s] < ess_fraction * K):
            out['resampled'][s] = True
            out['index'][s * K:(s + 1) * K] = s * K + torch.searchsorted(out['cumsum'][s], out['points'][s], right=False).clamp(max=K - 1)
        else:
            out['log_w_acc'][s * K:(s + 1) * K] = log_norm + math.log(K)
    out['log_proposal'] = d['log_prob'][out['index']]
    return out


def margins(S, K, ref, ess_fraction=ESS_FRACTION):
    """(smallest |ess - ess_fraction K| / K, smallest |point - cumulative sum| K, over every system): how far the discrete outputs
    are from changing."""
    ess = float(((ref['ess'] - ess_fraction * K).abs() / K).min())
    return ess, min(float((ref['points'][s][:, None] - ref['cumsum'][s][None, :]).abs().min()) * K for s in range(S))


def torch_float32_lines(K, inp, s, device):
    """genie2_amd/smc.py's lines for the weights of one system (the slice s of the inputs), as the sampler runs them for a whole
    batch today: float32 torch on `device`.  Returns (ess, log_w_acc after renormalisation), as float64 CPU tensors."""
    from genie2_amd.smc import compute_ess_from_log_w, log_normal_density, normalize_log_weights
    sl = slice(s * K, (s + 1) * K)
    new, mean_t, mean_u = (inp[k][sl].to(device) for k in ('x_new', 'mean_tw', 'mean_un'))
    sigma = inp['sigma'].to(device).reshape(())
    log_prob, log_proposal, log_w_acc = (inp[k][sl].to(device) for k in ('log_prob', 'log_proposal', 'log_w_acc'))
    log_rev = log_normal_density(new, mean_u, sigma ** 2).sum(dim=(1, 2))
    log_tw = log_normal_density(new, mean_t, sigma ** 2).sum(dim=(1, 2))
    log_w = (log_rev + log_prob - log_tw) - log_proposal
    log_w_acc = log_w + log_w_acc
    ess = compute_ess_from_log_w(log_w_acc)
    acc = normalize_log_weights(log_w_acc, dim=0) + torch.log(torch.tensor(float(K), device=device))
    return ess.double().cpu(), acc.double().cpu()


N_ARGS = 19


def raw_call(lib, S, K, N, ptrs, ess_fraction=ESS_FRACTION, work=None, work_bytes=0, stream=None):
    """genie_smc_reweight with raw addresses: `ptrs` maps the entry's 12 pointer arguments before `work`, in its order, to ints (0 = NULL)."""
    names = ('x_new', 'mean_tw', 'mean_un', 'sigma', 'log_prob', 'u', 'log_proposal', 'log_w_acc', 'x_out', 'index_out', 'ess_out',
             'resampled_out')
    p = [C.c_void_p(ptrs[k]) for k in names]
    return lib.genie_smc_reweight(C.c_void_p(stream), S, K, N, *p[:6], float(ess_fraction), *p[6:], C.c_void_p(work), work_bytes)


def cpu_model(T=10):
    """A Genie stand-in on the CPU device: anything that reaches the engine fails, so a ValueError shows the parameters were checked
    first."""
    from genie2_amd.config import Config
    from genie2_amd.model import Denoiser
    cfg = Config()
    cfg.model.update(n_pair_transform_layer=1, n_structure_layer=1)
    cfg.diffusion['n_timestep'] = T
    m = Denoiser(**cfg.model, n_timestep=T, max_n_res=64, max_n_chain=1)
    return types.SimpleNamespace(model=m, config=cfg, device=torch.device('cpu'), setup_schedule=lambda: None)
