"""float64 oracle of the superposed motif potential (genie_motif_potential_rigid, csrc/smc_kernels.hip; include/genie_hip.h states
the formulas): the selection by `starts`, Kabsch by torch.linalg.svd with the determinant correction, logp and its gradient by torch
autograd (through the SVD, or with R detached: the two agree because the derivative through R vanishes at the optimum)."""
import numpy as np
import torch


def placement_index(starts, seg_len):
    """int [P, S] starts -> long [P, M]: the residue of every motif position in every placement."""
    return torch.cat([starts[:, s:s + 1].long() + torch.arange(n) for s, n in enumerate(seg_len)], dim=1)


def centred_selection(x, idx):
    """x [B, N, 3], idx [P, M] -> [B, P, M, 3], every selection minus its mean."""
    sel = x[:, idx]
    return sel - sel.mean(dim=-2, keepdim=True)


def kabsch(c, tc):
    """The proper rotation R [..., 3, 3] that minimises sum_m |c(m) - R tc(m)|^2: c [..., M, 3], tc [M, 3] centred."""
    h = torch.einsum('ma,...mb->...ab', tc, c)                      # sum_m tc c^T
    u, _, vh = torch.linalg.svd(h)
    v, ut = vh.transpose(-1, -2), u.transpose(-1, -2)
    d = torch.sign(torch.linalg.det(v @ ut)).detach()
    one = torch.ones_like(d)
    return v @ torch.diag_embed(torch.stack([one, one, d], dim=-1)) @ ut


def residual_q(c, tc, detach_rotation=False):
    """q [...] = sum_m |c(m) - R tc(m)|^2 after the fit."""
    r = kabsch(c, tc)
    if detach_rotation:
        r = r.detach()
    e = c - torch.einsum('...ab,mb->...ma', r, tc)
    return (e ** 2).sum(dim=(-1, -2))


def rigid_oracle(x0, starts, seg_len, target, var, detach_rotation=False, want_grad=True, dtype=torch.float64):
    """{'logp' [B], 'grad' [B,N,3] (or None), 'score' [B,P], 'q' [B,P], 'best' [B], 'rmsd' [B]} in float64 on the CPU (`dtype`: the
    same statements in another precision, the float32 restatement that tells how much a bound may widen)."""
    x = x0.detach().to(dtype).cpu().requires_grad_(want_grad)
    t = target.detach().to(dtype).cpu()
    tc = t - t.mean(dim=0, keepdim=True)
    q = residual_q(centred_selection(x, placement_index(starts.cpu(), seg_len)), tc, detach_rotation)
    score = -q / (2 * float(var))
    logp = torch.logsumexp(score, dim=1) - np.log(score.shape[1])
    grad = torch.autograd.grad(logp.sum(), x)[0] if want_grad else None
    best = score.detach().argmax(dim=1)
    qb = q.detach().gather(1, best[:, None])[:, 0]
    return {'logp': logp.detach(), 'grad': grad, 'score': score.detach(), 'q': q.detach(), 'best': best,
            'rmsd': torch.sqrt(qb / tc.shape[0])}


def logp_only(x, starts, seg_len, target, var):
    """logp.sum() of a float64 x without autograd (for central differences)."""
    with torch.no_grad():
        t = target.double()
        q = residual_q(centred_selection(x, placement_index(starts, seg_len)), t - t.mean(dim=0, keepdim=True))
        return float((torch.logsumexp(-q / (2 * float(var)), dim=1) - np.log(q.shape[1])).sum())


def fit_rmsd(xyz, starts_row, seg_len, target):
    """Superposed motif RMSD of one structure xyz [N,3] at one placement (its segment starts)."""
    st = torch.as_tensor(starts_row, dtype=torch.int64).reshape(1, -1)
    t = torch.as_tensor(target).double()
    c = centred_selection(torch.as_tensor(xyz).double()[None], placement_index(st, seg_len))
    return float(torch.sqrt(residual_q(c, t - t.mean(dim=0, keepdim=True))[0, 0] / t.shape[0]))
