"""float64 oracle of the group-wise motif potential (genie_motif_potential_grouped, csrc/smc_kernels.hip; include/genie_hip.h states
the formulas) and the inputs its tests share: per-group selections through `placement_index`, a per-group Kabsch fit (or the identity),
q summed over the groups, logsumexp over the joint placements, the gradient by torch autograd."""
import numpy as np
import torch

from _motif import walk
from _motif_rigid import centred_selection, placement_index, residual_q


def canonical(groups):
    """Labels -> (labels by first appearance, index of every segment's group)."""
    labels = []
    for g in groups:
        if g not in labels:
            labels.append(g)
    return labels, [labels.index(g) for g in groups]


def position_groups(seg_len, seg_group):
    """long [M]: the group index of every motif position."""
    return torch.cat([torch.full((n,), g, dtype=torch.int64) for n, g in zip(seg_len, seg_group)])


def group_q(x, starts, seg_len, seg_group, target, rigid):
    """q^g [B, P, G] of a float64 x [B, N, 3]: every group centred and fitted on its own."""
    idx = placement_index(starts, seg_len)
    pg = position_groups(seg_len, seg_group)
    out = []
    for g in range(int(pg.max()) + 1):
        sel = pg == g
        tc = target[sel] - target[sel].mean(dim=0, keepdim=True)
        c = centred_selection(x, idx[:, sel])
        out.append(residual_q(c, tc) if rigid else ((c - tc) ** 2).sum(dim=(-1, -2)))
    return torch.stack(out, dim=-1)


def grouped_oracle(x0, starts, seg_len, seg_group, target, var, rigid=True, want_grad=True, dtype=torch.float64):
    """{'logp' [B], 'grad' [B,N,3] (or None), 'score' [B,P], 'q' [B,P], 'qg' [B,P,G], 'best' [B], 'rmsd' [B], 'group_rmsd' [B,G]} in
    float64 on the CPU (`dtype`: the same statements in another precision, the float32 restatement)."""
    x = x0.detach().to(dtype).cpu().requires_grad_(want_grad)
    qg = group_q(x, starts.cpu(), seg_len, seg_group, target.detach().to(dtype).cpu(), rigid)
    q = qg.sum(dim=-1)
    score = -q / (2 * float(var))
    logp = torch.logsumexp(score, dim=1) - np.log(score.shape[1])
    grad = torch.autograd.grad(logp.sum(), x)[0] if want_grad else None
    best = score.detach().argmax(dim=1)
    qgb = qg.detach()[torch.arange(len(best)), best]                       # [B, G]
    mg = torch.bincount(position_groups(seg_len, seg_group)).to(dtype)
    return {'logp': logp.detach(), 'grad': grad, 'score': score.detach(), 'q': q.detach(), 'qg': qg.detach(), 'best': best,
            'rmsd': torch.sqrt(qgb.sum(dim=1) / float(mg.sum())), 'group_rmsd': torch.sqrt(qgb / mg[None])}


def grouped_logp_only(x, starts, seg_len, seg_group, target, var, rigid=True):
    """logp.sum() of a float64 x without autograd (for central differences)."""
    with torch.no_grad():
        q = group_q(x, starts, seg_len, seg_group, target.double(), rigid).sum(dim=-1)
        return float((torch.logsumexp(-q / (2 * float(var)), dim=1) - np.log(q.shape[1])).sum())


def group_fit_rmsd(xyz, starts_row, seg_len, seg_group, target):
    """Superposed RMSD of every group [G] of one structure xyz [N,3] at one placement (its segment starts)."""
    st = torch.as_tensor(starts_row, dtype=torch.int64).reshape(1, -1)
    qg = group_q(torch.as_tensor(xyz).double()[None], st, seg_len, seg_group, torch.as_tensor(target).double(), True)[0, 0]
    return torch.sqrt(qg / torch.bincount(position_groups(seg_len, seg_group)).double())


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------

def segments_343():
    """Three synthetic segments of 3, 4 and 3 residues (4 randn), for groups A, B, A."""
    g = torch.Generator().manual_seed(77)
    return [4 * torch.randn(n, 3, generator=g) for n in (3, 4, 3)]


def random_rotation(g):
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def planted(segs, at=(5, 30), n_res=60, seed=61, mirror=None):
    """A walk [2, n_res, 3] with every segment of `segs` written into particle 0 at `at` under a proper rotation and a shift of its
    own (`mirror`: that segment's copy is reflected first, z negated)."""
    g = torch.Generator().manual_seed(seed)
    x = walk(2, n_res, seed + 1).double()
    for k, (seg, st) in enumerate(zip(segs, at)):
        m = seg.double() - seg.double().mean(dim=0, keepdim=True)
        r, shift = random_rotation(g), 10.0 * torch.randn(1, 3, generator=g, dtype=torch.float64)
        if mirror == k:
            m = m * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)
        x[0, st:st + len(seg)] = m @ r.T + shift
    return x.float()
