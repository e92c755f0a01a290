"""What the context potential's test files share (tests/test_context_host.py, test_context_gpu.py): two restatements of
genie_context_potential (include/genie_hip.h) in plain torch that never call the library -- `reference` in float64 on the CPU, the fit
through torch.linalg.eigh of Horn's matrix and the gradient from autograd (the oracle), and the same code in float32
(`restatement32`: the measure of what float32 arithmetic costs on an input, the timing reference of tools/context_potential_time.py
and the torch `twisting_function` of the end-to-end tests) -- the header's analytic gradient written out with loops, the margins of the
discontinuous report fields, and the inputs of the cases.

A configuration is a dict: clash_distance, clash_weight, contact_distance, contacts_min, contacts_max, contacts_weight (floats; a weight
of 0 switches the term off).  Anchors are `idx` [B, A] int64 (one row per particle), `t` [A, 3] their motif coordinates and `y` [C, 3]
the context, both in the motif file's frame."""
import math

import torch

REPORT = ('context_contacts', 'n_context_contacts', 'n_context_interface', 'context_min_distance', 'n_context_clash', 'anchor_rmsd',
          'e_context_clash', 'e_context_contact')
COUNTS = ('n_context_contacts', 'n_context_interface', 'n_context_clash')
CLASH_DISTANCE = 4.0
MIN_GAP = 0.1       # (lam_0 - lam_1) / lam_0 of every particle of a parity input: a well-conditioned fit

# (B, N, A, C, offset, seed): the parity shapes of test_context_gpu.py; the context is a walk placed `offset` Angstrom from particle
# 0's centroid, in particle 0's frame, before both it and the motif are moved to the file's frame.  Offsets and seeds are chosen by the
# oracle alone (`inputs` asserts the margins, the gap, that every term is active and that the anchors carry gradient).
CASES = [(3, 4, 3, 1, 0.0, 9), (3, 9, 4, 3, 4.0, 4), (3, 63, 7, 65, 10.0, 8), (3, 64, 9, 64, 10.0, 2), (3, 65, 12, 129, 15.0, 2),
         (2, 129, 21, 257, 15.0, 3)]
# 12 C = 66 000 bytes of staging: above the 65 536 a kernel gets without asking.  The centroid of a walk of 5500 atoms says little
# about where its atoms are, so this case's offset is that of the walk's middle atom, and it has its own clash distance (as the
# binder's LDS_CASE has).
LDS_CASE = (1, 12, 4, 5500, 6.0, 0)
LDS_CLASH_DISTANCE = 9.0


def case_id(case):
    return 'B%d-N%d-A%d-C%d' % tuple(case[:4])


def config(clash_distance=0.0, clash_weight=0.0, contact_distance=8.0, contacts_min=0.0, contacts_max=math.inf, contacts_weight=0.0):
    return dict(clash_distance=float(clash_distance), clash_weight=float(clash_weight), contact_distance=float(contact_distance),
                contacts_min=float(contacts_min), contacts_max=float(contacts_max), contacts_weight=float(contacts_weight))


def _norm(sq):
    """sqrt of a squared distance, with value 0 and gradient 0 where it is exactly 0 (the kernel's zero-distance rule)."""
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def horn_matrix(S):
    """Horn's symmetric 4x4 K of the correlation S [..., 3, 3] (S_ab = sum t_a c_b), as csrc/horn.h builds it."""
    xx, xy, xz = S[..., 0, 0], S[..., 0, 1], S[..., 0, 2]
    yx, yy, yz = S[..., 1, 0], S[..., 1, 1], S[..., 1, 2]
    zx, zy, zz = S[..., 2, 0], S[..., 2, 1], S[..., 2, 2]
    rows = [[xx + yy + zz, yz - zy, zx - xz, xy - yx], [yz - zy, xx - yy - zz, xy + yx, zx + xz],
            [zx - xz, xy + yx, -xx + yy - zz, yz + zy], [xy - yx, zx + xz, yz + zy, -xx - yy + zz]]
    return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)


def rotation(q):
    """R [..., 3, 3] of the unit quaternion q [..., 4] = (w, x, y, z), as mr_rotation writes it."""
    w, x, y, z = q.unbind(dim=-1)
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)


def fit(x, idx, t):
    """The superposition of the anchors t [A, 3] on x[b, idx[b]]: (R [B, 3, 3], abar [B, 3], tbar [3], lam [B, 4] ascending, V [B, 4, 4]),
    differentiable in x."""
    t = t.to(dtype=x.dtype, device=x.device)
    a = torch.gather(x, 1, idx.to(x.device)[:, :, None].expand(-1, -1, 3))
    abar, tbar = a.mean(dim=1), t.mean(dim=0)
    S = torch.einsum('ka,bkc->bac', t - tbar, a - abar[:, None])
    lam, V = torch.linalg.eigh(horn_matrix(S))
    return rotation(V[:, :, -1]), abar, tbar, lam, V


def place(R, abar, tbar, y):
    """y' [B, C, 3] = R (y - tbar) + abar."""
    return torch.einsum('bij,cj->bci', R, y - tbar) + abar[:, None]


def terms(x, idx, t, y, cfg):
    """Everything the entry reports of x [B, N, 3], in x's dtype and on its device, differentiable in x: the REPORT fields [B] each,
    'energy' = e_context_clash + e_context_contact, 'R' [B, 3, 3], 'trans' [B, 3] (y' = R y + trans), 'placed' [B, C, 3] and 'gap'
    [B] = (lam_0 - lam_1) / lam_0."""
    y, t = y.to(dtype=x.dtype, device=x.device), t.to(dtype=x.dtype, device=x.device)
    idx = idx.to(x.device)
    B, N = x.shape[:2]
    R, abar, tbar, lam, _ = fit(x, idx, t)
    yp = place(R, abar, tbar, y)
    pair = torch.ones(B, N, dtype=torch.bool, device=x.device).scatter_(1, idx, False)      # anchors sit out
    d2 = ((x[:, :, None, :] - yp[:, None]) ** 2).sum(dim=-1)
    d = _norm(d2)
    live = pair[:, :, None]
    s = torch.where(live, 1.0 / (1.0 + (d2 / cfg['contact_distance'] ** 2) ** 3), torch.zeros_like(d2))
    near = (d < cfg['contact_distance']) & live
    a = torch.gather(x, 1, idx[:, :, None].expand(-1, -1, 3))
    res = torch.einsum('bij,kj->bki', R, t - tbar) - (a - abar[:, None])
    out = {'context_contacts': s.sum(dim=(1, 2)), 'n_context_contacts': near.sum(dim=(1, 2)), 'n_context_interface': near.any(dim=2).sum(dim=1),
           'context_min_distance': torch.where(live, d, torch.full_like(d, math.inf)).amin(dim=(1, 2)),
           'n_context_clash': ((d < cfg['clash_distance']) & live).sum(dim=(1, 2)), 'anchor_rmsd': _norm((res ** 2).sum(dim=-1).mean(dim=1))}
    C = out['context_contacts']
    hinge = torch.where(live, torch.clamp(cfg['clash_distance'] - d, min=0), torch.zeros_like(d))
    out['e_context_clash'] = cfg['clash_weight'] * (hinge ** 2).sum(dim=(1, 2))
    upper = torch.clamp(C - cfg['contacts_max'], min=0) ** 2 if math.isfinite(cfg['contacts_max']) else torch.zeros_like(C)
    out['e_context_contact'] = cfg['contacts_weight'] * (torch.clamp(cfg['contacts_min'] - C, min=0) ** 2 + upper)
    out['energy'] = out['e_context_clash'] + out['e_context_contact']
    out.update(R=R, trans=abar - torch.einsum('bij,j->bi', R, tbar), placed=yp, gap=(lam[:, 3] - lam[:, 2]) / lam[:, 3])
    return out


def logp(x, idx, t, y, cfg, var):
    return -terms(x, idx, t, y, cfg)['energy'] / (2 * var)


def _evaluate(x, idx, t, y, cfg, var, grad=True):
    x = x.detach().clone().requires_grad_(grad)
    r = terms(x, idx, t, y, cfg)
    lp = -r['energy'] / (2 * var)
    out = {k: r[k].detach() for k in REPORT + ('R', 'trans', 'placed', 'gap')}
    out['logp'] = lp.detach()
    if grad:
        out['grad'], = torch.autograd.grad(lp.sum(), x)
    return out


def reference(x, idx, t, y, cfg, var, grad=True):
    """The float64 oracle on the CPU: 'logp' [B], 'grad' [B, N, 3] (autograd through eigh), the REPORT fields, 'R', 'trans', 'placed'."""
    return _evaluate(x.detach().double().cpu(), idx.cpu(), t.detach().double().cpu(), y.detach().double().cpu(), cfg, float(var), grad)


def restatement32(x, idx, t, y, cfg, var, grad=True):
    """The same code in float32, on x's device."""
    return _evaluate(x.detach().float(), idx, t.detach().float(), y.detach().float(), cfg, float(var), grad)


def twisting_function(idx, t, y, cfg, abar, tausq=1.0):
    """The float32 restatement as a TwistedSampler `twisting_function`, with ContextPotential's variance; idx [A]: one row for all."""
    from genie2_amd.smc import xstart_variance

    def twist(x0, step):
        rows = idx.to(x0.device).reshape(1, -1).expand(x0.shape[0], -1)
        return logp(x0.float(), rows, t, y, cfg, xstart_variance(abar[step], tausq).to(torch.float32))
    return twist


def analytic_gradient(x, idx, t, y, cfg, var, gap_floor=1e-6):
    """The gradient as include/genie_hip.h states it, written out with loops in float64 (small shapes only): the pair forces p_nc, their
    sum P and moment M, G_R = -M R, the adjoint of the fit through the three other eigenpairs, the anchors' shares."""
    x, t, y = x.detach().double(), t.detach().double(), y.detach().double()
    B, N, _ = x.shape
    A, Cn, cd, cl = t.shape[0], y.shape[0], cfg['contact_distance'], cfg['clash_distance']
    R, abar, tbar, lam, V = (v.detach() for v in fit(x, idx, t))
    yp = place(R, abar, tbar, y)
    g = torch.zeros_like(x)
    for b in range(B):
        anchors = idx[b].tolist()
        F, G = torch.zeros(N, 3, dtype=torch.float64), torch.zeros(N, 3, dtype=torch.float64)
        MF, MG = torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64)
        Cc = 0.0
        for n in range(N):
            if n in anchors:
                continue
            for c in range(Cn):
                v = x[b, n] - yp[b, c]
                w = yp[b, c] - abar[b]
                d = float(v.norm())
                r = d / cd
                s = 1.0 / (1.0 + r ** 6)
                Cc += s
                pg = r ** 4 * s ** 2 * v
                G[n] += pg
                MG += torch.outer(pg, w)
                if d > 0 and d < cl:
                    pf = (cl - d) * v / d
                    F[n] += pf
                    MF += torch.outer(pf, w)
        k = cfg['contacts_weight'] * (max(Cc - cfg['contacts_max'], 0.0) - max(cfg['contacts_min'] - Cc, 0.0))
        six_k = 6.0 / cd ** 2 * k
        direct = cfg['clash_weight'] * F + six_k * G
        P = direct.sum(dim=0)
        GR = -(cfg['clash_weight'] * MF + six_k * MG) @ R[b]
        # g_q = dR/dq : G_R, by the entries of mr_rotation
        q = V[b, :, 3]
        qw, qx, qy, qz = (float(v) for v in q)
        dR = torch.zeros(4, 3, 3, dtype=torch.float64)
        dR[0] = 2 * torch.tensor([[0, -qz, qy], [qz, 0, -qx], [-qy, qx, 0]], dtype=torch.float64)
        dR[1] = 2 * torch.tensor([[0, qy, qz], [qy, -2 * qx, -qw], [qz, qw, -2 * qx]], dtype=torch.float64)
        dR[2] = 2 * torch.tensor([[-2 * qy, qx, qw], [qx, 0, qz], [-qw, qz, -2 * qy]], dtype=torch.float64)
        dR[3] = 2 * torch.tensor([[-2 * qz, -qw, qx], [qw, -2 * qz, qy], [qx, qy, 0]], dtype=torch.float64)
        gq = (dR * GR[None]).sum(dim=(1, 2))
        gq = gq - (gq @ q) * q
        z = torch.zeros(4, dtype=torch.float64)
        for i in range(3):
            gap = float(lam[b, 3] - lam[b, i])
            if gap > gap_floor * float(lam[b, 3]):
                z += V[b, :, i] * float(V[b, :, i] @ gq) / gap
        Mk = torch.outer(z, q)
        Mk = Mk + Mk.T - torch.diag(torch.diag(Mk))                         # m_ij + m_ji off the diagonal
        D = torch.zeros(3, 3, dtype=torch.float64)
        D[0, 0] = Mk[0, 0] + Mk[1, 1] - Mk[2, 2] - Mk[3, 3]
        D[1, 1] = Mk[0, 0] - Mk[1, 1] + Mk[2, 2] - Mk[3, 3]
        D[2, 2] = Mk[0, 0] - Mk[1, 1] - Mk[2, 2] + Mk[3, 3]
        D[0, 1], D[1, 0] = Mk[1, 2] + Mk[0, 3], Mk[1, 2] - Mk[0, 3]
        D[1, 2], D[2, 1] = Mk[2, 3] + Mk[0, 1], Mk[2, 3] - Mk[0, 1]
        D[2, 0], D[0, 2] = Mk[1, 3] + Mk[0, 2], Mk[1, 3] - Mk[0, 2]
        g[b] = direct
        for k_, n in enumerate(anchors):
            g[b, n] = -P / A + D.T @ (t[k_] - tbar)
        g[b] /= var
    return g


def margins(x, idx, t, y, cfg):
    """How far the discontinuous report fields are from flipping, in Angstrom, in float64: the smallest |d - clash_distance| and
    |d - contact_distance| over all pairs (anchors excluded)."""
    x = x.detach().double().cpu()
    r = terms(x, idx.cpu(), t.double().cpu(), y.double().cpu(), cfg)
    pair = torch.ones(x.shape[:2], dtype=torch.bool).scatter_(1, idx.cpu(), False)
    d = ((x[:, :, None, :] - r['placed'][:, None]) ** 2).sum(dim=-1).sqrt()[pair]
    if d.numel() == 0:
        return math.inf
    return min(float((d - cfg['clash_distance']).abs().min()), float((d - cfg['contact_distance']).abs().min()))


def walk(N, seed, step=3.8):
    """One random walk of C-alpha spacing [N, 3], centred."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(N, 3, generator=g)
    w = torch.cumsum(step * v / v.norm(dim=-1, keepdim=True), dim=0)
    return w - w.mean(dim=0, keepdim=True)


def designs(B, N, seed=0):
    """B walks of seeds 100 N + k (+ 1000 seed), each centred: [B, N, 3] float32."""
    return torch.stack([walk(N, 100 * N + k + 1000 * seed) for k in range(B)])


def anchor_runs(N, A):
    """A anchor residues in three spread runs of A // 3 (+ 1 for the first A % 3): the first starts at residue 0, the last ends at
    residue N - 1 (so at N = 65 the anchors straddle the tile edge 63 / 64), the middle one sits half way: sorted, distinct."""
    out = []
    for i in range(3):
        n = A // 3 + (1 if i < A % 3 else 0)
        first = max((N - n) * i // 2, out[-1] + 1 if out else 0)
        out += list(range(first, first + n))
    assert len(set(out)) == A and out[-1] < N, (N, A, out)
    return out


def random_rotation(seed):
    """A proper rotation [3, 3] float64 from a seeded unit quaternion."""
    q = torch.randn(4, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return rotation(q / q.norm())


def full_config(x, idx, t, y, **kw):
    """Both terms on: clashes below CLASH_DISTANCE, and the contact count held between 1.5 and 3 times particle 0's own, so the lower
    hinge is active on particle 0."""
    C = float(terms(x[:1].double(), idx[:1], t.double(), y.double(), config())['context_contacts'][0])
    return config(**dict(dict(clash_distance=CLASH_DISTANCE, clash_weight=1.0, contacts_min=1.5 * C, contacts_max=3.0 * C, contacts_weight=1.0), **kw))


def only(cfg, term):
    """cfg with one term left on: 'clash' or 'contacts'."""
    out = dict(cfg)
    if term != 'clash':
        out['clash_weight'] = 0.0
    if term != 'contacts':
        out['contacts_weight'] = 0.0
    return out


def check_inputs(x, idx, t, y, cfg, anchors_matter=True):
    """The oracle's own conditions on an input: every discontinuous field at least 1e-4 A from flipping, every enabled term with
    positive energy on at least one particle, a well-conditioned fit on every particle, and, on some particle, an anchor whose
    largest gradient entry is at least 1e-2 of the largest overall.  Otherwise: take another seed."""
    m = margins(x, idx, t, y, cfg)
    assert m >= 1e-4, 'a pair of this input is %.1e A from a threshold: take another seed' % m
    ref = reference(x, idx, t, y, cfg, 1.0)
    for key, weight in (('e_context_clash', 'clash_weight'), ('e_context_contact', 'contacts_weight')):
        if cfg[weight] > 0:
            assert float(ref[key].max()) > 0, '%s is 0 on every particle of this input: take another seed' % key
    assert float(ref['gap'].min()) >= MIN_GAP, 'the fit of a particle has relative gap %.3f: take another seed' % float(ref['gap'].min())
    if anchors_matter:
        g = ref['grad'].abs().amax(dim=2)
        share = torch.gather(g, 1, idx).amax(dim=1) / g.amax(dim=1).clamp(min=1e-300)
        assert float(share.max()) >= 1e-2, 'no anchor carries 1e-2 of the largest gradient entry (%.1e): take another seed' % float(share.max())
    return m


def inputs(case):
    """(x [B, N, 3], idx [B, A] int64, t [A, 3], y [C, 3], cfg) of a case, both terms on, checked.  The anchors are the same three
    spread runs in every particle; the motif is particle 0's anchors plus 0.5 A of noise and the context a walk `offset` A from
    particle 0's centroid along x, both then rotated and shifted into a frame of their own."""
    B, N, A, C, offset, seed = case
    x = designs(B, N, seed)
    idx = torch.tensor(anchor_runs(N, A), dtype=torch.int64)[None].expand(B, -1).contiguous()
    g = torch.Generator().manual_seed(9000 + 10 * N + seed)
    t0 = x[0, idx[0]].double() + 0.5 * torch.randn(A, 3, generator=g, dtype=torch.float64)
    y0 = walk(C, 7000 + C + seed).double()
    y0 = y0 - (y0[C // 2] if case == LDS_CASE else 0.0) + torch.tensor([float(offset), 0.0, 0.0], dtype=torch.float64)
    Q, shift = random_rotation(500 + N + seed), torch.tensor([11.0, -7.0, 5.0], dtype=torch.float64)
    t, y = (t0 @ Q.T + shift).float(), (y0 @ Q.T + shift).float()
    cfg = full_config(x, idx, t, y, **(dict(clash_distance=LDS_CLASH_DISTANCE) if case == LDS_CASE else {}))
    check_inputs(x, idx, t, y, cfg)
    return x, idx, t, y, cfg


def potential(cfg, n_res, idx, t, y, abar, **kw):
    """The ContextPotential of a configuration in the fixed mode (every term always given: a weight of 0 is how cfg switches a term
    off); idx [A] or [B, A]."""
    from genie2_amd.smc import ContextPotential
    return ContextPotential(n_res, abar, t, y, anchor_index=idx, clash_distance=cfg['clash_distance'], clash_weight=cfg['clash_weight'],
                            contact_distance=cfg['contact_distance'], contacts=(cfg['contacts_min'], cfg['contacts_max']),
                            contacts_weight=cfg['contacts_weight'], device='cuda', **kw)


def write_context_pdb(path, xyz, chain_lengths, names=None):
    """A context file for the end-to-end tests: C-alpha ATOM records of glycines, chains lettered `names` (default H, L, ...) of the
    given lengths, numbered from 1 in every chain, coordinates rounded to the format's 1e-3 A."""
    names = names or 'HLMN'
    with open(path, 'w') as fh:
        k = 0
        for letter, n in zip(names, chain_lengths):
            for i in range(n):
                fh.write('ATOM  %5d  CA  GLY %s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n' % ((k + 1, letter, i + 1) + tuple(float(v) for v in xyz[k])))
                k += 1
        fh.write('END\n')
