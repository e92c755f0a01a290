"""What the aligned fold potential's test files share (tests/test_fold_align_host.py, test_fold_align_gpu.py,
tools/fold_align_time.py): the definition of genie_fold_align_potential (include/genie_hip.h) restated in plain torch, independently of
the library -- the search of genie_tm_align written again with the offset stride (tests/_tmalign.py's `align` cannot take one; its
ascent, table and traceback are used), the polish over the aligned pairs from the weights g(T*)^2 with the LAST iteration kept, the
hinges, the report and the gradient with every pair's alignment and fit held fixed -- which runs in float64 as the oracle and in
float32 as the restatement a user would write; an autograd form that serves as a torch `twisting_function`; the inputs and the case
list.  Nothing here calls the library."""
import math

import torch

import _similarity as S
from _fold import AVOID, BAND, COUNTS, GAP, MARGIN, REPORT, TEMPLATE  # noqa: F401
from _motif import walk
from _tmalign import ILL, NORMS, fill, fit_trace, indel, traceback  # noqa: F401

# (B, N, reference lengths): the certificate's shapes (test_fold_align_gpu.py); MANY is 300 references of 36..44 residues
MANY = tuple(36 + (r * 5) % 9 for r in range(300))
CASES = [(3, 4, (4, 5)), (3, 5, (4, 8)), (3, 24, (16, 17, 24, 31)), (3, 48, (32, 33, 48, 64)), (3, 65, (63, 64, 65, 80)),
         (2, 129, (120, 129, 140)), (2, 257, (256, 257, 300)), (1, 362, (362,)), (1, 128, (1024,)), (1, 1024, (128,)), (8, 40, MANY)]
# the seed offset of a case whose first choice the oracle turned down (check_inputs, a particle left out), found on the CPU
BASE = {}


def case_id(case):
    B, N, lengths = case
    return 'B%d-N%d-R%d' % (B, N, len(lengths))


def lnorm_of(norm, Lq, Lr):
    return {'query': Lq, 'reference': Lr, 'shorter': min(Lq, Lr), 'longer': max(Lq, Lr)}[norm]


def offsets_of(n_off, stride):
    """The offsets stage 0 visits: 0, s, 2 s, ... and always the last one, ascending."""
    return sorted(set(range(0, n_off, stride)) | {n_off - 1})


# ---- the search ----------------------------------------------------------------------------------------------------------------------

def stage0(a, b, lnorm, d0, n_iter, stride):
    """The seeded gapless search of a [La, 3] along b [Lb, 3] over the visited offsets, with the winning fit kept: 'value', 'offset',
    'R', 'cp', 'cq', 'gap', 'margin' (the best visited offset's lead over the second best); ties to the lowest offset, then the lowest
    seed, then the earliest iteration."""
    La, Lb = a.shape[0], b.shape[0]
    visited = offsets_of(Lb - La + 1, stride)
    Q = b.unfold(0, La, 1).transpose(1, 2)[visited]                    # [visited, La, 3]
    n_vis = len(visited)
    W = torch.zeros(S.SEEDS, La, dtype=a.dtype)
    for s, (start, length) in enumerate(S.windows(La)):
        W[s, start:start + length] = 1
    M = n_vis * S.SEEDS
    score, R, cp, cq, gap = fit_trace(a[None].expand(M, La, 3), Q[:, None].expand(n_vis, S.SEEDS, La, 3).reshape(M, La, 3),
                                      W[None].expand(n_vis, S.SEEDS, La).reshape(M, La), lnorm, d0, n_iter)
    flat = score.reshape(-1)                                            # (offset, seed, iteration) order
    k = int((flat == flat.max()).nonzero()[0])
    item, it = divmod(k, n_iter)
    top = torch.sort(score.reshape(n_vis, -1).amax(dim=1), descending=True).values
    return {'value': flat[k], 'offset': visited[item // S.SEEDS], 'R': R[item, it], 'cp': cp[item, it], 'cq': cq[item, it],
            'gap': float(gap.min()), 'margin': float(top[0] - top[1]) if n_vis > 1 else math.inf}


def search(q, r, norm='query', n_iter=16, n_rounds=8, gap_open=-0.6, stride=1, dtype=torch.float64):
    """Step 1 of the statement for one pair, query q [Lq, 3] against reference r [Lr, 3]: {'tm' (the search's value), 'n_aligned',
    'map' (a list of Lq entries), 'rot0' [3, 3], 'trans0' [3] (rot0 x_query + trans0 ~ x_reference), and the figures of
    well-posedness 'gap', 'margin', 'path_margin', 'stage_lead' that tests/_tmalign.py's `well_posed` reads}."""
    q, r = q.to(dtype), r.to(dtype)
    Lq, Lr = q.shape[0], r.shape[0]
    swap = Lr < Lq                                                      # a = the shorter chain; equal lengths: the query
    a, b = (r, q) if swap else (q, r)
    ca, cb = a.mean(0), b.mean(0)
    a, b = a - ca, b - cb
    La, Lb = a.shape[0], b.shape[0]
    lnorm = lnorm_of(norm, Lq, Lr)
    d0 = S.d0(lnorm)
    s0 = stage0(a, b, lnorm, d0, n_iter, stride)
    o = s0['offset']
    stages = [{'value': s0['value'], 'R': s0['R'], 'cp': s0['cp'], 'cq': s0['cq'], 'ia': list(range(La)), 'ib': list(range(o, o + La))}]
    gap, path_margin = s0['gap'], math.inf
    for _ in range(n_rounds):
        prev = stages[-1]
        Ta = (a - prev['cp']) @ prev['R'].T + prev['cq']
        move, lead = fill(1 / (1 + ((Ta[:, None] - b[None]) ** 2).sum(-1) / d0 ** 2), gap_open)
        ia, ib, margin = traceback(move, lead, La, Lb)
        path_margin = min(path_margin, margin)
        if (ia, ib) == (prev['ia'], prev['ib']) or len(ia) < 3:
            break
        score, R, cp, cq, g = fit_trace(a[ia][None], b[ib][None], torch.ones(1, len(ia), dtype=dtype), lnorm, d0, n_iter)
        gap = min(gap, float(g.min()))
        it = int((score[0] == score[0].max()).nonzero()[0])
        stages.append({'value': score[0, it], 'R': R[0, it], 'cp': cp[0, it], 'cq': cq[0, it], 'ia': ia, 'ib': ib})
    values = torch.stack([s['value'] for s in stages])
    best = stages[int((values == values.max()).nonzero()[0])]
    others = [float(s['value']) for s in stages if (s['ia'], s['ib']) != (best['ia'], best['ib'])]
    R = best['R']
    t = cb + best['cq'] - R @ (ca + best['cp'])                         # b ~ R a + t in the callers' frame
    amap = [-1] * Lq
    for i, j in zip(best['ia'], best['ib']):
        amap[j if swap else i] = i if swap else j
    rot0, trans0 = (R.T, -(R.T @ t)) if swap else (R, t)
    return {'tm': best['value'], 'n_aligned': len(best['ia']), 'map': amap, 'rot0': rot0, 'trans0': trans0, 'gap': gap,
            'margin': s0['margin'], 'path_margin': path_margin, 'stage_lead': float(best['value']) - max(others) if others else math.inf}


def search_all(x, refs, dtype=torch.float64, **kw):
    """`search` of every particle of x [B, N, 3] against every reference of the list `refs`: 'map' [B, R, N] int64, 'n_aligned' [B, R]
    int64, 'rot0' [B, R, 3, 3], 'trans0' [B, R, 3], 'tm' [B, R] in `dtype`, and 'gap', 'margin', 'path_margin', 'stage_lead' [B, R]
    float64."""
    B, N, R = x.shape[0], x.shape[1], len(refs)
    out = {'map': torch.full((B, R, N), -1, dtype=torch.int64), 'n_aligned': torch.zeros(B, R, dtype=torch.int64),
           'rot0': torch.zeros(B, R, 3, 3, dtype=dtype), 'trans0': torch.zeros(B, R, 3, dtype=dtype), 'tm': torch.zeros(B, R, dtype=dtype)}
    for k in ('gap', 'margin', 'path_margin', 'stage_lead'):
        out[k] = torch.zeros(B, R, dtype=torch.float64)
    for b in range(B):
        for r in range(R):
            one = search(x[b], refs[r], dtype=dtype, **kw)
            for k in out:
                out[k][b, r] = torch.tensor(one[k]) if k == 'map' else one[k]
    return out


# ---- the polish, the energy, the gradient --------------------------------------------------------------------------------------------

def polish_all(P, Q, mask, rot0, off0, lnorm, n_iter):
    """Step 2 for M pairs at once: P [M, N, 3] (every query residue, about the query's centroid), Q [M, N, 3] (its matched reference
    residue about the reference's centroid; anything where `mask` [M, N] is False), T0 x = rot0 x + off0 in these centred frames,
    lnorm [M].  n_iter weighted Horn steps over the masked pairs from the weights g(T0)^2, the last iteration kept -- tests/_tmalign.py's
    `fit_trace` with a mask, so that pairs of different counts share a batch.  Returns (n [M] the sum of g, dn [M, N, 3] = d n / d x_i
    with the fit held fixed (0 where unaligned), R [M, 3, 3], cp, cq [M, 3] with T x = R (x - cp) + cq, gap [M]: the smallest relative
    gap between the two largest Horn eigenvalues)."""
    m = mask.to(P.dtype)
    d0sq = torch.tensor([S.d0(int(L)) ** 2 for L in lnorm.tolist()], dtype=P.dtype)[:, None]
    e = P @ rot0.transpose(-1, -2) + off0[:, None] - Q
    t = m / (1 + (e ** 2).sum(-1) / d0sq)
    gap = None
    for _ in range(n_iter):
        W = t * t
        sw = W.sum(-1, keepdim=True)
        cp, cq = (W[:, None] @ P)[:, 0] / sw, (W[:, None] @ Q)[:, 0] / sw
        Pc, Qc = P - cp[:, None], Q - cq[:, None]
        ev, vec = torch.linalg.eigh(S.horn_matrix(torch.einsum('bl,bli,blj->bij', W, Pc, Qc)))
        g = (ev[..., 3] - ev[..., 2]) / ev.abs().amax(dim=-1).clamp(min=1e-30)
        gap = g if gap is None else torch.minimum(gap, g)
        R = S.quaternion_rotation(vec[..., :, 3])
        e = Pc @ R.transpose(-1, -2) - Qc
        t = m / (1 + (e ** 2).sum(-1) / d0sq)
    return t.sum(-1), -(2 / d0sq)[..., None] * (t * t)[..., None] * (e @ R), R, cp, cq, gap


def polish(xq, y, amap, rot0, trans0, lnorm, n_iter, dtype=torch.float64):
    """Step 2 for one pair: the aligned pairs of `amap` (per query residue the reference residue or -1) refitted from the weights
    g(T0)^2 (rot0 x_query + trans0 ~ x_reference), each chain taken about its own centroid as the kernel does.  Returns {'n' (sum of g),
    'dn' [Lq, 3], 'rot' [3, 3], 'trans' [3] (rot x_query + trans ~ x_reference), 'gap'}."""
    xq, y, rot0, trans0 = xq.to(dtype), y.to(dtype), rot0.to(dtype), trans0.to(dtype)
    amap = torch.as_tensor(amap).long()
    cx, cy = xq.mean(0), y.mean(0)
    n, dn, R, cp, cq, gap = polish_all((xq - cx)[None], (y[amap.clamp(min=0)] - cy)[None], (amap >= 0)[None], rot0[None],
                                       (rot0 @ cx + trans0 - cy)[None], torch.tensor([lnorm]), n_iter)
    return {'n': n[0], 'dn': dn[0], 'rot': R[0], 'trans': cy + cq[0] - R[0] @ (cx + cp[0]), 'gap': float(gap[0])}


def hinges(n, lnorm, bounds, upper=True):
    """(below, above) [B, R] of the soft counts n [B, R] under bounds [R, 3] and the normalising lengths lnorm [R]; `upper=False` leaves
    the upper hinge out altogether (what hi = inf must equal)."""
    lo, hi = bounds[:, 0].to(n), bounds[:, 1].to(n)
    lnorm = lnorm.to(n)
    below = torch.clamp(lnorm * lo - n, min=0)
    if not upper:
        return below, torch.zeros_like(n)
    finite = torch.isfinite(hi)
    above = torch.where(finite, torch.clamp(n - lnorm * torch.where(finite, hi, torch.zeros_like(hi)), min=0), torch.zeros_like(n))
    return below, above


def evaluate(x, refs, bounds, var, amap, rot0, trans0, norm='query', n_iter=16, dtype=torch.float64, upper=True):
    """Steps 2 to 5 on x [B, N, 3], the list `refs` and bounds [R, 3] from a given search result (amap [B, R, N], rot0 [B, R, 3, 3],
    trans0 [B, R, 3]: the oracle's own, or the kernel's for the certificate), in `dtype` on the CPU: 'logp' [B], 'grad' [B, N, 3],
    'tm', 'n', 'below', 'above', 'k', 'gap' [B, R], 'lnorm' [R], 'rot' [B, R, 3, 3], 'trans' [B, R, 3] and the REPORT fields [B]."""
    x = x.detach().to(dtype).cpu()
    bounds = torch.as_tensor(bounds, dtype=torch.float64)
    B, N, R = x.shape[0], x.shape[1], len(refs)
    lnorm = torch.tensor([lnorm_of(norm, N, len(y)) for y in refs], dtype=torch.float64)
    amap, rot0, trans0 = amap.cpu().long(), rot0.cpu().to(dtype), trans0.cpu().to(dtype)
    cx = x.mean(dim=1)                                                  # [B, 3]
    ys = [y.to(dtype).cpu() for y in refs]
    cy = torch.stack([y.mean(0) for y in ys])                           # [R, 3]
    P = (x - cx[:, None])[:, None].expand(B, R, N, 3).reshape(B * R, N, 3)
    Q = torch.stack([torch.stack([ys[r][amap[b, r].clamp(min=0)] - cy[r] for r in range(R)]) for b in range(B)]).reshape(B * R, N, 3)
    off0 = (torch.einsum('brij,bj->bri', rot0, cx) + trans0 - cy[None]).reshape(B * R, 3)
    n, dn, rot, cp, cq, gap = polish_all(P, Q, (amap >= 0).reshape(B * R, N), rot0.reshape(B * R, 3, 3), off0,
                                         lnorm[None].expand(B, R).reshape(-1), n_iter)
    trans = (cy[None] + cq.reshape(B, R, 3)) - torch.einsum('brij,brj->bri', rot.reshape(B, R, 3, 3), cx[:, None] + cp.reshape(B, R, 3))
    n, dn, rot, gap = n.reshape(B, R), dn.reshape(B, R, N, 3), rot.reshape(B, R, 3, 3), gap.reshape(B, R).double()
    below, above = hinges(n, lnorm, bounds, upper)
    w = bounds[:, 2].to(dtype)
    energy = (w * (below ** 2 + above ** 2)).sum(dim=1)
    k = w * (above - below)
    tm = n / lnorm.to(dtype)
    wanted = bounds[:, 0] > 0
    return {'logp': -energy / (2 * var), 'grad': -(k[:, :, None, None] * dn).sum(dim=1) / var, 'tm': tm, 'n': n, 'below': below,
            'above': above, 'k': k, 'gap': gap, 'lnorm': lnorm, 'rot': rot, 'trans': trans, 'tm_nearest': tm.amax(dim=1),
            'nearest': tm.argmax(dim=1),
            'tm_lowest_wanted': tm[:, wanted].amin(dim=1) if bool(wanted.any()) else torch.zeros(B, dtype=dtype),
            'n_fold_violations': ((below > 0) | (above > 0)).sum(dim=1), 'e_fold': energy}


def reference(x, refs, bounds, var, norm='query', n_iter=16, n_rounds=8, gap_open=-0.6, stride=1, dtype=torch.float64, upper=True):
    """The whole definition: `search_all`, then `evaluate` on its result; the search's outputs are kept under 'search'."""
    found = search_all(x.detach().cpu(), refs, dtype=dtype, norm=norm, n_iter=n_iter, n_rounds=n_rounds, gap_open=gap_open, stride=stride)
    out = evaluate(x, refs, bounds, float(var), found['map'], found['rot0'], found['trans0'], norm, n_iter, dtype, upper)
    out['search'] = found
    return out


def left_out(ref):
    """[B] bool: the particles left out of the certificate -- a Horn gap of the polish below GAP on a pair with an active hinge."""
    return ((ref['gap'] < GAP) & ((ref['below'] > 0) | (ref['above'] > 0))).any(dim=1)


def logp(x, refs, bounds, var, norm='query', n_iter=16, n_rounds=8, gap_open=-0.6, stride=1):
    """log p [B] in x's dtype, differentiable in x by autograd: the alignments and the polished fits come from a search that is not
    recorded, and the soft counts are formed again under them, so the derivative is the definition's (alignment and fit held fixed)."""
    bounds = torch.as_tensor(bounds).to(x)
    B, N, R = x.shape[0], x.shape[1], len(refs)
    with torch.no_grad():
        held = reference(x.detach().cpu(), refs, bounds.cpu(), 1.0, norm, n_iter, n_rounds, gap_open, stride, x.dtype)
    rows = []
    for b in range(B):
        row = []
        for r in range(R):
            amap = held['search']['map'][b, r]
            i = (amap >= 0).nonzero()[:, 0].to(x.device)
            y = refs[r].to(x)[amap[i.cpu()].to(x.device)]
            e = x[b, i] @ held['rot'][b, r].to(x).T + held['trans'][b, r].to(x) - y
            row.append((1 / (1 + (e ** 2).sum(-1) / S.d0(int(held['lnorm'][r])) ** 2)).sum())
        rows.append(torch.stack(row))
    n = torch.stack(rows)
    below, above = hinges(n, held['lnorm'].to(x.device), bounds)
    return -(bounds[:, 2] * (below ** 2 + above ** 2)).sum(dim=1) / (2 * var)


def twisting_function(refs, bounds, abar, tausq=1.0, **kw):
    """The float32 restatement as a TwistedSampler `twisting_function`, with AlignedFoldPotential's variance."""
    from genie2_amd.smc import xstart_variance

    def twist(x0, step):
        return logp(x0.float(), refs, bounds, xstart_variance(abar[step], tausq).to(torch.float32), **kw)
    return twist


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def relative(x, L, seed, noise):
    """A moved, noised relative of x [N, 3] with L residues: an indel relative where both lengths allow one (a cut from N / 2 on and an
    excursion spliced in at N / 4, in the manner of tests/_tmalign.py's families), else x cut short or extended by a walk."""
    N = x.shape[0]
    if N >= 16 and L >= 12:
        n_ins = 3 + seed % 3
        n_cut = N + n_ins - L
        if 0 < n_cut <= N - N // 2 - 1:
            return S.moved(indel(x, N // 2, n_cut, N // 4, n_ins, seed), seed, noise)
        if n_cut <= 0:                                                  # the reference is longer: the excursion takes the difference
            return S.moved(indel(x, N // 2, 2, N // 4, L - N + 2, seed), seed, noise)
    if L <= N:
        o = (N - L) // 2
        return S.moved(x[o:o + L], seed, noise)
    tail = walk(1, L - N + 1, seed)[0]
    return S.moved(torch.cat([x, x[-1] + tail[1:] - tail[0]]), seed, noise)


def particles(B, N, base=0):
    """B centred 3.8 A walks of seeds 100 N + base + k: [B, N, 3] float32."""
    out = [walk(1, N, 100 * N + base + k)[0] for k in range(B)]
    return torch.stack([w - w.mean(dim=0, keepdim=True) for w in out])


def references(x, lengths, base=0):
    """One reference per entry of `lengths` for the particles x [B, N, 3]: reference r is a relative of particle r mod B with
    S.NOISE[r mod 6] Angstrom of noise (scaled by d0(N) / d0(65) below 65 residues: short chains have a small d0), except every third one
    (r mod 3 == 2), an unrelated walk: a list of [L_r, 3] float32."""
    B, N = x.shape[0], x.shape[1]
    scale = min(1.0, S.d0(N) / S.d0(65))
    out = []
    for r, L in enumerate(lengths):
        seed = 100 * N + base + 1000 + r
        out.append(walk(1, L, seed)[0] + torch.tensor([3.0, -2.0, 1.0]) if r % 3 == 2 else relative(x[r % B], L, seed, scale * S.NOISE[r % len(S.NOISE)]))
    return out


def bounds_of(R, weight=1.0):
    """[R, 3] float64 rows (lo, hi, weight): TEMPLATE for reference 0, AVOID for the others; a single reference gets BAND."""
    return torch.tensor([list(BAND if R == 1 else TEMPLATE if r == 0 else AVOID) + [weight] for r in range(R)], dtype=torch.float64)


def inputs(case):
    """(x [B, N, 3], refs: a list of [L_r, 3], bounds [R, 3]) of a case.  The two limit cases with one long chain take tests/_tmalign.py's
    limit pair, so that the search has something to find."""
    from _tmalign import limit_pairs
    B, N, lengths = case
    base = BASE.get((B, N, len(lengths)), 0)
    if (N, lengths) == (128, (1024,)):
        q, r = limit_pairs()[1]
        return (q - q.mean(0))[None], [r], bounds_of(1)
    if (N, lengths) == (1024, (128,)):
        r, q = limit_pairs()[1]
        return (q - q.mean(0))[None], [r], bounds_of(1)
    if (N, lengths) == (362, (362,)):
        q, r = limit_pairs()[0]
        return (q - q.mean(0))[None], [r], bounds_of(1)
    x = particles(B, N, base)
    return x, references(x, lengths, base), bounds_of(len(lengths))


def check_inputs(ref, R):
    """The oracle's own conditions on a case: a lower and an upper hinge are active (one reference: one of the two), and no n_r lies
    within MARGIN Lnorm of an active bound (lo > 0, hi finite).  Otherwise: take other seeds."""
    bounds = bounds_of(R)
    lo, hi = ref['lnorm'] * bounds[:, 0], ref['lnorm'] * bounds[:, 1]
    n = ref['n'].double()
    d_lo = torch.where(lo > 0, (n - lo).abs(), torch.full_like(n, math.inf))
    d_hi = torch.where(torch.isfinite(hi), (n - torch.where(torch.isfinite(hi), hi, torch.zeros_like(hi))).abs(), torch.full_like(n, math.inf))
    m = float((torch.minimum(d_lo, d_hi) / ref['lnorm']).min())
    assert m >= MARGIN, 'an n_r of this input is %.1e Lnorm from a bound: take other seeds' % m
    lower, upper = bool((ref['below'] > 0).any()), bool((ref['above'] > 0).any())
    assert (lower and upper) if R >= 2 else (lower or upper), 'this input lacks an active hinge (lower %s, upper %s)' % (lower, upper)
