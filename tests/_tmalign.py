"""What the gapped TM alignment's tests share (tests/test_tmalign_host.py, test_tmalign_gpu.py, tools/tmalign_time.py): the score of
include/genie_hip.h (genie_tm_align) written out independently of the package as a torch oracle -- `eigh` on Horn's 4x4 matrix, the
offsets and seeds of stage 0 side by side in one batch, the table filled one anti-diagonal at a time with the scores of the whole table
formed first, a traceback in Python -- which runs in float64 as the oracle and in float32 as the restatement a user would write; the
four figures by which the oracle alone calls a pair ill-posed; the inputs and the case list.  Nothing here calls the library."""
import math

import torch

import _similarity as S
from _motif import walk

NORMS = ('query', 'reference', 'shorter', 'longer')
MAX_CELLS = 131072
INDEL_N = (24, 48, 65, 129)
TINY_N = (4, 5, 8)
NOISE = (0.2, 0.5, 1.0, 1.5, 2.0, 3.0)
ILL = 1e-4              # a pair whose gap, offset margin, path margin or stage lead is below this is ill-posed
FAMILY_BASE = {}        # per-N seed offsets of the families, changed (never a threshold) until every case is inside the cap


# ---- the ascent ----------------------------------------------------------------------------------------------------------------------

def fit_trace(P, Q, W0, lnorm, d0, n_iter):
    """B ascents at once over the pairs P[b, n] <-> Q[b, n] ([B, L, 3]) from the weights W0 [B, L]; every residue counts in the score.
    Returns (score [B, n_iter], R [B, n_iter, 3, 3], cp, cq [B, n_iter, 3]: the fit T x = R (x - cp) + cq of every iteration, gap [B]: the
    smallest relative gap between the two largest Horn eigenvalues)."""
    W, score, Rs, cps, cqs, gap = W0, [], [], [], [], None
    for _ in range(n_iter):
        sw = W.sum(-1, keepdim=True)
        cp = (W[:, None] @ P)[:, 0] / sw
        cq = (W[:, None] @ Q)[:, 0] / sw
        Pc, Qc = P - cp[:, None], Q - cq[:, None]
        ev, vec = torch.linalg.eigh(S.horn_matrix(torch.einsum('bl,bli,blj->bij', W, Pc, Qc)))
        g = (ev[..., 3] - ev[..., 2]) / ev.abs().amax(dim=-1).clamp(min=1e-30)
        gap = g if gap is None else torch.minimum(gap, g)
        R = S.quaternion_rotation(vec[..., :, 3])
        t = 1 / (1 + ((Pc @ R.transpose(-1, -2) - Qc) ** 2).sum(-1) / d0 ** 2)
        score.append(t.sum(-1) / lnorm)
        Rs.append(R)
        cps.append(cp)
        cqs.append(cq)
        W = t * t
    return torch.stack(score, 1), torch.stack(Rs, 1), torch.stack(cps, 1), torch.stack(cqs, 1), gap


def stage0(a, b, lnorm, d0, n_iter):
    """7.8's search of a [La, 3] along b [Lb, 3] with the winning fit kept: {'value', 'offset', 'R', 'cp', 'cq', 'gap', 'margin',
    'by_offset'}; ties to the lowest offset, then the lowest seed, then the earliest iteration."""
    La, Lb = a.shape[0], b.shape[0]
    Q = b.unfold(0, La, 1).transpose(1, 2)                             # [offsets, La, 3]
    n_off = Q.shape[0]
    W = torch.zeros(S.SEEDS, La, dtype=a.dtype, device=a.device)
    for s, (start, length) in enumerate(S.windows(La)):
        W[s, start:start + length] = 1
    B = n_off * S.SEEDS
    P = a[None].expand(B, La, 3)
    score, R, cp, cq, gap = fit_trace(P, Q[:, None].expand(n_off, S.SEEDS, La, 3).reshape(B, La, 3), W[None].expand(n_off, S.SEEDS, La).reshape(B, La),
                                      lnorm, d0, n_iter)
    flat = score.reshape(-1)                                            # (offset, seed, iteration) order
    k = int((flat == flat.max()).nonzero()[0])
    item, it = divmod(k, n_iter)
    by_offset = score.reshape(n_off, -1).amax(dim=1)
    top = torch.sort(by_offset, descending=True).values
    return {'value': flat[k], 'offset': item // S.SEEDS, 'R': R[item, it], 'cp': cp[item, it], 'cq': cq[item, it], 'gap': float(gap.min()),
            'margin': float(top[0] - top[1]) if n_off > 1 else math.inf, 'by_offset': by_offset}


# ---- the table -----------------------------------------------------------------------------------------------------------------------

def fill(Sc, gap_open):
    """The table of the statement over the scores Sc [La, Lb], one anti-diagonal at a time.  Returns (move, lead): [La + Lb + 1, La + 1]
    indexed [i + j, i]; move 0 diag, 1 up (i - 1), 2 left (j - 1); lead = the chosen move's lead over the moves not chosen."""
    La, Lb = Sc.shape
    flipped = Sc.flip(1)
    kw = dict(dtype=Sc.dtype, device=Sc.device)
    move = torch.zeros(La + Lb + 1, La + 1, dtype=torch.int8, device=Sc.device)
    lead = torch.full((La + Lb + 1, La + 1), math.inf, **kw)
    v1, v2 = torch.zeros(La + 1, **kw), torch.zeros(La + 1, **kw)     # val on diagonals d - 1, d - 2, by row; 0 on the borders
    p1 = torch.zeros(La + 1, dtype=torch.bool, device=Sc.device)
    g, z = torch.tensor(gap_open, **kw), torch.zeros((), **kw)
    for d in range(2, La + Lb + 1):
        lo, hi = max(1, d - Lb), min(La, d - 1)                         # rows i of the cells (i, d - i) inside the table
        D = v2[lo - 1:hi] + flipped.diagonal(Lb + 1 - d)                # S[i - 1, d - i - 1] for i = lo..hi
        H = v1[lo - 1:hi] + torch.where(p1[lo - 1:hi], g, z)
        V = v1[lo:hi + 1] + torch.where(p1[lo:hi + 1], g, z)
        hv = torch.maximum(H, V)
        diag = (D >= H) & (D >= V)
        v0 = torch.zeros(La + 1, **kw)
        p0 = torch.zeros(La + 1, dtype=torch.bool, device=Sc.device)
        v0[lo:hi + 1] = torch.where(diag, D, hv)
        p0[lo:hi + 1] = diag
        move[d, lo:hi + 1] = torch.where(diag, 0, torch.where(V >= H, 2, 1)).to(torch.int8)
        lead[d, lo:hi + 1] = torch.where(diag, D - hv, torch.minimum(hv - D, (H - V).abs()))
        v2, v1, p1 = v1, v0, p0
    return move, lead


def traceback(move, lead, La, Lb):
    """From (La, Lb) along the moves until a border: (ia, ib: the aligned residues, 0-based and ascending, as lists; the smallest lead
    on the way)."""
    move, lead = move.cpu().tolist(), lead.cpu().tolist()
    i, j, ia, ib, margin = La, Lb, [], [], math.inf
    while i > 0 and j > 0:
        m = move[i + j][i]
        margin = min(margin, lead[i + j][i])
        if m == 0:
            ia.append(i - 1)
            ib.append(j - 1)
            i, j = i - 1, j - 1
        elif m == 1:
            i -= 1
        else:
            j -= 1
    return ia[::-1], ib[::-1], margin


def plain_monotone(Sc):
    """The largest sum of scores over monotone alignments of Sc [La, Lb] by the plain row recursion (no gap penalty): a float."""
    La, Lb = Sc.shape
    rows = Sc.tolist()
    prev = [0.0] * (Lb + 1)
    for i in range(1, La + 1):
        cur = [0.0] * (Lb + 1)
        for j in range(1, Lb + 1):
            cur[j] = max(prev[j - 1] + rows[i - 1][j - 1], prev[j], cur[j - 1])
        prev = cur
    return prev[Lb]


def table_value(Sc, gap_open):
    """val(La, Lb) of the statement's table, by a plain double loop: a float (the host tests compare it with plain_monotone)."""
    La, Lb = Sc.shape
    rows = Sc.tolist()
    val = [[0.0] * (Lb + 1) for _ in range(La + 1)]
    path = [[False] * (Lb + 1) for _ in range(La + 1)]
    for i in range(1, La + 1):
        for j in range(1, Lb + 1):
            D = val[i - 1][j - 1] + rows[i - 1][j - 1]
            H = val[i - 1][j] + (gap_open if path[i - 1][j] else 0.0)
            V = val[i][j - 1] + (gap_open if path[i][j - 1] else 0.0)
            path[i][j] = D >= H and D >= V
            val[i][j] = D if path[i][j] else max(H, V)
    return val[La][Lb]


# ---- one pair ------------------------------------------------------------------------------------------------------------------------

def align(q, r, norm='query', n_iter=16, n_rounds=8, gap_open=-0.6, dtype=torch.float64):
    """One pair, query q [Lq, 3] against reference r [Lr, 3]: {'tm', 'rmsd' (tensors in `dtype`), 'n_aligned', 'rounds', 'map' (a list of
    Lq entries), 'rot' [3, 3], 'trans' [3] (rot x_query + trans ~ x_reference), 'stage0' (its value), 'stages' (the value of every fitted
    stage, stage 0 first), 'best' (the winning stage's index in it), and the figures of well-posedness 'gap', 'margin', 'path_margin',
    'stage_lead'}."""
    q, r = q.to(dtype), r.to(dtype)
    Lq, Lr = q.shape[0], r.shape[0]
    swap = Lr < Lq                                                      # a = the shorter chain; equal lengths: the query
    a, b = (r, q) if swap else (q, r)
    ca, cb = a.mean(0), b.mean(0)
    a, b = a - ca, b - cb                                               # (each about its own centroid: float32 keeps its digits)
    La, Lb = a.shape[0], b.shape[0]
    lnorm = {'query': Lq, 'reference': Lr, 'shorter': La, 'longer': Lb}[norm]
    d0 = S.d0(lnorm)
    s0 = stage0(a, b, lnorm, d0, n_iter)
    o = s0['offset']
    ia, ib = list(range(La)), list(range(o, o + La))
    stages = [{'value': s0['value'], 'R': s0['R'], 'cp': s0['cp'], 'cq': s0['cq'], 'ia': ia, 'ib': ib}]
    gap, path_margin, rounds = s0['gap'], math.inf, 0
    for _ in range(n_rounds):
        prev = stages[-1]
        Ta = (a - prev['cp']) @ prev['R'].T + prev['cq']
        Sc = 1 / (1 + ((Ta[:, None] - b[None]) ** 2).sum(-1) / d0 ** 2)
        move, lead = fill(Sc, gap_open)
        rounds += 1
        ia, ib, margin = traceback(move, lead, La, Lb)
        path_margin = min(path_margin, margin)
        if ib == prev['ib'] and ia == prev['ia']:
            break
        if len(ia) < 3:
            break
        P, Q = a[ia][None], b[ib][None]
        score, R, cp, cq, g = fit_trace(P, Q, torch.ones(1, len(ia), dtype=dtype, device=a.device), lnorm, d0, n_iter)
        gap = min(gap, float(g.min()))
        it = int((score[0] == score[0].max()).nonzero()[0])
        stages.append({'value': score[0, it], 'R': R[0, it], 'cp': cp[0, it], 'cq': cq[0, it], 'ia': ia, 'ib': ib})
    values = torch.stack([s['value'] for s in stages])
    k = int((values == values.max()).nonzero()[0])
    best = stages[k]
    others = [float(s['value']) for s in stages if (s['ia'], s['ib']) != (best['ia'], best['ib'])]
    d2 = (((a[best['ia']] - best['cp']) @ best['R'].T + best['cq'] - b[best['ib']]) ** 2).sum(-1)
    # b ~ R a + t in the callers' frame
    R = best['R']
    t = cb + best['cq'] - R @ (ca + best['cp'])
    amap = [-1] * Lq
    if swap:
        for i, j in zip(best['ia'], best['ib']):
            amap[j] = i
        rot, trans = R.T, -(R.T @ t)
    else:
        for i, j in zip(best['ia'], best['ib']):
            amap[i] = j
        rot, trans = R, t
    return {'tm': best['value'], 'rmsd': d2.mean().sqrt(), 'n_aligned': len(best['ia']), 'rounds': rounds, 'map': amap, 'rot': rot,
            'trans': trans, 'stage0': s0['value'], 'stages': values, 'best': k, 'gap': gap, 'margin': s0['margin'],
            'path_margin': path_margin, 'stage_lead': float(best['value']) - max(others) if others else math.inf}


def all_pairs(xq, lq, xr, lr, dtype=torch.float64, **kw):
    """Every query against every reference: {'tm', 'rmsd' [M, R] in `dtype`, 'n_aligned', 'rounds' [M, R] int64, 'map' [M, R, Nq] int64,
    'rot' [M, R, 3, 3], 'trans' [M, R, 3], 'stage0', 'gap', 'margin', 'path_margin', 'stage_lead' [M, R] float64}."""
    M, R, Nq = xq.shape[0], xr.shape[0], xq.shape[1]
    f = dict(dtype=dtype, device=xq.device)
    out = {'tm': torch.zeros(M, R, **f), 'rmsd': torch.zeros(M, R, **f), 'n_aligned': torch.zeros(M, R, dtype=torch.int64),
           'rounds': torch.zeros(M, R, dtype=torch.int64), 'map': torch.full((M, R, Nq), -1, dtype=torch.int64),
           'rot': torch.zeros(M, R, 3, 3, **f), 'trans': torch.zeros(M, R, 3, **f)}
    for k in ('stage0', 'gap', 'margin', 'path_margin', 'stage_lead'):
        out[k] = torch.zeros(M, R, dtype=torch.float64)
    for m in range(M):
        for r in range(R):
            one = align(xq[m, :lq[m]], xr[r, :lr[r]], dtype=dtype, **kw)
            for k in out:
                if k == 'map':
                    out[k][m, r, :lq[m]] = torch.tensor(one[k])
                else:
                    out[k][m, r] = one[k]
    return out


def well_posed(ref):
    """The pairs the oracle alone calls well-posed: every one of the four figures at least ILL."""
    return (ref['gap'] >= ILL) & (ref['margin'] >= ILL) & (ref['path_margin'] >= ILL) & (ref['stage_lead'] >= ILL)


def rescore(xq, lq, xr, lr, amap, rot, trans, norm):
    """tm, rmsd and the count of an alignment recomputed in float64 from what the entry returned: map [M, R, Nq], rot [M, R, 3, 3], trans
    [M, R, 3].  Returns (tm, rmsd [M, R] float64, n [M, R] int64)."""
    M, R = amap.shape[0], amap.shape[1]
    tm, rmsd, n = torch.zeros(M, R, dtype=torch.float64), torch.zeros(M, R, dtype=torch.float64), torch.zeros(M, R, dtype=torch.int64)
    for m in range(M):
        for r in range(R):
            La, Lb = min(lq[m], lr[r]), max(lq[m], lr[r])
            d0 = S.d0({'query': lq[m], 'reference': lr[r], 'shorter': La, 'longer': Lb}[norm])
            lnorm = {'query': lq[m], 'reference': lr[r], 'shorter': La, 'longer': Lb}[norm]
            i = (amap[m, r] >= 0).nonzero()[:, 0]
            j = amap[m, r][i].long()
            d2 = ((xq[m, i].double() @ rot[m, r].double().T + trans[m, r].double() - xr[r, j].double()) ** 2).sum(-1)
            tm[m, r] = (1 / (1 + d2 / d0 ** 2)).sum() / lnorm
            rmsd[m, r] = d2.mean().sqrt()
            n[m, r] = len(i)
    return tm, rmsd, n


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------

def excursion(p0, p1, n, seed):
    """n residues that leave the chain between p0 and p1 sideways and come back: a hairpin of C-alpha spacing."""
    g = torch.Generator().manual_seed(seed)
    side = torch.randn(3, generator=g)
    axis = p1 - p0
    side = side - axis * (side @ axis) / (axis @ axis).clamp(min=1e-6)
    side = side / side.norm()
    mid = 0.5 * (p0 + p1)
    out = []
    for t in range(n):
        depth = 1 + min(t, n - 1 - t)
        out.append(mid + 3.8 * depth * side + (0.95 if 2 * t >= n else -0.95) * axis / axis.norm().clamp(min=1e-6))
    return torch.stack(out)


def indel(x, cut, n_cut, at, n_ins, seed):
    """x [L, 3] with residues cut..cut+n_cut-1 removed and an n_ins-residue excursion spliced in before residue `at` (< cut); what
    follows is not displaced."""
    ins = excursion(x[at - 1], x[at], n_ins, seed)
    return torch.cat([x[:at], ins, x[at:cut], x[cut + n_cut:]])


def pad(chains):
    """Chains as (x float32 [K, N, 3] padded with zeros, lengths)."""
    lengths = [len(c) for c in chains]
    x = torch.zeros(len(chains), max(lengths), 3)
    for k, c in enumerate(chains):
        x[k, :len(c)] = c
    return x, lengths


def family(N, base=None):
    """The parity case of length N: six query walks; six references derived one per query (k = 0..5: a moved copy with NOISE[k] Angstrom of
    noise, residues 2N/3..2N/3+3+k removed and a 3+2k-residue excursion spliced in at N/3; below N = 16 the tiny form: one residue
    removed in the middle and two appended) and six unrelated walks of lengths N-5+4k (at least 4): (xq, lq, xr, lr), 72 pairs."""
    base = FAMILY_BASE.get(N, 0) if base is None else base
    seed = 1000 * N + base
    queries = [walk(1, N, seed + k)[0] for k in range(6)]
    refs = []
    for k, x in enumerate(queries):
        if N >= 16:
            y = indel(x, 2 * N // 3, 4 + k, N // 3, 3 + 2 * k, seed + 20 + k)
        else:
            tail = walk(1, 3, seed + 20 + k)[0]
            y = torch.cat([x[:N // 2], x[N // 2 + 1:], x[-1] + tail[1:] - tail[0]])
        refs.append(S.moved(y, seed + 40 + k, NOISE[k]))
    refs += [walk(1, max(4, N - 5 + 4 * k), seed + 60 + k)[0] for k in range(6)]
    xq, lq = pad(queries)
    xr, lr = pad(refs)
    return xq, lq, xr, lr


def insertion_pair(seed=6420):
    """(a, b): a 64-residue walk and a moved copy with a 10-residue excursion 40 A away spliced in at residue 32."""
    a = walk(1, 64, seed)[0]
    g = torch.Generator().manual_seed(seed + 1)
    side = torch.randn(3, generator=g)
    far = 0.5 * (a[31] + a[32]) + 40.0 * side / side.norm() + walk(1, 10, seed + 2)[0]
    return a, S.moved(torch.cat([a[:32], far, a[32:]]), seed + 3)


def limit_pairs():
    """The two largest calls: ((q, r) of 362 x 362: a walk and a moved, noised copy with a 6-residue deletion and a 6-residue
    excursion; (q, r) of 128 x 1024: a moved, noised stretch of the long walk from residue 500 on)."""
    a = walk(1, 362, 36200)[0]
    b = S.moved(indel(a, 240, 6, 120, 6, 36201), 36202, 0.5)
    long = walk(1, 1024, 102400)[0]
    return (a, b), (S.moved(long[500:628], 102401, 0.5), long)
