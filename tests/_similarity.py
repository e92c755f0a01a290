"""What the pairwise TM-score's tests share (tests/test_similarity_host.py, test_similarity_gpu.py, tools/similarity_time.py): the score
of include/genie_hip.h (genie_pairwise_tm) written out independently of the package as a torch oracle -- `eigh` on Horn's 4x4 matrix,
a loop over the pairs with their offsets and seeds side by side in one batch, the score of every iteration kept as a trace, and the
smallest relative gap between the two largest Horn eigenvalues of a pair -- which runs in float64 as the oracle and in float32 as the
restatement a user would write; the inputs and the case list.  Nothing here calls the library."""
import math

import torch

from _motif import walk

SEEDS, MIN_LEN = 11, 4

# equal-length parity cases (N; M = 12 designs each), the long one (M = 2), the mixed-length one (padded to its longest)
EQUAL_N = (4, 5, 63, 64, 65, 129, 256, 300)
LONG_N = 1706
MIXED = (20, 33, 33, 47, 64, 64, 90)


def d0(L):
    return max(0.5, 1.24 * (L - 15) ** (1.0 / 3.0) - 1.8) if L > 15 else 0.5


def windows(La):
    """The 11 seed windows (start, length) of a moving chain of La residues, from the statement in include/genie_hip.h."""
    out = [(0, La)]
    for k in (1, 2):
        length, n = max(math.ceil(La / 2 ** k), MIN_LEN), 2 ** (k + 1) - 1
        out += [(math.floor(j * (La - length) / (n - 1)), length) for j in range(n)]
    return out


def rotation(seed, dtype=torch.float64):
    """A random proper rotation [3, 3] (QR of a seeded Gaussian matrix, determinant fixed)."""
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    if torch.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.to(dtype)


def moved(x, seed, sigma=0.0, shift=(11.0, -7.0, 5.0)):
    """x [L, 3] under a random rigid motion, plus Gaussian noise of `sigma` Angstrom per coordinate: float32."""
    g = torch.Generator().manual_seed(seed + 7919)
    y = x.double() @ rotation(seed).T + torch.tensor(shift, dtype=torch.float64)
    return (y + sigma * torch.randn(x.shape, generator=g, dtype=torch.float64)).float()


NOISE = (0.2, 0.5, 1.0, 2.0, 3.0, 4.5)


def designs(N, M=12, base=0):
    """The parity set of length N: M / 2 walks of seeds 100 N + base + k and a moved, noised copy of each (seeds 100 N + base + M / 2 + k,
    noise NOISE[k] Angstrom), so that TM runs from about 0.1 (unrelated walks) to 0.99: float32 [M, N, 3]."""
    h = M // 2
    ws = [walk(1, N, 100 * N + base + k)[0] for k in range(h)]
    return torch.stack(ws + [moved(ws[k], 100 * N + base + h + k, NOISE[k % len(NOISE)]) for k in range(h)])


def mixed_designs(lengths=MIXED):
    """The mixed-length set: walks of seeds 100 N + m (N the longest) padded with zeros to N, design 0 a moved, noised excerpt of
    design 3 from residue 7 on and design 1 one of the last design from residue 40 on, so that threading has something to find:
    (x float32 [M, N, 3], lengths)."""
    N = max(lengths)
    chains = [walk(1, L, 100 * N + m)[0] for m, L in enumerate(lengths)]
    chains[0] = moved(chains[3][7:7 + lengths[0]], 100 * N + 50, 0.3)
    chains[1] = moved(chains[-1][40:40 + lengths[1]], 100 * N + 51, 0.8)
    x = torch.zeros(len(lengths), N, 3)
    for m, c in enumerate(chains):
        x[m, :len(c)] = c
    return x, list(lengths)


def horn_matrix(S):
    """Horn's symmetric 4x4 matrix [..., 4, 4] of a correlation S = sum p q^T [..., 3, 3]."""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (S[..., i, j] for i in range(3) for j in range(3))
    rows = [[xx + yy + zz, yz - zy, zx - xz, xy - yx], [yz - zy, xx - yy - zz, xy + yx, zx + xz],
            [zx - xz, xy + yx, -xx + yy - zz, yz + zy], [xy - yx, zx + xz, yz + zy, -xx - yy + zz]]
    return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)


def quaternion_rotation(q):
    """The rotation matrix [..., 3, 3] of unit quaternions (w, x, y, z) [..., 4]."""
    w, x, y, z = q.unbind(-1)
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)


def ascend(P, Q, lnorm, n_iter):
    """The ascents of B alignments at once.  P, Q [B, La, 3] (residue n of P corresponds to residue n of Q), lnorm [B] the normalising
    lengths.  Returns (trace [B, 11, n_iter]: the score of every seed at every iteration, rmsd [B]: sqrt(mean d^2) of seed 0 at
    iteration 0, gap [B]: the smallest relative gap between the two largest Horn eigenvalues over all fits), in P's dtype."""
    B, La, _ = P.shape
    dz = torch.tensor([d0(int(L)) for L in lnorm.tolist()], dtype=P.dtype, device=P.device)[:, None, None]
    ln = lnorm.to(P)[:, None]
    W = torch.zeros(SEEDS, La, dtype=P.dtype, device=P.device)
    for s, (start, length) in enumerate(windows(La)):
        W[s, start:start + length] = 1
    W = W[None].expand(B, SEEDS, La)
    trace, gap, rmsd = [], None, None
    for it in range(n_iter):
        sw = W.sum(-1, keepdim=True)
        Pc = P[:, None] - (W @ P / sw)[:, :, None]                   # [B, 11, La, 3]: about the weighted centroid of every seed
        Qc = Q[:, None] - (W @ Q / sw)[:, :, None]
        S = torch.einsum('bsl,bsli,bslj->bsij', W, Pc, Qc)
        ev, vec = torch.linalg.eigh(horn_matrix(S))
        g = ((ev[..., 3] - ev[..., 2]) / ev.abs().amax(dim=-1).clamp(min=1e-30)).amin(dim=1)
        gap = g if gap is None else torch.minimum(gap, g)
        R = quaternion_rotation(vec[..., :, 3])
        d2 = ((Pc @ R.transpose(-1, -2) - Qc) ** 2).sum(-1)         # [B, 11, La]: all residues, whatever the weights
        if it == 0:
            rmsd = d2[:, 0].mean(-1).sqrt()
        t = 1 / (1 + d2 / dz ** 2)
        trace.append(t.sum(-1) / ln)
        W = t * t
    return torch.stack(trace, dim=-1), rmsd, gap


def pair(a, b, norm='shorter', n_iter=16, dtype=torch.float64):
    """One pair, a [La, 3] moving along b [Lb, 3], La <= Lb: {'tm', 'rmsd', 'offset', 'gap', 'margin' (the best offset's lead over the
    second best in TM; inf with one offset), 'by_offset' [Lb - La + 1], 'trace' [offsets, 11, n_iter]}."""
    a, b = a.to(dtype), b.to(dtype)
    La, Lb = a.shape[0], b.shape[0]
    assert MIN_LEN <= La <= Lb
    Q = b.unfold(0, La, 1).transpose(1, 2)                              # [offsets, La, 3]
    n_off = Q.shape[0]
    lnorm = torch.full((n_off,), La if norm == 'shorter' else Lb, dtype=torch.int64, device=a.device)
    trace, rmsd, gap = ascend(a[None].expand(n_off, La, 3), Q, lnorm, n_iter)
    by_offset = trace.amax(dim=(1, 2))
    o = int((by_offset == by_offset.max()).nonzero()[0])
    top = torch.sort(by_offset, descending=True).values
    return {'tm': by_offset[o], 'rmsd': rmsd[o], 'offset': o, 'gap': gap.min(), 'by_offset': by_offset, 'trace': trace,
            'margin': top[0] - top[1] if n_off > 1 else torch.tensor(math.inf, dtype=dtype, device=a.device)}


def all_pairs(x, lengths=None, norm='shorter', n_iter=16, dtype=torch.float64, chunk=4096):
    """Every pair of x [M, N, 3]: {'tm', 'rmsd', 'gap', 'margin' [M, M] in `dtype`, 'offset' [M, M] int64}, symmetric, the diagonal
    (1, 0, 0) with gap and margin inf.  The shorter design moves; of equal lengths the one with the lower index.  Pairs of equal
    lengths (one offset each) go through `ascend` in batches of `chunk`; the others one pair at a time."""
    M, N = x.shape[0], x.shape[1]
    lengths = [N] * M if lengths is None else list(lengths)
    x = x.to(dtype)
    kw = dict(dtype=dtype, device=x.device)
    out = {'tm': torch.eye(M, **kw), 'rmsd': torch.zeros(M, M, **kw), 'gap': torch.full((M, M), math.inf, **kw),
           'margin': torch.full((M, M), math.inf, **kw), 'offset': torch.zeros(M, M, dtype=torch.int64, device=x.device)}

    def put(i, j, **v):
        for k, val in v.items():
            out[k][i, j] = out[k][j, i] = val

    equal = {}
    for i in range(M):
        for j in range(i + 1, M):
            if lengths[i] == lengths[j]:
                equal.setdefault(lengths[i], []).append((i, j))
                continue
            a, b = (i, j) if lengths[i] < lengths[j] else (j, i)
            r = pair(x[a, :lengths[a]], x[b, :lengths[b]], norm, n_iter, dtype)
            put(i, j, **{k: r[k] for k in out})
    for L, pairs in equal.items():
        for c in range(0, len(pairs), chunk):
            ij = torch.tensor(pairs[c:c + chunk], device=x.device)
            trace, rmsd, gap = ascend(x[ij[:, 0], :L], x[ij[:, 1], :L], torch.full((len(ij),), L, dtype=torch.int64), n_iter)
            tm = trace.amax(dim=(1, 2))
            for k, v in (('tm', tm), ('rmsd', rmsd), ('gap', gap)):
                out[k][ij[:, 0], ij[:, 1]] = v
                out[k][ij[:, 1], ij[:, 0]] = v
    return out


# ---- known answers ------------------------------------------------------------------------------------------------------------------

def core_pair(seed=6400):
    """A 64-residue walk and a rigidly moved copy whose last 16 residues were replaced by a segment 100 A away: the common core is
    48 / 64 = 0.75, and the plain superposition of all 64 is far off it."""
    a = walk(1, 64, seed)[0]
    b = a.clone()
    b[48:] = walk(1, 16, seed + 1)[0] + torch.tensor([100.0, 60.0, -80.0])
    return a, moved(b, seed + 2)


def mirror_pair(seed=6410, N=64):
    a = walk(1, N, seed)[0]
    return a, a * torch.tensor([-1.0, 1.0, 1.0])


def threading_pair(seed=4700):
    """(a, b): a a moved 20-residue excerpt of the 47-residue walk b, from residue 7 on."""
    b = walk(1, 47, seed)[0]
    return moved(b[7:27], seed + 1), b


def clusters_single(tm, threshold):
    """Connected components of tm >= threshold by flood fill, labels in the order of each component's lowest member: a list."""
    M = tm.shape[0]
    labels = [-1] * M
    for m in range(M):
        if labels[m] >= 0:
            continue
        labels[m] = c = max(labels) + 1
        todo = [m]
        while todo:
            u = todo.pop()
            for v in range(M):
                if labels[v] < 0 and float(tm[u, v]) >= threshold:
                    labels[v] = c
                    todo.append(v)
    return labels
