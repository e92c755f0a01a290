"""How different the designs of a set are: the TM-score of every pair as one HIP launch (genie_pairwise_tm,
csrc/similarity_kernels.hip; include/genie_hip.h states the score exactly), clustering of the matrix on the host, and the numbers a
diversity report is made of.  The score is the project's own gapless, seeded form of the TM objective: not a port of the TMscore or
TMalign programs, and a lower bound of theirs.

    x, lengths, names = load_designs(paths)
    out = PairwiseTM('cuda:0')(x, lengths)                  # {'tm', 'rmsd', 'offset'}: [M, M] on the device
    labels, representatives = cluster_single(out['tm'], 0.6)
    summary = diversity_summary(out['tm'], labels)

Not here: alignments with internal gaps (TM-align's dynamic programming), so designs of different lengths that differ by insertions
score lower than they would there; a query-versus-reference (novelty) form; designability.  (The score inside the sampling loop
is smc.FoldPotential, csrc/fold_kernels.hip.)"""
import math
import numbers

import numpy as np
import torch

from . import capi
from .smc import _HipEntry, _ptr

NORMS = ('shorter', 'longer')       # genie_pairwise_tm's norm 0, 1


def tm_d0(L):
    """d0 of the TM-score for a normalising length L: max(0.5, 1.24 (L - 15)^(1/3) - 1.8) above 15 residues, else 0.5."""
    return max(0.5, 1.24 * (L - 15) ** (1.0 / 3.0) - 1.8) if L > 15 else 0.5


def seed_windows(La):
    """The capi.TM_SEEDS windows (start, length) over a moving chain of La >= 4 residues that the ascents start from, in the
    entry's order: the whole chain, then for level k = 1, 2 the 2^(k+1) - 1 windows of length max(ceil(La / 2^k), 4) spread evenly
    from the first residue to the last (short chains repeat windows)."""
    if isinstance(La, bool) or not isinstance(La, numbers.Integral) or La < capi.TM_MIN_LENGTH:
        raise ValueError('La must be an integer >= %d, got %r' % (capi.TM_MIN_LENGTH, La))
    La = int(La)
    out = [(0, La)]
    for k in (1, 2):
        length, n = max(-(-La // 2 ** k), capi.TM_MIN_LENGTH), 2 ** (k + 1) - 1
        out += [(j * (La - length) // (n - 1), length) for j in range(n)]
    return out


def _check_lengths(lengths, M, N):
    """`lengths` as a list of M ints in 4..N (None: all N)."""
    if lengths is None:
        return [N] * M
    lengths = lengths.tolist() if torch.is_tensor(lengths) or isinstance(lengths, np.ndarray) else lengths
    if not isinstance(lengths, (list, tuple)):
        raise ValueError('lengths must hold %d integers, one per design, got %r' % (M, lengths))
    if len(lengths) != M or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in lengths):
        raise ValueError('lengths must hold %d integers, one per design, got %r' % (M, lengths))
    bad = [(m, v) for m, v in enumerate(lengths) if not capi.TM_MIN_LENGTH <= v <= N]
    if bad:
        raise ValueError('every length must be in %d..%d (N): design %d has %d' % (capi.TM_MIN_LENGTH, N, bad[0][0], bad[0][1]))
    return [int(v) for v in lengths]


class PairwiseTM(_HipEntry):
    """genie_pairwise_tm (include/genie_hip.h) on `device`: `PairwiseTM()(x [M,N,3], lengths=None, norm='shorter', n_iter=16)` returns
    {'tm' [M,M] float32, 'rmsd' [M,M] float32, 'offset' [M,M] int32} on the device, from one launch on torch's current stream.  Design m
    uses rows 0..lengths[m]-1 of x (None: all N); what lies beyond is never read.  `norm` picks the normalising length of a pair of
    unequal lengths, 'shorter' (the moving chain's) or 'longer'; `n_iter` the ascent steps per seed (1..32; 16 leaves at most 4e-3 to
    100 steps).  x may live anywhere (a tensor or an array); it is checked where it lives -- shape, a floating dtype, finite values,
    lengths in 4..N, norm, n_iter: ValueErrors -- before the device is touched.  A GPU entry only: a CPU device is a capi.GenieError."""

    def __init__(self, device='cuda'):
        self._bind(device, 'genie_pairwise_tm')

    def __call__(self, x, lengths=None, norm='shorter', n_iter=16):
        x = torch.as_tensor(x)
        if x.dim() != 3 or x.shape[2] != 3 or x.shape[0] < 1:
            raise ValueError('x must be [M >= 1, N, 3], got %s' % (tuple(x.shape),))
        M, N = int(x.shape[0]), int(x.shape[1])
        if not capi.TM_MIN_LENGTH <= N <= capi.TM_MAX_LENGTH:
            raise ValueError('N must be in %d..%d residues, got %d' % (capi.TM_MIN_LENGTH, capi.TM_MAX_LENGTH, N))
        if not x.dtype.is_floating_point:
            raise ValueError('x must have a floating dtype, got %s' % x.dtype)
        if norm not in NORMS:
            raise ValueError('norm must be one of %s, got %r' % (NORMS, norm))
        if isinstance(n_iter, bool) or not isinstance(n_iter, numbers.Integral) or not 1 <= n_iter <= capi.TM_MAX_ITER:
            raise ValueError('n_iter must be an integer in 1..%d, got %r' % (capi.TM_MAX_ITER, n_iter))
        lengths = _check_lengths(lengths, M, N)
        used = torch.arange(N, device=x.device)[None, :, None] < torch.as_tensor(lengths, device=x.device)[:, None, None]
        if not bool(torch.isfinite(torch.where(used, x.detach(), torch.zeros((), dtype=x.dtype, device=x.device))).all()):
            raise ValueError('x holds a NaN or an infinity inside a design')
        return self._launch(x.detach().to(self.device, torch.float32).contiguous(),
                            torch.tensor(lengths, dtype=torch.int32).to(self.device), NORMS.index(norm), int(n_iter))

    def _launch(self, x, lengths, norm, n_iter):
        """One call of the C entry on x [M,N,3] float32 and lengths [M] int32, both contiguous on the device."""
        M, N = x.shape[0], x.shape[1]
        out = {'tm': torch.empty(M, M, dtype=torch.float32, device=self.device),
               'rmsd': torch.empty(M, M, dtype=torch.float32, device=self.device),
               'offset': torch.empty(M, M, dtype=torch.int32, device=self.device)}
        self._call('genie_pairwise_tm', self._stream(), M, N, _ptr(x), _ptr(lengths), norm, n_iter, _ptr(out['tm']), _ptr(out['rmsd']),
                   _ptr(out['offset']))
        return out


def _matrix(tm):
    """A TM matrix as float64 numpy [M, M] on the host."""
    t = tm.detach().double().cpu().numpy() if torch.is_tensor(tm) else np.asarray(tm, dtype=np.float64)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or t.shape[0] < 1:
        raise ValueError('tm must be a square matrix [M >= 1, M], got %s' % (t.shape,))
    return t


def _threshold(threshold):
    if isinstance(threshold, bool) or not isinstance(threshold, numbers.Real) or not math.isfinite(threshold):
        raise ValueError('threshold must be a finite number, got %r' % (threshold,))
    return float(threshold)


def _representatives(t, labels):
    """Per cluster, the member with the highest mean TM to its cluster (itself included); ties to the lowest index."""
    reps = []
    for c in range(int(labels.max()) + 1):
        members = np.flatnonzero(labels == c)
        mean = t[np.ix_(members, members)].mean(axis=1)
        reps.append(int(members[int(np.argmax(mean))]))              # (argmax: the first of equal ones)
    return reps


def cluster_single(tm, threshold):
    """Single-linkage clusters of a TM matrix [M, M]: the connected components of tm >= threshold, by union-find on the host.  Returns
    (labels int64 [M], representatives): labels are 0, 1, ... in the order of each cluster's lowest member, representatives[c] is
    the member of cluster c with the highest mean TM to its cluster, ties to the lowest index."""
    t, threshold = _matrix(tm), _threshold(threshold)
    M = t.shape[0]
    parent = list(range(M))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in zip(*np.nonzero(np.triu(t >= threshold, 1))):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)                       # (the root is the component's lowest member)
    roots = [find(m) for m in range(M)]
    order = {r: c for c, r in enumerate(sorted(set(roots)))}
    labels = np.array([order[r] for r in roots], dtype=np.int64)
    return labels, _representatives(t, labels)


def cluster_leader(tm, threshold):
    """Leader clusters of a TM matrix [M, M]: the designs are taken in index order, each joins the first cluster whose representative
    (its founder) it matches at tm >= threshold and founds a new cluster otherwise.  Returns (labels int64 [M], representatives)."""
    t, threshold = _matrix(tm), _threshold(threshold)
    reps, labels = [], []
    for m in range(t.shape[0]):
        hit = [c for c, r in enumerate(reps) if t[m, r] >= threshold]
        if hit:
            labels.append(hit[0])
        else:
            labels.append(len(reps))
            reps.append(m)
    return np.array(labels, dtype=np.int64), reps


def diversity_summary(tm, labels, scored=None):
    """What a diversity report says of a TM matrix [M, M] and its cluster labels [M]: {'n_designs', 'n_clusters', 'diversity'
    (n_clusters / n_designs), 'mean_tm' and 'max_tm' over the off-diagonal entries (0 when there are none), 'nearest' int64 [M] (every
    design's most similar other design, ties to the lowest index; -1 when it has none) and 'nearest_tm' float64 [M] (0 with -1)}.
    `scored` bool [M, M] leaves the pairs it marks False out of all of them: pairs that were never computed."""
    t = _matrix(tm)
    labels = np.asarray(labels.detach().cpu().numpy() if torch.is_tensor(labels) else labels)
    M = t.shape[0]
    if labels.shape != (M,):
        raise ValueError('labels must be [%d], got %s' % (M, labels.shape))
    keep = ~np.eye(M, dtype=bool)
    if scored is not None:
        scored = np.asarray(scored.detach().cpu().numpy() if torch.is_tensor(scored) else scored, dtype=bool)
        if scored.shape != (M, M):
            raise ValueError('scored must be [%d, %d], got %s' % (M, M, scored.shape))
        keep &= scored
    n_clusters = len(set(labels.tolist()))
    off = np.where(keep, t, -np.inf)
    nearest = off.argmax(axis=1)
    nearest_tm = off[np.arange(M), nearest]
    alone = ~keep.any(axis=1)
    return {'n_designs': M, 'n_clusters': n_clusters, 'diversity': n_clusters / M,
            'mean_tm': float(t[keep].mean()) if keep.any() else 0.0, 'max_tm': float(t[keep].max()) if keep.any() else 0.0,
            'nearest': np.where(alone, -1, nearest).astype(np.int64), 'nearest_tm': np.where(alone, 0.0, nearest_tm)}


def load_designs(paths):
    """The C-alpha coordinates of the PDB files `paths` (features.parse_pdb; the chains of a file one after another) padded with
    zeros to the longest: (x float32 [M, N, 3], lengths [M] ints, names [M]: the file names without '.pdb' / '.pdb.gz')."""
    import os
    from .features import parse_pdb
    paths = list(paths)
    if not paths:
        raise ValueError('no design files given')
    coords, names = [], []
    for p in paths:
        xyz = [row for chain in parse_pdb(str(p))[1] for row in chain]
        if not xyz:
            raise ValueError('%s holds no C-alpha atom' % p)
        coords.append(np.asarray(xyz, dtype=np.float64))
        name = os.path.basename(str(p))
        names.append(name[:-7] if name.endswith('.pdb.gz') else name[:-4] if name.endswith('.pdb') else name)
    lengths = [len(c) for c in coords]
    x = np.zeros((len(coords), max(lengths), 3), dtype=np.float32)
    for m, c in enumerate(coords):
        x[m, :len(c)] = c
    return torch.from_numpy(x), lengths, names
