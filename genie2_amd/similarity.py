"""How different the designs of a set are: the TM-score of every pair as one HIP launch (genie_pairwise_tm,
csrc/similarity_kernels.hip; include/genie_hip.h states the score exactly), clustering of the matrix on the host, and the numbers a
diversity report is made of.  The score is the project's own gapless, seeded form of the TM objective: not a port of the TMscore or
TMalign programs, and a lower bound of theirs.

    x, lengths, names = load_designs(paths)
    out = PairwiseTM('cuda:0')(x, lengths)                  # {'tm', 'rmsd', 'offset'}: [M, M] on the device
    labels, representatives = cluster_single(out['tm'], 0.6)
    summary = diversity_summary(out['tm'], labels)

Designs that differ by an inserted loop or a deleted turn, and queries against references of any length (novelty), go through the
gapped form, one more HIP launch (genie_tm_align, csrc/tmalign_kernels.hip): the gapless search as a seed, then dynamic programming
under the TM objective, refitted, for every (query, reference) pair.

    out = TMAlign('cuda:0')(xq, lq, xr, lr, norm='query')   # {'tm', 'rmsd', 'n_aligned', 'rounds'}: [M, R] on the device

Not here: designability.  (The score inside the sampling loop is smc.FoldPotential, csrc/fold_kernels.hip.)"""
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


ALIGN_NORMS = ('query', 'reference', 'shorter', 'longer')       # genie_tm_align's norm 0, 1, 2, 3


def _chains(x, lengths, what):
    """A set of chains for TMAlign: (x as a tensor [M, N, 3], lengths as M ints in 4..N), shape, dtype, lengths and finiteness checked
    where x lives; `what` names the set in the messages."""
    x = torch.as_tensor(x)
    if x.dim() != 3 or x.shape[2] != 3 or x.shape[0] < 1:
        raise ValueError('%s must be [M >= 1, N, 3], got %s' % (what, tuple(x.shape)))
    M, N = int(x.shape[0]), int(x.shape[1])
    if N < capi.TM_MIN_LENGTH:
        raise ValueError('%s: N must be at least %d residues, got %d' % (what, capi.TM_MIN_LENGTH, N))
    if not x.dtype.is_floating_point:
        raise ValueError('%s must have a floating dtype, got %s' % (what, x.dtype))
    try:
        lengths = _check_lengths(lengths, M, N)
    except ValueError as e:
        raise ValueError('%s: %s' % (what, e)) from None
    if max(lengths) > capi.TMALIGN_MAX_LENGTH:
        raise ValueError('%s: a chain has %d residues, the gapped alignment takes %d..%d' % (what, max(lengths), capi.TM_MIN_LENGTH,
                                                                                          capi.TMALIGN_MAX_LENGTH))
    used = torch.arange(N, device=x.device)[None, :, None] < torch.as_tensor(lengths, device=x.device)[:, None, None]
    if not bool(torch.isfinite(torch.where(used, x.detach(), torch.zeros((), dtype=x.dtype, device=x.device))).all()):
        raise ValueError('%s holds a NaN or an infinity inside a chain' % what)
    return x, lengths


class TMAlign(_HipEntry):
    """genie_tm_align (include/genie_hip.h) on `device`: `TMAlign()(xq [M,Nq,3], lq, xr [R,Nr,3], lr, norm='query', n_iter=16, n_rounds=8,
    gap_open=-0.6, return_alignment=False)` returns {'tm', 'rmsd' [M,R] float32, 'n_aligned', 'rounds' [M,R] int32} on the device, from one
    launch on torch's current stream: every query aligned to every reference by the gapless seeded search (stage 0) and up to `n_rounds`
    rounds of dynamic programming under the TM objective with the gap opening penalty `gap_open` (-10..0), each refitted by `n_iter`
    ascent steps; the best stage is returned.  `norm` picks the normalising length: 'query', 'reference', 'shorter' or 'longer'.  Query
    m uses rows 0..lq[m]-1 (None: all Nq), reference r rows 0..lr[r]-1; the padding beyond the longest chain of each set is trimmed
    before the launch and never read.  With `return_alignment` the dict also holds 'map' [M,R,Nq] int32 (per query residue the matched
    reference residue, or -1), 'rot' [M,R,3,3] and 'trans' [M,R,3] with rot x_query + trans ~ x_reference.  Chains have 4..1024 residues
    and the longest query times the longest reference at most 131072 cells.  The inputs may live anywhere; they are checked where they
    live -- shapes, a floating dtype, finite values, lengths, the cell limit, every scalar: ValueErrors -- before the device is touched.
    A GPU entry only: a CPU device is a capi.GenieError."""

    def __init__(self, device='cuda'):
        self._bind(device, 'genie_tm_align')

    def __call__(self, xq, lq, xr, lr, norm='query', n_iter=16, n_rounds=8, gap_open=-0.6, return_alignment=False):
        xq, lq = _chains(xq, lq, 'xq')
        xr, lr = _chains(xr, lr, 'xr')
        Nq, Nr = max(lq), max(lr)
        if Nq * Nr > capi.TMALIGN_MAX_CELLS:
            raise ValueError('the longest query (%d) times the longest reference (%d) is above %d cells' % (Nq, Nr, capi.TMALIGN_MAX_CELLS))
        if norm not in ALIGN_NORMS:
            raise ValueError('norm must be one of %s, got %r' % (ALIGN_NORMS, norm))
        if isinstance(n_iter, bool) or not isinstance(n_iter, numbers.Integral) or not 1 <= n_iter <= capi.TM_MAX_ITER:
            raise ValueError('n_iter must be an integer in 1..%d, got %r' % (capi.TM_MAX_ITER, n_iter))
        if isinstance(n_rounds, bool) or not isinstance(n_rounds, numbers.Integral) or not 0 <= n_rounds <= capi.TMALIGN_MAX_ROUNDS:
            raise ValueError('n_rounds must be an integer in 0..%d, got %r' % (capi.TMALIGN_MAX_ROUNDS, n_rounds))
        if isinstance(gap_open, bool) or not isinstance(gap_open, numbers.Real) or not -10.0 <= gap_open <= 0.0:       # (NaN fails both)
            raise ValueError('gap_open must be a number in -10..0, got %r' % (gap_open,))
        if not isinstance(return_alignment, bool):
            raise ValueError('return_alignment must be a bool, got %r' % (return_alignment,))
        f32 = torch.float32
        out = self._launch(xq[:, :Nq].detach().to(self.device, f32).contiguous(), torch.tensor(lq, dtype=torch.int32).to(self.device),
                           xr[:, :Nr].detach().to(self.device, f32).contiguous(), torch.tensor(lr, dtype=torch.int32).to(self.device),
                           ALIGN_NORMS.index(norm), int(n_iter), int(n_rounds), float(gap_open), return_alignment)
        if return_alignment and Nq < xq.shape[1]:                  # map speaks of the caller's Nq
            pad = torch.full(out['map'].shape[:2] + (xq.shape[1] - Nq,), -1, dtype=torch.int32, device=self.device)
            out['map'] = torch.cat([out['map'], pad], dim=2)
        return out

    def _launch(self, xq, lq, xr, lr, norm, n_iter, n_rounds, gap_open, alignment=False):
        """One call of the C entry on xq [M,Nq,3], xr [R,Nr,3] float32 and lq [M], lr [R] int32, all contiguous on the device."""
        M, Nq, R, Nr = xq.shape[0], xq.shape[1], xr.shape[0], xr.shape[1]
        kw = dict(device=self.device)
        out = {'tm': torch.empty(M, R, dtype=torch.float32, **kw), 'rmsd': torch.empty(M, R, dtype=torch.float32, **kw),
               'n_aligned': torch.empty(M, R, dtype=torch.int32, **kw), 'rounds': torch.empty(M, R, dtype=torch.int32, **kw)}
        if alignment:
            out.update(map=torch.empty(M, R, Nq, dtype=torch.int32, **kw), rot=torch.empty(M, R, 3, 3, dtype=torch.float32, **kw),
                       trans=torch.empty(M, R, 3, dtype=torch.float32, **kw))
        self._call('genie_tm_align', self._stream(), M, Nq, _ptr(xq), _ptr(lq), R, Nr, _ptr(xr), _ptr(lr), norm, n_iter, n_rounds, gap_open,
                   _ptr(out['tm']), _ptr(out['rmsd']), _ptr(out['n_aligned']), _ptr(out['rounds']), _ptr(out.get('map')),
                   _ptr(out.get('rot')), _ptr(out.get('trans')))
        return out


def length_chunks(lengths, ratio=1.25, slack=16):
    """Indices into `lengths` sorted by length (ties by index) and cut into runs whose longest member is at most ratio x the shortest
    + slack: chains that share a call with little padding."""
    chunks = []
    for k in sorted(range(len(lengths)), key=lambda k: (lengths[k], k)):
        if chunks and lengths[k] <= ratio * lengths[chunks[-1][0]] + slack:
            chunks[-1].append(k)
        else:
            chunks.append([k])
    return chunks


def plan_calls(lq, lr, max_cells=None):
    """How a query-versus-reference run is dealt to calls of TMAlign: (calls, skipped_pairs).  Every call is (query indices, reference
    indices) with longest query x longest reference inside the cell limit; a pair is skipped exactly when its own Lq x Lr is above the
    limit, every other pair is in exactly one call.  Queries and references are chunked by length; a chunk pair that does not fit as a
    whole is dealt one query at a time to the references that fit it."""
    max_cells = capi.TMALIGN_MAX_CELLS if max_cells is None else max_cells
    calls, skipped = [], 0
    r_chunks = length_chunks(lr)
    for qc in length_chunks(lq):
        for rc in r_chunks:
            if max(lq[q] for q in qc) * max(lr[r] for r in rc) <= max_cells:
                calls.append((qc, rc))
                continue
            for q in qc:
                fit = [r for r in rc if lq[q] * lr[r] <= max_cells]
                skipped += len(rc) - len(fit)
                if fit:
                    calls.append(([q], fit))
    return calls, skipped


def align_sets(entry, xq, lq, xr, lr, **kw):
    """TMAlign of every query against every reference through plan_calls: ({'tm', 'rmsd' float32, 'n_aligned', 'rounds' int32} as numpy
    [M, R], scored bool [M, R], skipped_pairs).  Pairs above the cell limit are left at 0 and marked unscored."""
    xq, xr = torch.as_tensor(xq), torch.as_tensor(xr)
    M, R = len(lq), len(lr)
    out = {'tm': np.zeros((M, R), dtype=np.float32), 'rmsd': np.zeros((M, R), dtype=np.float32),
           'n_aligned': np.zeros((M, R), dtype=np.int32), 'rounds': np.zeros((M, R), dtype=np.int32)}
    scored = np.zeros((M, R), dtype=bool)
    calls, skipped = plan_calls(lq, lr)
    for qc, rc in calls:
        part = entry(xq[qc], [lq[q] for q in qc], xr[rc], [lr[r] for r in rc], **kw)
        for k in out:
            out[k][np.ix_(qc, rc)] = part[k].cpu().numpy()
        scored[np.ix_(qc, rc)] = True
    return out, scored, skipped


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
