"""Helpers of test_conditioned_host.py / test_conditioned_gpu.py: a scaffold-shaped conditioned batch at the lengths on either
side of one, two and three 64-wide j tiles of k_pair_static / k_pair_init, its inputs in two coordinate styles, and the oracle's
taps with the single representation added.

genie_prepare_features reads one flag per batch (any byte of fixed_structure_mask set) and picks the form of the pair feature
net's step-invariant term by it: with the flag set k_pair_static<true> writes pstatic (relative position + same chain + motif
template) and k_pair_init<false> reads it back; with it clear k_pair_init<true> looks the row up.  Both walk
(b, i, 64-wide j tile) and index fixed_structure_mask[B,N,N] themselves, so the batch here puts motif residues, the chain
break and a shorter conditioned entry with b > 0 across the tile edges.  No tests here."""
import functools

import torch

import _parity as P
from oracle import genie_oracle as O

LENGTHS = [130, 129, 128, 65, 64, 63, 5]        # descending: the engine's workspace is allocated once
STYLES = ('randn', 'walk')
S_TOL = 2e-5                                     # the single representation: test_denoiser_matches_oracle_small_dims' bound
TAIL_CHAIN = 23                                  # the second chain of entry 0: the break sits at N - 23, on no tile edge
INDEX_OFFSET = 100                               # residue_index of the first chain: both relpos clamps, table rows past N
N_POS = 512
WALK_TIMESTEPS = [1, 7, 40]
INGREDIENTS = ('structure_mask', 'sequence_mask', 'motif_coords', 'aatype', 'interface_mask', 'chain_split', 'index_offset')


def entry_lengths(N):
    return [N, max(5, N // 2 + 1), N - 1]


def motif_index(N):
    """[motif residues of entry 0, of entry 1]: entry 0 straddles the first tile edge (61 .. 67) and ends on the last rows of
    the last partial tile for N >= 70, and takes a few residues at each end below that; entry 1 its first three and last two.
    At 8 <= N < 70 the head is 1 .. 3, not 0 .. 2: with residue 0 in the motif, column 64 of the mask at N = 65 would equal
    column 0 on every row, and a kernel that dropped the tile offset from its mask index would read the same bytes."""
    L1 = entry_lengths(N)[1]
    if N >= 70:
        m0 = list(range(61, 68)) + list(range(N - 3, N))
    elif N >= 8:
        m0 = [1, 2, 3, N - 3, N - 2, N - 1]
    else:
        m0 = sorted(set(range(min(3, N // 2))) | set(range(max(N - 3, (N + 1) // 2), N)))
    m1 = sorted({0, 1, 2, L1 - 2, L1 - 1})
    return [m0, m1]


def interface_index(N):
    return sorted({0, N // 2, N - 1})


def motif_coords(n, seed):
    """CA-like: a cumulative sum of 3.8 A steps in random directions"""
    g = torch.Generator().manual_seed(seed)
    step = torch.randn(n, 3, generator=g)
    return torch.cumsum(3.8 * step / step.norm(dim=-1, keepdim=True), 0)


def scaffold_like(N, without=None):
    """The feature dict of the three-entry batch padded to N (entry 0: length N, two chains [N - 23, 23] for N > 40 with the
    first chain's residue_index + 100, one motif, three interface residues; entry 1: length max(5, N // 2 + 1), one chain, a
    motif on both ends; entry 2: length N - 1, unconditioned).  `without` names one of INGREDIENTS to leave out."""
    assert without is None or without in INGREDIENTS, without
    lengths = entry_lengths(N)
    split = N > 40 and without != 'chain_split'
    chains = [[N - TAIL_CHAIN, TAIL_CHAIN] if split else [N], [lengths[1]], [lengths[2]]]
    f = O.empty_features(lengths, n_pad=N, chains_per_sample=chains)
    if N > 40 and without != 'index_offset':
        f['residue_index'][0, :N - TAIL_CHAIN] += INDEX_OFFSET
    for b, idx in enumerate(motif_index(N)):
        O.add_motif(f, b, motif_coords(len(idx), 40 + b), idx, aatype_idx=[(3 + 7 * k) % 20 for k in range(len(idx))])
    if without != 'interface_mask':
        f['interface_mask'][0, interface_index(N)] = True
    if without == 'structure_mask':
        f['fixed_structure_mask'].zero_()
    if without == 'sequence_mask':
        f['fixed_sequence_mask'].zero_()
    if without == 'motif_coords':
        f['atom_positions'].zero_()
    if without == 'aatype':
        f['aatype'].zero_()
    return f


def frame_margin(features, trans):
    """max |float32 frames - float64 frames| of the oracle on these coordinates"""
    fr = O.prepare_features(features)
    a = O.compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask'])
    b = O.compute_frenet_frames(trans.double(), fr['chain_index'], fr['residue_mask'])
    return float((a.double() - b).abs().max())


def walk_inputs(features, seed):
    """(coordinates, timesteps [1, 7, 40]): per entry a centred random walk with 3.8 A steps, so pair distances run far past
    the last template bin (20 A); redrawn like P.conditioned_inputs until the float32 oracle's own frames are within a quarter
    of FRAME_TOL of its float64 frames (the oracle alone decides)."""
    B, N = features['residue_mask'].shape
    assert B == len(WALK_TIMESTEPS)
    for k in range(64):
        g = torch.Generator().manual_seed(seed + 100000 * k)
        step = torch.randn(B, N, 3, generator=g)
        x = torch.cumsum(3.8 * step / step.norm(dim=-1, keepdim=True), 1)
        x = (x - x.mean(1, keepdim=True)).contiguous()
        if frame_margin(features, x) <= P.FRAME_TOL / 4:
            return x, torch.tensor(WALK_TIMESTEPS, dtype=torch.int32)
    raise AssertionError('no well-conditioned draw in 64 tries')


@functools.lru_cache(maxsize=None)
def case(N, style='randn'):
    """(features, residue_mask, translations, timesteps, frames) of scaffold_like(N), shared and left unchanged: 'randn' is
    P.conditioned_inputs, 'walk' is walk_inputs; the frames are the float32 oracle's"""
    assert style in STYLES, style
    dims = O.small_dims()
    f = scaffold_like(N)
    fr = O.prepare_features(f)
    trans, ts = P.conditioned_inputs(f, dims['n_timestep'], 4000 + N) if style == 'randn' else walk_inputs(f, 4500 + N)
    rots = O.compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask'])
    return f, fr['residue_mask'], trans, ts, rots


def reference(sd, dims, f, rots, trans, ts, double=True):
    """P.oracle_taps plus 's', the single feature net's output (float64 arithmetic on the same float32 values when `double`)"""
    ref = P.oracle_taps(sd, dims, f, rots, trans, ts, double=double)
    cast = P.as64 if double else (lambda x: x)
    fr = O.prepare_features(f)
    with torch.no_grad():
        ref['s'] = O.single_feature_net({k: cast(v) for k, v in sd.items()}, dims, ts, fr, trans.shape[1])
    return ref


def compare(out, ref, residue_mask):
    """P.compare_taps with ('s', error, 2e-5) in front (all rows: the oracle masks padded residues of s to zero)"""
    s = float((out['s'].double() - ref['s'].to(out['s'].device).double()).abs().max())
    return [('s', s, S_TOL)] + P.compare_taps(out, ref, residue_mask)


def ratios(results):
    """{tap: error / bound} of the bounded entries"""
    return {tap: err / bound for tap, err, bound in results if bound > 0}
