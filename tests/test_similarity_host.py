"""The host side of the design-set similarity (genie2_amd/similarity.py, cluster_designs.py) and the float64 oracle of
tests/_similarity.py, without a GPU: d0 and the seed windows against the statement in include/genie_hip.h, the oracle's own properties
(a score that never decreases over the iterations, the three known answers), clustering and the summary on hand-made matrices, the
reader, every refusal that is made before the device is looked at, and the entry's declaration and export."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import _similarity as S
from genie2_amd import features as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dataset_100_0.pdb')


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


# ---- definitions ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L', (15, 16, 21, 22, 100, 256))
def test_d0_is_the_formula(L):
    from genie2_amd.similarity import tm_d0
    want = 0.5 if L <= 15 else max(0.5, 1.24 * (L - 15) ** (1.0 / 3.0) - 1.8)
    assert tm_d0(L) == pytest.approx(want, abs=1e-12) and tm_d0(L) >= 0.5
    assert tm_d0(L) == pytest.approx(S.d0(L), abs=1e-12)
    if L <= 21:
        assert tm_d0(L) == 0.5                                  # (1.24 cbrt(6) - 1.8 = 0.453: the floor holds up to 21)
    else:
        assert tm_d0(L) > 0.5


@pytest.mark.parametrize('La', (4, 5, 7, 16, 64, 1706))
def test_seed_windows(La):
    from genie2_amd.similarity import seed_windows
    w = seed_windows(La)
    assert len(w) == 11 and w == S.windows(La)
    assert all(start >= 0 and length >= 4 and start + length <= La for start, length in w)
    assert w[0] == (0, La)
    half, quarter = max(-(-La // 2), 4), max(-(-La // 4), 4)
    assert [length for _, length in w] == [La] + [half] * 3 + [quarter] * 7
    assert [s for s, _ in w[1:4]] == [j * (La - half) // 2 for j in range(3)]
    assert [s for s, _ in w[4:]] == [j * (La - quarter) // 6 for j in range(7)]
    assert w[1][0] == 0 and w[3][0] + half == La and w[4][0] == 0 and w[10][0] + quarter == La     # from the first residue to the last


def test_seed_windows_refuses_short_chains():
    from genie2_amd.similarity import seed_windows
    for bad in (3, 0, -1, 4.0, True):
        with pytest.raises(ValueError, match='La must be an integer >= 4'):
            seed_windows(bad)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', (4, 5, 16, 65))
def test_oracle_score_never_decreases(N):
    x = S.designs(N).double()
    i, j = torch.triu_indices(12, 12, 1)
    trace, _, _ = S.ascend(x[i], x[j], torch.full((len(i),), N), 16)
    assert float((trace[..., 1:] - trace[..., :-1]).min()) >= -1e-12
    assert float(trace.min()) > 0 and float(trace.max()) <= 1 + 1e-12


def test_oracle_known_answers():
    core = S.pair(*S.core_pair())
    assert float(core['tm']) >= 0.75 and float(core['tm']) < 0.76                  # the 48 / 64 core, found from a window seed
    assert float(core['trace'][0, 0, 0]) < 0.2 and float(core['rmsd']) > 20        # ... which the plain superposition misses
    assert float(S.pair(*S.mirror_pair())['tm']) < 0.6                             # a mirror image is not a match
    th = S.pair(*S.threading_pair())
    assert th['offset'] == 7 and float(th['tm']) >= 0.999 and float(th['rmsd']) < 1e-3
    others = torch.cat([th['by_offset'][:7], th['by_offset'][8:]])
    assert float(others.max()) < 0.3 and float(th['margin']) > 0.7
    # the same pair with the chains swapped by hand is what all_pairs computes for (longer, shorter)
    a, b = S.threading_pair()
    x = torch.zeros(2, 47, 3)
    x[0], x[1, :20] = b, a
    both = S.all_pairs(x, [47, 20])
    assert int(both['offset'][0, 1]) == 7 and float(both['tm'][0, 1]) == float(th['tm'])
    assert float(S.pair(a, b, norm='longer')['tm']) < float(th['tm']) * 20 / 47 + 0.05    # normalised by 47: at most 20 / 47 plus crumbs


# ---- clustering ----------------------------------------------------------------------------------------------------------------------

def _sym(M, entries, fill=0.1):
    t = np.full((M, M), fill)
    np.fill_diagonal(t, 1.0)
    for (a, b), v in entries.items():
        t[a, b] = t[b, a] = v
    return t


def test_chain_a_b_c_single_merges_leader_does_not():
    from genie2_amd.similarity import cluster_leader, cluster_single
    t = _sym(4, {(0, 1): 0.7, (1, 2): 0.7, (0, 2): 0.3})          # A-B, B-C linked, A-C not; design 3 alone
    labels, reps = cluster_single(t, 0.6)
    assert labels.tolist() == [0, 0, 0, 1] and reps == [1, 3]       # B has the highest mean TM to its cluster
    labels, reps = cluster_leader(t, 0.6)
    assert labels.tolist() == [0, 0, 1, 2] and reps == [0, 2, 3]    # C does not match the leader A
    assert labels.dtype == np.int64
    for fn in (cluster_single, cluster_leader):
        got = fn(torch.tensor(t, dtype=torch.float32), 0.6)        # tensors are taken too
        assert got[0].tolist() == fn(t, 0.6)[0].tolist()


def test_labels_follow_the_lowest_member_and_representatives_break_ties_low():
    from genie2_amd.similarity import cluster_leader, cluster_single
    t = _sym(6, {(1, 4): 0.9, (0, 5): 0.8, (2, 3): 0.65})
    labels, reps = cluster_single(t, 0.6)
    assert labels.tolist() == [0, 1, 2, 2, 1, 0] and reps == [0, 1, 2]         # two-member clusters: equal means, the lower index
    assert cluster_leader(t, 0.6)[0].tolist() == [0, 1, 2, 2, 1, 0]
    t = _sym(3, {(0, 1): 0.7, (0, 2): 0.7, (1, 2): 0.9})
    assert cluster_single(t, 0.6)[1] == [1]                                    # means 0.8, 0.867, 0.867: the first of the best


def test_threshold_edges():
    from genie2_amd.similarity import cluster_leader, cluster_single
    t = _sym(3, {(0, 1): 0.6, (1, 2): 0.59999})
    for fn in (cluster_single, cluster_leader):
        assert fn(t, 0.6)[0].tolist() == [0, 0, 1]                  # >= links, just below does not
        assert fn(t, 0.0)[0].tolist() == [0, 0, 0]
        assert fn(t, 1.0)[0].tolist() == [0, 1, 2]                  # only the diagonal reaches 1
        labels, reps = fn(np.ones((1, 1)), 0.6)
        assert labels.tolist() == [0] and reps == [0]
        for bad in (math.nan, math.inf, None, 'x'):
            with pytest.raises(ValueError, match='threshold must be a finite number'):
                fn(t, bad)
        with pytest.raises(ValueError, match='tm must be a square matrix'):
            fn(np.ones((2, 3)), 0.6)


def test_diversity_summary():
    from genie2_amd.similarity import cluster_single, diversity_summary
    t = _sym(4, {(0, 1): 0.7, (1, 2): 0.8, (0, 2): 0.3})
    labels, _ = cluster_single(t, 0.6)
    s = diversity_summary(t, labels)
    assert (s['n_designs'], s['n_clusters'], s['diversity']) == (4, 2, 0.5)
    assert s['mean_tm'] == pytest.approx((0.7 + 0.8 + 0.3 + 3 * 0.1) / 6) and s['max_tm'] == pytest.approx(0.8)
    assert s['nearest'].tolist() == [1, 2, 1, 0] and s['nearest_tm'].tolist() == pytest.approx([0.7, 0.8, 0.8, 0.1])
    one = diversity_summary(np.ones((1, 1)), np.zeros(1, dtype=np.int64))
    assert (one['n_designs'], one['n_clusters'], one['diversity'], one['mean_tm'], one['max_tm']) == (1, 1, 1.0, 0.0, 0.0)
    assert one['nearest'].tolist() == [-1] and one['nearest_tm'].tolist() == [0.0]
    # pairs that were never scored stay out of every figure
    scored = np.ones((4, 4), dtype=bool)
    scored[3, :3] = scored[:3, 3] = False
    s = diversity_summary(t, labels, scored)
    assert s['mean_tm'] == pytest.approx(0.6) and s['nearest'].tolist() == [1, 2, 1, -1] and s['nearest_tm'][3] == 0.0
    with pytest.raises(ValueError, match='labels must be'):
        diversity_summary(t, labels[:3])


# ---- the reader ----------------------------------------------------------------------------------------------------------------------

def test_load_designs(tmp_path):
    from genie2_amd.similarity import load_designs
    ca = np.array([[float(line[30:38]), float(line[38:46]), float(line[46:54])] for line in open(GOLDEN)
                   if line.startswith('ATOM') and line[13:15].strip() == 'CA'])
    f = F.create_empty_np_features([5, 7])                          # two chains: concatenated in file order
    f['atom_positions'] = S.walk(1, 12, 3)[0].double().numpy()
    two = str(tmp_path / 'two_chains.pdb')
    F.save_np_features_to_pdb(f, two)
    x, lengths, names = load_designs([GOLDEN, two])
    assert names == ['dataset_100_0', 'two_chains'] and lengths == [len(ca), 12]
    assert x.dtype == torch.float32 and tuple(x.shape) == (2, len(ca), 3)
    assert np.allclose(x[0].numpy(), ca, atol=1e-4)
    want = f['atom_positions'] - f['atom_positions'].mean(axis=0)
    assert np.allclose(x[1, :12].numpy(), want, atol=2e-3) and bool((x[1, 12:] == 0).all())
    assert len(F.parse_pdb(two)[1]) == 2
    with pytest.raises(ValueError, match='no design files'):
        load_designs([])
    empty = tmp_path / 'empty.pdb'
    empty.write_text('REMARK nothing\n')
    with pytest.raises(ValueError, match='holds no C-alpha atom'):
        load_designs([str(empty)])


# ---- refusals before the device is looked at --------------------------------------------------------------------------------------------

class _NoDevice:
    """PairwiseTM without a device: __call__ must refuse before it reaches _launch."""

    def __new__(cls):
        from genie2_amd.similarity import PairwiseTM
        e = PairwiseTM.__new__(PairwiseTM)
        e.device = torch.device('cpu')
        e._launch = lambda *a, **k: pytest.fail('the entry was launched')
        return e


def test_call_refuses_on_the_host():
    e = _NoDevice()
    x = S.designs(16, M=4)
    for bad, msg in ((x[0], r'x must be \[M >= 1, N, 3\]'), (x[:, :, :2], r'x must be \[M >= 1, N, 3\]'), (x[:0], r'x must be \[M >= 1, N, 3\]'),
                     (x[:, :3], 'N must be in 4..1706 residues, got 3'), (torch.zeros(2, 1707, 3), 'N must be in 4..1706 residues, got 1707'),
                     (x.long(), 'x must have a floating dtype')):
        with pytest.raises(ValueError, match=msg):
            e(bad)
    for bad in ('both', 0, None):
        with pytest.raises(ValueError, match='norm must be one of'):
            e(x, norm=bad)
    for bad in (0, 33, 16.0, True, None):
        with pytest.raises(ValueError, match=r'n_iter must be an integer in 1\.\.32'):
            e(x, n_iter=bad)
    for bad, msg in (([16, 16, 16], 'lengths must hold 4 integers'), ([16, 16, 16, 3], 'every length must be in 4..16'),
                     ([16, 17, 16, 16], r'every length must be in 4\.\.16 \(N\): design 1 has 17'), ([16.0, 16, 16, 16], 'lengths must hold 4 integers'),
                     (torch.tensor([16, 16, 2, 16]), 'design 2 has 2')):
        with pytest.raises(ValueError, match=msg):
            e(x, bad)
    for v in (math.nan, math.inf):
        y = x.clone()
        y[2, 5, 1] = v
        with pytest.raises(ValueError, match='NaN or an infinity inside a design'):
            e(y)
        with pytest.raises(ValueError, match='NaN or an infinity inside a design'):
            e(y.numpy(), [16, 16, 6, 16])
        with pytest.raises(pytest.fail.Exception, match='the entry was launched'):      # beyond the design's length nothing is read
            e(y, [16, 16, 5, 16])


def test_cpu_device_is_refused(lib):
    from genie2_amd import capi
    from genie2_amd.similarity import PairwiseTM
    with pytest.raises(capi.GenieError, match='genie_pairwise_tm runs on the GPU'):
        PairwiseTM('cpu')


def test_cli_parser_and_its_refusals(tmp_path):
    from genie2_amd import cluster_designs as CD
    import genie.cluster_designs as thin
    assert thin.main is CD.main and thin.build_parser is CD.build_parser
    p = CD.build_parser()
    a = p.parse_args(['--indir', 'out'])
    assert (a.outdir, a.tm_threshold, a.linkage, a.norm, a.n_iter, a.same_length_only, a.write_matrix, a.device) == \
        (None, 0.6, 'single', 'shorter', 16, False, False, 'cuda:0')
    for argv in ([], ['--indir', 'out', '--linkage', 'complete'], ['--indir', 'out', '--norm', 'mean']):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    for argv, msg in ((['--tm_threshold', '0'], 'tm_threshold must be above 0 and at most 1'), (['--tm_threshold', '1.5'], 'tm_threshold must be'),
                      (['--tm_threshold', 'nan'], 'tm_threshold must be'), (['--n_iter', '0'], r'n_iter must be in 1\.\.32, got 0'),
                      (['--n_iter', '33'], r'n_iter must be in 1\.\.32, got 33')):
        with pytest.raises(SystemExit, match=msg):
            CD.main(p.parse_args(['--indir', str(tmp_path)] + argv))
    with pytest.raises(SystemExit, match='is not a directory'):
        CD.main(p.parse_args(['--indir', str(tmp_path / 'missing')]))
    with pytest.raises(SystemExit, match='no .pdb files in'):
        CD.main(p.parse_args(['--indir', str(tmp_path)]))
    (tmp_path / 'pdbs').mkdir()
    with pytest.raises(SystemExit, match='no .pdb files in .*pdbs'):
        CD.main(p.parse_args(['--indir', str(tmp_path)]))
    for L, msg in ((3, 'short has 3 residues: a design needs 4..1706'), (1707, 'short has 1707 residues')):
        f = F.create_empty_np_features([L])
        f['atom_positions'] = S.walk(1, L, 1)[0].double().numpy() * 0.01       # (kept inside the PDB columns)
        F.save_np_features_to_pdb(f, str(tmp_path / 'pdbs' / 'short.pdb'))
        with pytest.raises(SystemExit, match=msg):
            CD.main(p.parse_args(['--indir', str(tmp_path)]))
    # the folder itself may hold the files
    flat = tmp_path / 'flat'
    flat.mkdir()
    (flat / 'b.pdb').write_text('')
    (flat / 'a.pdb').write_text('')
    assert [os.path.basename(f) for f in CD.design_files(str(flat))] == ['a.pdb', 'b.pdb']


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_and_exported(lib):
    from genie2_amd import build, capi
    assert 'similarity_kernels.hip' in build.SOURCES and os.path.exists(os.path.join(os.path.dirname(build.__file__), 'csrc', 'similarity_kernels.hip'))
    res, args = capi.SYMBOLS['genie_pairwise_tm']
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.genie_pairwise_tm is not None
    assert (capi.TM_SEEDS, capi.TM_MIN_LENGTH, capi.TM_MAX_LENGTH, capi.TM_MAX_ITER) == (11, 4, 1706, 32) == (S.SEEDS, S.MIN_LEN, S.LONG_N, 32)
    header = open(os.path.join(os.path.dirname(build.__file__), '..', 'include', 'genie_hip.h')).read()
    for line in ('#define GENIE_TM_SEEDS 11', '#define GENIE_TM_MIN_LENGTH 4', '#define GENIE_TM_MAX_LENGTH 1706', '#define GENIE_TM_MAX_ITER 32',
                 'int genie_pairwise_tm(genie_stream_t stream, int M, int N, const float* x'):
        assert line in header, line
    assert len(capi.SYMBOLS['genie_binder_potential'][1]) == 23                                # (the neighbour keeps its arguments)


def test_entry_refuses_before_any_launch(lib):
    """The argument checks of the C entry need no device: every one returns GENIE_E_ARG with its message."""
    one = C.c_void_p(16)                                            # (never dereferenced: the entry refuses first)
    ok = dict(M=2, N=16, x=one, length=one, norm=0, n_iter=16, tm=one, rmsd=one, offset=one)
    for change, msg in ((dict(M=0), 'M outside 1..65535'), (dict(M=65536), 'M outside 1..65535'), (dict(N=3), 'N outside 4..1706'),
                        (dict(N=1707), 'N outside 4..1706'), (dict(n_iter=0), 'n_iter outside 1..32'), (dict(n_iter=33), 'n_iter outside 1..32'),
                        (dict(norm=2), 'norm is neither 0 (shorter) nor 1 (longer)'), (dict(norm=-1), 'norm is neither'),
                        (dict(x=None), 'x is NULL'), (dict(length=None), 'length is NULL'), (dict(tm=None), 'tm is NULL'),
                        (dict(rmsd=None), 'rmsd is NULL'), (dict(offset=None), 'offset is NULL')):
        a = dict(ok, **change)
        rc = lib.genie_pairwise_tm(None, a['M'], a['N'], a['x'], a['length'], a['norm'], a['n_iter'], a['tm'], a['rmsd'], a['offset'])
        assert rc == -1, change
        assert lib.genie_last_error(None).decode().startswith('genie_pairwise_tm: ' + msg), change
