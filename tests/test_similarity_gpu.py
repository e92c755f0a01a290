"""The pairwise TM-score on the GPU (genie_pairwise_tm, csrc/similarity_kernels.hip; PairwiseTM in genie2_amd/similarity.py) against
the float64 oracle of tests/_similarity.py, the structure of its output, its invariances, the known answers, the entry's refusals, and
the command line end to end.

Bounds: the project's bar for a fused kernel, tm and rmsd within 1e-5 max(1, |value|), each widened per case to 4 x the error the
float32 restatement makes on the same input where that is larger (the kernel is held to float32 arithmetic; the factor covers another
summation order); offset exact.  A pair is left out only where the oracle alone calls it ill-posed -- the smallest relative gap
between the two largest Horn eigenvalues over its fits is below 1e-4, or, for offset, its two best offsets are within 1e-4 in TM --
and at most 5 % of a case's pairs may be: on the CPU the cases leave out 2 and 3 of 66 pairs at N = 4 and 5, 1 of 21 in the mixed case
under 'shorter', none elsewhere.

Worst error / bound over the parity cases, measured on an MI355X: 0.073 for tm (N = 65, the one case whose bar was widened, x1.63:
0.119 of the unwidened bar; 0.066 at N = 4 is the worst of the others), 0.042 for rmsd (N = 4); no offset differed."""
import os

import numpy as np
import pytest
import torch

import _similarity as S
from _motif import _ca_coordinates
from _parity import hard_time_limit

pytestmark = pytest.mark.gpu

BAR = 1e-5
_cache = {}


@pytest.fixture(autouse=True)
def _limit():
    with hard_time_limit(300):
        yield


@pytest.fixture(scope='module')
def entry():
    from genie2_amd.similarity import PairwiseTM
    return PairwiseTM('cuda:0')


def _reference(key, x, lengths=None, **kw):
    """The oracle and the float32 restatement of an input, computed once and left unchanged."""
    if key not in _cache:
        _cache[key] = (S.all_pairs(x, lengths, **kw), S.all_pairs(x, lengths, dtype=torch.float32, **kw))
    return _cache[key]


def _widen(err, bound):
    """The factor a bar is widened by: 4 x the float32 restatement's error / bound where that is above 1."""
    return max(1.0, 4.0 * float((err / bound).max()))


def _check(what, out, ref, r32):
    """tm, rmsd and offset of the entry against the oracle, over the pairs the oracle calls well-posed; returns the worst error / bound."""
    M = ref['tm'].shape[0]
    assert all(tuple(out[k].shape) == (M, M) and out[k].device.type == 'cuda' for k in ('tm', 'rmsd', 'offset'))
    assert out['tm'].dtype == torch.float32 and out['rmsd'].dtype == torch.float32 and out['offset'].dtype == torch.int32
    upper = torch.triu(torch.ones(M, M, dtype=torch.bool), 1)
    well = ref['gap'] >= 1e-4
    n_pairs = max(int(upper.sum()), 1)
    left_out = int((upper & ~well).sum()), int((upper & ~(well & (ref['margin'] >= 1e-4))).sum())
    assert max(left_out) <= 0.05 * n_pairs, '%s: %s of %d pairs are ill-posed: take another seed' % (what, left_out, n_pairs)
    worst = {}
    for k in ('tm', 'rmsd'):
        v, r = out[k].double().cpu(), ref[k]
        assert bool(torch.isfinite(v).all()), (what, k)
        bound = BAR * r.abs().clamp(min=1.0)
        widen = _widen((r32[k].double() - r).abs()[well], bound[well])
        ratio = ((v - r).abs() / (bound * widen))[well]
        worst[k] = float(ratio.max())
        print('%s: %s error / bound %.3f (bar x%.2f, %d of %d pairs left out)' % (what, k, worst[k], widen, left_out[0], n_pairs))
        assert worst[k] <= 1.0, (what, k, worst[k])
    sure = well & (ref['margin'] >= 1e-4)
    differ = int((out['offset'].cpu().long() != ref['offset'])[sure].sum())
    print('%s: %d offsets differ (%d of %d pairs left out)' % (what, differ, left_out[1], n_pairs))
    assert differ == 0, (what, out['offset'].cpu(), ref['offset'])
    return worst


# ---- parity with the oracle ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', S.EQUAL_N)
def test_equal_lengths_match_the_float64_oracle(entry, N):
    x = S.designs(N)
    ref, r32 = _reference(('equal', N), x)
    _check('N%d' % N, entry(x), ref, r32)
    off = ref['tm'][~torch.eye(12, dtype=torch.bool)]
    if N >= 63:
        assert float(off.min()) < 0.2 and float(off.max()) > 0.95           # the set spans unrelated walks to near-copies


def test_the_longest_chain_matches_the_float64_oracle(entry):
    x = S.designs(S.LONG_N, M=2)
    ref, r32 = _reference('long', x)
    _check('N%d' % S.LONG_N, entry(x), ref, r32)


@pytest.mark.parametrize('norm', ('shorter', 'longer'))
def test_mixed_lengths_match_the_float64_oracle(entry, norm):
    x, lengths = S.mixed_designs()
    ref, r32 = _reference(('mixed', norm), x, lengths, norm=norm)
    _check('mixed-%s' % norm, entry(x, lengths, norm=norm), ref, r32)
    assert int(ref['offset'][0, 3]) == 7 and int(ref['offset'][1, 6]) == 40     # the excerpts are found where they were cut
    assert float(ref['tm'][0, 3]) > 2 * float(ref['tm'][0, 4])


# ---- structure of the output ---------------------------------------------------------------------------------------------------------

def test_diagonal_symmetry_determinism_and_padding(entry):
    x, lengths = S.mixed_designs()
    a, b = entry(x, lengths), entry(x, lengths)
    M = len(lengths)
    for k in ('tm', 'rmsd', 'offset'):
        assert bool((a[k] == a[k].T).all()), k                                  # exactly symmetric
        assert bool((a[k] == b[k]).all()), k                                    # two calls: the same bits
    assert bool((a['tm'].diagonal() == 1).all()) and bool((a['rmsd'].diagonal() == 0).all()) and bool((a['offset'].diagonal() == 0).all())
    assert bool((a['tm'][~torch.eye(M, dtype=torch.bool, device='cuda')] < 1).all())
    # what lies beyond a design's length never reaches the result
    g = torch.Generator().manual_seed(1)
    junk = x.clone()
    for m, L in enumerate(lengths):
        junk[m, L:] = 1e3 * torch.randn(x.shape[1] - L, 3, generator=g)
    junk[0, lengths[0]] = float('nan')
    junk[1, -1] = float('inf')
    c = entry(junk, lengths)
    for k in ('tm', 'rmsd', 'offset'):
        assert bool((a[k] == c[k]).all()), k
    # equal lengths too, and a set of one
    x = S.designs(65)
    a, b = entry(x), entry(x)
    assert all(bool((a[k] == b[k]).all()) and bool((a[k] == a[k].T).all()) for k in a)
    one = entry(x[:1])
    assert one['tm'].tolist() == [[1.0]] and one['rmsd'].tolist() == [[0.0]] and one['offset'].tolist() == [[0]]
    same = entry(torch.stack([x[0], x[0]]))
    assert float(same['tm'][0, 1]) > 0.999999 and float(same['rmsd'][0, 1]) < 1e-4     # a design against itself


# ---- invariances ---------------------------------------------------------------------------------------------------------------------

def test_rigid_motion_and_permutation(entry):
    x = S.designs(64)
    ref, _ = _reference(('equal', 64), x)
    assert float(ref['gap'][~torch.eye(12, dtype=torch.bool)].min()) >= 1e-4      # every pair of this set is well-posed
    base = entry(x)
    y = x.clone()
    y[3] = S.moved(x[3], 77)
    moved = entry(y)
    for k in ('tm', 'rmsd'):
        d = (moved[k] - base[k]).abs().double().cpu() / (BAR * ref[k].abs().clamp(min=1.0))
        print('rigid motion of one design: %s change / bar %.3f' % (k, float(d.max())))
        assert float(d.max()) <= 1.0, k
    # a permutation of the designs permutes the matrices (of equal lengths the lower index moves: the fit is the inverse one)
    perm = torch.tensor([5, 0, 11, 3, 7, 1, 9, 2, 10, 4, 8, 6])
    got = entry(x[perm])
    for k in ('tm', 'rmsd'):
        want = base[k][perm.cuda()][:, perm.cuda()]
        d = (got[k] - want).abs().double().cpu() / (BAR * ref[k][perm][:, perm].abs().clamp(min=1.0))
        print('permutation: %s change / bar %.3f' % (k, float(d.max())))
        assert float(d.max()) <= 1.0, k
    x, lengths = S.mixed_designs()
    ref, _ = _reference(('mixed', 'shorter'), x, lengths, norm='shorter')
    perm = torch.tensor([6, 2, 0, 5, 3, 1, 4])
    base, got = entry(x, lengths), entry(x[perm], [lengths[int(p)] for p in perm])
    sure = ((ref['gap'] >= 1e-4) & (ref['margin'] >= 1e-4))[perm][:, perm]
    assert bool((got['offset'].cpu() == base['offset'].cpu()[perm][:, perm])[sure].all())
    d = (got['tm'].cpu() - base['tm'].cpu()[perm][:, perm]).abs().double() / BAR
    print('permutation of the mixed set: tm change / bar %.3f' % float(d[sure].max()))
    assert float(d[sure].max()) <= 1.0


def test_iteration_counts(entry):
    x = S.designs(65)
    one = _reference(('equal', 65, 1), x, n_iter=1)
    _check('N65-n_iter1', entry(x, n_iter=1), *one)
    full, _ = _reference(('equal', 65), x)
    assert float((full['tm'] - one[0]['tm']).max()) > 1e-2                        # the ascent moves these scores: 1 is not 16
    t1, t4, t16 = (entry(x, n_iter=n)['tm'] for n in (1, 4, 16))
    assert bool((t4 >= t1).all()) and bool((t16 >= t4).all())                     # the same first steps, bit for bit, then more
    assert bool((t16 > t1).any())
    t32 = entry(x, n_iter=32)['tm']
    assert bool((t32 >= t16).all())


# ---- known answers -------------------------------------------------------------------------------------------------------------------

def _two(entry, a, b, **kw):
    N = max(len(a), len(b))
    x = torch.zeros(2, N, 3)
    x[0, :len(a)], x[1, :len(b)] = a, b
    out = entry(x, [len(a), len(b)], **kw)
    return float(out['tm'][0, 1]), float(out['rmsd'][0, 1]), int(out['offset'][0, 1])


def test_known_answers_on_the_device(entry):
    tm, rmsd, _ = _two(entry, *S.core_pair())
    assert 0.75 <= tm < 0.76 and rmsd > 20                                        # the 48 / 64 core; plain Kabsch is far off
    tm, _, _ = _two(entry, *S.mirror_pair())
    assert 0.2 < tm < 0.6                                                         # a mirror image does not fit
    tm, rmsd, offset = _two(entry, *S.threading_pair())
    assert tm >= 0.999 and offset == 7 and rmsd < 1e-3
    a, b = S.threading_pair()
    assert _two(entry, b, a) == (tm, rmsd, offset)                                # the shorter chain moves, whichever comes first
    assert _two(entry, a, b, norm='longer')[0] <= 20 / 47 + 1e-6


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_entry_refusals_leave_the_next_call_working(entry):
    from genie2_amd import capi
    from genie2_amd.smc import _ptr
    x = S.designs(16, M=3).cuda()
    lengths = torch.full((3,), 16, dtype=torch.int32, device='cuda')
    good = entry._launch(x, lengths, 0, 16)
    big = torch.zeros(1, 1707, 3, device='cuda')
    for args, msg in (((big, torch.full((1,), 1707, dtype=torch.int32, device='cuda'), 0, 16), 'genie_pairwise_tm: N outside 4..1706'),
                      ((x, lengths, 0, 33), 'genie_pairwise_tm: n_iter outside 1..32'),
                      ((x, lengths, 2, 16), r'genie_pairwise_tm: norm is neither 0 \(shorter\) nor 1 \(longer\)')):
        with pytest.raises(capi.GenieError, match=msg):
            entry._launch(*args)
        again = entry._launch(x, lengths, 0, 16)
        assert all(bool((again[k] == good[k]).all()) for k in good)
    out = torch.empty(3, 3, device='cuda')
    with pytest.raises(capi.GenieError, match='genie_pairwise_tm: offset is NULL'):
        entry._call('genie_pairwise_tm', entry._stream(), 3, 16, _ptr(x), _ptr(lengths), 0, 16, _ptr(out), _ptr(out), _ptr(None))
    torch.cuda.synchronize()


# ---- the command line ----------------------------------------------------------------------------------------------------------------

def _write(folder, name, xyz):
    from genie2_amd import features as F
    f = F.create_empty_np_features([len(xyz)])
    f['atom_positions'] = xyz.double().numpy()
    F.save_np_features_to_pdb(f, os.path.join(folder, name + '.pdb'))


def _leader(tm, threshold):
    reps, labels = [], []
    for m in range(tm.shape[0]):
        hit = [c for c, r in enumerate(reps) if float(tm[m, r]) >= threshold]
        labels.append(hit[0] if hit else len(reps))
        if not hit:
            reps.append(m)
    return labels


def _read_clusters(path):
    header, rows = {}, []
    for line in open(path):
        if line.startswith('#'):
            _, k, v = line.split()
            header[k] = v
        else:
            name, length, cluster, rep, nearest, tm = line.split()
            rows.append((name, int(length), int(cluster), rep, nearest, tm))
    return header, rows


def test_cli_end_to_end(tmp_path):
    from genie2_amd import cluster_designs as CD
    run = tmp_path / 'run'
    os.makedirs(run / 'pdbs')
    fam_a, fam_b = S.walk(1, 40, 11)[0], S.walk(1, 40, 12)[0]
    designs = [('a%d' % k, S.moved(fam_a, 20 + k, 0.25)) for k in range(4)] + [('b%d' % k, S.moved(fam_b, 30 + k, 0.25)) for k in range(3)]
    designs += [('c0', S.walk(1, 40, 13)[0]), ('d0', S.walk(1, 30, 14)[0]), ('d1', S.moved(fam_a[5:35], 41, 0.2))]
    for name, xyz in designs:
        _write(str(run / 'pdbs'), name, xyz)
    names = sorted(n for n, _ in designs)
    # the oracle reads the files itself
    chains = [torch.tensor(_ca_coordinates(str(run / 'pdbs' / (n + '.pdb'))), dtype=torch.float32) for n in names]
    lengths = [len(c) for c in chains]
    x = torch.zeros(len(chains), max(lengths), 3)
    for m, c in enumerate(chains):
        x[m, :len(c)] = c
    ref = S.all_pairs(x, lengths)
    off = ~torch.eye(len(names), dtype=torch.bool)
    assert float((ref['tm'][off] - 0.6).abs().min()) > 1e-3                       # no pair sits on the threshold
    want = S.clusters_single(ref['tm'], 0.6)
    assert want == [0, 0, 0, 0, 1, 1, 1, 2, 3, 0]                                # a0-a3 with d1 (an excerpt of a), b0-b2, c0, d0

    p = CD.build_parser()
    summary = CD.main(p.parse_args(['--indir', str(run), '--write_matrix']))
    header, rows = _read_clusters(str(run / 'diversity' / 'clusters.txt'))
    assert list(header) == ['designs', 'threshold', 'norm', 'linkage', 'n_iter', 'clusters', 'diversity', 'mean_tm', 'max_tm']
    assert (header['designs'], header['threshold'], header['norm'], header['linkage'], header['n_iter'], header['clusters'], header['diversity']) == \
        ('10', '0.600', 'shorter', 'single', '16', '4', '0.400')
    assert header['mean_tm'] == '%.3f' % float(ref['tm'][off].mean()) and header['max_tm'] == '%.3f' % float(ref['tm'][off].max())
    assert [r[0] for r in rows] == names and [r[1] for r in rows] == lengths and [r[2] for r in rows] == want
    assert summary['n_clusters'] == 4 and summary['n_designs'] == 10
    near = torch.where(off, ref['tm'], torch.full_like(ref['tm'], -1.0)).argmax(dim=1)
    for m, r in enumerate(rows):
        assert r[4] == names[int(near[m])] and abs(float(r[5]) - float(ref['tm'][m, near[m]])) <= 1.1e-3, r
        members = [k for k in range(len(names)) if want[k] == want[m]]
        means = [float(ref['tm'][k][members].mean()) for k in members]
        assert r[3] == names[members[int(np.argmax(means))]], r
    z = np.load(str(run / 'diversity' / 'tm.npz'))
    assert z['names'].tolist() == names and z['lengths'].tolist() == lengths and bool(z['scored'].all())
    assert z['tm'].dtype == np.float32 and z['offset'].dtype == np.int32
    for k in ('tm', 'rmsd'):                                                      # the oracle read the same files: the ordinary bar
        d = np.abs(z[k] - ref[k].numpy()) / (BAR * np.maximum(1.0, np.abs(ref[k].numpy())))
        print('tm.npz: %s error / bound %.3f' % (k, float(d.max())))
        assert float(d.max()) <= 1.0, k
    assert bool((z['offset'] == ref['offset'].numpy()).all()) and int(z['offset'][names.index('d1'), names.index('a0')]) == 5

    # leader linkage, a folder that holds the files itself, another output folder
    out2 = tmp_path / 'leader'
    CD.main(p.parse_args(['--indir', str(run / 'pdbs'), '--outdir', str(out2), '--linkage', 'leader', '--tm_threshold', '0.6']))
    header, rows = _read_clusters(str(out2 / 'clusters.txt'))
    assert header['linkage'] == 'leader' and [r[2] for r in rows] == _leader(ref['tm'], 0.6) and not os.path.exists(out2 / 'tm.npz')
    assert all(r[3] == names[[k for k in range(len(names)) if rows[k][2] == r[2]][0]] for r in rows)      # the founder stands for a cluster

    # every length on its own: d1 no longer reaches the a family, d0 and d1 are scored against each other alone
    out3 = tmp_path / 'same'
    CD.main(p.parse_args(['--indir', str(run), '--outdir', str(out3), '--same_length_only', '--write_matrix']))
    header, rows = _read_clusters(str(out3 / 'clusters.txt'))
    same = torch.tensor(lengths)[:, None] == torch.tensor(lengths)[None, :]
    tm_same = torch.where(same, ref['tm'], torch.zeros_like(ref['tm']))
    assert [r[2] for r in rows] == S.clusters_single(tm_same, 0.6) == [0, 0, 0, 0, 1, 1, 1, 2, 3, 4] and header['clusters'] == '5'
    assert header['mean_tm'] == '%.3f' % float(ref['tm'][same & off].mean())
    assert rows[names.index('d1')][4] == 'd0' and rows[names.index('d0')][4] == 'd1'
    z = np.load(str(out3 / 'tm.npz'))
    assert bool((z['scored'] == same.numpy()).all()) and bool((z['tm'][~same.numpy()] == 0).all())
    assert float(np.abs(z['tm'] - tm_same.numpy()).max()) <= BAR
