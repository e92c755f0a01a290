"""The host side of the gapped TM alignment (genie2_amd/similarity.py: TMAlign and the call planner; novelty.py; cluster_designs.py
--align) and the float64 oracle of tests/_tmalign.py, without a GPU: the oracle's own properties (never below its seed, a table that
without a gap penalty is the plain monotone alignment, the known answers), the entry's declaration and export, every refusal that is
made before the device is looked at and every refusal of the C entry, the report writer and the chunking on hand-made inputs, and both
parsers."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import _similarity as S
import _tmalign as T
from genie2_amd import features as F


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

def test_oracle_is_never_below_its_seed_and_finds_the_gaps():
    xq, lq, xr, lr = T.family(24)
    ref = T.all_pairs(xq[:3], lq[:3], xr[:6], lr[:6])
    assert bool((ref['tm'] >= ref['stage0']).all())
    assert float(ref['tm'][0, 0]) > float(ref['stage0'][0, 0]) + 0.2             # the indel relative gains from the gaps
    zero = T.all_pairs(xq[:3], lq[:3], xr[:6], lr[:6], n_rounds=0)
    assert bool((zero['tm'] == ref['stage0']).all()) and bool((zero['rounds'] == 0).all())
    assert bool((zero['path_margin'] == math.inf).all()) and bool((zero['stage_lead'] == math.inf).all())
    tm, rmsd, n = T.rescore(xq[:3], lq[:3], xr[:6], lr[:6], ref['map'], ref['rot'], ref['trans'], 'query')
    assert float((tm - ref['tm']).abs().max()) < 1e-12 and float((rmsd - ref['rmsd']).abs().max()) < 1e-10      # its own certificate
    assert bool((n == ref['n_aligned']).all())


@pytest.mark.parametrize('shape', ((5, 5), (7, 19), (19, 7), (24, 31)))
def test_table_without_a_penalty_is_the_plain_monotone_alignment(shape):
    g = torch.Generator().manual_seed(shape[0] * 100 + shape[1])
    Sc = torch.rand(shape, generator=g, dtype=torch.float64) ** 4                  # mostly small scores: gaps pay
    move, lead = T.fill(Sc, 0.0)
    ia, ib, _ = T.traceback(move, lead, *shape)
    assert all(b > a for a, b in zip(ia, ia[1:])) and all(b > a for a, b in zip(ib, ib[1:]))
    want = T.plain_monotone(Sc)
    assert float(Sc[ia, ib].sum()) == pytest.approx(want, abs=1e-12) and T.table_value(Sc, 0.0) == pytest.approx(want, abs=1e-12)
    # with a penalty the vectorised fill still follows the statement's double loop, and never gains
    move, lead = T.fill(Sc, -0.6)
    ia, ib, _ = T.traceback(move, lead, *shape)
    opened = sum(1 for k in range(1, len(ia)) if ia[k] != ia[k - 1] + 1) + sum(1 for k in range(1, len(ib)) if ib[k] != ib[k - 1] + 1)
    assert T.table_value(Sc, -0.6) <= want + 1e-12
    assert float(Sc[ia, ib].sum()) - 0.6 * opened <= T.table_value(Sc, -0.6) + 1e-9


def test_oracle_known_answers():
    a = T.walk(1, 70, 7000)[0]
    same = T.align(a, a)
    assert float(same['tm']) > 0.999999 and same['map'] == list(range(70)) and same['rounds'] == 1
    th = T.align(*S.threading_pair())
    assert float(th['tm']) >= 0.999 and th['map'] == [7 + i for i in range(20)] and th['rounds'] == 1
    a, b = T.insertion_pair()
    assert float(S.pair(a, b)['tm']) < 0.6
    ins = T.align(a, b)
    assert float(ins['tm']) >= 0.999 and ins['n_aligned'] == 64 and ins['map'] == list(range(32)) + [i + 10 for i in range(32, 64)]
    assert float(ins['stage0']) == float(S.pair(a, b)['tm'])                       # stage 0 is 7.8's score
    back = T.align(b, a, norm='reference')                                         # the long chain as the query: the map is inverted
    assert float(back['tm']) == pytest.approx(float(ins['tm']), abs=1e-12)
    assert back['map'] == list(range(32)) + [-1] * 10 + list(range(32, 64))
    x = b.double() @ back['rot'].T + back['trans']
    assert float((x[[j for j in range(74) if back['map'][j] >= 0]] - a.double()).norm(dim=-1).max()) < 1e-4


# ---- declaration and export ----------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_and_exported(lib):
    from genie2_amd import build, capi
    assert 'tmalign_kernels.hip' in build.SOURCES and os.path.exists(os.path.join(os.path.dirname(build.__file__), 'csrc', 'tmalign_kernels.hip'))
    res, args = capi.SYMBOLS['genie_tm_align']
    assert res is C.c_int and len(args) == 20 and args[12] is C.c_float and args.count(C.c_void_p) == 12
    assert lib.genie_tm_align is not None
    assert (capi.TMALIGN_MAX_LENGTH, capi.TMALIGN_MAX_CELLS, capi.TMALIGN_MAX_ROUNDS) == (1024, 131072, 16) and T.MAX_CELLS == 131072
    header = open(os.path.join(os.path.dirname(build.__file__), '..', 'include', 'genie_hip.h')).read()
    for line in ('#define GENIE_TMALIGN_MAX_LENGTH 1024', '#define GENIE_TMALIGN_MAX_CELLS  131072', '#define GENIE_TMALIGN_MAX_ROUNDS 16',
                 'int genie_tm_align(genie_stream_t stream, int M, int Nq, const float* xq', 'The reference has no counterpart.'):
        assert line in header, line
    assert len(capi.SYMBOLS['genie_pairwise_tm'][1]) == 10                         # (the neighbour keeps its arguments)


def test_entry_refuses_before_any_launch(lib):
    """The argument checks of the C entry need no device: every one returns GENIE_E_ARG with its message."""
    one = C.c_void_p(16)                                            # (never dereferenced: the entry refuses first)
    ok = dict(M=2, Nq=16, xq=one, lq=one, R=3, Nr=20, xr=one, lr=one, norm=0, n_iter=16, n_rounds=8, gap_open=-0.6, tm=one, rmsd=one,
              n_aligned=one, rounds=one, map=one, rot=one, trans=one)
    cases = ((dict(M=0), 'M outside 1..65535'), (dict(M=65536), 'M outside 1..65535'), (dict(R=0), 'R outside 1..65535'),
             (dict(R=65536), 'R outside 1..65535'), (dict(Nq=3), 'Nq outside 4..1024'), (dict(Nq=1025), 'Nq outside 4..1024'),
             (dict(Nr=3), 'Nr outside 4..1024'), (dict(Nr=1025), 'Nr outside 4..1024'), (dict(Nq=363, Nr=362), 'Nq * Nr above 131072 cells'),
             (dict(Nq=129, Nr=1024), 'Nq * Nr above 131072 cells'), (dict(norm=4), 'norm outside 0..3'), (dict(norm=-1), 'norm outside 0..3'),
             (dict(n_iter=0), 'n_iter outside 1..32'), (dict(n_iter=33), 'n_iter outside 1..32'), (dict(n_rounds=-1), 'n_rounds outside 0..16'),
             (dict(n_rounds=17), 'n_rounds outside 0..16'), (dict(gap_open=0.1), 'gap_open is not a finite number in -10..0'),
             (dict(gap_open=-10.5), 'gap_open is not a finite number'), (dict(gap_open=math.nan), 'gap_open is not a finite number'),
             (dict(gap_open=-math.inf), 'gap_open is not a finite number'), (dict(xq=None), 'xq is NULL'), (dict(lq=None), 'lq is NULL'),
             (dict(xr=None), 'xr is NULL'), (dict(lr=None), 'lr is NULL'), (dict(tm=None), 'tm is NULL'), (dict(rmsd=None), 'rmsd is NULL'),
             (dict(n_aligned=None), 'n_aligned is NULL'), (dict(rounds=None), 'rounds is NULL'),
             (dict(rot=None), 'rot and trans are given together or not at all'), (dict(trans=None), 'rot and trans are given together or not at all'))
    for change, msg in cases:
        a = dict(ok, **change)
        rc = lib.genie_tm_align(None, a['M'], a['Nq'], a['xq'], a['lq'], a['R'], a['Nr'], a['xr'], a['lr'], a['norm'], a['n_iter'], a['n_rounds'],
                                a['gap_open'], a['tm'], a['rmsd'], a['n_aligned'], a['rounds'], a['map'], a['rot'], a['trans'])
        assert rc == -1, change
        assert lib.genie_last_error(None).decode().startswith('genie_tm_align: ' + msg), (change, lib.genie_last_error(None))


# ---- refusals before the device is looked at --------------------------------------------------------------------------------------------

class _NoDevice:
    """TMAlign without a device: __call__ must refuse before it reaches _launch."""

    def __new__(cls):
        from genie2_amd.similarity import TMAlign
        e = TMAlign.__new__(TMAlign)
        e.device = torch.device('cpu')
        e._launch = lambda *a, **k: pytest.fail('the entry was launched')
        return e


def test_call_refuses_on_the_host():
    e = _NoDevice()
    xq, lq, xr, lr = T.family(24)
    for bad, msg in ((xq[0], r'xq must be \[M >= 1, N, 3\]'), (xq[:, :, :2], r'xq must be \[M >= 1, N, 3\]'), (xq[:0], r'xq must be \[M >= 1, N, 3\]'),
                     (xq[:, :3], 'xq: N must be at least 4 residues, got 3'), (xq.long(), 'xq must have a floating dtype')):
        with pytest.raises(ValueError, match=msg):
            e(bad, None, xr, lr)
    for bad, msg in ((xr[0], r'xr must be \[M >= 1, N, 3\]'), (xr.int(), 'xr must have a floating dtype')):
        with pytest.raises(ValueError, match=msg):
            e(xq, lq, bad, lr)
    for bad, msg in (([24] * 5, 'xq: lengths must hold 6 integers'), ([24] * 5 + [3], 'xq: every length must be in 4..24'),
                     ([24] * 5 + [25], r'xq: every length must be in 4\.\.24 \(N\): design 5 has 25'), ([24.0] * 6, 'xq: lengths must hold 6 integers')):
        with pytest.raises(ValueError, match=msg):
            e(xq, bad, xr, lr)
    with pytest.raises(ValueError, match='xr: lengths must hold 12 integers'):
        e(xq, lq, xr, lr[:5])
    with pytest.raises(ValueError, match='xq: a chain has 1025 residues, the gapped alignment takes 4..1024'):
        e(torch.zeros(1, 1025, 3), None, xr, lr)
    with pytest.raises(ValueError, match=r'the longest query \(363\) times the longest reference \(362\) is above 131072 cells'):
        e(torch.zeros(1, 363, 3), None, torch.zeros(2, 400, 3), [362, 100])
    for bad in ('both', 0, None):
        with pytest.raises(ValueError, match='norm must be one of'):
            e(xq, lq, xr, lr, norm=bad)
    for bad in (0, 33, 16.0, True, None):
        with pytest.raises(ValueError, match=r'n_iter must be an integer in 1\.\.32'):
            e(xq, lq, xr, lr, n_iter=bad)
    for bad in (-1, 17, 8.0, True, None):
        with pytest.raises(ValueError, match=r'n_rounds must be an integer in 0\.\.16'):
            e(xq, lq, xr, lr, n_rounds=bad)
    for bad in (0.1, -10.5, math.nan, -math.inf, None, 'x', True):
        with pytest.raises(ValueError, match=r'gap_open must be a number in -10\.\.0'):
            e(xq, lq, xr, lr, gap_open=bad)
    with pytest.raises(ValueError, match='return_alignment must be a bool'):
        e(xq, lq, xr, lr, return_alignment=1)
    for v in (math.nan, math.inf):
        y = xr.clone()
        y[0, 5, 1] = v
        with pytest.raises(ValueError, match='xr holds a NaN or an infinity inside a chain'):
            e(xq, lq, y, lr)
        y = xq.clone()
        y[2, 23, 0] = v
        with pytest.raises(ValueError, match='xq holds a NaN or an infinity inside a chain'):
            e(y.numpy(), lq, xr, lr)
        with pytest.raises(pytest.fail.Exception, match='the entry was launched'):      # beyond the chain's length nothing is read
            e(y, [24, 24, 23, 24, 24, 24], xr, lr)
    # the cell limit speaks of the longest chains in use, not of the padding
    with pytest.raises(pytest.fail.Exception, match='the entry was launched'):
        e(torch.zeros(1, 500, 3), [300], torch.zeros(1, 500, 3), [400])


def test_cpu_device_is_refused(lib):
    from genie2_amd import capi
    from genie2_amd.similarity import TMAlign
    with pytest.raises(capi.GenieError, match='genie_tm_align runs on the GPU'):
        TMAlign('cpu')


def test_padding_is_trimmed_before_the_launch():
    from genie2_amd.similarity import ALIGN_NORMS, TMAlign
    assert ALIGN_NORMS == ('query', 'reference', 'shorter', 'longer') == T.NORMS
    e = TMAlign.__new__(TMAlign)
    e.device = torch.device('cpu')
    seen = {}

    def launch(xq, lq, xr, lr, norm, n_iter, n_rounds, gap_open, alignment):
        seen.update(xq=xq, lq=lq, xr=xr, lr=lr, scalars=(norm, n_iter, n_rounds, gap_open, alignment))
        return {'tm': torch.zeros(2, 3), 'map': torch.zeros(2, 3, xq.shape[1], dtype=torch.int32)}
    e._launch = launch
    out = e(torch.ones(2, 50, 3, dtype=torch.float64), [20, 31], torch.ones(3, 70, 3), [9, 44, 12], norm='longer', n_rounds=3, gap_open=-1,
            return_alignment=True)
    assert tuple(seen['xq'].shape) == (2, 31, 3) and tuple(seen['xr'].shape) == (3, 44, 3) and seen['xq'].dtype == torch.float32
    assert seen['lq'].tolist() == [20, 31] and seen['lr'].tolist() == [9, 44, 12] and seen['lq'].dtype == torch.int32
    assert seen['scalars'] == (3, 16, 3, -1.0, True)
    assert tuple(out['map'].shape) == (2, 3, 50) and bool((out['map'][:, :, 31:] == -1).all())      # map speaks of the caller's Nq


# ---- the chunking and the report writer ------------------------------------------------------------------------------------------------

def test_length_chunks_and_the_call_plan():
    from genie2_amd.similarity import length_chunks, plan_calls
    assert length_chunks([100, 40, 41, 300, 60, 99]) == [[1, 2, 4], [5, 0], [3]]     # sorted by length, cut where padding would grow
    assert length_chunks([]) == [] and length_chunks([7]) == [[0]]
    lq, lr = [100, 120, 300, 1000], [60, 64, 400, 1024, 130, 500]
    calls, skipped = plan_calls(lq, lr)
    seen = np.zeros((len(lq), len(lr)), dtype=int)
    for qc, rc in calls:
        assert max(lq[q] for q in qc) * max(lr[r] for r in rc) <= 131072
        seen[np.ix_(qc, rc)] += 1
    fits = np.array([[a * b <= 131072 for b in lr] for a in lq])
    assert bool((seen == fits).all()) and skipped == int((~fits).sum()) == 5       # every pair that fits exactly once, the others counted
    calls, skipped = plan_calls([50, 52], [40, 45, 50])
    assert calls == [([0, 1], [0, 1, 2])] and skipped == 0                         # one call where everything fits
    calls, skipped = plan_calls([10, 12], [10, 11], max_cells=120)
    assert skipped == 1 and sorted((tuple(q), tuple(r)) for q, r in calls) == [((0,), (0, 1)), ((1,), (0,))]


def test_report_writer_on_hand_made_matrices(tmp_path):
    from genie2_amd.novelty import HEADER, nearest_references, write_report
    tm = np.array([[0.30, 0.72, 0.72, 0.10], [0.20, 0.49, 0.10, 0.95], [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    scored = np.array([[1, 1, 1, 1], [1, 1, 1, 0], [0, 0, 0, 0]], dtype=bool)
    assert nearest_references(tm, scored).tolist() == [1, 1, -1]                   # ties to the lowest index; unscored pairs do not count
    out = {'tm': tm, 'n_aligned': np.full((3, 4), 17, dtype=np.int32), 'rmsd': np.full((3, 4), 2.5, dtype=np.float32)}
    path = str(tmp_path / 'novelty.txt')
    s = write_report(path, ['d0', 'd1', 'd2'], [50, 60, 70], ['r0', 'r1', 'r2', 'r3'], [40, 55, 66, 900], out, scored, 5, 'query', 16, 8, -0.6, 0.5)
    assert (s['n_designs'], s['n_references'], s['n_novel'], s['skipped_pairs']) == (3, 4, 2, 5) and s['novel'].tolist() == [False, True, True]
    lines = open(path).read().splitlines()
    assert lines[:10] == ['# designs 3', '# references 4', '# norm query', '# n_iter 16', '# n_rounds 8', '# gap_open -0.6', '# threshold 0.500',
                          '# novel 2', '# novelty 0.667', '# skipped_pairs 5'] and [ln.split()[1] for ln in lines[:10]] == list(HEADER)
    assert lines[10:] == ['d0 50 r1 55 0.720 17 2.500 0', 'd1 60 r1 55 0.490 17 2.500 1', 'd2 70 - 0 0.000 0 0.000 1']
    s = write_report(path, ['d0'], [50], ['r0'], [40], {k: v[:1, :1] for k, v in out.items()}, scored[:1, :1], 0, 'shorter', 4, 0, 0.0, 0.3)
    assert open(path).read().splitlines()[2:9] == ['# norm shorter', '# n_iter 4', '# n_rounds 0', '# gap_open 0', '# threshold 0.300', '# novel 0',
                                                   '# novelty 0.000']             # at the threshold is not below it
    with pytest.raises(ValueError, match='tm and scored must be'):
        nearest_references(tm, scored[:2])


def test_symmetrise():
    from genie2_amd.cluster_designs import symmetrise
    out = {'tm': np.array([[0.9, 0.4, 0.2], [0.5, 0.8, 0.3], [0.2, 0.1, 0.7]], dtype=np.float32),
           'rmsd': np.array([[0.1, 4.0, 2.0], [5.0, 0.2, 3.0], [2.5, 1.0, 0.3]], dtype=np.float32),
           'n_aligned': np.array([[9, 4, 2], [5, 8, 3], [6, 1, 7]], dtype=np.int32)}
    sym = symmetrise(out)
    assert bool((sym['tm'] == np.array([[1, 0.5, 0.2], [0.5, 1, 0.3], [0.2, 0.3, 1]], dtype=np.float32)).all())
    assert sym['rmsd'].tolist() == [[0.0, 5.0, 2.0], [5.0, 0.0, 3.0], [2.0, 3.0, 0.0]]       # from the direction that won; ties: the upper one
    assert sym['n_aligned'][0, 1] == sym['n_aligned'][1, 0] == 5 and sym['n_aligned'][0, 2] == sym['n_aligned'][2, 0] == 2


# ---- the parsers ---------------------------------------------------------------------------------------------------------------------

def _pdb(folder, name, L):
    f = F.create_empty_np_features([L])
    f['atom_positions'] = S.walk(1, L, 1)[0].double().numpy() * 0.01              # (kept inside the PDB columns)
    F.save_np_features_to_pdb(f, os.path.join(str(folder), name + '.pdb'))


def test_novelty_parser_and_its_refusals(tmp_path):
    from genie2_amd import novelty as NV
    import genie.novelty as thin
    assert thin.main is NV.main and thin.build_parser is NV.build_parser
    p = NV.build_parser()
    a = p.parse_args(['--indir', 'out', '--refdir', 'known'])
    assert (a.outdir, a.tm_threshold, a.norm, a.n_iter, a.n_rounds, a.gap_open, a.write_alignments, a.device) == \
        (None, 0.5, 'query', 16, 8, -0.6, False, 'cuda:0')
    for argv in ([], ['--indir', 'out'], ['--indir', 'out', '--refdir', 'k', '--norm', 'mean']):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    designs, known = tmp_path / 'designs', tmp_path / 'known'
    designs.mkdir()
    known.mkdir()
    base = ['--indir', str(designs), '--refdir', str(known)]
    for argv, msg in ((['--tm_threshold', '0'], 'tm_threshold must be above 0 and at most 1'), (['--tm_threshold', '1.5'], 'tm_threshold must be'),
                      (['--tm_threshold', 'nan'], 'tm_threshold must be'), (['--n_iter', '0'], r'n_iter must be in 1\.\.32, got 0'),
                      (['--n_iter', '33'], r'n_iter must be in 1\.\.32'), (['--n_rounds', '-1'], r'n_rounds must be in 0\.\.16, got -1'),
                      (['--n_rounds', '17'], r'n_rounds must be in 0\.\.16'), (['--gap_open', '0.5'], r'gap_open must be in -10\.\.0'),
                      (['--gap_open', '-11'], r'gap_open must be in -10\.\.0'), (['--gap_open', 'nan'], r'gap_open must be in -10\.\.0')):
        with pytest.raises(SystemExit, match=msg):
            NV.main(p.parse_args(base + argv))
    with pytest.raises(SystemExit, match='is not a directory'):
        NV.main(p.parse_args(['--indir', str(tmp_path / 'missing'), '--refdir', str(known)]))
    with pytest.raises(SystemExit, match='no .pdb files in .*designs'):
        NV.main(p.parse_args(base))
    _pdb(designs, 'd0', 12)
    with pytest.raises(SystemExit, match='no .pdb files in .*known'):
        NV.main(p.parse_args(base))
    with pytest.raises(SystemExit, match='is not a directory'):
        NV.main(p.parse_args(['--indir', str(designs), '--refdir', str(tmp_path / 'missing')]))
    _pdb(known, 'short', 3)
    with pytest.raises(SystemExit, match='short has 3 residues: a reference needs 4..1024'):
        NV.main(p.parse_args(base))
    _pdb(known, 'short', 1025)
    with pytest.raises(SystemExit, match='short has 1025 residues: a reference needs 4..1024'):
        NV.main(p.parse_args(base))
    _pdb(known, 'short', 12)
    _pdb(designs, 'd0', 3)
    with pytest.raises(SystemExit, match='d0 has 3 residues: a design needs 4..1024'):
        NV.main(p.parse_args(base))


def test_cluster_designs_align_switch(tmp_path):
    from genie2_amd import cluster_designs as CD
    p = CD.build_parser()
    a = p.parse_args(['--indir', 'out'])
    assert (a.align, a.n_rounds, a.gap_open) == ('gapless', 8, -0.6)
    a = p.parse_args(['--indir', 'out', '--align', 'gapped', '--n_rounds', '3', '--gap_open', '-1.5'])
    assert (a.align, a.n_rounds, a.gap_open) == ('gapped', 3, -1.5)
    with pytest.raises(SystemExit):
        p.parse_args(['--indir', 'out', '--align', 'local'])
    (tmp_path / 'pdbs').mkdir()
    _pdb(tmp_path / 'pdbs', 'long', 363)
    _pdb(tmp_path / 'pdbs', 'ok', 40)
    for argv, msg in ((['--n_rounds', '17'], r'n_rounds must be in 0\.\.16, got 17'), (['--gap_open', '1'], r'gap_open must be in -10\.\.0'),
                      ([], 'the longest design has 363 residues, and its square is above the 131072 cells')):
        with pytest.raises(SystemExit, match=msg):
            CD.main(p.parse_args(['--indir', str(tmp_path), '--align', 'gapped'] + argv))
    CD.check_args(p.parse_args(['--indir', 'out', '--n_rounds', '17']))              # gapless does not look at the gapped scalars
