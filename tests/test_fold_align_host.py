"""The aligned fold potential without a device: the float64 oracle of tests/_fold_align.py against tests/_tmalign.py's alignment at
stride 1, against central differences of its own log p with the alignment held fixed, against its autograd form and on known answers;
AlignedFoldPotential's host side, both command lines' flags, the reference and length filters under --fold_align gapped, the report
writer in both forms, and the C entry's declaration, export, work size and refusals (genie_fold_align_potential, include/genie_hip.h).

What holds the kernel to the oracle is tests/test_fold_align_gpu.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import _fold_align as Fa
import _similarity as S
import _tmalign as Ta
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')
TEMPLATE = os.path.join(GOLDEN, 'dataset_100_0.pdb')     # 100 residues

# The fixed-alignment, fixed-fit gradient against central differences of the converged log p (polish of n_iter = 200, h = 1e-5 A, the
# alignment held): the worst error measured over FD_CASES on the CPU is 4.2e-9 of the largest entry; the tolerance is
# 4 x that.
FD_TOLERANCE = 1.7e-8
# (N, L, bounds row): an indel relative at 40 against 45 under an active lower hinge; 48 against 40, the reference moving, upper hinge
FD_CASES = [(40, 45, (0.95, math.inf, 1.0)), (48, 40, (0.0, 0.1, 1.0))]


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

def test_oracle_at_stride_1_is_the_gapped_alignment():
    """The restated search finds tests/_tmalign.py's map and transform on a family's pairs, and the polish only ascends."""
    xq, lq, xr, lr = Ta.family(24)
    for m, r in ((0, 0), (1, 1), (2, 8), (5, 5), (3, 11), (4, 6)):
        for norm in ('query', 'longer'):
            q, y = xq[m, :lq[m]], xr[r, :lr[r]]
            want = Ta.align(q, y, norm=norm)
            got = Fa.search(q, y, norm=norm)
            assert got['map'] == want['map'] and got['n_aligned'] == want['n_aligned'], (m, r, norm)
            assert torch.equal(got['rot0'], want['rot']) and torch.equal(got['trans0'], want['trans']) and torch.equal(got['tm'], want['tm'])
            lnorm = Fa.lnorm_of(norm, len(q), len(y))
            polished = Fa.polish(q, y, got['map'], got['rot0'], got['trans0'], lnorm, 16)
            assert float(polished['n']) / lnorm >= float(want['tm']) - 1e-12, (m, r, norm)
            assert abs(float(torch.linalg.det(polished['rot'])) - 1) < 1e-12
    assert Fa.offsets_of(9, 1) == list(range(9)) and Fa.offsets_of(9, 4) == [0, 4, 8] and Fa.offsets_of(8, 3) == [0, 3, 6, 7]
    assert Fa.offsets_of(1, 5) == [0] and Fa.offsets_of(3, 64) == [0, 2]


def _fd_pair(N, L):
    x = Fa.particles(1, N, 7)
    return x, [Fa.relative(x[0], L, 4100 + N, 0.5)]


@pytest.mark.parametrize('N,L,row', FD_CASES)
def test_oracle_fixed_alignment_gradient_matches_central_differences(N, L, row):
    """With the alignment held and the polish converged (n_iter = 200, the oracle only) the gradient with the fit held fixed is the total
    derivative of log p on the alignment's piece (envelope theorem): central differences of the oracle's own log p, every one of them
    polishing afresh from the same T*."""
    x, refs = _fd_pair(N, L)
    bounds, var = torch.tensor([row], dtype=torch.float64), 0.5
    found = Fa.search_all(x, refs)
    held = (found['map'], found['rot0'], found['trans0'])
    ref = Fa.evaluate(x, refs, bounds, var, *held, n_iter=200)
    assert float((ref['below'] + ref['above']).max()) > 0 and 3 <= int(found['n_aligned']) and float(ref['tm']) > 0.3
    unaligned = found['map'][0, 0] < 0
    assert bool(unaligned.any()) and bool((ref['grad'][0][unaligned] == 0).all())      # a cut, or the longer particle: exactly 0 there
    h, xd = 1e-5, x.double()
    rows = list(range(xd.numel()))
    steps = h * torch.eye(xd.numel(), dtype=torch.float64).reshape(-1, N, 3)
    both = torch.cat([xd + steps, xd - steps])                          # one batch, every particle under the same held alignment
    lp = Fa.evaluate(both, refs, bounds, var, *(t.expand(len(both), *t.shape[1:]) for t in held), n_iter=200)['logp']
    fd = (lp[:len(rows)] - lp[len(rows):]) / (2 * h)
    scale = float(ref['grad'].abs().max())
    err = float((ref['grad'].reshape(-1)[rows] - fd).abs().max()) / scale
    print('N = %d, L = %d, TM %.3f, %d aligned: fixed-alignment gradient against central differences %.2e of the largest entry'
          % (N, L, float(ref['tm']), int(found['n_aligned']), err))
    assert scale > 0 and err <= FD_TOLERANCE


def test_oracle_exact_behaviour_and_the_autograd_form():
    x = Fa.particles(2, 48, 3)
    refs = Fa.references(x, (40, 48, 55), 3)
    bounds = torch.tensor([[0.6, math.inf, 2.0], [0.0, 0.5, 0.5], [0.3, 0.4, 1.0]], dtype=torch.float64)
    r = Fa.reference(x, refs, bounds, 0.7)
    assert r['lnorm'].tolist() == [48.0, 48.0, 48.0] and bool(((r['below'] > 0) | (r['above'] > 0)).any())
    e = (bounds[:, 2] * (r['below'] ** 2 + r['above'] ** 2)).sum(dim=1)
    assert torch.allclose(r['e_fold'], e, rtol=1e-13) and torch.allclose(r['logp'], -e / 1.4, rtol=1e-13) and bool((e > 0).all())
    assert torch.equal(r['tm_nearest'], r['tm'].amax(dim=1)) and torch.equal(r['tm_lowest_wanted'], torch.minimum(r['tm'][:, 0], r['tm'][:, 2]))
    assert bool((r['tm'] >= r['search']['tm'] - 1e-12).all())           # the polish only ascends
    # an unaligned residue gets exactly 0: the 40-residue reference alone leaves at least 8 of the particle's 48 out
    one = Fa.reference(x, refs[:1], torch.tensor([[0.99, math.inf, 1.0]]), 0.7)
    out = one['search']['map'][:, 0] < 0
    assert bool((one['below'] > 0).all()) and int(out.sum()) >= 16 and bool((one['grad'][out] == 0).all())
    assert bool((one['grad'][~out].abs().amax(dim=1) > 0).all())
    # other norms: Lnorm and d0 are per reference
    assert Fa.reference(x, refs, bounds, 0.7, norm='reference')['lnorm'].tolist() == [40.0, 48.0, 55.0]
    assert Fa.reference(x, refs, bounds, 0.7, norm='shorter')['lnorm'].tolist() == [40.0, 48.0, 48.0]
    # hi = inf is the upper hinge absent; weights 0 remove energy and force; an inactive reference contributes exactly 0
    open_ = bounds.clone()
    open_[:, 1] = math.inf
    a, b = Fa.reference(x, refs, open_, 0.7), Fa.reference(x, refs, bounds, 0.7, upper=False)
    assert torch.equal(a['logp'], b['logp']) and torch.equal(a['grad'], b['grad']) and bool((a['above'] == 0).all())
    off = Fa.reference(x, refs, torch.tensor([[0.6, math.inf, 0.0], [0.0, 0.5, 0.0], [0.3, 0.4, 0.0]]), 0.7)
    assert bool((off['logp'] == 0).all()) and bool((off['grad'] == 0).all())
    idle = Fa.reference(x, refs, torch.tensor([[0.0, 1.0, 1.0], [0.0, math.inf, 1.0], [0.0, 1.0, 3.0]]), 0.7)
    assert bool((idle['logp'] == 0).all()) and bool((idle['grad'] == 0).all()) and idle['n_fold_violations'].tolist() == [0, 0]
    # the autograd form (alignment and fit not recorded) is the same function and the same derivative
    xg = x.double().requires_grad_(True)
    lp = Fa.logp(xg, refs, bounds, 0.7)
    g, = torch.autograd.grad(lp.sum(), xg)
    assert torch.allclose(lp.detach(), r['logp'], rtol=1e-12, atol=0) and float((g - r['grad']).abs().max()) <= 1e-12 * float(r['grad'].abs().max())
    r32 = Fa.reference(x, refs, bounds, 0.7, dtype=torch.float32)
    assert r32['grad'].dtype == torch.float32 and torch.allclose(r32['logp'].double(), r['logp'], rtol=1e-3)


def test_oracle_sees_through_an_inserted_excursion():
    """A rigidly moved copy with a 10-residue excursion spliced in: all 64 residues align and superpose, where the gapless score of the
    same pair stops at about one half."""
    a, b = Ta.insertion_pair()
    r = Fa.reference(a[None], [b], torch.tensor([[0.0, 0.5, 1.0]]), 1.0)
    assert float(r['tm']) >= 0.999 and int(r['search']['n_aligned']) == 64 and float(r['above']) > 0
    assert r['search']['map'][0, 0].tolist() == list(range(32)) + list(range(42, 74))
    # the last offset is always visited: an excerpt that ends the reference, under a stride that does not divide its offset
    long = Ta.walk(1, 61, 8800)[0]
    tail = S.moved(long[-24:], 8801)
    for stride in (1, 5, 64):
        assert Fa.offsets_of(61 - 24 + 1, stride)[-1] == 37
        one = Fa.reference(tail[None], [long], torch.tensor([[0.0, 0.5, 1.0]]), 1.0, stride=stride)
        assert float(one['tm']) >= 0.999 and one['search']['map'][0, 0].tolist() == list(range(37, 61)), stride


def test_parity_inputs_pass_the_oracles_conditions():
    """The small certificate cases of test_fold_align_gpu.py on the CPU: shapes, the oracle's conditions (an active lower and upper
    hinge, no n_r within 1e-4 Lnorm of an active bound) and no particle left out."""
    for case in Fa.CASES[:5]:
        B, N, lengths = case
        x, refs, bounds = Fa.inputs(case)
        assert tuple(x.shape) == (B, N, 3) and [len(y) for y in refs] == list(lengths) and x.dtype == torch.float32
        r64 = Fa.reference(x, refs, bounds, 0.8)
        Fa.check_inputs(r64, len(lengths))
        assert not bool(Fa.left_out(r64).any()), case
        maps = r64['search']['map']
        for b in range(B):
            for r, L in enumerate(lengths):
                hit = maps[b, r][maps[b, r] >= 0]
                assert bool((hit[1:] > hit[:-1]).all()) and int(hit.max()) < L and len(hit) == int(r64['search']['n_aligned'][b, r])


# ---- AlignedFoldPotential's host side ------------------------------------------------------------------------------------------------

def test_constructor_validates_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import AlignedFoldPotential
    import genie.sampler.fold as mirror
    assert mirror.AlignedFoldPotential is AlignedFoldPotential
    abar = torch.linspace(0.999, 0.001, 13)
    refs = [Fa.particles(1, 45, 1)[0], Fa.particles(1, 36, 2)[0]]
    ok = [(0.6, math.inf), (0.0, 0.5, 2.0)]
    inf, nan = math.inf, math.nan
    make = lambda references=refs, bounds=ok, n_res=40, **kw: AlignedFoldPotential(n_res, abar, references, bounds, device='cpu', **kw)      # noqa: E731
    for n_res in (3, 1025, 0, 40.0, True):
        with pytest.raises(ValueError, match=r'n_res must be an integer in 4\.\.1024'):
            make(n_res=n_res)
    for bad, msg in (('file.pdb', 'references must be a list'), ([refs[0], refs[1][:, :2]], r'reference 1 must be \[L, 3\]'),
                     ([refs[0][None]], r'reference 0 must be \[L, 3\]'), ([], 'references must hold 1..1024 backbones, got 0'),
                     ([refs[0]] * 1025, 'references must hold 1..1024 backbones, got 1025'),
                     ([refs[0], refs[1][:3]], r'reference 1 has 3 residues, the gapped alignment takes 4\.\.1024'),
                     ([torch.zeros(1025, 3), refs[1]], 'reference 0 has 1025 residues')):
        with pytest.raises(ValueError, match=msg):
            make(bad, ok[:max(1, min(len(bad), 2))] if not isinstance(bad, str) and len(bad) <= 2 else [(0.0, 0.5)] * len(bad))
    with pytest.raises(ValueError, match=r'reference 1 has 400 residues: n_res \(400\) times that is above 131072 cells'):
        make([refs[0], torch.zeros(400, 3)], n_res=400)
    for v in (nan, inf):
        bad = refs[1].clone()
        bad[3, 2] = v
        with pytest.raises(ValueError, match='reference 1 has a coordinate that is not finite'):
            make([refs[0], bad])
    # the padded form: [R, Nr, 3] with lengths=; what lies beyond a length is never looked at
    padded = torch.full((2, 50, 3), nan)
    padded[0, :45], padded[1, :36] = refs[0], refs[1]
    for lengths, msg in (([45], 'lengths must hold one integer per reference'), ([45, 36.0], 'lengths must hold one integer'),
                         ([45, 51], 'lengths holds 51, references has 50 rows'), ([45, 3], 'reference 1 has 3 residues')):
        with pytest.raises(ValueError, match=msg):
            make(padded, lengths=lengths)
    with pytest.raises(ValueError, match=r'references must be \[R, Nr, 3\] where lengths is given'):
        make(padded[0], lengths=[45])
    with pytest.raises(ValueError, match='reference 0 has a coordinate that is not finite'):
        make(padded, lengths=[46, 36])
    for bounds, msg in ((ok[:1], '1 rows for 2 references'), (5.0, 'bounds must hold'), ([(0.6, 0.5), (0, 0.5)], r'bounds of reference 0 must be \(lo, hi\)'),
                        ([(0.6, inf), (0, 0.5, nan)], 'weight of reference 1')):
        with pytest.raises(ValueError, match=msg):
            make(bounds=bounds)
    for norm in ('Query', 0, None, 'length'):
        with pytest.raises(ValueError, match='norm must be one of'):
            make(norm=norm)
    for n_iter in (0, 33, 16.0, True, None):
        with pytest.raises(ValueError, match=r'n_iter must be an integer in 1\.\.32'):
            make(n_iter=n_iter)
    for n_rounds in (-1, 17, 8.0, True, None):
        with pytest.raises(ValueError, match=r'n_rounds must be an integer in 0\.\.16'):
            make(n_rounds=n_rounds)
    for gap_open in (0.1, -10.5, nan, True, None, 'x'):
        with pytest.raises(ValueError, match=r'gap_open must be a number in -10\.\.0'):
            make(gap_open=gap_open)
    for stride in (0, 65, 2.0, True, None):
        with pytest.raises(ValueError, match=r'offset_stride must be an integer in 1\.\.64'):
            make(offset_stride=stride)
    for tausq in (0.0, -1.0, inf, nan, 'x'):
        with pytest.raises(ValueError, match='tausq must be finite and > 0'):
            make(tausq=tausq)
    with pytest.raises(ValueError, match='no term enabled'):
        make(bounds=[(0.6, inf, 0.0), (0.0, 0.5, 0.0)])
    # what is allowed gets as far as the device: a CPU potential is a GenieError
    for kw in (dict(), dict(references=[y.double().numpy() for y in refs]), dict(references=padded, lengths=[45, 36]),
               dict(references=padded, lengths=torch.tensor([45, 36])), dict(norm='longer', n_iter=1, n_rounds=0, gap_open=0, offset_stride=64),
               dict(references=[torch.zeros(1024, 3) + torch.arange(1024)[:, None]], bounds=[(0.0, 0.5)], n_res=128)):
        with pytest.raises(capi.GenieError, match='AlignedFoldPotential runs on the GPU'):
            make(**kw)
    from genie2_amd.smc import FoldPotential
    for doc in (AlignedFoldPotential.__doc__, FoldPotential.__doc__):
        assert 'design choices' in doc and 'unmeasured' in doc and 'Not built' in doc
    assert 'AlignedFoldPotential' in FoldPotential.__doc__ and 'piecewise constant' in AlignedFoldPotential.__doc__


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

BASE = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']


def _write_design(path, xyz):
    from genie2_amd import features as F
    f = F.create_empty_np_features([len(xyz)])
    f['atom_positions'] = np.asarray(xyz, dtype=np.float64)
    F.save_np_features_to_pdb(f, str(path))


def _avoid_dir(tmp_path, lengths=(40, 40, 50, 40, 1100, 900)):
    d = tmp_path / 'run'
    (d / 'pdbs').mkdir(parents=True)
    for m, L in enumerate(lengths):
        _write_design(d / 'pdbs' / ('%d_%d.pdb' % (L, m)), Fa.particles(1, L, 10 + m)[0].numpy() * 0.5)
    return d


def test_parsers_and_constants(tmp_path):
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    d = _avoid_dir(tmp_path, (40, 50))
    defaults = dict(fold_align='gapless', fold_norm='query', fold_rounds=8, fold_gap_open=-0.6, fold_offset_stride=1)
    assert Sh.FOLD_ALIGN_DEFAULTS == defaults and not set(defaults) & set(Sh.FOLD_DEFAULTS)
    given = ['--template_pdb', TEMPLATE, '--fold_align', 'gapped', '--fold_norm', 'shorter', '--fold_rounds', '4', '--fold_gap_open', '-1',
             '--fold_offset_stride', '4']
    values = dict(template_pdb=TEMPLATE, fold_align='gapped', fold_norm='shorter', fold_rounds=4, fold_gap_open=-1.0, fold_offset_stride=4)
    for parser, more in ((Sh.build_parser(), []), (M.build_parser(), ['--motif_file', MOTIF])):
        a = vars(parser.parse_args(BASE + more))
        assert {k: a[k] for k in defaults} == defaults
        a = vars(parser.parse_args(BASE + more + given))
        assert {k: a[k] for k in values} == values
        for flags in (['--fold_align', 'local'], ['--fold_norm', 'mean'], ['--fold_rounds', '2.5'], ['--fold_offset_stride', 'x']):
            with pytest.raises(SystemExit):
                parser.parse_args(BASE + more + flags)
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + given)))
    assert {k: c[k] for k in values} == values and Sh.has_fold_terms(c) and Sh.fold_gapped(c)
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF, '--avoid_dir', str(d), '--fold_align', 'gapped'])))
    assert Sh.has_fold_terms(c) and Sh.fold_gapped(c) and len(c['fold']) == 2
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF])))
    assert {k: c[k] for k in defaults} == defaults and c['fold'] is None and not Sh.fold_gapped(c)
    assert not Sh.fold_gapped(Sh.fold_constants({})) and not Sh.fold_gapped({})
    # an alignment flag without --fold_align gapped says so, in both CLIs; a gapped run without a reference too; values out of range
    for flags in (['--fold_norm', 'longer'], ['--fold_rounds', '4'], ['--fold_gap_open', '-1'], ['--fold_offset_stride', '2']):
        with pytest.raises(SystemExit, match='an alignment flag needs --fold_align gapped'):
            Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + ['--template_pdb', TEMPLATE] + flags)))
        with pytest.raises(SystemExit, match='an alignment flag needs --fold_align gapped'):
            M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF, '--avoid_dir', str(d)] + flags)))
    with pytest.raises(SystemExit, match='--fold_align: a fold flag needs --template_pdb or --avoid_dir'):
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + ['--fold_align', 'gapped'])))
    for flags, msg in ((['--fold_rounds', '-1'], r'fold_rounds must be in 0\.\.16'), (['--fold_rounds', '17'], 'fold_rounds must be'),
                       (['--fold_gap_open', '0.5'], r'fold_gap_open must be in -10\.\.0'), (['--fold_gap_open', '-11'], 'fold_gap_open must be'),
                       (['--fold_gap_open', 'nan'], 'fold_gap_open must be'), (['--fold_offset_stride', '0'], r'fold_offset_stride must be in 1\.\.64'),
                       (['--fold_offset_stride', '65'], 'fold_offset_stride must be'), (['--fold_iterations', '33'], 'fold_iterations must be')):
        with pytest.raises(SystemExit, match=msg):
            Sh.fold_constants(vars(Sh.build_parser().parse_args(BASE + ['--template_pdb', TEMPLATE, '--fold_align', 'gapped'] + flags)))
    # the message of a run with no term still ends as tests/test_symmetry_host.py reads it
    with pytest.raises(SystemExit, match='no shape term.*--symmetry$'):
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE)))


def test_fold_references_and_lengths_under_gapped(tmp_path, capsys):
    from genie2_amd import sample_unconditional_shape as Sh
    d = _avoid_dir(tmp_path)
    tasks = [{'length': L} for L in (40, 45, 100, 140, 2000)]
    parse = lambda flags: Sh.fold_constants(vars(Sh.build_parser().parse_args(BASE + flags)))      # noqa: E731
    assert Sh.fold_fits(1024, 128) and Sh.fold_fits(362, 362) and not Sh.fold_fits(1024, 129) and not Sh.fold_fits(3, 40) and not Sh.fold_fits(40, 1025)
    # gapless, as before: own length only
    c = parse(['--avoid_dir', str(d)])
    assert [t['length'] for t in Sh.fold_lengths(tasks, c)] == [40]
    assert capsys.readouterr().out == 'skipping lengths without a fold reference of their own length: 45, 100, 140, 2000\n'
    assert [r['name'] for r in Sh.fold_references(c, 40)] == ['40_0', '40_1', '40_3']
    c = parse(['--template_pdb', TEMPLATE, '--avoid_dir', str(d)])
    assert [t['length'] for t in Sh.fold_lengths(tasks, c)] == [100] and Sh.fold_references(c, 40) == []
    assert capsys.readouterr().out == 'skipping lengths without a fold reference of their own length: 40, 45, 140, 2000\n'
    # gapped: every reference that fits applies at every length; the 1100-residue backbone never does, the 900-residue one up to 145
    c = parse(['--avoid_dir', str(d), '--fold_align', 'gapped'])
    assert [r['name'] for r in Sh.fold_references(c, 45)] == ['40_0', '40_1', '40_3', '50_2', '900_5']
    assert [r['name'] for r in Sh.fold_references(c, 146)] == ['40_0', '40_1', '40_3', '50_2'] and Sh.fold_references(c, 2000) == []
    assert [t['length'] for t in Sh.fold_lengths(tasks, c)] == [40, 45, 100, 140]
    assert capsys.readouterr().out == ('skipping lengths without a fold reference that fits them: 2000\n' + ''.join(
        'length %d: 1 avoided backbones dropped (outside 4..1024 residues or above 131072 cells)\n' % L for L in (40, 45, 100, 140)))
    # a template of another length is now kept; where it does not fit, the length is skipped whatever the folder holds
    c = parse(['--template_pdb', TEMPLATE, '--avoid_dir', str(d), '--fold_align', 'gapped'])
    assert [r['name'] for r in Sh.fold_references(c, 40)] == ['dataset_100_0', '40_0', '40_1', '40_3', '50_2', '900_5']
    assert [r['name'] for r in Sh.fold_references(c, 1024)] == ['dataset_100_0', '40_0', '40_1', '40_3', '50_2']
    long_tasks = [{'length': L} for L in (40, 1024, 1400)]
    assert [t['length'] for t in Sh.fold_lengths(long_tasks, c)] == [40, 1024]
    assert capsys.readouterr().out == ('skipping lengths without a fold reference that fits them: 1400\n'
                                       'length 40: 1 avoided backbones dropped (outside 4..1024 residues or above 131072 cells)\n'
                                       'length 1024: 2 avoided backbones dropped (outside 4..1024 residues or above 131072 cells)\n')
    assert [t['length'] for t in Sh.GuidedRunner().guided_lengths(tasks, vars(Sh.build_parser().parse_args(
        BASE + ['--avoid_dir', str(d), '--fold_align', 'gapped'])))] == [40, 45, 100, 140]
    capsys.readouterr()
    # weight 0 everywhere that fits: skipped; more than 1024 applicable references end the run
    zero = dict(c, fold=[dict(r, weight=0.0) if len(r['xyz']) < 900 else r for r in c['fold']])
    assert Sh.fold_references(zero, 200) == [] and len(Sh.fold_references(zero, 100)) == 6
    short = next(r for r in c['fold'] if r['name'] == '40_0')
    many = dict(c, fold=[dict(short, name='m%d' % k) for k in range(1025)])
    with pytest.raises(SystemExit, match='1025 fold references apply at 40 residues: at most 1024'):
        Sh.fold_lengths(tasks[:1], many)
    assert [t['length'] for t in Sh.fold_lengths(tasks[:2], dict(many, fold=many['fold'][:1024]))] == [40, 45]
    assert [t['length'] for t in Sh.fold_lengths(tasks[:1], dict(many, fold_align='gapless'))] == [40]      # (4096 of one length there)


def test_report_writer_in_both_forms(tmp_path):
    from genie2_amd import capi
    from genie2_amd import sample_unconditional_shape as Sh
    merged = {'rog': torch.tensor([12.3, 9.0]), 'tm_nearest': torch.tensor([0.71239, 0.3]), 'nearest': torch.tensor([1, 0]),
              'tm_lowest_wanted': torch.tensor([0.41251, 0.0]), 'n_fold_violations': torch.tensor([2, 0]), 'e_fold': torch.tensor([1234.5678, 0.0])}
    tm, names, ranges = torch.tensor([[0.41251, 0.71239], [0.3, 0.25]]), ['dataset_100_0', '40_1'], [(0.6, math.inf), (0.0, 0.5)]
    tail = 'tm_nearest 0.712\nnearest 1\ntm_lowest_wanted 0.413\nn_fold_violations 2\ne_fold 1234.568\n'
    Sh.write_fold_report(tm, names, ranges, Sh.report_fields(merged, capi.FOLD_REPORT), str(tmp_path / 'a'), 40, 4)
    assert (tmp_path / 'a' / '40_4.txt').read_text() == 'ref dataset_100_0 0.413 0.6 inf\nref 40_1 0.712 0 0.5\n' + tail
    Sh.write_fold_report(tm, names, ranges, Sh.report_fields(merged, capi.FOLD_REPORT), str(tmp_path / 'b'), 40, 4, [100, 40],
                         torch.tensor([[38, 40], [12, 9]], dtype=torch.int32))
    assert sorted(os.listdir(tmp_path / 'b')) == ['40_4.txt', '40_5.txt']
    assert (tmp_path / 'b' / '40_4.txt').read_text() == 'ref dataset_100_0 0.413 0.6 inf 100 38\nref 40_1 0.712 0 0.5 40 40\n' + tail
    assert (tmp_path / 'b' / '40_5.txt').read_text().splitlines()[:3] == ['ref dataset_100_0 0.300 0.6 inf 100 12', 'ref 40_1 0.250 0 0.5 40 9',
                                                                        'tm_nearest 0.300']


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_exported(lib):
    from genie2_amd import build, capi
    csrc = os.path.join(os.path.dirname(build.__file__), 'csrc')
    assert 'fold_align_kernels.hip' in build.SOURCES and os.path.exists(os.path.join(csrc, 'fold_align_kernels.hip'))
    res, args = capi.SYMBOLS['genie_fold_align_potential']
    assert res is C.c_int and args == ([C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_int, C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 12 + [C.c_size_t])
    assert capi.SYMBOLS['genie_fold_align_potential_work_bytes'] == (C.c_size_t, [C.c_int, C.c_int, C.c_int])
    assert lib.genie_fold_align_potential is not None and lib.genie_fold_align_potential_work_bytes is not None
    assert capi.FOLD_ALIGN_MAX_REFERENCES == 1024 and capi.FOLD_ALIGN_MAX_STRIDE == 64 and capi.TMALIGN_NORMS == Ta.NORMS
    header = open(os.path.join(os.path.dirname(build.__file__), '..', 'include', 'genie_hip.h')).read()
    for line in ('#define GENIE_FOLD_ALIGN_MAX_REFERENCES 1024', '#define GENIE_FOLD_ALIGN_MAX_STRIDE 64',
                 'int genie_fold_align_potential(genie_stream_t stream, int B, int N, const float* x0',
                 'size_t genie_fold_align_potential_work_bytes(int B, int N, int R);', 'piecewise constant in x'):
        assert line in header, line
    assert len(capi.SYMBOLS['genie_fold_potential'][1]) == 15 and len(capi.SYMBOLS['genie_tm_align'][1]) == 20      # (the neighbours keep theirs)
    wb = lib.genie_fold_align_potential_work_bytes                  # 4 B R (20 + N) bytes; 0 for sizes the entry refuses
    for B, N, R in ((1, 4, 1), (3, 64, 5), (8, 40, 300), (1, 1024, 1024), (65535, 4, 1)):
        assert wb(B, N, R) == 4 * B * R * (20 + N), (B, N, R)
    assert all(wb(*a) == 0 for a in ((0, 40, 1), (65536, 40, 1), (1, 3, 1), (1, 1025, 1), (1, 40, 0), (1, 40, 1025)))


def test_entry_refuses_before_any_launch(lib):
    """The argument checks of the C entry need no device: every one returns GENIE_E_ARG with its message."""
    d = C.c_void_p(64)                                              # (never dereferenced: the entry refuses first)
    names = ('logp', 'grad', 'report', 'tm', 'n_aligned', 'map', 'rot', 'trans', 'rot0', 'trans0')

    def call(B=2, N=40, x0=d, R=3, Nr=48, ref=d, lr=d, bounds=d, norm=0, n_iter=16, n_rounds=8, gap_open=-0.6, stride=1, var=d, work=d,
             work_bytes=1 << 30, **outs):
        ptrs = [outs.get(k, d) for k in names]
        rc = lib.genie_fold_align_potential(None, B, N, x0, R, Nr, ref, lr, bounds, norm, n_iter, n_rounds, gap_open, stride, var, *ptrs,
                                            work, work_bytes)
        return rc, lib.genie_last_error(None).decode()

    none = {k: None for k in names}
    for change, msg in ((dict(B=0), 'B outside 1..65535'), (dict(B=65536), 'B outside 1..65535'), (dict(N=3), 'N outside 4..1024'),
                        (dict(N=1025), 'N outside 4..1024'), (dict(Nr=3), 'Nr outside 4..1024'), (dict(Nr=1025), 'Nr outside 4..1024'),
                        (dict(N=363, Nr=362), 'N * Nr above 131072 cells'), (dict(N=129, Nr=1024), 'N * Nr above 131072 cells'),
                        (dict(R=0), 'R outside 1..GENIE_FOLD_ALIGN_MAX_REFERENCES (1024)'), (dict(R=1025), 'R outside'),
                        (dict(norm=-1), 'norm outside 0..3'), (dict(norm=4), 'norm outside 0..3'), (dict(n_iter=0), 'n_iter outside 1..32'),
                        (dict(n_iter=33), 'n_iter outside 1..32'), (dict(n_rounds=-1), 'n_rounds outside 0..16'), (dict(n_rounds=17), 'n_rounds outside 0..16'),
                        (dict(gap_open=0.1), 'gap_open is not a finite number in -10..0'), (dict(gap_open=-10.5), 'gap_open is not'),
                        (dict(gap_open=math.nan), 'gap_open is not'), (dict(stride=0), 'offset_stride outside 1..64'), (dict(stride=65), 'offset_stride outside 1..64'),
                        (dict(x0=None), 'x0 is NULL'), (dict(ref=None), 'ref is NULL'), (dict(lr=None), 'lr is NULL'), (dict(bounds=None), 'bounds is NULL'),
                        (dict(var=None), 'var is NULL'), (none, 'no output asked for'), (dict(logp=None), 'logp_out and grad_out are given together'),
                        (dict(grad=None), 'logp_out and grad_out are given together'), (dict(rot=None), 'rot_out and trans_out are given together'),
                        (dict(trans=None), 'rot_out and trans_out are given together'), (dict(rot0=None), 'rot0_out and trans0_out are given together'),
                        (dict(trans0=None), 'rot0_out and trans0_out are given together'), (dict(work=None), 'work is NULL or work_bytes below'),
                        (dict(work_bytes=4 * 2 * 3 * 60 - 1), 'work is NULL or work_bytes below'), (dict(work=C.c_void_p(66)), 'work not 4-byte aligned')):
        rc, text = call(**change)
        assert rc == -1 and text.startswith('genie_fold_align_potential: ' + msg), (change, rc, text)
    # what is allowed passes every check (and then fails on the device instead, with another code)
    if not torch.cuda.is_available():
        for kw in (dict(), dict(logp=None, grad=None), dict(none, tm=d), dict(none, map=d), dict(none, rot0=d, trans0=d), dict(work_bytes=4 * 2 * 3 * 60),
                   dict(N=4, Nr=4, R=1), dict(N=362, Nr=362), dict(N=128, Nr=1024, R=1024, work_bytes=1 << 40), dict(N=1024, Nr=128),
                   dict(norm=3, n_iter=1, n_rounds=0, gap_open=0.0, stride=64), dict(n_iter=32, n_rounds=16, gap_open=-10.0)):
            assert call(**kw)[0] != -1, kw


def test_cpu_device_is_refused(lib):
    from genie2_amd import capi
    from genie2_amd.smc import AlignedFoldPotential
    with pytest.raises(capi.GenieError, match='AlignedFoldPotential runs on the GPU'):
        AlignedFoldPotential(40, torch.linspace(0.999, 0.001, 13), [Fa.particles(1, 45, 0)[0]], [(0.6, math.inf)], device='cpu')
