"""The fold potential without a device: the float64 oracle of tests/_fold.py on known answers and against central differences of its
own score, the parity inputs against the oracle's own conditions, FoldPotential's host side, both command lines' flags, the length
filter, the reader of clusters.txt and the report writer, and the C entry's declaration, export and refusals (genie_fold_potential,
include/genie_hip.h).

What holds the kernel to the oracle is tests/test_fold_gpu.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import _fold as Fd
import _similarity as S
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')
TEMPLATE = os.path.join(GOLDEN, 'dataset_100_0.pdb')     # 100 residues

# The fixed-fit gradient against central differences of the converged score (n_iter = 200, h = 1e-5 A): the worst error measured over
# FD_CASES on the CPU is 6.1e-9 of the largest entry; the tolerance is 4 x that.
FD_TOLERANCE = 2.5e-8
FD_CASES = [(40, 0.3), (40, 0.8), (48, 1.2), (56, 1.8), (64, 1.0)]      # (N, noise in A per coordinate): TM about 0.3 to 0.9


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

def _one(x, y, n_iter=16, bounds=((0.0, 0.0, 1.0),), var=0.5):
    """The oracle on one pair under the row (0, 0, 1): E = n^2, so log p = -n^2 / (2 var) and the gradient is -(n / var) dn/dx."""
    return Fd.reference(x[None], y[None], torch.tensor(bounds), var, n_iter)


def test_oracle_known_answers():
    a = Fd.walk(64, 6400)
    same = _one(a, a.double() @ S.rotation(6401).T + torch.tensor([11.0, -7.0, 5.0], dtype=torch.float64))
    assert float(same['tm']) == pytest.approx(1.0, abs=1e-12)
    # the fit is exact, every e_n is 0: the gradient of the score vanishes although the upper hinge is fully active
    assert float(same['above']) == pytest.approx(64.0, abs=1e-9) and float(same['grad'].abs().max()) < 1e-9
    assert float(_one(*S.mirror_pair())['tm']) < 0.6                                # a mirror image is not a match
    core = _one(*S.core_pair())
    assert 0.75 <= float(core['tm']) < 0.76                                         # the 48 / 64 core
    # the last iteration's score is the largest of the ascent (7.8's value) to rounding: the ascent is monotone
    for x, y in (S.core_pair(), S.mirror_pair(), (a, S.moved(a, 3, 2.0))):
        trace, _, _ = S.ascend(x[None].double(), y[None].double(), torch.tensor([len(x)]), 16)
        last = _one(x, y)['n_seeds'][0, 0] / len(x)
        assert float((trace.amax(dim=2)[0] - last).abs().max()) <= 1e-12
        assert float(_one(x, y)['tm']) == pytest.approx(float(S.pair(x, y)['tm']), abs=1e-12)


def test_oracle_report_energy_and_limits():
    x = Fd.designs(2, 30)
    ref = torch.stack([S.moved(x[0], 1, 0.3), S.moved(x[1], 2, 1.0), Fd.walk(30, 77)])
    bounds = torch.tensor([[0.6, math.inf, 2.0], [0.0, 0.5, 0.5], [0.3, 0.4, 1.0]], dtype=torch.float64)
    r = Fd.reference(x, ref, bounds, 0.7)
    n, N = r['n'], 30
    below = torch.clamp(N * bounds[:, 0] - n, min=0)
    above = torch.stack([torch.zeros(2, dtype=torch.float64), torch.clamp(n[:, 1] - 15, min=0), torch.clamp(n[:, 2] - 12, min=0)], dim=1)
    e = (bounds[:, 2] * (below ** 2 + above ** 2)).sum(dim=1)
    assert torch.allclose(r['e_fold'], e, rtol=1e-13) and torch.allclose(r['logp'], -e / 1.4, rtol=1e-13) and bool((e > 0).all())
    assert r['nearest'].tolist() == [0, 1] and torch.equal(r['tm_nearest'], r['tm'].amax(dim=1))
    assert torch.equal(r['tm_lowest_wanted'], torch.minimum(r['tm'][:, 0], r['tm'][:, 2]))
    assert r['n_fold_violations'].tolist() == [int(v) for v in ((below > 0) | (above > 0)).sum(dim=1)]
    assert float(Fd.reference(x, ref[1:2], torch.tensor([[0.0, 0.5, 1.0]]), 1.0)['tm_lowest_wanted'].abs().max()) == 0.0      # no lo > 0
    # hi = inf is the upper hinge absent; weights 0 remove energy and force; an inactive reference contributes exactly 0
    open_ = bounds.clone()
    open_[:, 1] = math.inf
    a, b = Fd.reference(x, ref, open_, 0.7), Fd.reference(x, ref, bounds, 0.7, upper=False)
    assert torch.equal(a['logp'], b['logp']) and torch.equal(a['grad'], b['grad']) and bool((a['above'] == 0).all())
    off = Fd.reference(x, ref, torch.tensor([[0.6, math.inf, 0.0], [0.0, 0.5, 0.0], [0.3, 0.4, 0.0]]), 0.7)
    assert bool((off['logp'] == 0).all()) and bool((off['grad'] == 0).all())
    idle = Fd.reference(x, ref, torch.tensor([[0.0, 1.0, 1.0], [0.0, math.inf, 1.0], [0.0, 1.0, 3.0]]), 0.7)
    assert bool((idle['logp'] == 0).all()) and bool((idle['grad'] == 0).all()) and idle['n_fold_violations'].tolist() == [0, 0]
    # the autograd form of the restatement (fits not recorded) is the same function and the same derivative
    xg = x.double().requires_grad_(True)
    lp = Fd.logp(xg, ref.double(), bounds, 0.7)
    g, = torch.autograd.grad(lp.sum(), xg)
    assert torch.allclose(lp.detach(), r['logp'], rtol=1e-12) and float((g - r['grad']).abs().max()) <= 1e-12 * float(r['grad'].abs().max())
    r32 = Fd.restatement32(x, ref, bounds, 0.7)
    assert torch.allclose(r32['logp'].double(), r['logp'], rtol=1e-4) and r32['grad'].dtype == torch.float32


@pytest.mark.parametrize('N,noise', FD_CASES)
def test_oracle_fixed_fit_gradient_matches_central_differences(N, noise):
    """At a converged ascent (n_iter = 200, the oracle only) the gradient with the winning transform held fixed is the total derivative
    of the score (envelope theorem): central differences of the oracle's own log p, every one of them ascending afresh."""
    x = Fd.walk(N, 900 + N).double()
    y = S.moved(x, 901 + N, noise).double()
    bounds, var = ((0.0, 0.0, 1.0),), 0.5
    ref = _one(x, y, 200, bounds, var)
    assert 0.25 < float(ref['tm']) < 0.95
    h = 1e-5
    steps = h * torch.eye(x.numel(), dtype=torch.float64).reshape(-1, N, 3)
    lp = Fd.reference(torch.cat([x[None] + steps, x[None] - steps]), y[None], torch.tensor(bounds), var, 200)['logp']      # one batch
    fd = ((lp[:x.numel()] - lp[x.numel():]) / (2 * h)).reshape(N, 3)
    scale = float(ref['grad'].abs().max())
    err = float((ref['grad'][0] - fd).abs().max()) / scale
    print('N = %d, noise %.1f A, TM %.3f: fixed-fit gradient against central differences %.2e of the largest entry' % (N, noise, float(ref['tm']), err))
    assert err <= FD_TOLERANCE


def test_parity_inputs_pass_the_oracles_conditions():
    """Every parity case of test_fold_gpu.py, float64 oracle against float32 restatement on the CPU: the oracle's conditions hold
    (no n_r within 1e-4 N of an active bound, both hinges active), no more than 5 % of the particles are left out as ill-posed, and
    the restatement, which may pick another seed on a pair the rule calls well-posed, stays within a few bars of the oracle."""
    for case in Fd.CASES:
        x, ref, bounds = Fd.inputs(case)
        assert tuple(x.shape) == (case[0], case[1], 3) and tuple(ref.shape) == (case[2], case[1], 3) and x.dtype == ref.dtype == torch.float32
        assert float(x.mean(dim=1).abs().max()) < 1e-4
        r64 = Fd.reference(x, ref, bounds, 0.8)
        Fd.check_inputs(r64, case)
        out = Fd.left_out(r64)
        assert int(out.sum()) <= 0.05 * case[0], (case, out)
        if case[2] > 1 and case[1] >= 63:                               # (shorter chains: d0 is at its floor of 0.5 A, the span is narrower)
            assert float(r64['tm'].min()) < 0.35 and float(r64['tm'].max()) > 0.9, case
        r32 = Fd.restatement32(x, ref, bounds, 0.8)
        bar = 1e-5 * r64['grad'].abs().amax(dim=(1, 2))
        err = (r32['grad'].double() - r64['grad']).abs().amax(dim=(1, 2))
        assert bool((err[~out] <= 40 * bar[~out]).all()), (case, err / bar)


# ---- FoldPotential's host side ------------------------------------------------------------------------------------------------------

def test_constructor_validates_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import FoldPotential, check_fold_bounds
    import genie.sampler.fold as mirror
    assert mirror.FoldPotential is FoldPotential
    abar = torch.linspace(0.999, 0.001, 13)
    y = Fd.designs(2, 40)
    ok = [(0.6, math.inf), (0.0, 0.5, 2.0)]
    inf, nan = math.inf, math.nan
    for refs, msg in ((y[0], r'references must be \[R, 40, 3\]'), (y[:, :39], r'references must be \[R, 40, 3\]'), (y[:, :, :2], 'references must be'),
                      (y[:0], 'references must hold 1..4096 backbones, got 0'), ('file.pdb', 'references must be'),
                      (torch.zeros(4097, 40, 3), 'references must hold 1..4096 backbones, got 4097')):
        with pytest.raises(ValueError, match=msg):
            FoldPotential(40, abar, refs, ok[:len(refs)] if not isinstance(refs, str) else ok, device='cpu')
    for v in (nan, inf):
        bad = y.clone()
        bad[1, 3, 2] = v
        with pytest.raises(ValueError, match='references has a coordinate that is not finite'):
            FoldPotential(40, abar, bad, ok, device='cpu')
    for n_res in (3, 1707, 0, 40.0, True):
        with pytest.raises(ValueError, match=r'n_res must be an integer in 4\.\.1706'):
            FoldPotential(n_res, abar, y, ok, device='cpu')
    for bounds, msg in ((ok[:1], '1 rows for 2 references'), ([(0.6, inf), (0.5,)], 'one .* row per reference'), (5.0, 'bounds must hold'),
                        ([(0.6, inf), ('a', 'b')], 'bounds must hold'), ([(0.6, 0.5), (0, 0.5)], r'bounds of reference 0 must be \(lo, hi\)'),
                        ([(0.6, inf), (-0.1, 0.5)], 'bounds of reference 1'), ([(inf, inf), (0, 0.5)], 'bounds of reference 0'),
                        ([(0.6, nan), (0, 0.5)], 'bounds of reference 0'), ([(0.6, inf, -1.0), (0, 0.5)], 'weight of reference 0'),
                        ([(0.6, inf), (0, 0.5, inf)], 'weight of reference 1'), ([(0.6, inf), (0, 0.5, nan)], 'weight of reference 1')):
        with pytest.raises(ValueError, match=msg):
            FoldPotential(40, abar, y, bounds, device='cpu')
    for n_iter in (0, 33, 16.0, True, None):
        with pytest.raises(ValueError, match=r'n_iter must be an integer in 1\.\.32'):
            FoldPotential(40, abar, y, ok, n_iter=n_iter, device='cpu')
    for tausq in (0.0, -1.0, inf, nan, 'x'):
        with pytest.raises(ValueError, match='tausq must be finite and > 0'):
            FoldPotential(40, abar, y, ok, tausq=tausq, device='cpu')
    with pytest.raises(ValueError, match='no term enabled'):
        FoldPotential(40, abar, y, [(0.6, inf, 0.0), (0.0, 0.5, 0.0)], device='cpu')
    # what is allowed gets as far as the device: a CPU potential is a GenieError
    for refs, bounds in ((y, ok), (y.double().numpy(), torch.tensor([[0.6, inf, 1.0], [0.0, 0.5, 0.0]])), (y[:1], [(0.0, 0.0)]), (y[:1], [(1.0, 1.0, 3.0)])):
        with pytest.raises(capi.GenieError, match='FoldPotential runs on the GPU'):
            FoldPotential(40, abar, refs, bounds, device='cpu')
    assert check_fold_bounds(ok, 2).tolist() == [[0.6, inf, 1.0], [0.0, 0.5, 2.0]]
    doc = FoldPotential.__doc__
    assert 'design choices' in doc and 'unmeasured' in doc and 'Not built' in doc


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

BASE = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']


def _write_design(path, xyz):
    from genie2_amd import features as F
    f = F.create_empty_np_features([len(xyz)])
    f['atom_positions'] = np.asarray(xyz, dtype=np.float64)
    F.save_np_features_to_pdb(f, str(path))


def _avoid_dir(tmp_path, lengths=(40, 40, 50, 40)):
    d = tmp_path / 'run'
    (d / 'pdbs').mkdir(parents=True)
    for m, L in enumerate(lengths):
        _write_design(d / 'pdbs' / ('%d_%d.pdb' % (L, m)), Fd.walk(L, 10 + m).numpy() * 0.5)
    return d


def test_parsers_constants_and_the_no_term_message(tmp_path):
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    import genie.sample_unconditional_shape as mirror
    assert mirror.add_fold_arguments is Sh.add_fold_arguments and mirror.fold_potential is Sh.fold_potential
    d = _avoid_dir(tmp_path)
    defaults = dict(template_pdb=None, template_tm_min=0.6, template_weight=1.0, avoid_dir=None, avoid_tm_max=0.5, avoid_weight=1.0,
                    avoid_representatives=False, fold_iterations=16, fold_tausq=1.0, write_fold=False)
    assert Sh.FOLD_DEFAULTS == defaults
    given = ['--template_pdb', TEMPLATE, '--template_tm_min', '0.7', '--template_weight', '2', '--avoid_dir', str(d), '--avoid_tm_max', '0.4',
             '--avoid_weight', '0.5', '--fold_iterations', '8', '--fold_tausq', '4', '--write_fold']
    values = dict(template_pdb=TEMPLATE, template_tm_min=0.7, template_weight=2.0, avoid_dir=str(d), avoid_tm_max=0.4, avoid_weight=0.5,
                  avoid_representatives=False, fold_iterations=8, fold_tausq=4.0, write_fold=True)
    for parser, more in ((Sh.build_parser(), []), (M.build_parser(), ['--motif_file', MOTIF])):
        a = vars(parser.parse_args(BASE + more))
        assert {k: a[k] for k in defaults} == defaults
        assert a['rog_max'] is None and a['target_pdb'] is None and a['symmetry'] is None             # (the flags that were there)
        a = vars(parser.parse_args(BASE + more + given))
        assert {k: a[k] for k in values} == values

    # constants: a fold term is enough on its own for the shape CLI; the references arrive read and picklable, the template first
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + given)))
    assert {k: c[k] for k in values} == values and Sh.has_fold_terms(c)
    assert not (Sh.has_shape_terms(c) or Sh.has_secstruct_terms(c) or Sh.has_sheet_terms(c) or Sh.has_symmetry_terms(c) or Sh.has_binder_terms(c))
    refs = c['fold']
    assert [r['name'] for r in refs] == ['dataset_100_0', '40_0', '40_1', '40_3', '50_2']
    assert [(r['lo'], r['hi'], r['weight'], r['template']) for r in refs] == [(0.7, math.inf, 2.0, True)] + [(0.0, 0.4, 0.5, False)] * 4
    assert [r['xyz'].shape for r in refs] == [(100, 3), (40, 3), (40, 3), (40, 3), (50, 3)] and all(r['xyz'].dtype == np.float32 for r in refs)
    import pickle
    assert [r['name'] for r in pickle.loads(pickle.dumps(refs))] == [r['name'] for r in refs]
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF, '--avoid_dir', str(d)])))
    assert Sh.has_fold_terms(c) and len(c['fold']) == 4 and c['tausq'] == 0.012
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF])))
    assert {k: c[k] for k in defaults} == defaults and c['fold'] is None and not Sh.has_fold_terms(c)
    assert Sh.fold_potential(c, 60, None, 'cuda') is None                                      # no term: no potential, no device

    # a fold flag without a reference says so, in both CLIs; values out of range and folders that do not hold up end the run
    for flags in (['--template_tm_min', '0.7'], ['--avoid_tm_max', '0.4'], ['--avoid_weight', '2'], ['--avoid_representatives'],
                  ['--fold_iterations', '8'], ['--fold_tausq', '2'], ['--write_fold'], ['--template_weight', '3']):
        with pytest.raises(SystemExit, match='needs --template_pdb or --avoid_dir'):
            Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + flags)))
        with pytest.raises(SystemExit, match='needs --template_pdb or --avoid_dir'):
            M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF] + flags)))
    for flags, msg in ((['--template_tm_min', '0'], 'template_tm_min must be'), (['--template_tm_min', '1.5'], 'template_tm_min must be'),
                       (['--template_tm_min', 'nan'], 'template_tm_min must be'), (['--avoid_dir', str(d), '--avoid_tm_max', '1'], 'avoid_tm_max must be'),
                       (['--avoid_dir', str(d), '--avoid_tm_max', '-0.1'], 'avoid_tm_max must be'), (['--template_weight', '-1'], 'template_weight must be'),
                       (['--template_weight', '0'], 'every fold reference has weight 0'), (['--fold_iterations', '0'], r'fold_iterations must be in 1\.\.32'),
                       (['--fold_iterations', '33'], 'fold_iterations must be'), (['--fold_tausq', '0'], 'fold_tausq must be'),
                       (['--avoid_representatives'], 'needs --avoid_dir'), (['--avoid_dir', str(tmp_path / 'missing')], 'is not a directory'),
                       (['--avoid_dir', str(tmp_path)], 'no .pdb files in'), (['--avoid_dir', str(d), '--avoid_representatives'], 'clusters.txt')):
        with pytest.raises(SystemExit, match=msg):
            Sh.fold_constants(vars(Sh.build_parser().parse_args(BASE + ['--template_pdb', TEMPLATE] + flags)))
    with pytest.raises(SystemExit, match='template_pdb'):
        Sh.fold_constants(vars(Sh.build_parser().parse_args(BASE + ['--template_pdb', str(tmp_path / 'no_such_file.pdb')])))
    # the message of a run with no term names the fold flags, and still ends as tests/test_symmetry_host.py reads it
    with pytest.raises(SystemExit, match='no shape term.*--symmetry$') as info:
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE)))
    assert '--template_pdb' in str(info.value) and '--avoid_dir' in str(info.value) and '--target_pdb' in str(info.value)


def test_avoid_representatives_reads_clusters_txt(tmp_path):
    from genie2_amd import sample_unconditional_shape as Sh
    d = _avoid_dir(tmp_path)
    (d / 'diversity').mkdir()
    (d / 'diversity' / 'clusters.txt').write_text(
        '# designs 4\n# threshold 0.600\n# clusters 2\n'
        '40_0 40 0 40_1 40_1 0.812\n40_1 40 0 40_1 40_0 0.812\n50_2 50 1 50_2 - 0.000\n40_3 40 0 40_1 40_1 0.700\n')
    assert Sh.cluster_representatives(str(d / 'diversity' / 'clusters.txt')) == ['40_1', '50_2']
    c = Sh.fold_constants(vars(Sh.build_parser().parse_args(BASE + ['--avoid_dir', str(d), '--avoid_representatives'])))
    assert [r['name'] for r in c['fold']] == ['40_1', '50_2'] and all(not r['template'] and (r['lo'], r['hi']) == (0.0, 0.5) for r in c['fold'])
    (d / 'diversity' / 'clusters.txt').write_text('# designs 1\nother 40 0 other - 0.000\n')
    with pytest.raises(SystemExit, match='names no design of'):
        Sh.fold_constants(vars(Sh.build_parser().parse_args(BASE + ['--avoid_dir', str(d), '--avoid_representatives'])))


def test_fold_lengths(tmp_path, capsys):
    from genie2_amd import sample_unconditional_shape as Sh
    d = _avoid_dir(tmp_path)
    tasks = [{'length': L} for L in (40, 45, 50, 100)]
    parse = lambda flags: Sh.fold_constants(vars(Sh.build_parser().parse_args(BASE + flags)))      # noqa: E731
    assert Sh.fold_lengths(tasks, Sh.fold_constants({})) == tasks                                  # no term: every length
    # avoided backbones count at their own length only; a length without one is skipped, in one line
    c = parse(['--avoid_dir', str(d)])
    assert [t['length'] for t in Sh.fold_lengths(tasks, c)] == [40, 50]
    assert capsys.readouterr().out == 'skipping lengths without a fold reference of their own length: 45, 100\n'
    assert [r['name'] for r in Sh.fold_references(c, 40)] == ['40_0', '40_1', '40_3'] and [r['name'] for r in Sh.fold_references(c, 50)] == ['50_2']
    # a template of another length skips the length, as a blueprint does, whatever the folder holds
    c = parse(['--template_pdb', TEMPLATE, '--avoid_dir', str(d)])
    assert [t['length'] for t in Sh.fold_lengths(tasks, c)] == [100]
    assert capsys.readouterr().out == 'skipping lengths without a fold reference of their own length: 40, 45, 50\n'
    assert [r['name'] for r in Sh.fold_references(c, 100)] == ['dataset_100_0'] and Sh.fold_references(c, 40) == []
    # the guided runner applies it when it makes its tasks
    assert [t['length'] for t in Sh.GuidedRunner().guided_lengths(tasks, vars(Sh.build_parser().parse_args(BASE + ['--avoid_dir', str(d)])))] == [40, 50]
    # more than 4096 references of one length end the run
    many = dict(c, fold=[dict(name='r%d' % m, xyz=np.zeros((40, 3), dtype=np.float32), lo=0.0, hi=0.5, weight=1.0, template=False) for m in range(4097)])
    with pytest.raises(SystemExit, match='4097 fold references of 40 residues: at most 4096'):
        Sh.fold_lengths(tasks, many)
    assert [t['length'] for t in Sh.fold_lengths(tasks, dict(many, fold=many['fold'][:4096]))] == [40]


def test_report_writer(tmp_path):
    from genie2_amd import capi
    from genie2_amd import sample_unconditional_shape as Sh
    merged = {'rog': torch.tensor([12.3, 9.0]), 'tm_nearest': torch.tensor([0.71239, 0.3]), 'nearest': torch.tensor([1, 0]),
              'tm_lowest_wanted': torch.tensor([0.41251, 0.0]), 'n_fold_violations': torch.tensor([2, 0]), 'e_fold': torch.tensor([1234.5678, 0.0])}
    assert list(Sh.report_fields(merged, capi.FOLD_REPORT)) == list(capi.FOLD_REPORT)
    Sh.write_fold_report(torch.tensor([[0.41251, 0.71239], [0.3, 0.25]]), ['dataset_100_0', '40_1'], [(0.6, math.inf), (0.0, 0.5)],
                         Sh.report_fields(merged, capi.FOLD_REPORT), str(tmp_path / 'fold'), 40, 4)
    assert sorted(os.listdir(tmp_path / 'fold')) == ['40_4.txt', '40_5.txt']
    assert (tmp_path / 'fold' / '40_4.txt').read_text() == (
        'ref dataset_100_0 0.413 0.6 inf\nref 40_1 0.712 0 0.5\ntm_nearest 0.712\nnearest 1\ntm_lowest_wanted 0.413\nn_fold_violations 2\n'
        'e_fold 1234.568\n')
    assert (tmp_path / 'fold' / '40_5.txt').read_text().splitlines()[:3] == ['ref dataset_100_0 0.300 0.6 inf', 'ref 40_1 0.250 0 0.5', 'tm_nearest 0.300']


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_exported(lib):
    from genie2_amd import build, capi
    assert 'fold_kernels.hip' in build.SOURCES and os.path.exists(os.path.join(os.path.dirname(build.__file__), 'csrc', 'fold_kernels.hip'))
    res, args = capi.SYMBOLS['genie_fold_potential']
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_size_t]
    assert capi.SYMBOLS['genie_fold_potential_work_bytes'] == (C.c_size_t, [C.c_int, C.c_int, C.c_int])
    assert lib.genie_fold_potential is not None and lib.genie_fold_potential_work_bytes is not None
    assert capi.FOLD_REPORT == Fd.REPORT and len(capi.FOLD_REPORT) == 5 and capi.FOLD_COUNTS == Fd.COUNTS and capi.FOLD_MAX_REFERENCES == 4096
    header = open(os.path.join(os.path.dirname(build.__file__), '..', 'include', 'genie_hip.h')).read()
    for line in ('#define GENIE_FOLD_REPORT 5', '#define GENIE_FOLD_MAX_REFERENCES 4096',
                 'int genie_fold_potential(genie_stream_t stream, int B, int N, const float* x0', 'size_t genie_fold_potential_work_bytes(int B, int N, int R);'):
        assert line in header, line
    assert len(capi.SYMBOLS['genie_binder_potential'][1]) == 23 and len(capi.SYMBOLS['genie_pairwise_tm'][1]) == 10      # (the neighbours keep theirs)
    wb = lib.genie_fold_potential_work_bytes                       # 96 B R bytes; 0 for sizes the entry refuses
    for B, N, R in ((1, 4, 1), (3, 64, 5), (8, 40, 300), (1, 1706, 4096), (65535, 4, 1)):
        assert wb(B, N, R) == 96 * B * R, (B, N, R)
    assert all(wb(*a) == 0 for a in ((0, 40, 1), (1, 3, 1), (1, 1707, 1), (1, 40, 0), (1, 40, 4097)))


def test_entry_refuses_before_any_launch(lib):
    """The argument checks of the C entry need no device: every one returns GENIE_E_ARG with its message."""
    d = C.c_void_p(64)                                              # (never dereferenced: the entry refuses first)

    def call(B=2, N=40, x0=d, R=3, ref=d, bounds=d, n_iter=16, var=d, logp=d, grad=d, report=d, tm=d, work=d, work_bytes=1 << 30):
        rc = lib.genie_fold_potential(None, B, N, x0, R, ref, bounds, n_iter, var, logp, grad, report, tm, work, work_bytes)
        return rc, lib.genie_last_error(None).decode()

    for change, msg in ((dict(B=0), 'B outside 1..65535'), (dict(B=65536), 'B outside 1..65535'), (dict(N=3), 'N outside 4..1706'),
                        (dict(N=1707), 'N outside 4..1706'), (dict(R=0), 'R outside 1..GENIE_FOLD_MAX_REFERENCES (4096)'), (dict(R=4097), 'R outside'),
                        (dict(n_iter=0), 'n_iter outside 1..32'), (dict(n_iter=33), 'n_iter outside 1..32'), (dict(x0=None), 'x0 is NULL'),
                        (dict(ref=None), 'ref is NULL'), (dict(bounds=None), 'bounds is NULL'), (dict(var=None), 'var is NULL'),
                        (dict(logp=None, grad=None, report=None, tm=None), 'no output asked for'), (dict(logp=None), 'logp_out and grad_out are given together'),
                        (dict(grad=None), 'logp_out and grad_out are given together'), (dict(work=None), 'work is NULL or work_bytes below'),
                        (dict(work_bytes=96 * 2 * 3 - 1), 'work is NULL or work_bytes below'), (dict(work=C.c_void_p(66)), 'work not 4-byte aligned')):
        rc, text = call(**change)
        assert rc == -1 and text.startswith('genie_fold_potential: ' + msg), (change, rc, text)
    # what is allowed passes every check (and then fails on the device instead, with another code)
    if not torch.cuda.is_available():
        for kw in (dict(), dict(logp=None, grad=None), dict(report=None, tm=None), dict(logp=None, grad=None, report=None), dict(work_bytes=96 * 2 * 3),
                   dict(N=4, R=1), dict(N=1706, R=4096, work_bytes=1 << 40), dict(n_iter=1), dict(n_iter=32)):
            assert call(**kw)[0] != -1, kw


def test_cpu_device_is_refused(lib):
    from genie2_amd import capi
    from genie2_amd.smc import FoldPotential
    with pytest.raises(capi.GenieError, match='FoldPotential runs on the GPU'):
        FoldPotential(40, torch.linspace(0.999, 0.001, 13), Fd.designs(1, 40), [(0.6, math.inf)], device='cpu')
