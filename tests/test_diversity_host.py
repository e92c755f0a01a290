"""The diversity potential without a device: the float64 oracle of tests/_diversity.py on hand cases and against central differences
of its own score on both sides of a pair, the parity inputs against the oracle's own conditions, DiversityPotential's host side, both
command lines' flags, the report writer, and the C entry's declaration, export and refusals (genie_diversity_potential,
include/genie_hip.h).

What holds the kernel to the oracle is tests/test_diversity_gpu.py."""
import ctypes as C
import math
import os

import pytest
import torch

import _diversity as Dv
import _fold as Fd
import _similarity as S
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')

# The fixed-fit gradient against central differences of the converged score (n_iter = 200, h = 1e-5 A), moving x_b only.  Measured on
# the CPU over FD_CASES, as a fraction of the gradient's largest entry: the moving side 1.7e-9, 2.6e-9, 2.5e-9, the
# reference side 2.2e-9, 2.2e-9, 2.4e-9; the tolerance is 4 x the worst.
FD_TOLERANCE = 1.1e-8
FD_CASES = [(40, 0.3), (56, 0.8), (64, 1.0)]      # (N, noise in A per coordinate): TM about 0.94, 0.78, 0.76


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

def test_oracle_hand_cases():
    a = Fd.walk(64, 6400)
    copy = (a.double() @ S.rotation(6401).T + torch.tensor([11.0, -7.0, 5.0], dtype=torch.float64))
    x = torch.stack([a.double(), copy])
    # a rigidly moved copy in another system scores 1; the fit is exact, every e_n is 0: the gradient vanishes under a full hinge
    r = Dv.reference(x, 1, 0.5)
    assert float(r['tm'][0, 1]) == pytest.approx(1.0, abs=1e-12) and float(r['tm'][1, 0]) == float(r['tm'][0, 1])
    assert float(r['a'][0, 1]) == pytest.approx(32.0, abs=1e-9) and float(r['grad'].abs().max()) < 1e-9
    assert r['e_diversity'].tolist() == pytest.approx([1024.0, 1024.0], abs=1e-6) and r['logp'].tolist() == pytest.approx([-1024.0, -1024.0], abs=1e-6)
    assert r['nearest_design'].tolist() == [1, 0] and r['n_similar'].tolist() == [1, 1] and float(r['tm'][0, 0]) == 0.0
    assert r['tm_mean_design'].tolist() == pytest.approx([1.0, 1.0], abs=1e-12)
    # the same copy in the same system is not scored; S = 1 gives zeros
    for batch, K in ((x, 2), (x[:1], 1), (torch.cat([x, x]), 4)):
        r = Dv.reference(batch, K, 0.5)
        assert not bool(r['scored'].any()) and len(r['pairs'][0]) == 0
        assert bool((r['logp'] == 0).all()) and bool((r['grad'] == 0).all()) and bool((r['tm'] == 0).all())
        assert r['nearest_design'].tolist() == [-1] * len(batch) and bool((r['tm_nearest_design'] == 0).all())
        assert bool((r['tm_mean_design'] == 0).all()) and bool((r['n_similar'] == 0).all()) and bool((r['e_diversity'] == 0).all())
        assert r['margin'] == math.inf and not bool(Dv.left_out(r).any())
    with pytest.raises(ValueError):
        Dv.reference(torch.cat([x, x[:1]]), 2, 0.5)


def test_oracle_energy_scales_with_weight_and_one_over_k():
    x = Dv.inputs((2, 2, 40))                                            # systems {0, 1} and {2, 3}; particle 2 is the unrelated walk
    r = Dv.reference(x, 2, 0.7)
    n, N = r['n'], 40
    assert r['scored'].tolist() == [[False, False, True, True], [False, False, True, True], [True, True, False, False], [True, True, False, False]]
    assert torch.equal(n, n.T) and torch.equal(r['tm'], n / N)
    a = torch.where(r['scored'], torch.clamp(n - 20, min=0), torch.zeros_like(n))
    assert torch.equal(r['a'], a) and bool((a > 0).any()) and bool((a[r['scored']] == 0).any())
    assert torch.allclose(r['e_diversity'], (a ** 2).sum(dim=1) / 2, rtol=1e-13) and torch.allclose(r['logp'], -r['e_diversity'] / 1.4, rtol=1e-13)
    assert r['n_similar'].tolist() == (a > 0).sum(dim=1).tolist()
    assert r['nearest_design'].tolist() == [int(torch.where(r['scored'][b], r['tm'][b], -torch.ones(4, dtype=torch.float64)).argmax()) for b in range(4)]
    heavy = Dv.reference(x, 2, 0.7, weight=2.5)
    assert torch.allclose(heavy['e_diversity'], 2.5 * r['e_diversity'], rtol=1e-13) and torch.allclose(heavy['grad'], 2.5 * r['grad'], rtol=1e-12, atol=0)
    assert torch.equal(heavy['tm'], r['tm'])
    # 1 / K: a particle's energy and gradient are those of the batch without its system-mate, as systems of one, over K
    for b, mate in ((0, 1), (1, 0), (2, 3), (3, 2)):
        rest = [k for k in range(4) if k != mate]
        alone = Dv.reference(x[rest], 1, 0.7)
        at = rest.index(b)
        assert float(r['e_diversity'][b]) == pytest.approx(float(alone['e_diversity'][at]) / 2, rel=1e-12)
        assert float((r['grad'][b] - alone['grad'][at] / 2).abs().max()) <= 1e-12 * max(1.0, float(alone['grad'][at].abs().max()))
    # the bound: nothing above it, nothing happens
    idle = Dv.reference(x, 2, 0.7, tm_max=1.0)
    assert bool((idle['logp'] == 0).all()) and bool((idle['grad'] == 0).all()) and bool((idle['n_similar'] == 0).all())


def test_oracle_scores_a_pair_once_and_loses_nothing():
    """The pair with j moving instead gives the same n to 1e-14 N in float64 (include/genie_hip.h says so); and the moving-side
    gradient rebuilt from the rotations of `rotations_last` is `Fd.ascend_last`'s own."""
    for case in ((3, 1, 5), (2, 2, 63), (3, 2, 64), (4, 2, 129)):
        x = Dv.inputs(case).double()
        i, j = Dv.pair_index(x.shape[0], case[1])
        n_ij, dp, gap = Fd.ascend_last(x[i], x[j], 16)
        n_ji = Fd.ascend_last(x[j], x[i], 16)[0]
        assert float((n_ij.amax(dim=1) - n_ji.amax(dim=1)).abs().max()) <= 1e-14 * case[2], case
        # d n / d Q = -(d n / d P) R^T: a rotation of the moving side's rows, sign turned
        n, dp2, dq, _ = Dv.score_pairs(x[i], x[j], 16)
        assert torch.equal(n, n_ij) and torch.equal(dp2, dp)
        assert torch.allclose(dq.norm(dim=-1), dp.norm(dim=-1), rtol=1e-10, atol=1e-14)
        assert float(dq.sum(dim=2).abs().max()) > 0                 # (the reference side is no mirror of the moving one)


@pytest.mark.parametrize('N,noise', FD_CASES)
def test_oracle_gradient_matches_central_differences_on_both_sides(N, noise):
    """At a converged ascent (n_iter = 200, the oracle only) the gradient with the fit held fixed is the total derivative of the
    particle's own log p in its own coordinates (envelope theorem), for the particle that moved in the fit (b = 0) and for the one
    that was its reference (b = 1): central differences of the oracle's converged log p_b, every one of them ascending afresh, moving
    x_b only."""
    tm_max, var, n_iter, h = 0.05, 0.5, 200, 1e-5
    x0 = Fd.walk(N, 900 + N).double()
    x1 = S.moved(x0, 901 + N, noise).double()
    ref = Dv.evaluate(torch.stack([x0, x1]), 1, var, tm_max, 1.0, n_iter)
    assert 0.25 < float(ref['tm'][0, 1]) < 0.95 and float(ref['a'][0, 1]) > 0
    steps = h * torch.eye(3 * N, dtype=torch.float64).reshape(-1, N, 3)

    def logp_of(P, Q):                                             # one pair per row: log p of either member, K = 1, weight 1
        n = Fd.ascend_last(P, Q, n_iter)[0].amax(dim=1)
        return -torch.clamp(n - N * tm_max, min=0) ** 2 / (2 * var)

    for b, side in ((0, 'moving'), (1, 'reference')):
        if b == 0:
            P = torch.cat([x0[None] + steps, x0[None] - steps])
            lp = logp_of(P, x1[None].expand_as(P))
        else:
            Q = torch.cat([x1[None] + steps, x1[None] - steps])
            lp = logp_of(x0[None].expand_as(Q), Q)
        fd = ((lp[:3 * N] - lp[3 * N:]) / (2 * h)).reshape(N, 3)
        err = float((ref['grad'][b] - fd).abs().max()) / float(ref['grad'][b].abs().max())
        print('N = %d, noise %.1f A, TM %.3f, %s side: fixed-fit gradient against central differences %.2e of the largest entry'
              % (N, noise, float(ref['tm'][0, 1]), side, err))
        assert err <= FD_TOLERANCE, (side, err)


def test_autograd_form_is_the_analytic_one_in_float64():
    for case, weight in (((3, 2, 40), 1.0), ((2, 3, 33), 2.5), ((4, 1, 24), 1.0)):
        x = Dv.inputs(case)
        r = Dv.reference(x, case[1], 0.7, weight=weight)
        xg = x.double().requires_grad_(True)
        lp = Dv.logp(xg, case[1], 0.7, weight=weight)
        g, = torch.autograd.grad(lp.sum(), xg)
        assert float(r['grad'].abs().max()) > 0
        assert torch.allclose(lp.detach(), r['logp'], rtol=1e-12, atol=0)
        assert float((g - r['grad']).abs().max()) <= 1e-12 * float(r['grad'].abs().max())
    one = Dv.inputs((1, 3, 24)).double().requires_grad_(True)            # one system: a zero that still has a graph
    lp = Dv.logp(one, 3, 0.7)
    assert bool((lp == 0).all()) and bool((torch.autograd.grad(lp.sum(), one)[0] == 0).all())
    r32 = Dv.restatement32(Dv.inputs((3, 2, 40)), 2, 0.7)
    assert r32['grad'].dtype == torch.float32 and torch.allclose(r32['logp'].double(), Dv.reference(Dv.inputs((3, 2, 40)), 2, 0.7)['logp'], rtol=1e-4)


def test_parity_inputs_pass_the_oracles_conditions():
    """Every parity case of test_diversity_gpu.py from the oracle alone: no n_ij within 1e-4 N of the bound, an active and an idle
    pair wherever a case has more than one pair, at most 5 % of the particles left out as ill-posed."""
    for case in Dv.CASES:
        x = Dv.inputs(case)
        assert tuple(x.shape) == (case[0] * case[1], case[2], 3) and x.dtype == torch.float32
        r64 = Dv.reference(x, case[1], 0.8)
        Dv.check_inputs(r64, case)
        assert len(r64['pairs'][0]) == case[0] * (case[0] - 1) // 2 * case[1] ** 2
        assert bool((r64['logp'] <= 0).all()) and float(r64['logp'].min()) < 0 and int(r64['n_similar'].sum()) > 0


# ---- DiversityPotential's host side -------------------------------------------------------------------------------------------------

def test_constructor_validates_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import DiversityPotential
    import genie.sampler.diversity as mirror
    assert mirror.DiversityPotential is DiversityPotential
    abar = torch.linspace(0.999, 0.001, 13)
    inf, nan = math.inf, math.nan
    for n_res in (3, 1707, 0, 40.0, True):
        with pytest.raises(ValueError, match=r'n_res must be an integer in 4\.\.1706'):
            DiversityPotential(n_res, abar, 2, device='cpu')
    for K in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError, match=r'num_particles must be an integer in 1\.\.64'):
            DiversityPotential(40, abar, K, device='cpu')
    for tm_max in (0.0, -0.1, 1.5, nan, inf, 'x', None):
        with pytest.raises(ValueError, match=r'tm_max must be in \(0, 1\]'):
            DiversityPotential(40, abar, 2, tm_max=tm_max, device='cpu')
    for weight in (0.0, -1.0, inf, nan, 'x'):
        with pytest.raises(ValueError, match='weight must be finite and > 0'):
            DiversityPotential(40, abar, 2, weight=weight, device='cpu')
    for n_iter in (0, 33, 16.0, True, None):
        with pytest.raises(ValueError, match=r'n_iter must be an integer in 1\.\.32'):
            DiversityPotential(40, abar, 2, n_iter=n_iter, device='cpu')
    for tausq in (0.0, -1.0, inf, nan, 'x'):
        with pytest.raises(ValueError, match='tausq must be finite and > 0'):
            DiversityPotential(40, abar, 2, tausq=tausq, device='cpu')
    # what is allowed gets as far as the device: a CPU potential is a GenieError
    for kw in (dict(), dict(tm_max=1.0), dict(tm_max=0.01, weight=3.0, n_iter=1, tausq=0.012), dict(n_iter=32)):
        with pytest.raises(capi.GenieError, match='DiversityPotential runs on the GPU'):
            DiversityPotential(40, abar, 1, device='cpu', **kw)
    doc = DiversityPotential.__doc__
    assert 'depends on its batch neighbours, on purpose' in doc and 'one system spanning the whole batch has nothing to repel' in doc
    assert 'design choices' in doc and 'unmeasured' in doc and 'Not built' in doc
    assert not set(capi.DIVERSITY_REPORT) & set(capi.FOLD_REPORT)        # SumPotential merges both reports


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

BASE = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']


def test_parsers_constants_and_the_messages():
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    import genie.sample_unconditional_shape as mirror
    assert mirror.add_diversity_arguments is Sh.add_diversity_arguments and mirror.diversity_potential is Sh.diversity_potential
    defaults = dict(diversity_tm_max=None, diversity_weight=1.0, diversity_iterations=16, diversity_tausq=1.0, write_diversity=False)
    assert Sh.DIVERSITY_DEFAULTS == defaults
    given = ['--diversity_tm_max', '0.4', '--diversity_weight', '2', '--diversity_iterations', '8', '--diversity_tausq', '4', '--write_diversity']
    values = dict(diversity_tm_max=0.4, diversity_weight=2.0, diversity_iterations=8, diversity_tausq=4.0, write_diversity=True)
    for parser, more in ((Sh.build_parser(), []), (M.build_parser(), ['--motif_file', MOTIF])):
        a = vars(parser.parse_args(BASE + more))
        assert {k: a[k] for k in defaults} == defaults
        assert a['rog_max'] is None and a['template_pdb'] is None and a['num_particles'] is None      # (the flags that were there)
        a = vars(parser.parse_args(BASE + more + given + ['--num_particles', '3']))
        assert {k: a[k] for k in values} == values and a['num_particles'] == 3

    # constants: a diversity term is enough on its own for the shape CLI
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + given + ['--num_particles', '3'])))
    assert {k: c[k] for k in values} == values and Sh.has_diversity_terms(c) and c['num_particles'] == 3
    assert not (Sh.has_shape_terms(c) or Sh.has_secstruct_terms(c) or Sh.has_sheet_terms(c) or Sh.has_symmetry_terms(c) or Sh.has_binder_terms(c)
                or Sh.has_fold_terms(c))
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + ['--diversity_tm_max', '0.5', '--num_particles', '1'])))
    assert Sh.has_diversity_terms(c) and c['num_particles'] == 1                                 # single coupled trajectories
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF, '--diversity_tm_max', '0.5', '--num_particles', '2'])))
    assert Sh.has_diversity_terms(c) and c['tausq'] == 0.012
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF])))
    assert {k: c[k] for k in defaults} == defaults and not Sh.has_diversity_terms(c)
    assert Sh.diversity_potential(c, 60, None, 'cuda') is None                                   # no term: no potential, no device

    # the term without --num_particles ends the run, naming both flags, in both CLIs
    for run in (lambda f: Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + f))),
                lambda f: M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF] + f)))):
        with pytest.raises(SystemExit, match='--diversity_tm_max needs --num_particles') as info:
            run(['--diversity_tm_max', '0.5'])
        assert '--num_particles 1' in str(info.value)
        with pytest.raises(SystemExit, match='--diversity_tm_max needs --num_particles'):
            run(given)
        # a diversity flag without the term says so
        for flags in (['--diversity_weight', '2'], ['--diversity_iterations', '8'], ['--diversity_tausq', '2'], ['--write_diversity']):
            with pytest.raises(SystemExit, match='a diversity flag needs --diversity_tm_max'):
                run(flags + ['--num_particles', '2'])
    for flags, msg in ((['--diversity_tm_max', '0'], r'diversity_tm_max must be in \(0, 1\]'), (['--diversity_tm_max', '1.5'], 'diversity_tm_max must be'),
                       (['--diversity_tm_max', 'nan'], 'diversity_tm_max must be'), (['--diversity_tm_max', '0.5', '--diversity_weight', '0'], 'diversity_weight must be'),
                       (['--diversity_tm_max', '0.5', '--diversity_weight', 'inf'], 'diversity_weight must be'),
                       (['--diversity_tm_max', '0.5', '--diversity_iterations', '0'], r'diversity_iterations must be in 1\.\.32'),
                       (['--diversity_tm_max', '0.5', '--diversity_iterations', '33'], 'diversity_iterations must be'),
                       (['--diversity_tm_max', '0.5', '--diversity_tausq', '0'], 'diversity_tausq must be')):
        with pytest.raises(SystemExit, match=msg):
            Sh.diversity_constants(vars(Sh.build_parser().parse_args(BASE + ['--num_particles', '2'] + flags)))
    # the message of a run with no term names the flag, keeps every name it had, and still ends as tests/test_symmetry_host.py reads it
    with pytest.raises(SystemExit, match='no shape term.*--symmetry$') as info:
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE)))
    for name in ('--diversity_tm_max', '--num_particles', '--template_pdb', '--avoid_dir', '--target_pdb', '--rog_max', '--helix_min', '--ladder_file'):
        assert name in str(info.value), name
    doc = Sh.__doc__
    assert 'within one device batch only' in doc and '--avoid_dir' in doc and 'batch_diversity' in doc


def test_report_writer(tmp_path):
    from genie2_amd import capi
    from genie2_amd import sample_unconditional_shape as Sh
    merged = {'rog': torch.tensor([12.3, 9.0, 8.0]), 'tm_nearest_design': torch.tensor([0.71239, 0.71239, 0.3]), 'nearest_design': torch.tensor([1, 0, 0]),
              'tm_mean_design': torch.tensor([0.50645, 0.4812, 0.275]), 'n_similar': torch.tensor([1, 1, 0]), 'e_diversity': torch.tensor([1234.5678, 1234.5678, 0.0])}
    assert list(Sh.report_fields(merged, capi.DIVERSITY_REPORT)) == list(capi.DIVERSITY_REPORT)
    tm = torch.tensor([[0.0, 0.71239, 0.3004], [0.71239, 0.0, 0.25], [0.3004, 0.25, 0.0]])
    Sh.write_diversity_report(tm, ['40_4', '40_5', '40_6'], Sh.report_fields(merged, capi.DIVERSITY_REPORT), str(tmp_path / 'batch_diversity'), 40, 4)
    assert sorted(os.listdir(tmp_path / 'batch_diversity')) == ['40_4.txt', '40_5.txt', '40_6.txt']
    assert (tmp_path / 'batch_diversity' / '40_4.txt').read_text() == (
        'design 40_5 0.712\ndesign 40_6 0.300\ntm_nearest_design 0.712\nnearest_design 1\ntm_mean_design 0.506\nn_similar 1\ne_diversity 1234.568\n')
    assert (tmp_path / 'batch_diversity' / '40_6.txt').read_text() == (
        'design 40_4 0.300\ndesign 40_5 0.250\ntm_nearest_design 0.300\nnearest_design 0\ntm_mean_design 0.275\nn_similar 0\ne_diversity 0.000\n')
    # a batch of one design: no `design` line, the report of a design without a partner
    alone = {k: v[:1] for k, v in Sh.report_fields(merged, capi.DIVERSITY_REPORT).items()}
    alone.update(tm_nearest_design=torch.tensor([0.0]), nearest_design=torch.tensor([-1]))
    Sh.write_diversity_report(torch.zeros(1, 1), ['40_9'], alone, str(tmp_path / 'single'), 40, 9)
    assert (tmp_path / 'single' / '40_9.txt').read_text().splitlines()[:2] == ['tm_nearest_design 0.000', 'nearest_design -1']


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_exported(lib):
    from genie2_amd import build, capi
    assert 'diversity_kernels.hip' in build.SOURCES and os.path.exists(os.path.join(os.path.dirname(build.__file__), 'csrc', 'diversity_kernels.hip'))
    res, args = capi.SYMBOLS['genie_diversity_potential']
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 6 + [C.c_size_t]
    assert capi.SYMBOLS['genie_diversity_potential_work_bytes'] == (C.c_size_t, [C.c_int, C.c_int, C.c_int])
    assert lib.genie_diversity_potential is not None and lib.genie_diversity_potential_work_bytes is not None
    assert capi.DIVERSITY_REPORT == Dv.REPORT and len(capi.DIVERSITY_REPORT) == 5 and capi.DIVERSITY_COUNTS == Dv.COUNTS
    assert capi.DIVERSITY_MAX_BATCH == 1448
    header = open(os.path.join(os.path.dirname(build.__file__), '..', 'include', 'genie_hip.h')).read()
    for line in ('#define GENIE_DIVERSITY_REPORT 5', '#define GENIE_DIVERSITY_MAX_BATCH 1448',
                 'int genie_diversity_potential(genie_stream_t stream, int B, int K, int N, const float* x0',
                 'size_t genie_diversity_potential_work_bytes(int B, int K, int N);'):
        assert line in header, line
    assert len(capi.SYMBOLS['genie_fold_potential'][1]) == 15 and len(capi.SYMBOLS['genie_pairwise_tm'][1]) == 10      # (the neighbours keep theirs)
    wb = lib.genie_diversity_potential_work_bytes                  # 96 bytes per unordered pair, one slot at least; 0 for sizes the entry refuses
    for B, K, N in ((2, 1, 4), (6, 2, 64), (128, 16, 256), (128, 64, 24), (1448, 1, 1706), (1448, 8, 4)):
        assert wb(B, K, N) == 96 * (B * (B - 1) // 2), (B, K, N)
    assert wb(1, 1, 40) == 96 and 1448 * 1447 // 2 <= 1 << 20 < 1449 * 1448 // 2
    assert all(wb(*a) == 0 for a in ((0, 1, 40), (1449, 1, 40), (4, 0, 40), (4, 3, 40), (130, 65, 40), (4, 2, 3), (4, 2, 1707), (4, -2, 40)))


def test_entry_refuses_before_any_launch(lib):
    """The argument checks of the C entry need no device: every one returns GENIE_E_ARG with its message."""
    d = C.c_void_p(64)                                              # (never dereferenced: the entry refuses first)

    def call(B=6, K=2, N=40, x0=d, tm_max=0.5, weight=1.0, n_iter=16, var=d, logp=d, grad=d, report=d, tm=d, work=d, work_bytes=1 << 30):
        rc = lib.genie_diversity_potential(None, B, K, N, x0, tm_max, weight, n_iter, var, logp, grad, report, tm, work, work_bytes)
        return rc, lib.genie_last_error(None).decode()

    inf, nan = math.inf, math.nan
    for change, msg in ((dict(B=0), 'B outside 1..GENIE_DIVERSITY_MAX_BATCH (1448)'), (dict(B=1449, K=1), 'B outside 1..GENIE_DIVERSITY_MAX_BATCH (1448)'),
                        (dict(K=0), 'K outside 1..64 or not a divisor of B'), (dict(K=65, B=130), 'K outside 1..64 or not a divisor of B'),
                        (dict(K=4), 'K outside 1..64 or not a divisor of B'), (dict(K=-1), 'K outside 1..64'),
                        (dict(N=3), 'N outside 4..1706'), (dict(N=1707), 'N outside 4..1706'),
                        (dict(n_iter=0), 'n_iter outside 1..32'), (dict(n_iter=33), 'n_iter outside 1..32'),
                        (dict(tm_max=0.0), 'tm_max not in (0, 1]'), (dict(tm_max=-0.5), 'tm_max not in (0, 1]'), (dict(tm_max=1.0001), 'tm_max not in (0, 1]'),
                        (dict(tm_max=nan), 'tm_max not in (0, 1]'), (dict(tm_max=inf), 'tm_max not in (0, 1]'),
                        (dict(weight=-1.0), 'weight not finite or negative'), (dict(weight=inf), 'weight not finite or negative'),
                        (dict(weight=nan), 'weight not finite or negative'), (dict(x0=None), 'x0 is NULL'), (dict(var=None), 'var is NULL'),
                        (dict(logp=None, grad=None, report=None, tm=None), 'no output asked for'), (dict(logp=None), 'logp_out and grad_out are given together'),
                        (dict(grad=None), 'logp_out and grad_out are given together'), (dict(work=None), 'work is NULL or work_bytes below'),
                        (dict(work_bytes=96 * 15 - 1), 'work is NULL or work_bytes below'), (dict(B=2, K=2, work_bytes=95), 'work is NULL or work_bytes below'),
                        (dict(work=C.c_void_p(66)), 'work not 4-byte aligned')):
        rc, text = call(**change)
        assert rc == -1 and text.startswith('genie_diversity_potential: ' + msg), (change, rc, text)
    # what is allowed passes every check (and then fails on the device instead, with another code)
    if not torch.cuda.is_available():
        for kw in (dict(), dict(logp=None, grad=None), dict(report=None, tm=None), dict(logp=None, grad=None, report=None), dict(work_bytes=96 * 15),
                   dict(B=1, K=1, N=4, work_bytes=96), dict(B=1448, K=1, N=1706, work_bytes=1 << 40), dict(B=128, K=64), dict(n_iter=1), dict(n_iter=32),
                   dict(tm_max=1.0), dict(weight=0.0)):
            assert call(**kw)[0] != -1, kw


def test_cpu_device_is_refused(lib):
    from genie2_amd import capi
    from genie2_amd.smc import DiversityPotential
    with pytest.raises(capi.GenieError, match='DiversityPotential runs on the GPU'):
        DiversityPotential(40, torch.linspace(0.999, 0.001, 13), 2, device='cpu')
