"""The burial potential without a device: the float64 oracle of tests/_burial.py against the header's gradient formula written with
loops, its invariance under rigid motion and the straight chain; the C entry's symbols, work sizes and refusals
(genie_burial_potential, include/genie_hip.h); load_burial_targets', check_burial_targets', parse_residue_ranges' and
BurialPotential's host side; both command lines' parsers and constants, and the report writer.

What holds the kernel to the oracle is tests/test_burial_gpu.py."""
import ctypes as C
import math
import os

import pytest
import torch

import _burial as Bu
from _motif import walk
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')
BASE = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', [3, 4, 7, 12])
def test_analytic_gradient_equals_autograd(N):
    """The header's formula, written out with loops, against autograd of the oracle: 1e-10 of the largest entry.  Separation 1 at the
    two smallest lengths, so that they have pairs at all."""
    x = walk(2, N, N).double()
    cfg = Bu.walk_config(x, N, separation=1 if N < 7 else 3)
    ref = Bu.reference(x, cfg, 0.7)
    scale = float(ref['grad'].abs().max())
    assert scale > 0 and bool((ref['e_burial_target'] > 0).all()) and float(ref['e_burial_mean'][0]) > 0
    assert float((ref['grad'] - Bu.analytic_gradient(x, cfg, 0.7)).abs().max()) <= 1e-10 * scale


def test_a_single_target_pulls_on_its_stencil_and_on_distant_residues():
    """One violated target at n: the gradient reaches n - 1 and n + 1 through the direction u_n, and a residue far away in sequence
    through the count itself."""
    N, n = 12, 5
    x = walk(1, N, 21).double()
    c = float(Bu.counts(x, Bu.config())[0, n])
    cfg = Bu.config(targets=[(n, 1.5 * c + 1.0, math.inf, 2.0)])
    ref = Bu.reference(x, cfg, 0.9)
    assert float(ref['e_burial_target'][0]) > 0 and int(ref['n_burial_violated'][0]) == 1
    g = ref['grad'][0]
    scale = float(g.abs().max())
    assert float((g - Bu.analytic_gradient(x, cfg, 0.9)[0]).abs().max()) <= 1e-10 * scale
    assert all(float(g[i].abs().max()) > 0 for i in (n - 1, n, n + 1))
    far = max(range(N), key=lambda j: abs(j - n))
    assert float(g[far].abs().max()) > 0
    # residues inside the separation window, other than the stencil, feel nothing
    assert float(g[n + 2].abs().max()) == 0 and float(g[n - 2].abs().max()) == 0


def test_oracle_is_invariant_under_rigid_motion():
    x = walk(3, 30, 5).double()
    cfg = Bu.walk_config(x, 5)
    q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1)))
    if float(torch.det(q)) < 0:
        q[:, 0] = -q[:, 0]
    y = x @ q.T + torch.tensor([3.0, -20.0, 7.5], dtype=torch.float64)
    a, b = Bu.reference(x, cfg, 1.0), Bu.reference(y, cfg, 1.0)
    assert float((a['logp'] - b['logp']).abs().max()) <= 1e-9 * float(a['logp'].abs().max())
    assert float((a['burial'] - b['burial']).abs().max()) <= 1e-9 * float(a['burial'].abs().max())
    assert float((a['grad'] @ q.T - b['grad']).abs().max()) <= 1e-9 * float(a['grad'].abs().max())


def test_straight_chain_counts_half_of_the_full_sphere():
    """b_n = 0 on a straight chain with equal spacing: u = 0, h = 0, g = 1/2 exactly, so c_n = 1/2 sum_j s, and nothing is divided by
    |b|: the gradient is finite.  (The spacing is float32's 3.8, so that every coordinate, and with it b_n = 0, is exact.)"""
    N = 20
    x = torch.zeros(1, N, 3, dtype=torch.float64)
    x[0, :, 0] = float(torch.tensor(3.8, dtype=torch.float32)) * torch.arange(N, dtype=torch.float64)
    assert float(Bu.directions(x)[0].abs().max()) == 0.0
    cfg = Bu.config(targets=[(4, 9.0, math.inf, 1.0), (10, 0.0, 1.0, 1.0)], mean_min=8.0, mean_weight=1.0)
    q = (x[0, :, None, 0] - x[0, None, :, 0]) ** 2
    idx = torch.arange(N)
    s = (1.0 / (1.0 + (q / 100.0) ** 3)) * ((idx[:, None] - idx[None]).abs() >= 3)
    ref = Bu.reference(x, cfg, 1.0)
    assert torch.equal(ref['burial'][0], 0.5 * s.sum(dim=1))
    assert bool(torch.isfinite(ref['grad']).all()) and float(ref['grad'].abs().max()) > 0 and float(ref['logp'][0]) < 0


def test_parity_inputs_keep_their_margins():
    """Every parity case of test_burial_gpu.py from the oracle alone (the longest left to the GPU file, which builds it anyway)."""
    for case in Bu.CASES[:-1]:
        x, cfg = Bu.inputs(case)
        assert tuple(x.shape) == (case[0], case[1], 3) and x.dtype == torch.float32
        assert len(cfg['targets']) == max(1, case[1] // 3) and Bu.margins(x, cfg) >= 1e-4


# ---- the host side of smc.py ---------------------------------------------------------------------------------------------------------

def test_constructor_validates_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import BurialPotential
    import genie.sampler.burial as mirror
    assert mirror.BurialPotential is BurialPotential
    abar = torch.linspace(0.999, 0.001, 13)
    inf, nan = math.inf, math.nan
    ok = dict(targets=[(3, 2.0, inf)], device='cpu')
    for n_res in (0, -1, 1729, 40.0, True):
        with pytest.raises(ValueError, match=r'n_res must be an integer in 1\.\.1728'):
            BurialPotential(n_res, abar, **ok)
    with pytest.raises(ValueError, match='no term enabled'):
        BurialPotential(40, abar, device='cpu')
    with pytest.raises(ValueError, match='no term enabled'):
        BurialPotential(40, abar, targets=[], mean=(1.0, 2.0), mean_weight=0.0, device='cpu')
    for targets, msg in (([(40, 1.0, 2.0)], r'residue 40 must lie in 0\.\.39'), ([(-1, 1.0, 2.0)], 'must lie in'),
                         ([(3, 1.0, 2.0), (3, 0.0, 5.0)], 'residue 3 is listed twice'), ([(3, 2.0, 1.0)], 'needs 0 <= lo <= hi'),
                         ([(3, -1.0, 1.0)], 'needs 0 <= lo <= hi'), ([(3, inf, inf)], 'lo finite'), ([(3, nan, 1.0)], 'needs 0 <= lo <= hi'),
                         ([(3, 1.0, 2.0, -1.0)], 'weight must be finite and >= 0'), ([(3, 1.0, 2.0, inf)], 'weight must be finite'),
                         ([(3.0, 1.0, 2.0)], 'residue must be an integer'), ([(True, 1.0, 2.0)], 'residue must be an integer'),
                         ([(3, 1.0)], r'expected \(i, lo, hi\[, weight\]\)'), ([(3, 'a', 2.0)], 'must be numbers')):
        with pytest.raises(ValueError, match=msg):
            BurialPotential(40, abar, targets=targets, device='cpu')
    for mean in ((2.0, 1.0), (-1.0, 1.0), (inf, inf), (nan, 1.0), 3.0, (1.0,), ('a', 'b')):
        with pytest.raises(ValueError, match=r'mean must be \(min, max\)'):
            BurialPotential(40, abar, mean=mean, device='cpu')
    for name in ('radius', 'width', 'tausq'):
        for v in (0.0, -1.0, inf, nan, 'x'):
            with pytest.raises(ValueError, match='%s must be finite and > 0' % name):
                BurialPotential(40, abar, **dict(ok, **{name: v}))
    for v in (-1.0, inf, nan, 'x'):
        with pytest.raises(ValueError, match='mean_weight must be finite and >= 0'):
            BurialPotential(40, abar, mean=(1.0, 2.0), mean_weight=v, device='cpu')
    for v in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='separation must be an integer >= 1'):
            BurialPotential(40, abar, separation=v, **ok)
    # what is allowed gets as far as the device: a CPU potential is a GenieError
    for kw in (ok, dict(mean=(5.0, inf), device='cpu'), dict(targets=[(0, 0.0, 3.0, 0.0), (39, 1.0, 1.0, 2.5)], mean=(0.0, 9.0), device='cpu'),
               dict(ok, radius=8.0, width=0.5, separation=1, tausq=0.012)):
        with pytest.raises(capi.GenieError, match='BurialPotential runs on the GPU'):
            BurialPotential(40, abar, **kw)
    doc = BurialPotential.__doc__
    assert 'design choices' in doc and 'unmeasured' in doc and 'Not built' in doc
    for words in ("motif's placement", '--unit_chains', 'full-atom or C-beta', "binder target's atoms"):
        assert words in doc, words
    others = (capi.SHAPE_REPORT, capi.SECSTRUCT_REPORT, capi.SHEET_REPORT, capi.SYMMETRY_REPORT, capi.BINDER_REPORT, capi.FOLD_REPORT,
              capi.DIVERSITY_REPORT)
    assert capi.BURIAL_REPORT == Bu.REPORT and capi.BURIAL_COUNTS == Bu.COUNTS
    assert not any(set(capi.BURIAL_REPORT) & set(o) for o in others)                   # SumPotential merges the reports


def test_loaders(tmp_path):
    from genie2_amd.smc import check_burial_targets, load_burial_targets, parse_residue_ranges
    path = tmp_path / 'burial.txt'
    path.write_text('# core\n5 8 inf\n9 8.5 inf 2\n\n30 0 3.5 0.5  # loop\n')
    assert load_burial_targets(str(path)) == [(5, 8.0, math.inf, 1.0), (9, 8.5, math.inf, 2.0), (30, 0.0, 3.5, 0.5)]
    assert check_burial_targets(load_burial_targets(str(path))[::-1], 31)[0] == (5, 8.0, math.inf, 1.0)
    for text, msg in (('5 8\n', r'burial.txt:1: expected `i lo hi \[weight\]`, got 2 fields'), ('# x\n5 8 inf 1 1\n', r'burial.txt:2: expected'),
                      ('5 8 inf\nfive 8 inf\n', r'burial.txt:2: the residue is an integer'), ('5 8 high\n', r'burial.txt:1: the residue is an integer'),
                      ('5.0 8 9\n', r'burial.txt:1: ')):
        path.write_text(text)
        with pytest.raises(ValueError, match=msg):
            load_burial_targets(str(path))
    with pytest.raises(OSError):
        load_burial_targets(str(tmp_path / 'none.txt'))
    assert parse_residue_ranges('3,10-20,35') == [3] + list(range(10, 21)) + [35]
    assert parse_residue_ranges('7') == [7] and parse_residue_ranges(' 4-4 , 0 ') == [0, 4]
    for spec in ('', '3,,4', '5-3', '3,3', '1-4,4-6', 'a', '-3', '3-', '1-2-3', '2.5'):
        with pytest.raises(ValueError):
            parse_residue_ranges(spec)


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

FLAGS = ('--burial_file', '--bury', '--bury_min', '--expose', '--expose_max', '--burial_mean_min', '--burial_mean_max', '--burial_weight',
         '--burial_mean_weight', '--burial_radius', '--burial_width', '--burial_separation', '--burial_tausq', '--write_burial')


def test_parsers_constants_and_the_messages(tmp_path, capsys):
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    import genie.sample_unconditional_shape as mirror
    assert mirror.add_burial_arguments is Sh.add_burial_arguments and mirror.burial_potential is Sh.burial_potential
    defaults = dict(burial_file=None, bury=None, bury_min=None, expose=None, expose_max=None, burial_mean_min=None, burial_mean_max=None,
                    burial_weight=1.0, burial_mean_weight=1.0, burial_radius=10.0, burial_width=2.0, burial_separation=3, burial_tausq=1.0,
                    write_burial=False)
    assert Sh.BURIAL_DEFAULTS == defaults
    path = tmp_path / 'burial.txt'
    path.write_text('2 7 inf 2\n')
    given = ['--burial_file', str(path), '--bury', '5,9-10', '--bury_min', '8', '--expose', '30-32', '--expose_max', '3.5', '--burial_mean_min',
             '6', '--burial_mean_max', '12', '--burial_weight', '0.5', '--burial_mean_weight', '3', '--burial_radius', '9', '--burial_width', '1.5',
             '--burial_separation', '2', '--burial_tausq', '4', '--write_burial']
    values = dict(burial_file=str(path), bury='5,9-10', bury_min=8.0, expose='30-32', expose_max=3.5, burial_mean_min=6.0, burial_mean_max=12.0,
                  burial_weight=0.5, burial_mean_weight=3.0, burial_radius=9.0, burial_width=1.5, burial_separation=2, burial_tausq=4.0,
                  write_burial=True)
    for parser, more in ((Sh.build_parser(), []), (M.build_parser(), ['--motif_file', MOTIF])):
        text = parser.format_help()
        assert all(flag + ' ' in text or flag + '\n' in text for flag in FLAGS)
        a = vars(parser.parse_args(BASE + more))
        assert {k: a[k] for k in defaults} == defaults
        assert a['rog_max'] is None and a['symmetry'] is None and a['diversity_tm_max'] is None      # (the flags that were there)
        a = vars(parser.parse_args(BASE + more + given))
        assert {k: a[k] for k in values} == values

    # constants: a burial term is enough on its own for the shape CLI; every source in one table, the weights scaled
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + given)))
    assert {k: c[k] for k in values} == values and Sh.has_burial_terms(c) and c['burial_mean'] == (6.0, 12.0)
    assert c['burial_targets'] == [(2, 7.0, math.inf, 1.0), (5, 8.0, math.inf, 0.5), (9, 8.0, math.inf, 0.5), (10, 8.0, math.inf, 0.5),
                                   (30, 0.0, 3.5, 0.5), (31, 0.0, 3.5, 0.5), (32, 0.0, 3.5, 0.5)]
    assert not (Sh.has_shape_terms(c) or Sh.has_secstruct_terms(c) or Sh.has_sheet_terms(c) or Sh.has_symmetry_terms(c) or Sh.has_binder_terms(c)
                or Sh.has_fold_terms(c) or Sh.has_diversity_terms(c))
    for flags, want in ((['--burial_mean_min', '5'], (5.0, math.inf)), (['--burial_mean_max', '7'], (0.0, 7.0))):
        c = Sh.burial_constants(vars(Sh.build_parser().parse_args(BASE + flags)))
        assert c['burial_mean'] == want and c['burial_targets'] == [] and Sh.has_burial_terms(c)
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF] + given)))
    assert {k: c[k] for k in values} == values and c['tausq'] == 0.012 and Sh.has_burial_terms(c)

    # no burial flag: no term, and sum_potentials gets None for it
    for c in (M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF]))),
              Sh.GuidedRunner().create_constants(vars(Sh.build_parser().parse_args(BASE))),
              Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + ['--rog_max', '12'])))):
        assert {k: c[k] for k in defaults} == defaults and c['burial_targets'] == [] and c['burial_mean'] is None
        assert not Sh.has_burial_terms(c)
        pot = Sh.burial_potential(c, 60, None, 'cuda')                                              # no term: no potential, no device
        assert pot is None
        marker = object()
        assert Sh.sum_potentials(marker, pot) is marker and Sh.sum_potentials(pot) is None

    # every way the flags end a run, in both CLIs
    for run in (lambda f: Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + f))),
                lambda f: M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF] + f)))):
        with pytest.raises(SystemExit, match='--bury needs --bury_min'):
            run(['--bury', '5'])
        with pytest.raises(SystemExit, match='--expose needs --expose_max'):
            run(['--expose', '5-9'])
        with pytest.raises(SystemExit, match='--bury_min needs --bury'):
            run(['--bury_min', '5', '--burial_mean_min', '3'])
        with pytest.raises(SystemExit, match='--expose_max needs --expose'):
            run(['--expose_max', '5', '--burial_mean_min', '3'])
        with pytest.raises(SystemExit, match='residue 7 is named twice'):
            run(['--bury', '5-7', '--bury_min', '8', '--expose', '7-9', '--expose_max', '3'])
        with pytest.raises(SystemExit, match='residue 2 is named twice'):
            run(['--burial_file', str(path), '--expose', '0-3', '--expose_max', '3'])
        for flags in (['--burial_weight', '2'], ['--burial_mean_weight', '2'], ['--burial_radius', '8'], ['--burial_width', '1'],
                      ['--burial_separation', '4'], ['--burial_tausq', '2'], ['--write_burial'], ['--bury_min', '8'], ['--expose_max', '3']):
            with pytest.raises(SystemExit, match='a burial flag needs a term'):
                run(flags)
    term = ['--burial_mean_min', '5']
    for flags, msg in ((['--bury', '5', '--bury_min', '-1'], 'bury_min must be finite and >= 0'), (['--bury', '5', '--bury_min', 'inf'], 'bury_min must be'),
                       (['--expose', '5', '--expose_max', 'nan'], 'expose_max must be'), (['--burial_mean_min', '-2'], 'burial_mean_min must be'),
                       (['--burial_mean_min', '5', '--burial_mean_max', '4'], '--burial_mean_max is below --burial_mean_min'),
                       (term + ['--burial_weight', '-1'], 'burial_weight must be'), (term + ['--burial_mean_weight', 'inf'], 'burial_mean_weight must be'),
                       (term + ['--burial_radius', '0'], 'burial_radius must be finite and > 0'), (term + ['--burial_width', '0'], 'burial_width must be'),
                       (term + ['--burial_tausq', '0'], 'burial_tausq must be'), (term + ['--burial_separation', '0'], 'burial_separation must be at least 1'),
                       (term + ['--burial_mean_weight', '0'], 'nothing to guide'), (['--bury', '9-5', '--bury_min', '3'], 'runs backwards'),
                       (['--bury', 'x', '--bury_min', '3'], 'residue ranges look like'), (['--burial_file', str(tmp_path / 'none.txt')], '--burial_file'),):
        with pytest.raises(SystemExit, match=msg):
            Sh.burial_constants(vars(Sh.build_parser().parse_args(BASE + flags)))
    path.write_text('2 7\n')
    with pytest.raises(SystemExit, match=r'burial.txt:1: expected'):
        Sh.burial_constants(vars(Sh.build_parser().parse_args(BASE + ['--burial_file', str(path)])))
    path.write_text('2 7 3\n')
    with pytest.raises(SystemExit, match='needs 0 <= lo <= hi'):
        Sh.burial_constants(vars(Sh.build_parser().parse_args(BASE + ['--burial_file', str(path)])))

    # a length too short for a listed residue is skipped, with one line
    tasks = [{'length': n} for n in (30, 33, 40)]
    capsys.readouterr()
    assert Sh.burial_lengths(tasks, [(5, 8.0, math.inf, 1.0), (32, 0.0, 3.0, 1.0)]) == tasks[1:]
    assert capsys.readouterr().out == 'skipping lengths shorter than the 33 residues the burial targets name: 30\n'
    assert Sh.burial_lengths(tasks, []) == tasks and capsys.readouterr().out == ''
    params = vars(Sh.build_parser().parse_args(BASE + ['--expose', '30-32', '--expose_max', '3']))
    assert Sh.GuidedRunner().guided_lengths(tasks, params) == tasks[1:]

    # the message of a run with no term names the flags, keeps every name it had, and still ends as tests/test_symmetry_host.py reads it
    with pytest.raises(SystemExit, match='no shape term.*--symmetry$') as info:
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE)))
    for name in ('--burial_file', '--bury', '--bury_min', '--expose', '--expose_max', '--burial_mean_min', '--burial_mean_max', '--diversity_tm_max',
                 '--template_pdb', '--target_pdb', '--rog_max', '--helix_min', '--ladder_file'):
        assert name in str(info.value), name
    for doc in (Sh.__doc__, M.__doc__):
        assert '--bury' in doc and '--expose_max' in doc and 'outdir/burial/{length}_{index}.txt' in doc
    assert 'Not built' in Sh.__doc__ and 'half-sphere exposure' in Sh.__doc__


def test_report_writer(tmp_path):
    from genie2_amd import capi
    from genie2_amd import sample_unconditional_shape as Sh
    merged = {'rog': torch.tensor([12.3, 9.0]), 'burial_mean': torch.tensor([7.12345, 0.0]), 'burial_min': torch.tensor([0.5, 0.0]),
              'burial_max': torch.tensor([15.25, 0.0]), 'n_burial_violated': torch.tensor([2, 0]), 'max_burial_violation': torch.tensor([3.0004, 0.0]),
              'e_burial_target': torch.tensor([1234.5678, 0.0]), 'e_burial_mean': torch.tensor([0.25, 0.0])}
    assert list(Sh.report_fields(merged, capi.BURIAL_REPORT)) == list(capi.BURIAL_REPORT)
    burial = torch.tensor([[0.5, 7.61239, 15.25], [0.0, 0.0, 1e-7]])
    Sh.write_burial_report(burial, [(0, 2.0, math.inf, 1.0), (2, 0.0, 3.5, 0.5)], Sh.report_fields(merged, capi.BURIAL_REPORT),
                           str(tmp_path / 'burial'), 3, 4)
    assert sorted(os.listdir(tmp_path / 'burial')) == ['3_4.txt', '3_5.txt']
    assert (tmp_path / 'burial' / '3_4.txt').read_text() == (
        'residue 0 0.500 2 inf\nresidue 1 7.612 - -\nresidue 2 15.250 0 3.5\nburial_mean 7.123\nburial_min 0.500\nburial_max 15.250\n'
        'n_burial_violated 2\nmax_burial_violation 3.000\ne_burial_target 1234.568\ne_burial_mean 0.250\n')
    assert (tmp_path / 'burial' / '3_5.txt').read_text().splitlines()[:4] == ['residue 0 0.000 2 inf', 'residue 1 0.000 - -', 'residue 2 0.000 0 3.5',
                                                                              'burial_mean 0.000']


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_exported(lib):
    from genie2_amd import build, capi
    assert 'burial_kernels.hip' in build.SOURCES and os.path.exists(os.path.join(os.path.dirname(build.__file__), 'csrc', 'burial_kernels.hip'))
    res, args = capi.SYMBOLS['genie_burial_potential']
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 3 + \
        [C.c_float] * 3 + [C.c_void_p] * 6 + [C.c_size_t]
    assert capi.SYMBOLS['genie_burial_potential_work_bytes'] == (C.c_size_t, [C.c_int, C.c_int])
    assert lib.genie_burial_potential and lib.genie_burial_potential_work_bytes
    header = open(os.path.join(os.path.dirname(build.__file__), '..', 'include', 'genie_hip.h')).read()
    assert 'int genie_burial_potential(genie_stream_t stream, int B, int N, const float* x0' in header
    assert 'size_t genie_burial_potential_work_bytes(int B, int N);' in header
    assert '#define GENIE_BURIAL_REPORT %d ' % len(capi.BURIAL_REPORT) in header and '#define GENIE_BURIAL_EPS 0.1f' in header
    assert '#define GENIE_BURIAL_MAX_LENGTH %d' % capi.BURIAL_MAX_LENGTH in header
    assert lib.genie_burial_potential_work_bytes(8, 256) == 28 * 8 * 256 and lib.genie_burial_potential_work_bytes(1, 1) == 28
    assert lib.genie_burial_potential_work_bytes(1, 1728) == 28 * 1728
    for B, N in ((0, 10), (65536, 10), (1, 0), (1, 1729), (-1, -1)):
        assert lib.genie_burial_potential_work_bytes(B, N) == 0


def test_entry_refuses_bad_arguments_before_the_device(lib):
    """Every refusal names the entry and the argument and comes back before the device is touched: the pointers are made up."""
    inf, nan = math.inf, math.nan
    P = C.c_void_p
    x, var, out, work, tab = P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x5000)
    null = P(0)

    def call(B=2, N=10, x0=x, radius=10.0, width=2.0, separation=3, lo=null, hi=null, w=null, mean_min=1.0, mean_max=inf, mean_weight=1.0, v=var,
             logp=out, grad=out, report=null, burial=null, wk=work, wbytes=10 ** 6):
        return lib.genie_burial_potential(null, B, N, x0, radius, width, separation, lo, hi, w, mean_min, mean_max, mean_weight, v, logp, grad,
                                          report, burial, wk, wbytes)

    cases = [(dict(B=0), 'B outside'), (dict(B=65536), 'B outside'), (dict(N=0), 'N below 1'), (dict(N=1729), 'N above GENIE_BURIAL_MAX_LENGTH'),
             (dict(x0=null), 'x0 is NULL'), (dict(v=null), 'var is NULL'), (dict(separation=0), 'separation below 1'),
             (dict(radius=0.0), 'radius'), (dict(radius=-1.0), 'radius'), (dict(radius=inf), 'radius'), (dict(radius=nan), 'radius'),
             (dict(radius=1e-30), 'radius'), (dict(width=0.0), 'width'), (dict(width=inf), 'width'), (dict(width=nan), 'width'),
             (dict(lo=tab), 'lo, hi and w'), (dict(lo=tab, hi=tab), 'lo, hi and w'), (dict(hi=tab, w=tab), 'lo, hi and w'),
             (dict(mean_weight=-1.0), 'mean_weight'), (dict(mean_weight=inf), 'mean_weight'), (dict(mean_weight=nan), 'mean_weight'),
             (dict(mean_min=-1.0), 'mean_min'), (dict(mean_min=inf), 'mean_min'), (dict(mean_max=-1.0), 'mean_max'), (dict(mean_max=nan), 'mean_max'),
             (dict(mean_min=3.0, mean_max=2.0), 'mean_max below mean_min'), (dict(mean_weight=0.0), 'no term enabled'),
             (dict(logp=null, grad=null), 'no output asked for'), (dict(logp=null), 'given together'), (dict(grad=null), 'given together'),
             (dict(wk=null), 'work is NULL'), (dict(wbytes=28 * 2 * 10 - 1), 'work_bytes below'), (dict(wk=P(0x4002)), 'work not 4-byte aligned')]
    for kw, words in cases:
        assert call(**kw) == -1, kw                                                         # GENIE_E_ARG
        msg = lib.genie_last_error(None).decode()
        assert msg.startswith('genie_burial_potential: ') and words in msg, (kw, msg)
