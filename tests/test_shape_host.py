"""The shape potential without a device: the C entry's symbols, refusals and work size (genie_shape_potential, include/genie_hip.h),
ShapePotential's host-side validation and restraint table, load_restraints, SumPotential's attribute rules, both command lines'
parsers and the report writer, and the float64 oracle of tests/_shape.py against finite differences and against the header's
analytic gradient."""
import ctypes as C
import math
import os

import pytest
import torch

import _shape as S
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


def test_symbols_are_declared_and_load(lib):
    from genie2_amd import capi
    assert len(capi.SYMBOLS['genie_shape_potential'][1]) == 21 and capi.SYMBOLS['genie_shape_potential'][0] is C.c_int
    assert capi.SYMBOLS['genie_shape_potential_work_bytes'] == (C.c_size_t, [C.c_int, C.c_int])
    assert lib.genie_shape_potential is not None and lib.genie_shape_potential_work_bytes is not None
    assert len(capi.SHAPE_REPORT) == 8 and capi.SHAPE_REPORT == S.REPORT


def test_work_bytes_are_eight_slots_per_tile(lib):
    wb = lib.genie_shape_potential_work_bytes
    assert wb(1, 1) == 32 and wb(3, 64) == 3 * 32 and wb(3, 65) == 3 * 2 * 32 and wb(128, 256) == 128 * 4 * 32 and wb(1, 1512) == 24 * 32
    assert wb(0, 64) == 0 and wb(3, 0) == 0


def test_entry_refuses_before_the_device_is_touched(lib):
    """Every refusal returns GENIE_E_ARG without a device, and genie_last_error(NULL) names the entry and the argument."""
    d = C.c_void_p(64)                                           # never dereferenced: every call below fails its checks
    inf, nan = math.inf, math.nan

    def call(B=2, N=60, x0=d, rog_max=10.0, rog_weight=1.0, clash_distance=4.0, sep=2, clash_weight=1.0, R2=4, table=(d,) * 5, var=d,
             logp=d, grad=d, report=d, work=d, work_bytes=None):
        if work_bytes is None:
            work_bytes = lib.genie_shape_potential_work_bytes(max(B, 1), max(N, 1))
        rc = lib.genie_shape_potential(None, B, N, x0, rog_max, rog_weight, clash_distance, sep, clash_weight, R2, *table, var, logp, grad,
                                       report, work, work_bytes)
        return rc, lib.genie_last_error(None)

    cases = [(dict(B=0), b'B'), (dict(N=0), b'N'), (dict(x0=None), b'x0'), (dict(var=None), b'var'),
             (dict(logp=None, grad=None, report=None), b'no output'), (dict(logp=None), b'logp_out and grad_out'),
             (dict(grad=None), b'logp_out and grad_out'), (dict(sep=0), b'clash_separation'), (dict(sep=-3), b'clash_separation'),
             (dict(R2=-2), b'R2'), (dict(R2=3), b'R2'), (dict(work_bytes=2 * 32 - 1), b'work_bytes'), (dict(work=None), b'work'),
             (dict(N=20000), b'LDS')]
    for name, word in (('rog_max', b'rog_max'), ('rog_weight', b'rog_weight'), ('clash_distance', b'clash_distance'),
                       ('clash_weight', b'clash_weight')):
        cases += [({name: v}, word) for v in (-1.0, inf, nan)]
    for k in range(5):
        cases.append((dict(table=tuple(None if i == k else d for i in range(5))), b'restraint table'))
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b'genie_shape_potential: ') and word in msg, (kw, rc, msg)
    # what is allowed passes every check (and then fails on the device instead, with another code, or runs): R2 = 0 with a NULL
    # table, a report alone, the potential alone, the longest N genie_create accepts
    if not torch.cuda.is_available():
        for kw in (dict(R2=0, table=(None,) * 5), dict(logp=None, grad=None), dict(report=None), dict(N=1512), dict(rog_max=0.0, rog_weight=0.0)):
            assert call(**kw)[0] != -1, kw


def test_restraints_are_validated_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import ShapePotential, check_restraints
    abar = torch.linspace(0.999, 0.001, 13)
    bad = [[(1, 1, 0, 5)], [(-1, 2, 0, 5)], [(0, 8, 0, 5)], [(0, 1, -1.0, 5)], [(0, 1, 6.0, 5.0)], [(0, 1, math.inf, math.inf)],
           [(0, 1, math.nan, 5)], [(0, 1, 0, 5, -1.0)], [(0, 1, 0, 5, math.inf)], [(0, 1, 0, 5, math.nan)], [(0, 1, 0, 5), (1, 0, 2, 3)],
           [(0, 1, 0, 5), (0, 1, 0, 5)], [(0, 1, 0)], [(0.5, 1, 0, 5)], [(True, 1, 0, 5)]]
    for r in bad:
        with pytest.raises(ValueError):
            ShapePotential(8, abar, restraints=r, device='cpu')      # (before the device: a CPU potential is a GenieError)
    for kw in (dict(), dict(restraints=[]), dict(rog_max=-1.0), dict(rog_max=math.inf), dict(rog_max=5.0, rog_weight=-1.0),
               dict(clash_distance=math.nan), dict(clash_distance=4.0, clash_weight=math.inf), dict(clash_distance=4.0, clash_separation=0),
               dict(clash_distance=4.0, clash_separation=1.5), dict(rog_max=5.0, tausq=0.0)):
        with pytest.raises(ValueError):
            ShapePotential(8, abar, device='cpu', **kw)
    with pytest.raises(ValueError):
        ShapePotential(0, abar, rog_max=5.0, device='cpu')
    with pytest.raises(capi.GenieError, match='no CPU path'):
        ShapePotential(8, abar, rog_max=5.0, device='cpu')
    assert check_restraints([(3, 1, 0, math.inf), (0, 1, 2.0, 2.0, 0.0)], 4) == [(3, 1, 0.0, math.inf, 1.0), (0, 1, 2.0, 2.0, 0.0)]


def test_restraint_table_lists_every_restraint_at_both_residues():
    from genie2_amd.smc import check_restraints, restraint_table
    r = check_restraints([(4, 1, 3.0, 9.0, 2.0), (0, 4, 0.0, math.inf), (1, 2, 5.0, 5.5, 0.5), (1, 0, 1.0, 2.0)], 6)
    offset, partner, lo, hi, weight = restraint_table(r, 6)
    assert offset.dtype == partner.dtype == torch.int32 and lo.dtype == hi.dtype == weight.dtype == torch.float32
    assert offset.tolist() == [0, 2, 5, 6, 6, 8, 8]
    assert partner.tolist() == [1, 4, 0, 2, 4, 1, 0, 1]                                  # residue 0: 1, 4; residue 1: 0, 2, 4; 2: 1; 4: 0, 1
    assert lo.tolist() == [1.0, 0.0, 1.0, 5.0, 3.0, 5.0, 0.0, 3.0]
    assert hi.tolist() == [2.0, math.inf, 2.0, 5.5, 9.0, 5.5, math.inf, 9.0]
    assert weight.tolist() == [1.0, 1.0, 1.0, 0.5, 2.0, 0.5, 1.0, 2.0]
    offset, partner, lo, hi, weight = restraint_table([], 3)
    assert offset.tolist() == [0, 0, 0, 0] and partner.numel() == lo.numel() == hi.numel() == weight.numel() == 0


def test_load_restraints(tmp_path):
    from genie2_amd.smc import load_restraints
    path = tmp_path / 'r.txt'
    path.write_text('# i j lo hi [weight]\n\n0 5 4.0 8.5\n 7\t2 0 inf 2.5   # trailing comment\n   \n3 4 1e1 12\n')
    assert load_restraints(str(path)) == [(0, 5, 4.0, 8.5, 1.0), (7, 2, 0.0, math.inf, 2.5), (3, 4, 10.0, 12.0, 1.0)]
    for text, line in (('0 1 2\n', 1), ('0 1 2 3\n0 1 2 3 4 5\n', 2), ('# x\n0 a 2 3\n', 2), ('0 1 2 3\n\n0.5 1 2 3\n', 3), ('0 1 x 3\n', 1)):
        path.write_text(text)
        with pytest.raises(ValueError, match=r'r\.txt:%d: ' % line):
            load_restraints(str(path))


def test_sum_potential_attribute_rules():
    from genie2_amd.smc import SumPotential

    class Plain:
        def __init__(self, v):
            self.v = v

        def __call__(self, x0, step):
            return x0.sum(dim=(1, 2)) * self.v + step

    class Locating(Plain):
        has_fit = False

        def locate(self, x):
            return {'who': self.v}

    class Describing(Plain):
        def describe(self, x):
            return {'who': self.v}

    class LocatingWithoutFlag(Plain):
        def locate(self, x):
            return {'who': self.v}

    x = torch.arange(12.0).reshape(2, 2, 3)
    s = SumPotential(Plain(1.0), Plain(2.0), Plain(0.5))
    assert torch.equal(s(x, 3), (Plain(1.0)(x, 3) + Plain(2.0)(x, 3)) + Plain(0.5)(x, 3))
    assert not hasattr(s, 'locate') and not hasattr(s, 'has_fit') and not hasattr(s, 'describe')
    s = SumPotential(Plain(1.0), Locating(2.0), Describing(3.0), Locating(4.0), Describing(5.0))
    assert s.locate(x) == {'who': 2.0} and s.has_fit is False and s.describe(x) == {'who': 3.0}
    s = SumPotential(LocatingWithoutFlag(7.0))
    assert s.locate(x) == {'who': 7.0} and s.has_fit is True and not hasattr(s, 'describe')
    s = SumPotential(Describing(1.0), Plain(2.0))
    assert s.describe(x) == {'who': 1.0} and not hasattr(s, 'locate') and not hasattr(s, 'has_fit')
    with pytest.raises(ValueError):
        SumPotential()


def test_parsers_constants_and_report(tmp_path, capsys):
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    base = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']
    shape_defaults = dict(rog_max=None, rog_weight=1.0, clash_distance=None, clash_separation=2, clash_weight=1.0, restraint_file=None,
                          shape_tausq=1.0, write_shape_report=False)
    rfile = tmp_path / 'r.txt'
    rfile.write_text('0 45 5 12\n3 9 0 inf 2\n')
    given = ['--rog_max', '14.5', '--rog_weight', '2', '--clash_distance', '3.8', '--clash_separation', '3', '--clash_weight', '0.5',
             '--restraint_file', str(rfile), '--shape_tausq', '4', '--write_shape_report']
    values = dict(rog_max=14.5, rog_weight=2.0, clash_distance=3.8, clash_separation=3, clash_weight=0.5, restraint_file=str(rfile),
                  shape_tausq=4.0, write_shape_report=True)
    for parser, more in ((Sh.build_parser(), []), (M.build_parser(), ['--motif_file', MOTIF])):
        a = vars(parser.parse_args(base + more))
        assert {k: a[k] for k in shape_defaults} == shape_defaults
        a = vars(parser.parse_args(base + more + given))
        assert {k: a[k] for k in values} == values
    a = Sh.build_parser().parse_args(base)
    assert (a.num_samples, a.batch_size, a.min_length, a.max_length, a.length_step, a.num_devices) == (5, 4, 50, 256, 1, 1)
    assert (a.guidance_alpha, a.ess_threshold, a.last_unguided_steps, a.num_steps, a.num_particles) == (0.012, 0.5, 50, None, None)
    assert a.resume is False and a.input_pdb is None and a.start_step is None and a.write_start_rmsd is False
    with pytest.raises(SystemExit):
        Sh.build_parser().parse_args(base + ['--start_step', '5'])                        # --input_pdb and --start_step come together
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(base + given)                                         # --motif_file stays required
    help_text = ' '.join(M.build_parser().format_help().split())
    assert help_text.count('(not in the reference CLI)') == 7
    assert help_text.count('(an addition to the reference CLI, like --align)') == 2 + 8

    # the shape-only CLI needs a term; both runners carry the shape keys and skip lengths the restraints do not fit in
    with pytest.raises(SystemExit, match='no shape term'):
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base)))
    want = dict(rog_max=14.5, rog_weight=2.0, clash_distance=3.8, clash_separation=3, clash_weight=0.5, shape_tausq=4.0,
                write_shape_report=True, restraints=[(0, 45, 5.0, 12.0, 1.0), (3, 9, 0.0, math.inf, 2.0)])
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base + given + ['--num_particles', '3', '--guidance_alpha', '0.1'])))
    assert {k: c[k] for k in want} == want and c['num_particles'] == 3 and c['guidance_alpha'] == 0.1 and c['ess_threshold'] == 0.5
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF] + given)))
    assert {k: c[k] for k in want} == want and c['tausq'] == 0.012
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF])))
    assert c['restraints'] == [] and c['rog_max'] is None and not Sh.has_shape_terms(c)
    assert Sh.shape_potential(c, 50, None, 'cuda') is None                                # no term: no potential, no device
    capsys.readouterr()
    tasks = Sh.ShapeRunner().create_tasks(dict(min_length=44, max_length=48, length_step=1, restraint_file=str(rfile)))
    assert [t['length'] for t in tasks] == [48, 47, 46]
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and '46' in out[0] and '45, 44' in out[0]
    tasks = M.MotifRunner().create_tasks(dict(min_length=10, max_length=47, length_step=1, motif_file=MOTIF, restraint_file=str(rfile)))
    assert [t['length'] for t in tasks] == [47, 46]
    assert len(capsys.readouterr().out.strip().splitlines()) == 2                         # one line for the motif, one for the restraints
    assert [t['length'] for t in Sh.ShapeRunner().create_tasks(dict(min_length=5, max_length=6, length_step=1))] == [6, 5]

    report = {'rog': torch.tensor([12.34567, 9.0]), 'min_distance': torch.tensor([3.8004, math.inf]), 'n_clash': torch.tensor([3, 0]),
              'e_rog': torch.tensor([0.0, 1.5]), 'e_clash': torch.tensor([2.25, 0.0]), 'e_restraint': torch.tensor([10.0006, 0.0]),
              'n_violated': torch.tensor([2, 0]), 'max_violation': torch.tensor([1.0, 0.0])}
    Sh.write_shape_report(report, str(tmp_path / 'shape'), 60, 4)
    assert sorted(os.listdir(tmp_path / 'shape')) == ['60_4.txt', '60_5.txt']
    assert (tmp_path / 'shape' / '60_4.txt').read_text() == ('rog 12.346\nmin_distance 3.800\nn_clash 3\ne_rog 0.000\ne_clash 2.250\n'
                                                             'e_restraint 10.001\nn_violated 2\nmax_violation 1.000\n')
    assert (tmp_path / 'shape' / '60_5.txt').read_text() == ('rog 9.000\nmin_distance inf\nn_clash 0\ne_rog 1.500\ne_clash 0.000\n'
                                                             'e_restraint 0.000\nn_violated 0\nmax_violation 0.000\n')


def test_oracle_gradient_is_the_headers_and_matches_finite_differences():
    """N = 5 with every term active: a clash, a lower and an upper violation, a satisfied restraint with an open upper bound, and a
    radius of gyration above its cap.  Autograd of the float64 oracle against central differences of its logp, and against the
    analytic gradient of include/genie_hip.h."""
    x = torch.tensor([[[0.0, 0.0, 0.0], [3.8, 0.0, 0.0], [5.0, 2.5, 0.3], [2.0, 2.0, 0.5], [-1.0, 4.0, 2.0]],
                      [[0.0, 0.0, 0.0], [3.0, 2.0, 1.0], [0.5, 1.0, 3.0], [6.0, 5.0, 1.0], [9.0, 2.0, -2.0]]], dtype=torch.float64)
    cfg = S.config(rog_max=1.5, rog_weight=0.7, clash_distance=4.0, clash_separation=2, clash_weight=1.3,
                   restraints=[(0, 4, 6.0, 9.0, 2.0), (1, 3, 0.0, 1.5, 0.5), (2, 0, 1.0, math.inf, 1.0), (4, 1, 2.0, 3.0, 1.5)])
    var = 0.8
    ref = S.reference(x, cfg, var)
    assert bool((ref['rog'] > 1.5).all()) and bool((ref['n_clash'] >= 1).all()) and int(ref['n_violated'][0]) == 3
    assert bool((ref['e_rog'] > 0).all()) and bool((ref['e_clash'] > 0).all()) and bool((ref['e_restraint'] > 0).all())
    d04, d13 = float((x[0, 0] - x[0, 4]).norm()), float((x[0, 1] - x[0, 3]).norm())
    assert d04 < 6.0 and d13 > 1.5                                                        # a lower and an upper violation
    assert torch.allclose(ref['logp'], -(ref['e_rog'] + ref['e_clash'] + ref['e_restraint']) / (2 * var), rtol=1e-14, atol=0)
    h, fd = 1e-6, torch.zeros_like(x)
    for idx in range(x.numel()):
        e = torch.zeros(x.numel(), dtype=torch.float64)
        e[idx] = h
        e = e.view_as(x)
        fd.view(-1)[idx] = (S.logp(x + e, cfg, var).sum() - S.logp(x - e, cfg, var).sum()) / (2 * h)
    scale = float(ref['grad'].abs().max())
    assert float((ref['grad'] - fd).abs().max()) <= 1e-7 * scale, float((ref['grad'] - fd).abs().max()) / scale
    assert float((ref['grad'] - S.analytic_gradient(x, cfg, var)).abs().max()) <= 1e-12 * scale
    # coincident residues: no direction, finite everywhere
    y = x.clone()
    y[0, 3] = y[0, 0]
    ref = S.reference(y, S.config(clash_distance=4.0, clash_weight=1.0, restraints=[(0, 3, 1.0, 2.0, 1.0)]), var)
    assert bool(torch.isfinite(ref['grad']).all()) and float(ref['min_distance'][0]) == 0.0
    assert float((ref['grad'] - S.analytic_gradient(y, S.config(clash_distance=4.0, clash_weight=1.0, restraints=[(0, 3, 1.0, 2.0, 1.0)]),
                                                    var)).abs().max()) <= 1e-12 * scale
