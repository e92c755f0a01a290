"""The secondary-structure potential without a device: the C entry's symbol and refusals (genie_secstruct_potential,
include/genie_hip.h), SecStructPotential's and load_ss_target's host-side validation, SumPotential's merge rule, both command lines'
parsers, length skipping and the report writer, and the float64 oracle of tests/_secstruct.py against closed forms and finite
differences."""
import ctypes as C
import math
import os

import pytest
import torch

import _secstruct as S
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


def test_symbol_is_declared_and_loads(lib):
    from genie2_amd import build, capi
    assert 'secstruct_kernels.hip' in build.SOURCES
    assert len(capi.SYMBOLS['genie_secstruct_potential'][1]) == 18 and capi.SYMBOLS['genie_secstruct_potential'][0] is C.c_int
    assert lib.genie_secstruct_potential is not None
    assert len(capi.SECSTRUCT_REPORT) == 8 and capi.SECSTRUCT_REPORT == S.REPORT and capi.SECSTRUCT_TABLE == S.TABLE
    assert len(capi.SYMBOLS['genie_shape_potential'][1]) == 21                                 # (the shape entry keeps its arguments)


def test_entry_refuses_before_the_device_is_touched(lib):
    """Every refusal returns GENIE_E_ARG without a device, and genie_last_error(NULL) names the entry and the argument."""
    d = C.c_void_p(64)                                           # never dereferenced: every call below fails its checks
    inf, nan = math.inf, math.nan

    def call(B=2, N=60, x0=d, table=S.TABLE, helix=(0.2, 0.8), helix_weight=1.0, extended=(0.0, 0.5), extended_weight=1.0, target=d,
             target_weight=1.0, var=d, logp=d, grad=d, report=d, assign=d):
        tab = None if table is None else (C.c_float * 16)(*table)
        rc = lib.genie_secstruct_potential(None, B, N, x0, tab, helix[0], helix[1], helix_weight, extended[0], extended[1],
                                           extended_weight, target, target_weight, var, logp, grad, report, assign)
        return rc, lib.genie_last_error(None)

    cases = [(dict(B=0), b'B'), (dict(B=65536), b'B'), (dict(N=4), b'N'), (dict(N=0), b'N'), (dict(x0=None), b'x0'), (dict(var=None), b'var'),
             (dict(table=None), b'table'), (dict(logp=None, grad=None, report=None, assign=None), b'no output'),
             (dict(logp=None), b'logp_out and grad_out'), (dict(grad=None), b'logp_out and grad_out'),
             (dict(target=None), b'target'), (dict(N=20000), b'LDS')]
    for k in (4, 5, 6, 7, 12, 13, 14, 15):                                                      # every sigma
        for v in (0.0, -0.5, inf, nan):
            cases.append((dict(table=S.TABLE[:k] + (v,) + S.TABLE[k + 1:]), b'sigma'))
    for name in ('helix_weight', 'extended_weight', 'target_weight'):
        cases += [({name: v}, name.encode()) for v in (-1.0, inf, nan)]
    for name in ('helix', 'extended'):
        cases += [({name: v}, name.encode()) for v in ((-0.1, 0.5), (0.2, 1.1), (0.6, 0.4), (nan, 0.5), (0.1, nan), (0.0, inf))]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b'genie_secstruct_potential: ') and word in msg, (kw, rc, msg)
    # what is allowed passes every check (and then fails on the device instead, with another code, or runs): a NULL target at weight
    # 0, a report or an assignment alone, the potential alone, weights of 0, the longest N genie_create accepts, the shortest N
    if not torch.cuda.is_available():
        for kw in (dict(target=None, target_weight=0.0), dict(logp=None, grad=None, assign=None), dict(logp=None, grad=None, report=None),
                   dict(report=None, assign=None), dict(helix_weight=0.0, extended_weight=0.0), dict(N=1512), dict(N=5),
                   dict(helix=(0.0, 0.0)), dict(extended=(1.0, 1.0))):
            assert call(**kw)[0] != -1, kw


def test_constructor_validates_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import SecStructPotential
    abar = torch.linspace(0.999, 0.001, 13)
    good = 'HHHHHH--EEEEE-'
    for kw in (dict(), dict(helix=(0.5,)), dict(helix=0.5), dict(helix=(-0.1, 0.5)), dict(helix=(0.6, 0.5)), dict(helix=(0.5, 1.5)),
               dict(helix=(math.nan, 1.0)), dict(extended=(0.2, 0.1)), dict(extended=(0.0, math.inf)),
               dict(helix=(0.5, 1.0), helix_weight=-1.0), dict(helix=(0.5, 1.0), helix_weight=math.inf),
               dict(extended=(0.0, 0.3), extended_weight=math.nan), dict(target=good, target_weight=-2.0),
               dict(helix=(0.5, 1.0), tausq=0.0), dict(helix=(0.5, 1.0), tausq=math.inf),
               dict(target=good[:-1]), dict(target=good + '-'), dict(target='HHHHHHCCEEEEE-'), dict(target='hhhhhh--EEEEE-'),
               dict(target='HHHH-EEEE-HHHH'), dict(target='-' * 14), dict(target=[1] * 14),
               dict(helix=(0.5, 1.0), table=S.TABLE[:15]), dict(helix=(0.5, 1.0), table=S.TABLE[:4] + (0.0,) + S.TABLE[5:]),
               dict(helix=(0.5, 1.0), table=S.TABLE[:13] + (-1.0,) + S.TABLE[14:]), dict(helix=(0.5, 1.0), table=(math.nan,) + S.TABLE[1:])):
        with pytest.raises(ValueError):
            SecStructPotential(14, abar, device='cpu', **kw)      # (before the device: a CPU potential is a GenieError)
    with pytest.raises(ValueError):
        SecStructPotential(4, abar, helix=(0.5, 1.0), device='cpu')
    for kw in (dict(helix=(0.5, 1.0)), dict(extended=(0.0, 0.2)), dict(target=good), dict(helix=(0.0, 1.0), target=good, table=S.TABLE)):
        with pytest.raises(capi.GenieError, match='no CPU path'):
            SecStructPotential(14, abar, device='cpu', **kw)


def test_load_ss_target(tmp_path):
    from genie2_amd.smc import load_ss_target, ss_string, ss_target_windows
    assert load_ss_target('HHHHH--CCEEEEE') == 'HHHHH----EEEEE'
    assert load_ss_target(' HH HHH\n-E ') == 'HHHHH-E'
    path = tmp_path / 'bp.txt'
    path.write_text('# a helix, a turn, a strand\nHHHHHHH   # helix\n\n--CC\n EEEEE\t# strand\n')
    assert load_ss_target(str(path)) == 'HHHHHHH----EEEEE'
    for bad in ('HHXHH', 'hhhhh', '', '   ', str(tmp_path / 'missing.txt')):
        with pytest.raises(ValueError):
            load_ss_target(bad)
    path.write_text('HHHHH\nEEEEE 5\n')
    with pytest.raises(ValueError, match='bp.txt'):
        load_ss_target(str(path))
    path.write_text('# nothing\n')
    with pytest.raises(ValueError):
        load_ss_target(str(path))
    assert ss_target_windows('HHHHHH--EEEEE-') == 3 and ss_target_windows('HHHH-EEEE') == 0 and ss_target_windows('HHHHEEEEE') == 1
    assert ss_target_windows('-----') == 0 and ss_target_windows('HHHH') == 0
    assert [ss_target_windows(S.blueprint(n)) for n in (5, 6, 8, 9, 24)] == [int((S.target_windows(S.blueprint(n), n) > 0).sum())
                                                                              for n in (5, 6, 8, 9, 24)]
    assert ss_string([0, 1, 1, 2, 0]) == 'CHHEC' and ss_string(torch.tensor([2, 2, 0], dtype=torch.int8)) == 'EEC'


def test_sum_potential_merges_reports_and_takes_the_first_assign():
    from genie2_amd.smc import SumPotential

    class Plain:
        def __call__(self, x0, step):
            return x0.sum(dim=(1, 2)) + step

    class Describing(Plain):
        def __init__(self, **report):
            self.report = report

        def describe(self, x):
            return dict(self.report)

    class Assigning(Describing):
        def assign(self, x):
            return ('assign', tuple(self.report))

    x = torch.zeros(2, 5, 3)
    s = SumPotential(Plain(), Describing(a=1, b=2), Plain(), Assigning(c=3, a=10), Describing(d=4, b=20), Assigning(e=5))
    got = s.describe(x)
    assert got == dict(a=1, b=2, c=3, d=4, e=5) and list(got) == ['a', 'b', 'c', 'd', 'e']          # member order, the first one wins
    assert s.assign(x) == ('assign', ('c', 'a')) and not hasattr(s, 'locate')
    s = SumPotential(Describing(a=1), Describing(a=2))
    assert s.describe(x) == dict(a=1) and not hasattr(s, 'assign')
    s = SumPotential(Plain(), Plain())
    assert not hasattr(s, 'describe') and not hasattr(s, 'assign')
    assert torch.equal(s(x, 3), Plain()(x, 3) + Plain()(x, 3))


def test_parsers_constants_lengths_and_report(tmp_path, capsys):
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    import genie.sample_unconditional_shape as mirror
    import genie.sampler.secstruct as mirror_s
    from genie2_amd.smc import SecStructPotential, load_ss_target
    assert mirror.add_secstruct_arguments is Sh.add_secstruct_arguments and mirror.secstruct_potential is Sh.secstruct_potential
    assert mirror_s.SecStructPotential is SecStructPotential and mirror_s.load_ss_target is load_ss_target
    base = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']
    defaults = dict(helix_min=None, helix_max=None, helix_weight=1.0, extended_min=None, extended_max=None, extended_weight=1.0,
                    ss_target=None, ss_target_weight=1.0, ss_tausq=1.0, write_secstruct=False)
    bp = tmp_path / 'bp.txt'
    bp.write_text('# 46 residues\n' + 'HHHHHHHHHH\n' + 'CC--\n' + 'E' * 12 + '\n' + '-' * 20 + '\n')
    given = ['--helix_min', '0.4', '--helix_max', '0.9', '--helix_weight', '2', '--extended_max', '0.1', '--extended_weight', '0.5',
             '--ss_target', str(bp), '--ss_target_weight', '3', '--ss_tausq', '4', '--write_secstruct']
    values = dict(helix_min=0.4, helix_max=0.9, helix_weight=2.0, extended_min=None, extended_max=0.1, extended_weight=0.5,
                  ss_target=str(bp), ss_target_weight=3.0, ss_tausq=4.0, write_secstruct=True)
    for parser, more in ((Sh.build_parser(), []), (M.build_parser(), ['--motif_file', MOTIF])):
        a = vars(parser.parse_args(base + more))
        assert {k: a[k] for k in defaults} == defaults
        a = vars(parser.parse_args(base + more + given))
        assert {k: a[k] for k in values} == values

    # constants: one of min / max given leaves the other at 0 / 1; the blueprint is read once
    want = dict(helix=(0.4, 0.9), helix_weight=2.0, extended=(0.0, 0.1), extended_weight=0.5, ss_target='H' * 10 + '----' + 'E' * 12 + '-' * 20,
                ss_target_weight=3.0, ss_tausq=4.0, write_secstruct=True)
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base + given)))          # no shape term: a secstruct term is enough
    assert {k: c[k] for k in want} == want and not Sh.has_shape_terms(c) and Sh.has_secstruct_terms(c)
    assert Sh.shape_potential(c, 46, None, 'cuda') is None
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF] + given)))
    assert {k: c[k] for k in want} == want and c['tausq'] == 0.012
    c = Sh.secstruct_constants(vars(Sh.build_parser().parse_args(base + ['--helix_min', '0.5'])))
    assert c['helix'] == (0.5, 1.0) and c['extended'] is None and c['ss_target'] is None and Sh.has_secstruct_terms(c)
    c = Sh.secstruct_constants(vars(Sh.build_parser().parse_args(base + ['--extended_max', '0.25', '--ss_target', 'HHHHHC'])))
    assert c['helix'] is None and c['extended'] == (0.0, 0.25) and c['ss_target'] == 'HHHHH-'
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF])))
    assert c['helix'] is None and c['extended'] is None and c['ss_target'] is None and not Sh.has_secstruct_terms(c)
    assert Sh.secstruct_potential(c, 50, None, 'cuda') is None                               # no term: no potential, no device
    with pytest.raises(SystemExit, match='no shape term'):
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base + ['--helix_weight', '2', '--write_secstruct'])))
    with pytest.raises(ValueError):
        Sh.secstruct_constants(dict(ss_target='HHHXH'))

    # the potentials asked for, in the order given; None when there is none
    a, b = object(), object()
    assert Sh.sum_potentials(None, None) is None and Sh.sum_potentials(None, a, None) is a
    both = Sh.sum_potentials(lambda x, s: 1, None, lambda x, s: 2)
    assert type(both).__name__ == 'SumPotential' and len(both.potentials) == 2 and both(None, 0) == 3

    # a sampled length other than the blueprint's is skipped with one printed line
    capsys.readouterr()
    tasks = Sh.ShapeRunner().create_tasks(dict(min_length=44, max_length=48, length_step=1, ss_target=str(bp)))
    assert [t['length'] for t in tasks] == [46]
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and '46 residues' in out[0] and '48, 47, 45, 44' in out[0]
    tasks = M.MotifRunner().create_tasks(dict(min_length=10, max_length=47, length_step=1, motif_file=MOTIF, ss_target=str(bp)))
    assert [t['length'] for t in tasks] == [46]
    assert len(capsys.readouterr().out.strip().splitlines()) == 2                            # one line for the motif, one for the blueprint
    assert [t['length'] for t in Sh.ShapeRunner().create_tasks(dict(min_length=5, max_length=6, length_step=1))] == [6, 5]
    assert [t['length'] for t in Sh.ShapeRunner().create_tasks(dict(min_length=46, max_length=46, length_step=1, ss_target=str(bp)))] == [46]
    assert capsys.readouterr().out.strip() == ''                                             # nothing skipped: nothing printed

    # the report files: the shape file keeps its eight fields of a merged report, the secstruct file is the string and its eight
    from genie2_amd import capi
    merged = {'rog': torch.tensor([12.34567, 9.0]), 'min_distance': torch.tensor([3.8004, math.inf]), 'n_clash': torch.tensor([3, 0]),
              'e_rog': torch.tensor([0.0, 1.5]), 'e_clash': torch.tensor([2.25, 0.0]), 'e_restraint': torch.tensor([10.0006, 0.0]),
              'n_violated': torch.tensor([2, 0]), 'max_violation': torch.tensor([1.0, 0.0]),
              'helix_content': torch.tensor([0.41239, 0.0]), 'extended_content': torch.tensor([0.1, 0.25]), 'n_helix': torch.tensor([4, 0]),
              'n_extended': torch.tensor([0, 5]), 'e_helix': torch.tensor([1.23456, 0.0]), 'e_extended': torch.tensor([0.0, 2.0]),
              'e_target': torch.tensor([100.0004, 0.5]), 'n_target_missed': torch.tensor([1, 6])}
    assert list(Sh.report_fields(merged, capi.SHAPE_REPORT)) == list(capi.SHAPE_REPORT)
    Sh.write_shape_report(Sh.report_fields(merged, capi.SHAPE_REPORT), str(tmp_path / 'shape'), 6, 4)
    assert (tmp_path / 'shape' / '6_4.txt').read_text() == ('rog 12.346\nmin_distance 3.800\nn_clash 3\ne_rog 0.000\ne_clash 2.250\n'
                                                            'e_restraint 10.001\nn_violated 2\nmax_violation 1.000\n')
    assign = torch.tensor([[1, 1, 1, 1, 0, 0], [0, 2, 2, 2, 2, 2]], dtype=torch.int8)
    Sh.write_secstruct_report(assign, Sh.report_fields(merged, capi.SECSTRUCT_REPORT), str(tmp_path / 'secstruct'), 6, 4)
    assert sorted(os.listdir(tmp_path / 'secstruct')) == ['6_4.txt', '6_5.txt']
    assert (tmp_path / 'secstruct' / '6_4.txt').read_text() == ('HHHHCC\nhelix_content 0.412\nextended_content 0.100\nn_helix 4\nn_extended 0\n'
                                                                'e_helix 1.235\ne_extended 0.000\ne_target 100.000\nn_target_missed 1\n')
    assert (tmp_path / 'secstruct' / '6_5.txt').read_text() == ('CEEEEE\nhelix_content 0.000\nextended_content 0.250\nn_helix 0\nn_extended 5\n'
                                                                'e_helix 0.000\ne_extended 2.000\ne_target 0.500\nn_target_missed 6\n')


def test_reference_against_closed_forms():
    """Ideal coordinates against the figures the table was chosen by: a right-handed helix is a helix, its mirror image is not (its
    distances are the same: only chi tells them apart), an extended chain is extended."""
    cfg = S.config()
    helix, mirror, ext = (S.terms(x[None], cfg) for x in (S.ideal_helix(14), S.ideal_helix(14, -1.0), S.ideal_extended(14)))
    assert float(helix['u'][0, :, 0].max()) < 0.2 and float(mirror['u'][0, :, 0].min()) > 5 and float(ext['u'][0, :, 1].max()) < 0.3
    assert float(ext['u'][0, :, 0].min()) > 50 and float(helix['u'][0, :, 1].min()) > 10
    f, fm = S.features(S.ideal_helix(14)[None]), S.features(S.ideal_helix(14, -1.0)[None])
    assert torch.allclose(f[..., :3], fm[..., :3], rtol=1e-13, atol=0) and torch.allclose(f[..., 3], -fm[..., 3], rtol=1e-13, atol=0)
    assert abs(float(f[0, 0, 3]) - 0.767) < 1e-3 and abs(float(S.features(S.ideal_extended(9)[None])[0, 0, 3]) + 0.217) < 1e-3
    assert helix['assign'].tolist() == [[1] * 14] and mirror['assign'].tolist() == [[0] * 14] and ext['assign'].tolist() == [[2] * 14]
    assert float(helix['helix_content']) > 1 / 1.2 and float(mirror['helix_content']) < 1 / 6
    # the content hinge and the blueprint, by hand, on the helix: W = 10 windows
    cfg = S.config(helix=(0.0, 0.5), helix_weight=2.0, extended=(0.3, 1.0), extended_weight=3.0, target='-' * 4 + 'E' * 6 + 'HHHH', target_weight=0.5)
    t = S.terms(S.ideal_helix(14)[None], cfg)
    n_h, n_e = float((1 / (1 + t['u'][0, :, 0])).sum()), float((1 / (1 + t['u'][0, :, 1])).sum())
    assert float(t['e_helix']) == pytest.approx(2.0 * (n_h - 5.0) ** 2, rel=1e-12) and n_h > 5
    assert float(t['e_extended']) == pytest.approx(3.0 * (3.0 - n_e) ** 2, rel=1e-12) and n_e < 3
    assert float(t['e_target']) == pytest.approx(0.5 * float(t['u'][0, 4:6, 1].sum()), rel=1e-12)      # windows 4 and 5 are all E
    assert int(t['n_target_missed']) == 6 and int(t['n_helix']) == 14                           # the four H residues are met


def test_reference_gradient_matches_finite_differences():
    x = S.mixed_chain(2, 24, 1).double()
    cfg = S.chain_config(x)
    var = 0.8
    ref = S.reference(x, cfg, var)
    assert bool((ref['e_helix'] > 0).all()) and bool((ref['e_extended'] > 0).all()) and bool((ref['e_target'] > 0).all())
    assert torch.allclose(ref['logp'], -(ref['e_helix'] + ref['e_extended'] + ref['e_target']) / (2 * var), rtol=1e-14, atol=0)
    h, fd = 1e-6, torch.zeros_like(x)
    for idx in range(x.numel()):
        e = torch.zeros(x.numel(), dtype=torch.float64)
        e[idx] = h
        e = e.view_as(x)
        fd.view(-1)[idx] = (S.logp(x + e, cfg, var).sum() - S.logp(x - e, cfg, var).sum()) / (2 * h)
    scale = float(ref['grad'].abs().max())
    assert float((ref['grad'] - fd).abs().max()) <= 1e-7 * scale, float((ref['grad'] - fd).abs().max()) / scale
    # degenerate inputs: coincident residues and a chain in one point are finite, with no force from what has no direction
    y = x.clone()
    y[0, 7] = y[0, 5]                                              # d2 of window 5 is 0
    y[1, 11] = y[1, 10]                                            # a bond of length 0: chi of the windows 8..10 is 0
    ref = S.reference(y, cfg, var)
    assert bool(torch.isfinite(ref['grad']).all()) and bool(torch.isfinite(ref['logp']).all())
    f = S.features(y)
    assert float(f[0, 5, 0]) == 0.0 and f[1, 8:11, 3].tolist() == [0.0, 0.0, 0.0] and float(f[1, 7, 3]) != 0.0
    ref = S.reference(torch.full((1, 9, 3), 2.5), S.config(helix=(0.5, 1.0), helix_weight=1.0, target='HHHHHEEEE', target_weight=1.0), var)
    assert bool((ref['grad'] == 0).all()) and bool(torch.isfinite(ref['logp']).all()) and ref['assign'].tolist() == [[0] * 9]
