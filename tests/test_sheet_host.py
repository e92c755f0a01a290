"""The sheet potential without a device: the C entry's symbol and refusals (genie_sheet_potential, include/genie_hip.h),
SheetPotential's, load_ladder's, check_ladder's and ladder_table's host side, SumPotential's `pairs` rule, both command lines' parsers,
length skipping and the report writer, and the float64 oracle of tests/_sheet.py against closed forms, an analytic gradient written
with loops and finite differences.

The last two tests (test_reference_...) run tests/_sheet.py alone: they pin the oracle and the defaults' figures, not the kernel or
the package, and so pass on a tree without the sheet potential.  What holds the kernel to the oracle is tests/test_sheet_gpu.py."""
import ctypes as C
import math
import os

import pytest
import torch

import _sheet as S
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


def test_symbol_is_declared_and_loads(lib):
    from genie2_amd import build, capi
    assert 'sheet_kernels.hip' in build.SOURCES
    assert len(capi.SYMBOLS['genie_sheet_potential'][1]) == 29 and capi.SYMBOLS['genie_sheet_potential'][0] is C.c_int
    assert capi.SYMBOLS['genie_sheet_potential_work_bytes'] == (C.c_size_t, [C.c_int, C.c_int])
    assert lib.genie_sheet_potential is not None
    assert len(capi.SHEET_REPORT) == 9 and capi.SHEET_REPORT == S.REPORT and capi.SHEET_COUNTS == S.COUNTS and capi.SHEET_TABLE == S.TABLE
    assert lib.genie_sheet_potential_work_bytes(3, 65) == 3 * (36 * 65 + 32 * 2) and lib.genie_sheet_potential_work_bytes(1, 64) == 36 * 64 + 32
    assert lib.genie_sheet_potential_work_bytes(0, 5) == 0 and lib.genie_sheet_potential_work_bytes(2, 0) == 0
    assert len(capi.SYMBOLS['genie_secstruct_potential'][1]) == 18                             # (the neighbours keep their arguments)


def test_entry_refuses_before_the_device_is_touched(lib):
    """Every refusal returns GENIE_E_ARG without a device, and genie_last_error(NULL) names the entry and the argument."""
    d = C.c_void_p(64)                                           # never dereferenced: every call below fails its checks
    inf, nan = math.inf, math.nan

    def call(B=2, N=60, x0=d, table=S.TABLE, separation=(3, 5), antiparallel=(0.1, 0.8), antiparallel_weight=1.0, parallel=(0.0, inf),
             parallel_weight=1.0, L2=4, lad=(d, d, d, d), ladder_weight=1.0, var=d, logp=d, grad=d, report=d, pairs=d, work=d,
             work_bytes=None):
        if work_bytes is None:
            work_bytes = lib.genie_sheet_potential_work_bytes(B, N) if B >= 1 and N >= 1 else 0
        rc = lib.genie_sheet_potential(None, B, N, x0, *table, *separation, antiparallel[0], antiparallel[1], antiparallel_weight,
                                       parallel[0], parallel[1], parallel_weight, L2, *lad, ladder_weight, var, logp, grad, report,
                                       pairs, work, work_bytes)
        return rc, lib.genie_last_error(None)

    cases = [(dict(B=0), b'B'), (dict(B=65536), b'B'), (dict(N=0), b'N'), (dict(x0=None), b'x0'), (dict(var=None), b'var'),
             (dict(logp=None, grad=None, report=None, pairs=None), b'no output'),
             (dict(logp=None), b'logp_out and grad_out'), (dict(grad=None), b'logp_out and grad_out'),
             (dict(separation=(2, 5)), b'separation_antiparallel'), (dict(separation=(3, 2)), b'separation_parallel'),
             (dict(separation=(0, 5)), b'separation_antiparallel'), (dict(separation=(3, -1)), b'separation_parallel'),
             (dict(L2=-2), b'L2'), (dict(L2=3), b'L2'), (dict(work=None), b'work'), (dict(work_bytes=0), b'work_bytes'),
             (dict(work_bytes=2 * (36 * 60 + 32) - 1), b'work_bytes'), (dict(work=C.c_void_p(66)), b'aligned'), (dict(N=12459), b'LDS'),
             (dict(N=20000), b'LDS')]
    for k in range(4):
        cases.append((dict(lad=tuple(None if i == k else d for i in range(4))), b'ladder table'))
    for k, word in ((1, b'sigma_antiparallel'), (3, b'sigma_parallel')):
        for v in (0.0, -0.5, inf, nan):
            cases.append((dict(table=S.TABLE[:k] + (v,) + S.TABLE[k + 1:]), word))
    for k, word in ((0, b'mu_antiparallel'), (2, b'mu_parallel')):
        for v in (inf, nan):
            cases.append((dict(table=S.TABLE[:k] + (v,) + S.TABLE[k + 1:]), word))
    for name in ('antiparallel_weight', 'parallel_weight', 'ladder_weight'):
        cases += [({name: v}, name.encode()) for v in (-1.0, inf, nan)]
    for name in ('antiparallel', 'parallel'):
        cases += [({name: v}, name.encode() + b'_min') for v in ((-0.1, 0.5), (0.6, 0.4), (nan, 0.5), (0.1, nan), (inf, inf), (0.2, -1.0))]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b'genie_sheet_potential: ') and word in msg, (kw, rc, msg)
    # what is allowed passes every check (and then fails on the device instead, with another code, or runs): no ladder, a report or
    # the pairs alone, the potential alone, weights of 0, N below 6 (no eligible rung), the longest N that fits, no upper bound
    if not torch.cuda.is_available():
        for kw in (dict(L2=0, lad=(None,) * 4), dict(logp=None, grad=None, pairs=None), dict(logp=None, grad=None, report=None),
                   dict(report=None, pairs=None), dict(antiparallel_weight=0.0, parallel_weight=0.0, ladder_weight=0.0), dict(N=1),
                   dict(N=5), dict(N=1512), dict(N=12458), dict(antiparallel=(0.0, 0.0)), dict(parallel=(2.0, inf)),
                   dict(separation=(3, 3)), dict(separation=(7, 9))):
            assert call(**kw)[0] != -1, kw


def test_constructor_validates_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import SheetPotential
    abar = torch.linspace(0.999, 0.001, 13)
    good = [(2, 11, 3, 'A'), (3, 9, 2, 'P', 0.5)]
    a = dict(antiparallel=(0.2, math.inf))
    for kw in (dict(), dict(ladder=[]), dict(antiparallel=(0.5,)), dict(antiparallel=0.5), dict(antiparallel=(-0.1, 0.5)),
               dict(antiparallel=(0.6, 0.5)), dict(antiparallel=(math.nan, 1.0)), dict(antiparallel=(math.inf, math.inf)),
               dict(parallel=(0.2, 0.1)), dict(parallel=(0.0, math.nan)), dict(a, antiparallel_weight=-1.0),
               dict(a, antiparallel_weight=math.inf), dict(parallel=(0.0, 0.3), parallel_weight=math.nan),
               dict(ladder=good, ladder_weight=-2.0), dict(a, tausq=0.0), dict(a, tausq=math.inf),
               dict(a, separation=(2, 5)), dict(a, separation=(3, 2)), dict(a, separation=(3,)), dict(a, separation=3),
               dict(a, separation=(3.0, 5)), dict(a, table=S.TABLE[:3]), dict(a, table=(5.0, 0.0, 4.8, 0.5)),
               dict(a, table=(5.0, 0.6, 4.8, -1.0)), dict(a, table=(math.nan,) + S.TABLE[1:]),
               dict(ladder=[(0, 9, 1, 'A')]), dict(ladder=[(2, 13, 1, 'A')]), dict(ladder=[(2, 11, 5, 'A')]), dict(ladder=[(3, 9, 5, 'P')]),
               dict(ladder=[(4, 6, 1, 'A')]), dict(ladder=[(2, 11, 0, 'A')]), dict(ladder=[(2, 11, 1, 'X')]),
               dict(ladder=[(2, 11, 1, 'A', -1.0)]), dict(ladder=[(2, 11, 1, 'A', math.inf)]), dict(ladder=[(2.0, 11, 1, 'A')]),
               dict(ladder=[(2, 11, 2, 'A'), (10, 3, 1, 'A')]), dict(ladder=[(2, 11, 1)])):
        with pytest.raises(ValueError):
            SheetPotential(14, abar, device='cpu', **kw)         # (before the device: a CPU potential is a GenieError)
    with pytest.raises(ValueError):
        SheetPotential(0, abar, device='cpu', **a)
    for kw in (a, dict(parallel=(0.0, 0.2)), dict(ladder=good), dict(a, ladder=good, table=S.TABLE, separation=(4, 4)),
               dict(ladder=[(2, 11, 1, 'A'), (2, 11, 1, 'P')])):
        with pytest.raises(capi.GenieError, match='no CPU path'):
            SheetPotential(14, abar, device='cpu', **kw)
    with pytest.raises(capi.GenieError, match='no CPU path'):
        SheetPotential(3, abar, device='cpu', **a)              # (a chain without an eligible rung is allowed)


def test_load_check_and_table_of_a_ladder(tmp_path):
    from genie2_amd import capi
    from genie2_amd.smc import check_ladder, ladder_table, load_ladder
    path = tmp_path / 'ladder.txt'
    path.write_text('# a hairpin and a parallel pair\n2 9 2 A 0.5   # 2-9, 3-8\n\n3 12 1 P\n')
    ladder = load_ladder(str(path))
    assert ladder == [(2, 9, 2, 'A', 0.5), (3, 12, 1, 'P', 1.0)]
    for bad in ('2 9 2\n', '2 9 2 A 1 7\n', 'a 9 2 A\n', '2 9 2.5 A\n', '2 9 2 B\n', '2 9 2 a\n', '2 9 2 A x\n'):
        path.write_text('# ok\n' + bad)
        with pytest.raises(ValueError, match='ladder.txt:2'):
            load_ladder(str(path))
    rungs = check_ladder(ladder, 16)
    assert rungs == [(2, 9, 'A', 0.5), (3, 8, 'A', 0.5), (3, 12, 'P', 1.0)]
    assert check_ladder([(9, 2, 2, 'A')], 16) == [(2, 9, 'A', 1.0), (1, 10, 'A', 1.0)]          # ordered: i < j
    assert [(r[0], r[1], 'AP'[r[2]], r[3]) for r in S.rungs(ladder)] == rungs                    # the oracle's own expansion agrees
    with pytest.raises(ValueError):
        check_ladder(ladder, 13)                                  # the centre 12 of 3-12 P is above N - 2: its d2 would need residue 13
    assert check_ladder(ladder, 14) == rungs

    # the table by hand: every rung gives (d0, d1, d2) terms of weight / (3 sigma^2); D[3, 8] is the d2 of 2-9 and the d0 of 3-8,
    # D[2, 9] the d0 of 2-9 and the d1 of 3-8
    offset, word, mu, coef = ladder_table(rungs, 16)
    ca, cp = 0.5 / (3 * 0.6 ** 2), 1.0 / (3 * 0.5 ** 2)
    want = {(2, 9, 0): (2 * ca, True), (1, 10, 0): (ca, False), (3, 8, 0): (2 * ca, True), (4, 7, 0): (ca, False),
            (3, 12, 1): (cp, True), (2, 11, 1): (cp, False), (4, 13, 1): (cp, False)}
    assert offset.dtype == torch.int32 and word.dtype == torch.int32 and mu.dtype == torch.float32 and coef.dtype == torch.float32
    assert offset.tolist()[0] == 0 and offset.tolist()[-1] == 2 * len(want) == word.numel() == mu.numel() == coef.numel()
    got = {}
    for n in range(16):
        partners = []
        for k in range(int(offset[n]), int(offset[n + 1])):
            w = int(word[k])
            p, c, rung = w & (capi.SHEET_PARALLEL - 1), int(bool(w & capi.SHEET_PARALLEL)), bool(w & capi.SHEET_RUNG)
            partners.append((p, c))
            assert float(mu[k]) == pytest.approx(S.TABLE[2 * c], rel=1e-7)
            got.setdefault((min(n, p), max(n, p), c), []).append((float(coef[k]), rung))
        assert partners == sorted(partners)                       # partners ascending within a residue
    assert set(got) == set(want)
    for key, (cf, rung) in want.items():
        assert len(got[key]) == 2 and all(g[1] == rung and g[0] == pytest.approx(cf, rel=1e-6) for g in got[key]), key
    # the table's energy is the oracle's ladder energy
    x = S.sheet_chain(1, 16, 3).double()
    e = sum(cf * (float((x[0, p] - x[0, q]).norm()) - S.TABLE[2 * c]) ** 2 for (p, q, c), (cf, _) in want.items())
    t = S.terms(x, S.config(ladder=ladder, ladder_weight=1.0))
    assert float(t['e_ladder']) == pytest.approx(e, rel=1e-12)
    # another table changes mu and the coefficients; no rung: an empty table
    _, _, mu2, coef2 = ladder_table(rungs, 16, (6.0, 1.2, 4.0, 0.25))
    assert set(mu2.tolist()) == {6.0, 4.0} and float(coef2.max()) == pytest.approx(1.0 / (3 * 0.25 ** 2), rel=1e-6)
    offset, word, mu, coef = ladder_table([], 7)
    assert offset.tolist() == [0] * 8 and word.numel() == 0


def test_sum_potential_takes_the_first_pairs():
    from genie2_amd.smc import SumPotential

    class Plain:
        def __call__(self, x0, step):
            return x0.sum(dim=(1, 2)) + step

    class Pairing(Plain):
        def __init__(self, tag):
            self.tag = tag

        def pairs(self, x):
            return ('pairs', self.tag)

        def describe(self, x):
            return {self.tag: 1}

    x = torch.zeros(2, 5, 3)
    s = SumPotential(Plain(), Pairing('a'), Pairing('b'))
    assert s.pairs(x) == ('pairs', 'a') and s.describe(x) == dict(a=1, b=1) and not hasattr(s, 'assign') and not hasattr(s, 'locate')
    assert not hasattr(SumPotential(Plain(), Plain()), 'pairs')


def test_parsers_constants_lengths_and_report(tmp_path, capsys):
    from genie2_amd import capi
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    import genie.sample_unconditional_shape as mirror
    import genie.sampler.sheet as mirror_s
    from genie2_amd.smc import SheetPotential, check_ladder, load_ladder
    assert mirror.add_sheet_arguments is Sh.add_sheet_arguments and mirror.sheet_potential is Sh.sheet_potential
    assert mirror_s.SheetPotential is SheetPotential and mirror_s.load_ladder is load_ladder
    base = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']
    defaults = dict(antiparallel_min=None, antiparallel_max=None, antiparallel_weight=1.0, parallel_min=None, parallel_max=None,
                    parallel_weight=1.0, ladder_file=None, ladder_weight=1.0, sheet_tausq=1.0, write_sheet=False)
    lad = tmp_path / 'ladder.txt'
    lad.write_text('# a hairpin\n4 44 5 A\n10 30 3 P 0.5\n')
    given = ['--antiparallel_min', '0.3', '--antiparallel_weight', '2', '--parallel_max', '0.05', '--parallel_weight', '0.5',
             '--ladder_file', str(lad), '--ladder_weight', '3', '--sheet_tausq', '4', '--write_sheet']
    values = dict(antiparallel_min=0.3, antiparallel_max=None, antiparallel_weight=2.0, parallel_min=None, parallel_max=0.05,
                  parallel_weight=0.5, ladder_file=str(lad), ladder_weight=3.0, sheet_tausq=4.0, write_sheet=True)
    for parser, more in ((Sh.build_parser(), []), (M.build_parser(), ['--motif_file', MOTIF])):
        a = vars(parser.parse_args(base + more))
        assert {k: a[k] for k in defaults} == defaults
        a = vars(parser.parse_args(base + more + given))
        assert {k: a[k] for k in values} == values

    # constants: only a min leaves the content unbounded above, only a max starts at 0; the ladder file is read into 'ladder'
    want = dict(antiparallel=(0.3, math.inf), antiparallel_weight=2.0, parallel=(0.0, 0.05), parallel_weight=0.5,
                ladder=[(4, 44, 5, 'A', 1.0), (10, 30, 3, 'P', 0.5)], ladder_weight=3.0, sheet_tausq=4.0, write_sheet=True)
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base + given)))          # a sheet term is enough on its own
    assert {k: c[k] for k in want} == want and Sh.has_sheet_terms(c) and not Sh.has_shape_terms(c) and not Sh.has_secstruct_terms(c)
    assert Sh.shape_potential(c, 46, None, 'cuda') is None and Sh.secstruct_potential(c, 46, None, 'cuda') is None
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF] + given)))
    assert {k: c[k] for k in want} == want and c['tausq'] == 0.012
    c = Sh.sheet_constants(vars(Sh.build_parser().parse_args(base + ['--parallel_min', '0.2', '--parallel_max', '0.6'])))
    assert c['parallel'] == (0.2, 0.6) and c['antiparallel'] is None and c['ladder'] == [] and Sh.has_sheet_terms(c)
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF])))
    assert c['antiparallel'] is None and c['parallel'] is None and c['ladder'] == [] and not Sh.has_sheet_terms(c)
    assert Sh.sheet_potential(c, 50, None, 'cuda') is None                                   # no term: no potential, no device
    with pytest.raises(SystemExit, match='no shape term'):
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base + ['--antiparallel_weight', '2', '--write_sheet'])))
    for flag in ('--ladder_file', '--antiparallel_max', '--parallel_min'):
        args = base + [flag, str(lad) if flag == '--ladder_file' else '0.5']
        assert Sh.has_sheet_terms(Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(args))))

    # a sampled length that cannot hold the ladder (its highest centre is 44, and a centre is at most N - 2) is skipped
    assert Sh.sum_potentials(None, None, None, None) is None
    capsys.readouterr()
    tasks = Sh.ShapeRunner().create_tasks(dict(min_length=44, max_length=48, length_step=1, ladder_file=str(lad)))
    assert [t['length'] for t in tasks] == [48, 47, 46]
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and 'ladder' in out[0] and '45, 44' in out[0]
    lad2 = tmp_path / 'ladder2.txt'
    lad2.write_text('4 41 5 A\n')                                                             # highest centre 41: N >= 43
    assert [t['length'] for t in Sh.ladder_lengths([{'length': n} for n in (44, 43, 42)], load_ladder(str(lad2)))] == [44, 43]
    capsys.readouterr()
    tasks = M.MotifRunner().create_tasks(dict(min_length=10, max_length=47, length_step=1, motif_file=MOTIF, ladder_file=str(lad)))
    assert [t['length'] for t in tasks] == [47, 46]
    assert len(capsys.readouterr().out.strip().splitlines()) == 2                            # one line for the motif, one for the ladder
    assert [t['length'] for t in Sh.ShapeRunner().create_tasks(dict(min_length=5, max_length=6, length_step=1))] == [6, 5]
    assert capsys.readouterr().out.strip() == ''                                             # nothing skipped: nothing printed
    assert len(check_ladder(load_ladder(str(lad)), 46)) == 8                                 # the skip rule is check_ladder's rule
    with pytest.raises(ValueError):
        check_ladder(load_ladder(str(lad)), 45)

    # the report files: the sheet file is its rungs and its nine fields of a merged report; the others keep theirs
    merged = {'rog': torch.tensor([12.34567, 9.0]), 'helix_content': torch.tensor([0.41239, 0.0]),
              'antiparallel_content': torch.tensor([0.41239, 0.0]), 'parallel_content': torch.tensor([0.1, 0.25]),
              'n_antiparallel': torch.tensor([2, 0]), 'n_parallel': torch.tensor([1, 0]), 'n_paired': torch.tensor([6, 0]),
              'e_antiparallel': torch.tensor([1.23456, 0.0]), 'e_parallel': torch.tensor([0.0, 2.0]),
              'e_ladder': torch.tensor([100.0004, 0.5]), 'n_ladder_missed': torch.tensor([1, 6])}
    assert list(Sh.report_fields(merged, capi.SHEET_REPORT)) == list(capi.SHEET_REPORT)
    none = [-1, -1]
    pairs = torch.tensor([[none, [8, -1], [7, 6], none, none, none, [-1, 2], [2, -1], [1, -1]], [none] * 9], dtype=torch.int32)
    assert Sh.formed_rungs(pairs[0]) == ['1 8 A', '2 7 A', '2 6 P'] and Sh.formed_rungs(pairs[1]) == []
    Sh.write_sheet_report(pairs, Sh.report_fields(merged, capi.SHEET_REPORT), str(tmp_path / 'sheet'), 9, 4)
    assert sorted(os.listdir(tmp_path / 'sheet')) == ['9_4.txt', '9_5.txt']
    fields = ('antiparallel_content 0.412\nparallel_content 0.100\nn_antiparallel 2\nn_parallel 1\nn_paired 6\ne_antiparallel 1.235\n'
              'e_parallel 0.000\ne_ladder 100.000\nn_ladder_missed 1\n')
    assert (tmp_path / 'sheet' / '9_4.txt').read_text() == '1 8 A\n2 7 A\n2 6 P\n' + fields
    assert (tmp_path / 'sheet' / '9_5.txt').read_text() == ('antiparallel_content 0.000\nparallel_content 0.250\nn_antiparallel 0\nn_parallel 0\n'
                                                            'n_paired 0\ne_antiparallel 0.000\ne_parallel 2.000\ne_ladder 0.500\n'
                                                            'n_ladder_missed 6\n')


def test_reference_on_ideal_geometry():
    """The figures the defaults were chosen by, on ideal coordinates: flat pleated strands 4.8 A apart (3.3 A rise, a
    +-0.94 A pleat in z, neighbours' pleats in phase in space), the ideal helix and the ideal extended chain of tests/_secstruct.py.
    This oracle's own values are pinned to 1e-3: n_A = 5.372 (two strands, antiparallel), n_P = 6.161 (parallel), n_A = 10.751 (three
    strands).  The figures quoted when the defaults were proposed, 5.41, 6.17 and 10.8, were computed on ideal strands whose exact
    construction is not recorded; this geometry reproduces them to 0.7 %, and they stay asserted at 1 %, the small counts at their
    quoted size.  (Oracle only: no library call.)"""
    cfg = S.config()
    anti, par, three = (S.terms(x[None], cfg) for x in (S.ideal_sheet(2), S.ideal_sheet(2, parallel=True), S.ideal_sheet(3)))
    assert float(anti['n'][0, 0]) == pytest.approx(5.372, rel=1e-3) and float(par['n'][0, 1]) == pytest.approx(6.161, rel=1e-3)
    assert float(three['n'][0, 0]) == pytest.approx(10.751, rel=1e-3) and float(anti['n'][0, 1]) == pytest.approx(0.0080, rel=2e-2)
    assert float(par['n'][0, 0]) == pytest.approx(0.026, rel=3e-2)
    assert float(anti['n'][0, 0]) == pytest.approx(5.41, rel=0.01) and int(anti['n_antiparallel']) == 6 and int(anti['n_parallel']) == 0
    assert float(anti['n'][0, 1]) == pytest.approx(0.008, abs=0.001)
    assert float(par['n'][0, 1]) == pytest.approx(6.17, rel=0.01) and int(par['n_parallel']) == 6 and int(par['n_antiparallel']) == 0
    assert float(par['n'][0, 0]) == pytest.approx(0.03, abs=0.005)
    assert float(three['n'][0, 0]) == pytest.approx(10.8, rel=0.01) and int(three['n_antiparallel']) == 12
    # partners: residue k of strand 0 faces 15 - k, residue 8 + k faces 23 - k; the middle strand's better rung is the lower partner
    # or the upper one by a hair of float64 rounding, so only its being paired is pinned
    pa = anti['pairs'][0]
    assert pa[:, 1].tolist() == [-1] * 16 and pa[:, 0].tolist() == [-1] + [15 - k for k in range(1, 7)] + [-1, -1] + [15 - k for k in range(9, 15)] + [-1]
    assert int(anti['n_paired']) == 12 and int(three['n_paired']) == 18
    pp = par['pairs'][0]
    assert pp[:, 0].tolist() == [-1] * 16 and pp[:, 1].tolist() == [-1] + list(range(9, 15)) + [-1, -1] + list(range(1, 7)) + [-1]
    helix = S.terms(S.ideal_helix(30)[None], cfg)
    assert float(helix['n'][0, 0]) == pytest.approx(0.18, abs=0.005) and float(helix['n'][0, 1]) == pytest.approx(0.01, abs=0.001)
    assert float(helix['n'][0, 0]) == pytest.approx(0.178, rel=1e-2) and float(helix['n'][0, 1]) == pytest.approx(0.0103, rel=2e-2)
    assert int(helix['n_paired']) == 0
    # with a parallel separation of 3 the helix's (i, i+3) pairs would count: that is why the default is 5
    assert float(S.terms(S.ideal_helix(30)[None], S.config(separation=(3, 3)))['n'][0, 1]) > 10 * float(helix['n'][0, 1])
    for chain in (S.ideal_extended(16), S.strand(16)):
        t = S.terms(chain[None], cfg)
        assert float(t['n'].max()) < 0.01 and int(t['n_paired']) == 0
    # the squared score is what keeps a compact random chain's far pairs below a sheet's signal
    g = torch.Generator().manual_seed(0)
    walks = torch.stack([S.walk64(256, g) for _ in range(8)])
    n = S.terms(walks, cfg)['n'].mean(dim=0)
    z = S.zscores(walks, cfg)
    plain = torch.where(S.eligible(256, cfg)[None], 1.0 / (1.0 + (z ** 2).sum(dim=-1) / 3.0), torch.zeros(())).sum(dim=(2, 3)).mean(dim=0)
    print('3.8 A walks of 256: n_A, n_P squared %.1f %.1f, plain %.1f %.1f' % (n[0], n[1], plain[0], plain[1]))
    # (8 walks of generator seed 0: 35.6 / 16.6 against 234 / 131; other walks gave 27.2 / 9.6 against 205 / 110 -- the sums depend on
    # how compact the walks drawn are; the ratio between the two score forms is 6.6 to 11.5 over both)
    assert float(n[0]) == pytest.approx(35.6, abs=0.1) and float(n[1]) == pytest.approx(16.6, abs=0.1)
    assert float(plain[0]) == pytest.approx(234.2, abs=0.5) and float(plain[1]) == pytest.approx(131.3, abs=0.5)
    assert float(n[0]) < 0.25 * float(plain[0]) and float(n[1]) < 0.25 * float(plain[1]) and float(n[0]) < 45 and float(n[1]) < 20

    # the hinges and the ladder by hand, on the two-stranded sheet (N = 16)
    cfg = S.config(antiparallel=(0.0, 0.25), antiparallel_weight=2.0, parallel=(0.1, math.inf), parallel_weight=3.0,
                   ladder=[(2, 13, 2, 'A', 0.5), (3, 9, 1, 'P')], ladder_weight=0.5)
    t = S.terms(S.ideal_sheet(2)[None], cfg)
    n_a, n_p = float(t['n'][0, 0]), float(t['n'][0, 1])
    assert float(t['e_antiparallel']) == pytest.approx(2.0 * (n_a - 4.0) ** 2, rel=1e-12) and n_a > 4
    assert float(t['e_parallel']) == pytest.approx(3.0 * (1.6 - n_p) ** 2, rel=1e-12) and n_p < 1.6
    x = S.ideal_sheet(2)
    d = lambda p, q: float((x[p] - x[q]).norm())      # noqa: E731
    u = lambda ds, mu, sg: sum(((v - mu) / sg) ** 2 for v in ds) / 3      # noqa: E731
    by_hand = 0.5 * (0.5 * u((d(2, 13), d(1, 14), d(3, 12)), 5.0, 0.6) + 0.5 * u((d(3, 12), d(2, 13), d(4, 11)), 5.0, 0.6)
                     + 1.0 * u((d(3, 9), d(2, 8), d(4, 10)), 4.8, 0.5))
    assert float(t['e_ladder']) == pytest.approx(by_hand, rel=1e-12)
    assert int(t['n_ladder_missed']) == 1                                                     # the two listed A rungs are formed, 3-9 P is not


def test_reference_gradient_matches_loops_and_finite_differences():
    """The oracle's autograd gradient against the analytic one written out with loops (1e-12 of the largest entry) and central
    differences (1e-7), at N = 24 with every term active, and on degenerate and short chains.  (Oracle only: no library call.)"""
    x = S.sheet_chain(2, 24, 1).double()
    cfg = S.chain_config(x)
    var = 0.8
    ref = S.reference(x, cfg, var)
    assert bool((ref['e_antiparallel'] > 0).all()) and bool((ref['e_parallel'] > 0).all()) and bool((ref['e_ladder'] > 0).all())
    assert torch.allclose(ref['logp'], -(ref['e_antiparallel'] + ref['e_parallel'] + ref['e_ladder']) / (2 * var), rtol=1e-14, atol=0)
    scale = float(ref['grad'].abs().max())
    loops = S.analytic_gradient(x, cfg, var)
    assert float((ref['grad'] - loops).abs().max()) <= 1e-12 * scale, float((ref['grad'] - loops).abs().max()) / scale
    h, fd = 1e-6, torch.zeros_like(x)
    for idx in range(x.numel()):
        e = torch.zeros(x.numel(), dtype=torch.float64)
        e[idx] = h
        e = e.view_as(x)
        fd.view(-1)[idx] = (S.logp(x + e, cfg, var).sum() - S.logp(x - e, cfg, var).sum()) / (2 * h)
    assert float((ref['grad'] - fd).abs().max()) <= 1e-7 * scale, float((ref['grad'] - fd).abs().max()) / scale
    # degenerate inputs: coincident residues inside a rung and a chain in one point are finite, with no force from what has no direction
    y = x.clone()
    y[0, 9] = y[0, 3]                                              # d0 of the rung (3, 9) is 0 in both classes
    ref = S.reference(y, cfg, var)
    assert bool(torch.isfinite(ref['grad']).all()) and bool(torch.isfinite(ref['logp']).all())
    assert float((ref['grad'] - S.analytic_gradient(y, cfg, var)).abs().max()) <= 1e-12 * float(ref['grad'].abs().max())
    ref = S.reference(torch.full((1, 9, 3), 2.5), S.config(antiparallel=(0.5, math.inf), antiparallel_weight=1.0, ladder=[(1, 7, 1, 'A')],
                                                           ladder_weight=1.0), var)
    assert bool((ref['grad'] == 0).all()) and bool(torch.isfinite(ref['logp']).all()) and bool((ref['pairs'] == -1).all())
    # short chains: no eligible rung below N = 6, the first antiparallel one at 6, the first parallel one at 8 (separation 5)
    for n, rungs_a, rungs_p in ((3, 0, 0), (5, 0, 0), (6, 1, 0), (7, 3, 0), (8, 6, 1), (9, 10, 3)):
        ok = S.eligible(n, S.config())
        assert int(ok[0].sum()) == rungs_a and int(ok[1].sum()) == rungs_p, n
    ref = S.reference(S.sheet_chain(2, 5, 1), S.config(antiparallel=(0.2, math.inf), antiparallel_weight=1.5), var)
    assert bool((ref['grad'] == 0).all()) and torch.allclose(ref['logp'], torch.full((2,), -1.5 / (2 * var), dtype=torch.float64))
