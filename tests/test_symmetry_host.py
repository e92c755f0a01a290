"""The symmetry potential without a device: the float64 oracle of tests/_symmetry.py against its own loop gradient, central
differences and exact assemblies; the C entry's symbol and refusals (genie_symmetry_potential, include/genie_hip.h);
symmetry_generators', check_generators' and SymmetryPotential's host side; both command lines' parsers, the length filter and the
report writer; chain_lengths and UnconditionalSampler.create_np_features with and without them.

What holds the kernel to the oracle is tests/test_symmetry_gpu.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import _symmetry as S
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')
ORACLE_CASES = [(2, 60, 'C3', 20, 0, 0), (2, 70, 'C4', 15, 2, 3), (2, 60, 'R4', 15, 0, 0), (2, 12, 'C2', 6, 0, 0), (2, 30, 'D2', 7, 0, 1)]


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ORACLE_CASES, ids=S.case_id)
def test_oracle_gradient_matches_loops_and_central_differences(case):
    """Autograd through the SVD fit against the header's formula written with loops (1e-10 of the largest entry) and against central
    differences of the oracle's own logp (h = 1e-5 A on coordinates of tens of A: truncation h^2 |f'''| / 6 and rounding
    1e-16 |logp| / h stay below 1e-6 of the largest entry)."""
    B, N, sym, m, linker, offset = case
    from genie2_amd.smc import symmetry_generators
    gens = S.generators(sym, m, N, linker, offset)
    assert symmetry_generators(sym, m, N, linker, offset) == gens            # (the package expands the symbol to the same lists)
    x = S.walks(B, N).double()
    weights, var = [1.0, 0.5][:len(gens)], 0.8
    ref = S.reference(x, gens, var, weights, weight=1.5)
    scale = float(ref['grad'].abs().max())
    loops = S.analytic_gradient(x, gens, var, weights, weight=1.5)
    assert float((ref['grad'] - loops).abs().max()) <= 1e-10 * scale
    assert torch.allclose(ref['logp'], -1.5 * sum(w * ref['E'][:, g] for g, w in enumerate(weights)) / (2 * var), rtol=1e-13, atol=0)
    assert torch.allclose(ref['e_symmetry'], 1.5 * sum(w * ref['E'][:, g] for g, w in enumerate(weights)), rtol=1e-13, atol=0)
    h, fd = 1e-5, torch.zeros_like(x)
    f = lambda y: float((-1.5 * S.energy(y, gens, weights) / (2 * var)).sum())      # noqa: E731
    for idx in range(x.numel()):
        e = torch.zeros(x.numel(), dtype=torch.float64)
        e[idx] = h
        fd.view(-1)[idx] = (f(x + e.view_as(x)) - f(x - e.view_as(x))) / (2 * h)
    assert float((ref['grad'] - fd).abs().max()) <= 1e-6 * scale, float((ref['grad'] - fd).abs().max()) / scale
    # free residues: a gradient of exactly 0
    used = sorted({i for src, dst in gens for i in src + dst})
    free = [i for i in range(N) if i not in used]
    assert len(free) == N - (2 if sym[0] == 'D' else 1) * int(sym[1:]) * m and bool((ref['grad'][:, free] == 0).all())
    # the float32 restatement (the rotation held fixed) is the same function to float32 rounding
    r32 = S.restatement32(x, gens, var, weights, weight=1.5)
    assert torch.allclose(r32['logp'].double(), ref['logp'], rtol=1e-5) and float((r32['grad'].double() - ref['grad']).abs().max()) <= 1e-4 * scale


def test_oracle_on_exact_assemblies_and_a_mirror_image():
    """Assemblies built by applying one rigid motion repeatedly: E <= 1e-20 sum |p|^2 with the motion's angle and rise."""
    for name, x, gens, expect in (
            ('C3', S.exact_cyclic(3, 20), S.generators('C3', 20, 60), [(120.0, 0.0)]),
            ('D2', S.exact_dihedral(2, 10), S.generators('D2', 10, 40), [(180.0, 0.0), (180.0, 0.0)]),
            ('D3', S.exact_dihedral(3, 10), S.generators('D3', 10, 60), [(120.0, 0.0), (180.0, 0.0)]),
            ('R4', S.exact_repeat(4, 15, 40.0, 7.0), S.generators('R4', 15, 60), [(40.0, 7.0)])):
        d = S.describe(x[None], gens)
        assert bool((d['E'] <= 1e-20 * d['norm']).all()), (name, d['E'] / d['norm'])
        for g, (angle, rise) in enumerate(expect):
            assert float(d['angle_%d' % g]) == pytest.approx(angle, abs=1e-9) and float(d['rise_%d' % g]) == pytest.approx(rise, abs=1e-9), (name, g)
        assert float(d['symmetry_rmsd']) < 1e-9
    # a unit rotated by 120 degrees twice, by hand
    unit = S.exact_unit(12, 7)
    R = S.axis_rotation((0.3, -1.0, 0.2), 120.0)
    x = torch.cat([unit, unit @ R.T, unit @ R.T @ R.T])
    d = S.describe(x[None], S.generators('C3', 12, 36))
    assert float(d['E']) <= 1e-20 * float(d['norm']) and float(d['angle_0']) == pytest.approx(120.0, abs=1e-9)
    # a mirror-image dimer does not fit: the rotation is proper.  The improper fit would be exact.
    mirror = torch.cat([unit, unit * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)])
    d = S.describe(mirror[None], S.generators('C2', 12, 24))
    assert float(d['E']) > 1e-2 * float(d['norm']) and float(d['symmetry_rmsd']) > 1.0
    _, Rm, _, _, p, q = S.fit(mirror[None], S.generators('C2', 12, 24)[0])
    assert float(torch.linalg.det(Rm)) == pytest.approx(1.0, abs=1e-12)
    # an open repeat is not a closed ring: R4's screw leaves C4's closing pair far off
    x = S.exact_repeat(4, 15, 40.0, 7.0)
    assert float(S.describe(x[None], S.generators('C4', 15, 60))['symmetry_rmsd']) > 1.0


@pytest.mark.parametrize('n', [2, 3, 4, 5])
def test_dihedral_generators_obey_the_group_relations(n):
    """As permutations of the residues in units: g0^n = id, g1^2 = id and g1 g0 g1 = g0^-1, for the oracle's and the package's lists."""
    from genie2_amd.smc import symmetry_generators
    m, linker, offset = 4, 2, 3
    N = offset + 2 * n * m + (2 * n - 1) * linker + 1
    for gens in (S.generators('D%d' % n, m, N, linker, offset), symmetry_generators('D%d' % n, m, N, linker, offset)):
        g0, g1 = (dict(zip(src, dst)) for src, dst in gens)
        assert sorted(g0) == sorted(g0.values()) == sorted(g1) == sorted(g1.values()) and len(g0) == 2 * n * m
        for i in g0:
            j = i
            for _ in range(n):
                j = g0[j]
            assert j == i and g1[g1[i]] == i
            assert g0[g1[g0[g1[i]]]] == i                                # g1 g0 g1 is the inverse of g0
        assert S.is_swap(gens[1]) and S.is_swap(gens[0]) == (n == 2)


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_and_loads(lib):
    from genie2_amd import build, capi
    assert 'symmetry_kernels.hip' in build.SOURCES and any(h.endswith('horn.h') for h in build.HEADERS)
    assert len(capi.SYMBOLS['genie_symmetry_potential'][1]) == 14 and capi.SYMBOLS['genie_symmetry_potential'][0] is C.c_int
    assert capi.SYMBOLS['genie_symmetry_potential_work_bytes'] == (C.c_size_t, [C.c_int, C.c_int])
    assert lib.genie_symmetry_potential is not None
    assert len(capi.SYMMETRY_REPORT) == 8 and capi.SYMMETRY_REPORT == S.REPORT and capi.SYMMETRY_MAX_GENERATORS == 2
    # one work-group carries a particle from the first sum to the gradient: no scratch memory at any size
    assert all(lib.genie_symmetry_potential_work_bytes(B, N) == 0 for B, N in ((1, 6), (3, 65), (128, 256), (1, 1512), (0, 5)))
    assert len(capi.SYMBOLS['genie_sheet_potential'][1]) == 29                                # (the neighbours keep their arguments)
    # the quaternion fit is shared with the motif kernels, not copied
    csrc = os.path.join(os.path.dirname(build.__file__), 'csrc')
    for name in ('smc_kernels.hip', 'symmetry_kernels.hip'):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "horn.h"' in text and 'float4 mr_quaternion(' not in text, name
    assert 'float4 mr_quaternion(' in open(os.path.join(csrc, 'horn.h')).read()


def test_entry_refuses_before_the_device_is_touched(lib):
    """Every refusal returns GENIE_E_ARG without a device, and genie_last_error(NULL) names the entry and the argument."""
    d = C.c_void_p(64)                                           # never dereferenced: every call below fails its checks
    inf, nan = math.inf, math.nan

    def call(B=2, N=60, x0=d, G=2, partner=d, weights=(1.0, 1.0), var=d, logp=d, grad=d, report=d, work=None, work_bytes=0):
        rc = lib.genie_symmetry_potential(None, B, N, x0, G, partner, weights[0], weights[1], var, logp, grad, report, work, work_bytes)
        return rc, lib.genie_last_error(None)

    cases = [(dict(B=0), b'B'), (dict(B=65536), b'B'), (dict(N=0), b'N'), (dict(N=-3), b'N'), (dict(x0=None), b'x0'),
             (dict(G=0), b'G'), (dict(G=3), b'G'), (dict(G=-1), b'G'), (dict(partner=None), b'partner'), (dict(var=None), b'var'),
             (dict(logp=None, grad=None, report=None), b'no output'), (dict(logp=None), b'logp_out and grad_out'),
             (dict(grad=None), b'logp_out and grad_out'), (dict(work=None, work_bytes=16), b'work'), (dict(N=13627), b'LDS'),
             (dict(N=100000), b'LDS')]
    for k, word in ((0, b'weight0'), (1, b'weight1')):
        for v in (-1.0, inf, nan):
            cases.append((dict(weights=tuple(v if i == k else 1.0 for i in range(2))), word))
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b'genie_symmetry_potential: ') and word in msg, (kw, rc, msg)
    # what is allowed passes every check (and then fails on the device instead, with another code): one generator, the report or
    # the potential alone, weights of 0, a work buffer nobody needs, the longest N that fits
    if not torch.cuda.is_available():
        for kw in (dict(G=1), dict(logp=None, grad=None), dict(report=None), dict(weights=(0.0, 0.0)), dict(work=d, work_bytes=64),
                   dict(N=1), dict(N=1512), dict(N=13626), dict(B=65535)):
            assert call(**kw)[0] != -1, kw


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------

def test_symmetry_generators_and_layout_validate_on_the_host():
    from genie2_amd.smc import check_generators, parse_symmetry, partner_table, symmetry_generators, symmetry_layout
    assert parse_symmetry('C3') == ('C', 3, 3) and parse_symmetry('d2') == ('D', 2, 4) and parse_symmetry(' R12 ') == ('R', 12, 12)
    for bad in ('C1', 'C0', 'C', 'D', 'X3', 'C3.0', 'C-3', '3C', '', None, 3, 'CC3', 'R1'):
        with pytest.raises(ValueError, match='symmetry must be'):
            parse_symmetry(bad)
    # the layout: unit k starts at offset + k (m + linker); unit_length None divides what is left evenly
    assert symmetry_layout('C3', 60) == (3, 20) and symmetry_layout('C3', 65, None, 1, 0) == (3, 21) and symmetry_layout('D2', 129, 31, 1, 2) == (4, 31)
    assert symmetry_layout('R5', 300, 50, 10, 5) == (5, 50) and symmetry_layout('C3', 65, 21, 0, 1) == (3, 21)
    assert symmetry_layout('C2', 4) == (2, 2) and symmetry_layout('R2', 9, 4, 1) == (2, 4)
    for args in (('C3', 61), ('C3', 65, None, 0, 0), ('D2', 10, None, 1, 0), ('C3', 60, 21), ('C3', 65, 21, 1, 1), ('C4', 3),
                 ('C3', 60, 0), ('C3', 60, -2), ('C3', 60, 20, -1), ('C3', 60, 20, 0, -1), ('C3', 0), ('C3', 60, 20.0), ('C3', 60.0),
                 ('C3', 60, 20, True), ('C2', 2), ('R2', 4), ('R2', 5, 2, 1), ('Q3', 60)):
        with pytest.raises(ValueError):
            symmetry_layout(*args)
    for case in S.CASES:
        B, N, sym, m, linker, offset = case
        gens = symmetry_generators(sym, m, N, linker, offset)
        assert gens == S.generators(sym, m, N, linker, offset) and check_generators(gens, N) == gens
        kind, n = sym[0], int(sym[1:])
        assert [len(src) for src, _ in gens] == {'C': [n * m], 'R': [(n - 1) * m], 'D': [2 * n * m] * 2}[kind]
    src, dst = symmetry_generators('C3', 2, 9, 1, 1)[0]
    assert (src, dst) == ([1, 2, 4, 5, 7, 8], [4, 5, 7, 8, 1, 2])
    src, dst = symmetry_generators('R3', 2, 7, 0, 1)[0]
    assert (src, dst) == ([1, 2, 3, 4], [3, 4, 5, 6])
    # explicit generators: check_generators' rules
    ok = ([0, 1, 2], [3, 4, 5])
    assert check_generators([ok], 6) == [ok] and check_generators([(torch.tensor([0, 1, 2]), (3, 4, 5))], 6) == [ok]
    for bad in ([], [ok, ok, ok], [([0, 1], [3, 4])], [([0, 1, 2], [3, 4])], [([0, 1, 2], [3, 4, 6])], [([0, 1, -1], [3, 4, 5])],
                [([0, 1, 2], [0, 4, 5])], [([0, 1, 1], [3, 4, 5])], [([0, 1, 2], [3, 4, 4])], [([0.0, 1, 2], [3, 4, 5])],
                [([0, 1, True], [3, 4, 5])], [([0, 1, 2],)], [(ok[0], ok[1], ok[1])], 5):
        with pytest.raises(ValueError):
            check_generators(bad, 6)
    # the table: each row of a generator is the inverse of the other, -1 where a residue has no such role
    table = partner_table(symmetry_generators('R3', 2, 7, 0, 1), 7)
    assert table.dtype == torch.int32 and tuple(table.shape) == (1, 2, 7)
    assert table[0, 0].tolist() == [-1, 3, 4, 5, 6, -1, -1] and table[0, 1].tolist() == [-1, -1, -1, 1, 2, 3, 4]
    table = partner_table(symmetry_generators('D2', 3, 12), 12)
    assert tuple(table.shape) == (2, 2, 12) and table[1, 0].tolist() == table[1, 1].tolist() == [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5]
    assert table[0, 0].tolist() == [3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8]


def test_constructor_validates_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import SymmetryPotential
    import genie.sampler.symmetry as mirror
    assert mirror.SymmetryPotential is SymmetryPotential
    abar = torch.linspace(0.999, 0.001, 13)
    ok = [([0, 1, 2], [3, 4, 5])]
    for kw in (dict(), dict(symmetry='C3', generators=ok), dict(symmetry='C7'), dict(symmetry='C3', unit_length=21), dict(symmetry='X3'),
               dict(symmetry='C3', linker=1), dict(symmetry='C3', offset=-1), dict(symmetry='C3', unit_length=0),
               dict(symmetry='C3', weight=-1.0), dict(symmetry='C3', weight=math.nan), dict(symmetry='C3', weight=math.inf),
               dict(symmetry='C3', tausq=0.0), dict(symmetry='C3', tausq=math.inf), dict(symmetry='C3', generator_weights=(1.0, 1.0)),
               dict(symmetry='D2', generator_weights=(1.0,)), dict(symmetry='D2', generator_weights=(1.0, -0.5)),
               dict(symmetry='D2', generator_weights=(1.0, math.nan)), dict(symmetry='D2', generator_weights=5),
               dict(symmetry='D2', generator_weights=('a', 'b')), dict(generators=[]), dict(generators=[([0, 1], [2, 3])]),
               dict(generators=[([0, 1, 60], [3, 4, 5])]), dict(generators=ok, unit_length=3), dict(generators=ok, linker=1),
               dict(generators=ok, offset=2), dict(generators=ok * 3)):
        with pytest.raises(ValueError):
            SymmetryPotential(60, abar, device='cpu', **kw)          # (before the device: a CPU potential is a GenieError)
    for n_res in (0, -5, 60.0, True):
        with pytest.raises(ValueError):
            SymmetryPotential(n_res, abar, symmetry='C2', device='cpu')
    for kw in (dict(symmetry='C3'), dict(symmetry='c3', unit_length=19, linker=1, offset=1), dict(symmetry='D2', generator_weights=(1, 0)),
               dict(symmetry='R4', weight=0.0), dict(generators=ok), dict(generators=ok + [([5, 6, 7], [0, 1, 2])], generator_weights=[2, 3])):
        with pytest.raises(capi.GenieError, match='no CPU path'):
            SymmetryPotential(60, abar, device='cpu', **kw)


def _host_potential(n_res, **kw):
    """A SymmetryPotential's host side, built without a device: the constructor stops at the base class, which looks at the device
    first, so the attributes chain_lengths reads are set by then, except n_res."""
    from genie2_amd import capi
    from genie2_amd.smc import SymmetryPotential
    pot = SymmetryPotential.__new__(SymmetryPotential)
    with pytest.raises(capi.GenieError, match='no CPU path'):
        pot.__init__(n_res, torch.linspace(0.999, 0.001, 13), device='cpu', **kw)
    pot.n_res = n_res
    return pot


def test_chain_lengths_and_features_with_and_without_them():
    import _partial as P
    from genie2_amd import features as F
    from genie2_amd import pack
    from genie2_amd.sampler import UnconditionalSampler
    assert _host_potential(60, symmetry='C3').chain_lengths() == [20, 20, 20]
    assert _host_potential(48, symmetry='D2', unit_length=12).chain_lengths() == [12] * 4
    assert _host_potential(40, symmetry='R2').chain_lengths() == [20, 20]
    for n_res, kw in ((61, dict(symmetry='C3', unit_length=20)), (62, dict(symmetry='C3', linker=1)), (61, dict(symmetry='C3', offset=1)),
                      (6, dict(generators=[([0, 1, 2], [3, 4, 5])]))):
        with pytest.raises(ValueError):
            _host_potential(n_res, **kw).chain_lengths()
    sampler = UnconditionalSampler(P.host_model(10))
    today = F.create_empty_np_features([40])
    for params in ({'length': 40}, {'length': 40, 'chain_lengths': None}):
        got = sampler.create_np_features(params)
        assert list(got) == list(today) and all(np.array_equal(got[k], today[k]) and got[k].dtype == today[k].dtype for k in today)
    got = sampler.create_np_features({'length': 40, 'chain_lengths': [20, 20]})
    assert got['chain_index'].tolist() == [0] * 20 + [1] * 20 and got['residue_index'].tolist() == list(range(20)) * 2
    assert int(got['num_chains']) == 2 and got['num_residues_per_chain'].tolist() == [20, 20] and int(got['num_residues']) == 40
    want = F.create_empty_np_features([20, 20])
    assert all(np.array_equal(got[k], want[k]) for k in want)
    rows = pack.chain_table_rows(sampler.model.model.dims)
    assert rows == 8 and len(sampler.create_np_features({'length': 40, 'chain_lengths': [5] * 8})['num_residues_per_chain']) == 8
    for chains in ([20, 19], [20, 21], [], [40, 0], [20.0, 20.0], [True, 39], [4] * 10, [-1, 41]):
        with pytest.raises(ValueError):
            sampler.create_np_features({'length': 40, 'chain_lengths': chains})


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

def test_parsers_constants_lengths_and_report(tmp_path, capsys):
    from genie2_amd import capi
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    import genie.sample_unconditional_shape as mirror
    assert mirror.add_symmetry_arguments is Sh.add_symmetry_arguments and mirror.symmetry_potential is Sh.symmetry_potential
    base = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']
    defaults = dict(symmetry=None, unit_length=None, unit_linker=0, unit_offset=0, symmetry_weight=1.0, symmetry_tausq=1.0,
                    unit_chains=False, write_symmetry=False)
    given = ['--symmetry', 'C3', '--unit_length', '20', '--unit_linker', '2', '--unit_offset', '1', '--symmetry_weight', '2.5',
             '--symmetry_tausq', '4', '--write_symmetry']
    values = dict(symmetry='C3', unit_length=20, unit_linker=2, unit_offset=1, symmetry_weight=2.5, symmetry_tausq=4.0, unit_chains=False,
                  write_symmetry=True)
    for parser, more in ((Sh.build_parser(), []), (M.build_parser(), ['--motif_file', MOTIF])):
        a = vars(parser.parse_args(base + more))
        assert {k: a[k] for k in defaults} == defaults
        # (the flags that were there keep their defaults)
        assert a['rog_max'] is None and a['clash_distance'] is None and a['sheet_tausq'] == 1.0 and a['ladder_file'] is None and a['ss_target'] is None
        a = vars(parser.parse_args(base + more + given))
        assert {k: a[k] for k in values} == values
        assert vars(parser.parse_args(base + more + ['--symmetry', 'D2', '--unit_chains']))['unit_chains'] is True

    # constants: a symmetry term is enough on its own for the shape CLI
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base + given)))
    assert {k: c[k] for k in values} == values and Sh.has_symmetry_terms(c)
    assert not Sh.has_shape_terms(c) and not Sh.has_secstruct_terms(c) and not Sh.has_sheet_terms(c)
    assert Sh.shape_potential(c, 70, None, 'cuda') is None and Sh.sheet_potential(c, 70, None, 'cuda') is None
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF] + given)))
    assert {k: c[k] for k in values} == values and c['tausq'] == 0.012
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF])))
    assert {k: c[k] for k in defaults} == defaults and not Sh.has_symmetry_terms(c)
    assert Sh.symmetry_potential(c, 60, None, 'cuda') is None                                # no term: no potential, no device
    with pytest.raises(SystemExit, match='no shape term.*--symmetry$'):
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base + ['--symmetry_weight', '2', '--write_symmetry'])))
    for flags in (['--symmetry', 'C1'], ['--symmetry', 'T'], ['--unit_chains'], ['--symmetry', 'C2', '--unit_chains', '--unit_linker', '1'],
                  ['--symmetry', 'C2', '--unit_chains', '--unit_offset', '2']):
        with pytest.raises(SystemExit):
            Sh.symmetry_constants(vars(Sh.build_parser().parse_args(base + flags)))

    # lengths the layout does not fit are skipped with one printed line
    capsys.readouterr()
    tasks = Sh.ShapeRunner().create_tasks(dict(min_length=58, max_length=63, length_step=1, symmetry='C3'))
    assert [t['length'] for t in tasks] == [63, 60]
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and 'C3' in out[0] and '62, 61, 59, 58' in out[0]
    tasks = Sh.ShapeRunner().create_tasks(dict(min_length=58, max_length=63, length_step=1, symmetry='C3', unit_length=20))
    assert [t['length'] for t in tasks] == [63, 62, 61, 60]                                  # a given unit length only needs room
    assert '59, 58' in capsys.readouterr().out
    tasks = Sh.ShapeRunner().create_tasks(dict(min_length=58, max_length=63, length_step=1, symmetry='C3', unit_length=20, unit_chains=True))
    assert [t['length'] for t in tasks] == [60]                                              # chains: the units fill the length
    capsys.readouterr()
    tasks = M.MotifRunner().create_tasks(dict(min_length=10, max_length=41, length_step=1, motif_file=MOTIF, symmetry='R2', unit_linker=1))
    assert [t['length'] for t in tasks] == list(range(41, 12, -2))                             # (two units and one linker: odd lengths)
    assert len(capsys.readouterr().out.strip().splitlines()) == 2                            # one line for the motif, one for the layout
    assert [t['length'] for t in Sh.ShapeRunner().create_tasks(dict(min_length=5, max_length=6, length_step=1))] == [6, 5]
    assert capsys.readouterr().out.strip() == ''                                             # no symmetry: nothing skipped, nothing printed

    # the report file: the layout line, then the eight fields of a merged report; the others keep theirs
    merged = {'rog': torch.tensor([12.34567, 9.0]), 'e_symmetry': torch.tensor([1234.5678, 0.0]), 'symmetry_rmsd': torch.tensor([4.53649, 0.0]),
              'rmsd_0': torch.tensor([4.5, 0.0]), 'angle_0': torch.tensor([119.99951, 180.0]), 'rise_0': torch.tensor([0.0004, 7.0]),
              'rmsd_1': torch.tensor([0.0, 0.0]), 'angle_1': torch.tensor([0.0, 0.0]), 'rise_1': torch.tensor([0.0, 0.0])}
    assert list(Sh.report_fields(merged, capi.SYMMETRY_REPORT)) == list(capi.SYMMETRY_REPORT)
    pot = _host_potential(60, symmetry='C3')
    assert Sh.symmetry_header(pot) == 'symmetry C3 units 3 unit_length 20 linker 0 offset 0'
    assert Sh.symmetry_header(_host_potential(129, symmetry='d2', unit_length=31, linker=1, offset=2)) == 'symmetry D2 units 4 unit_length 31 linker 1 offset 2'
    Sh.write_symmetry_report(Sh.report_fields(merged, capi.SYMMETRY_REPORT), Sh.symmetry_header(pot), str(tmp_path / 'symmetry'), 60, 4)
    assert sorted(os.listdir(tmp_path / 'symmetry')) == ['60_4.txt', '60_5.txt']
    assert (tmp_path / 'symmetry' / '60_4.txt').read_text() == (
        'symmetry C3 units 3 unit_length 20 linker 0 offset 0\ne_symmetry 1234.568\nsymmetry_rmsd 4.536\nrmsd_0 4.500\nangle_0 120.000\n'
        'rise_0 0.000\nrmsd_1 0.000\nangle_1 0.000\nrise_1 0.000\n')
    assert (tmp_path / 'symmetry' / '60_5.txt').read_text().splitlines()[4:6] == ['angle_0 180.000', 'rise_0 7.000']
