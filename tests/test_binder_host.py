"""The binder potential without a device: the float64 oracle of tests/_binder.py against its own loop gradient and central
differences; the C entry's symbols, work sizes and refusals (genie_binder_potential, include/genie_hip.h); load_target's,
parse_hotspots', place_target's and BinderPotential's host side; both command lines' parsers, the report writer and the complex
writer.

What holds the kernel to the oracle is tests/test_binder_gpu.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import _binder as Bd
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')
TARGET = os.path.join(GOLDEN, 'dataset_100_0.pdb')       # 100 residues, chain A, numbered from 1


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', Bd.CASES[:3], ids=Bd.case_id)
def test_oracle_gradient_matches_loops_and_central_differences(case):
    """Autograd against the header's formula written with loops (1e-12 of the largest entry) and, at the two smallest shapes, against
    central differences of the oracle's own logp (h = 1e-5 A on coordinates of tens of A: truncation h^2 |f'''| / 6 and rounding
    1e-16 |logp| / h stay below 1e-6 of the largest entry)."""
    x, y, cfg = Bd.inputs(case)
    x, var = x.double(), 0.8
    ref = Bd.reference(x, y, cfg, var)
    scale = float(ref['grad'].abs().max())
    assert float((ref['grad'] - Bd.analytic_gradient(x, y, cfg, var)).abs().max()) <= 1e-12 * scale
    assert torch.allclose(ref['logp'], -(ref['e_target_clash'] + ref['e_contact'] + ref['e_hotspot']) / (2 * var), rtol=1e-13, atol=0)
    for term in ('clash', 'contacts', 'hotspots'):
        one = Bd.only(cfg, term)
        part = Bd.reference(x, y, one, var)
        assert float((part['grad'] - Bd.analytic_gradient(x, y, one, var)).abs().max()) <= 1e-12 * scale, term
        assert float(part['grad'].abs().max()) > 0, term
    if x.numel() <= 50:
        h, fd = 1e-5, torch.zeros_like(x)
        f = lambda z: float(Bd.logp(z, y.double(), cfg, var).sum())      # noqa: E731
        for idx in range(x.numel()):
            e = torch.zeros(x.numel(), dtype=torch.float64)
            e[idx] = h
            fd.view(-1)[idx] = (f(x + e.view_as(x)) - f(x - e.view_as(x))) / (2 * h)
        assert float((ref['grad'] - fd).abs().max()) <= 1e-6 * scale, float((ref['grad'] - fd).abs().max()) / scale
    # the float32 restatement is the same function to float32 rounding
    r32 = Bd.restatement32(x, y, cfg, var)
    assert torch.allclose(r32['logp'].double(), ref['logp'], rtol=1e-5) and float((r32['grad'].double() - ref['grad']).abs().max()) <= 1e-4 * scale


def test_oracle_inputs_report_and_limits():
    """Every parity input passes the oracle's own conditions; the report's counts are what their definitions say on a hand-made
    input; contacts_max = inf has no upper hinge; a weight of 0 removes energy and force."""
    for case in Bd.CASES + [Bd.LDS_CASE]:
        x, y, cfg = Bd.inputs(case)
        assert Bd.margins(x, y, cfg) >= 1e-4 and len(cfg['hotspots']) == min(64, max(1, case[2] // 8))
    for H in (0, 1, 64):
        assert len(Bd.inputs(Bd.CASES[4], H)[2]['hotspots']) == H
    y = torch.tensor([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [100.0, 0.0, 0.0]])
    x = torch.tensor([[[0.0, 3.0, 0.0], [10.0, 7.0, 0.0], [50.0, 0.0, 0.0]]])
    cfg = Bd.config(clash_distance=4.0, clash_weight=2.0, contacts_min=5.0, contacts_max=6.0, contacts_weight=0.5, hotspot_contacts=1.0,
                    hotspot_weight=3.0, hotspots=[1, 2])
    t = Bd.reference(x, y, cfg, 1.0)
    assert int(t['n_contacts']) == 2 and int(t['n_interface']) == 2 and int(t['n_target_clash']) == 1 and int(t['n_hotspots_contacted']) == 1
    assert float(t['target_min_distance']) == 3.0 and float(t['e_target_clash']) == 2.0
    s = lambda d: 1.0 / (1.0 + (d / 8.0) ** 6)      # noqa: E731
    d = [[3.0, math.hypot(10, 3), math.hypot(100, 3)], [math.hypot(10, 7), 7.0, math.hypot(90, 7)], [50.0, 40.0, 50.0]]
    total = sum(s(v) for row in d for v in row)
    c = [sum(s(row[h]) for row in d) for h in (1, 2)]
    assert float(t['contacts']) == pytest.approx(total, rel=1e-14) and t['hotspot'][0].tolist() == pytest.approx(c, rel=1e-14)
    assert float(t['e_contact']) == pytest.approx(0.5 * (5.0 - total) ** 2, rel=1e-13)
    assert float(t['e_hotspot']) == pytest.approx(3.0 * sum(max(1.0 - v, 0.0) ** 2 for v in c), rel=1e-13)
    above = Bd.reference(x, y, dict(cfg, contacts_min=0.0, contacts_max=1.0), 1.0)
    assert float(above['e_contact']) == pytest.approx(0.5 * (total - 1.0) ** 2, rel=1e-13)
    assert float(Bd.reference(x, y, dict(cfg, contacts_min=0.0, contacts_max=math.inf), 1.0)['e_contact']) == 0.0
    off = Bd.reference(x, y, dict(cfg, clash_weight=0.0, contacts_weight=0.0, hotspot_weight=0.0), 1.0)
    assert float(off['logp']) == 0.0 and bool((off['grad'] == 0).all())


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_load(lib):
    from genie2_amd import build, capi
    assert 'binder_kernels.hip' in build.SOURCES and os.path.exists(os.path.join(os.path.dirname(build.__file__), 'csrc', 'binder_kernels.hip'))
    assert len(capi.SYMBOLS['genie_binder_potential'][1]) == 23 and capi.SYMBOLS['genie_binder_potential'][0] is C.c_int
    assert capi.SYMBOLS['genie_binder_potential_work_bytes'] == (C.c_size_t, [C.c_int, C.c_int, C.c_int])
    assert lib.genie_binder_potential is not None and lib.genie_binder_potential_work_bytes is not None
    assert capi.BINDER_REPORT == Bd.REPORT and len(capi.BINDER_REPORT) == 9 and capi.BINDER_COUNTS == Bd.COUNTS and capi.BINDER_MAX_HOTSPOTS == 64
    header = open(os.path.join(os.path.dirname(build.__file__), '..', 'include', 'genie_hip.h')).read()
    assert '#define GENIE_BINDER_REPORT 9' in header and '#define GENIE_BINDER_MAX_HOTSPOTS 64' in header
    assert len(capi.SYMBOLS['genie_symmetry_potential'][1]) == 14                              # (the neighbours keep their arguments)
    # 4 B (6 N + (8 + 2 H) ceil(N / 64)) bytes; 0 for sizes the entry refuses
    wb = lib.genie_binder_potential_work_bytes
    for B, N, H in ((1, 1, 0), (3, 64, 8), (3, 65, 16), (2, 129, 64), (128, 256, 8), (65535, 1, 1)):
        assert wb(B, N, H) == 4 * B * (6 * N + (8 + 2 * H) * ((N + 63) // 64)), (B, N, H)
    assert all(wb(*a) == 0 for a in ((0, 5, 1), (1, 0, 1), (1, 5, -1), (1, 5, 65)))


def test_entry_refuses_before_the_device_is_touched(lib):
    """Every refusal returns GENIE_E_ARG without a device, and genie_last_error(NULL) names the entry and the argument."""
    d = C.c_void_p(64)                                           # never dereferenced: every call below fails its checks
    inf, nan = math.inf, math.nan
    floats = dict(clash_distance=4.0, clash_weight=1.0, contact_distance=8.0, contacts_min=1.0, contacts_max=inf, contacts_weight=1.0,
                  hotspot_contacts=1.0, hotspot_weight=1.0)

    def call(B=2, N=60, x0=d, M=100, target=d, H=3, hotspot=d, var=d, logp=d, grad=d, report=d, hotspot_out=d, work=d, work_bytes=1 << 30, **kw):
        f = dict(floats, **kw)
        rc = lib.genie_binder_potential(None, B, N, x0, M, target, H, hotspot, *(f[k] for k in floats), var, logp, grad, report, hotspot_out,
                                        work, work_bytes)
        return rc, lib.genie_last_error(None)

    cases = [(dict(B=0), b'B'), (dict(B=65536), b'B'), (dict(N=0), b'N'), (dict(N=-3), b'N'), (dict(M=0), b'M'), (dict(M=-1), b'M'),
             (dict(x0=None), b'x0'), (dict(target=None), b'target'), (dict(var=None), b'var'), (dict(H=-1), b'H'), (dict(H=65), b'H'),
             (dict(hotspot=None), b'hotspot'), (dict(H=0, hotspot=None), b'hotspot_out'),
             (dict(logp=None, grad=None, report=None, hotspot_out=None), b'no output'), (dict(logp=None), b'logp_out and grad_out'),
             (dict(grad=None), b'logp_out and grad_out'), (dict(contacts_min=3.0, contacts_max=2.0), b'contacts_max'),
             (dict(contacts_max=nan), b'contacts_max'), (dict(contacts_max=-1.0), b'contacts_max'), (dict(contacts_min=inf), b'contacts_min'),
             (dict(contact_distance=0.0), b'contact_distance'), (dict(work=None), b'work'), (dict(work_bytes=16), b'work'),
             (dict(work=C.c_void_p(66)), b'aligned'), (dict(M=12715), b'LDS'), (dict(M=1000000), b'LDS')]
    for k in floats:
        if k != 'contacts_max':
            cases += [(dict([(k, v)]), k.encode()) for v in (-1.0, nan)] + ([(dict([(k, inf)]), k.encode())] if k != 'contacts_min' else [])
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b'genie_binder_potential: ') and word in msg, (kw, rc, msg)
    # what is allowed passes every check (and then fails on the device instead, with another code)
    if not torch.cuda.is_available():
        need = lib.genie_binder_potential_work_bytes(2, 60, 3)
        for kw in (dict(), dict(H=0, hotspot=None, hotspot_out=None), dict(logp=None, grad=None), dict(report=None, hotspot_out=None),
                   dict(logp=None, grad=None, report=None), dict(clash_weight=0.0, contacts_weight=0.0, hotspot_weight=0.0),
                   dict(clash_distance=0.0), dict(contacts_min=0.0, contacts_max=0.0), dict(contacts_max=5.0), dict(work_bytes=need),
                   dict(N=1, M=1), dict(M=12714), dict(M=5500), dict(B=65535, work_bytes=1 << 40), dict(H=64)):
            assert call(**kw)[0] != -1, kw
        assert call(work_bytes=need - 1)[0] == -1


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------

def test_load_target_and_parse_hotspots(tmp_path):
    from genie2_amd.features import parse_pdb
    from genie2_amd.smc import load_target, parse_hotspots
    import genie.sampler.binder as mirror
    assert mirror.load_target is load_target and mirror.parse_hotspots is parse_hotspots
    xyz, labels, lengths, aatype = load_target(TARGET)
    seqs, coords = parse_pdb(TARGET)
    assert xyz.dtype == torch.float64 and tuple(xyz.shape) == (100, 3) and lengths == [100] and labels == [('A', i) for i in range(1, 101)]
    assert np.array_equal(xyz.numpy(), np.array(coords[0])) and aatype.tolist() == seqs[0]
    assert load_target(TARGET, 'A')[1] == labels
    for chains in ('B', 'AB', '', 'AA', 5):
        with pytest.raises(ValueError):
            load_target(TARGET, chains)
    # two chains with their own numbering, a hetero atom, an unknown residue name and a side-chain atom
    lines = [ln for ln in open(TARGET) if ln.startswith('ATOM')]
    two = tmp_path / 'two.pdb'
    with open(two, 'w') as fh:
        fh.writelines(lines[:5])
        fh.write(lines[5][:13] + 'CB' + lines[5][15:])
        fh.write('HETATM' + lines[6][6:])
        for k, ln in enumerate(lines[10:14]):
            fh.write(ln[:17] + ('MSE' if k == 0 else ln[17:20]) + ' B' + str(40 + 2 * k).rjust(4) + ln[26:])
        fh.write(lines[20][:21] + 'C' + '  -3' + lines[20][26:])
    xyz, labels, lengths, aatype = load_target(str(two))
    assert labels == [('A', 1), ('A', 2), ('A', 3), ('A', 4), ('A', 5), ('B', 40), ('B', 42), ('B', 44), ('B', 46), ('C', -3)]
    assert lengths == [5, 4, 1] and int(aatype[5]) == 0 and tuple(xyz.shape) == (10, 3)
    xyz_b, labels_b, lengths_b, _ = load_target(str(two), 'CB')
    assert labels_b == labels[5:] and lengths_b == [4, 1] and torch.equal(xyz_b, xyz[5:])      # file order, not the order of `chains`
    with pytest.raises(ValueError, match='no C-alpha'):
        empty = tmp_path / 'empty.pdb'
        empty.write_text('REMARK nothing\n')
        load_target(str(empty))

    assert parse_hotspots('A5,B44 , C-3', labels) == [4, 7, 9] and parse_hotspots('B46 A1', labels) == [0, 8]
    assert parse_hotspots('', labels) == []
    listed = tmp_path / 'hot.txt'
    listed.write_text('# the patch\nB40, B42   # two of them\n\nA3\n')
    assert parse_hotspots(str(listed), labels) == [2, 5, 6]
    for bad, word in (('A6', 'A6'), ('D1', 'D1'), ('A1,A1', 'A1'), ('A', "'A'"), ('45', '45'), ('A4x', 'A4x'), ('B41', 'B41')):
        with pytest.raises(ValueError, match=word):
            parse_hotspots(bad, labels)
    with pytest.raises(ValueError, match='A7'):
        parse_hotspots('A7', labels + [('A', 7), ('A', 7)])                  # (a label two residues carry)
    with pytest.raises(ValueError, match='at most 64'):
        parse_hotspots(','.join('A%d' % i for i in range(1, 66)), [('A', i) for i in range(1, 101)])
    with pytest.raises(ValueError):
        parse_hotspots(['A1'], labels)


def test_place_target_is_a_translation_that_faces_the_hotspots():
    from genie2_amd.smc import load_target, place_target
    xyz = load_target(TARGET)[0]
    hot = [9, 10, 11]
    for standoff in (0.0, 12.0, 30.5):
        out = place_target(xyz, hot, standoff)
        shift = out - xyz
        assert out.dtype == torch.float64 and float((shift - shift[0]).abs().max()) < 1e-12       # one translation, no rotation
        h, t = out[hot].mean(dim=0), out.mean(dim=0)
        assert float(h.norm()) == pytest.approx(standoff, abs=1e-10)
        # the origin lies on the ray from the target centroid through the hotspot centroid, beyond it
        u = (h - t) / (h - t).norm()
        assert float((-h - standoff * u).abs().max()) < 1e-10 and float(t.norm()) == pytest.approx(standoff + float((h - t).norm()), abs=1e-10)
    same = place_target(xyz, hot, None)
    assert torch.equal(same, xyz) and same.data_ptr() != xyz.data_ptr()
    assert torch.equal(place_target(xyz.numpy(), None, None), xyz)
    for args in ((xyz, [], 5.0), (xyz, None, 5.0), (xyz, hot, -1.0), (xyz, hot, math.nan), (xyz, hot, math.inf), (xyz[:, :2], hot, 5.0),
                 (xyz[:0], [], None), (xyz, list(range(100)), 5.0), (torch.zeros(4, 3, dtype=torch.float64), [1], 2.0)):
        with pytest.raises(ValueError):
            place_target(*args)


def test_constructor_validates_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import BinderPotential
    import genie.sampler.binder as mirror
    assert mirror.BinderPotential is BinderPotential
    abar = torch.linspace(0.999, 0.001, 13)
    y = Bd.target(20, 5.0)
    inf, nan = math.inf, math.nan
    for kw in (dict(), dict(hotspots=[]), dict(clash_weight=2.0, contacts_weight=2.0, hotspot_weight=2.0), dict(hotspots=[20]), dict(hotspots=[-1]),
               dict(hotspots=[1, 1]), dict(hotspots=[1.0]), dict(hotspots=[True]), dict(hotspots=5), dict(clash_distance=-1.0),
               dict(clash_distance=nan), dict(clash_distance=inf), dict(clash_distance=4.0, clash_weight=-1.0),
               dict(clash_distance=4.0, contact_distance=0.0), dict(clash_distance=4.0, contact_distance=None),
               dict(clash_distance=4.0, contact_distance=inf), dict(contacts=(3.0, 2.0)), dict(contacts=(-1.0, 2.0)), dict(contacts=(inf, inf)),
               dict(contacts=(1.0, nan)), dict(contacts=5.0), dict(contacts=(1.0,)), dict(contacts=('a', 'b')),
               dict(contacts=(1.0, 2.0), contacts_weight=nan), dict(hotspots=[1], hotspot_contacts=-1.0), dict(hotspots=[1], hotspot_contacts=inf),
               dict(hotspots=[1], hotspot_weight=-0.5), dict(hotspots=[1], tausq=0.0), dict(hotspots=[1], tausq=inf)):
        with pytest.raises(ValueError):
            BinderPotential(40, abar, y, device='cpu', **kw)          # (before the device: a CPU potential is a GenieError)
    with pytest.raises(ValueError, match='no term enabled'):
        BinderPotential(40, abar, y, device='cpu')
    for n_res in (0, -5, 40.0, True):
        with pytest.raises(ValueError):
            BinderPotential(n_res, abar, y, hotspots=[1], device='cpu')
    bad = y.clone()
    bad[3, 1] = nan
    for target in (y[:, :2], y[:0], y.reshape(-1), bad, torch.zeros(12715, 3), 'file.pdb', None):
        with pytest.raises(ValueError):
            BinderPotential(40, abar, target, hotspots=[0], device='cpu')
    with pytest.raises(ValueError, match='at most 64'):
        BinderPotential(40, abar, torch.randn(100, 3), hotspots=list(range(65)), device='cpu')
    for kw in (dict(hotspots=[3, 1]), dict(clash_distance=4.0), dict(contacts=(5.0, inf)), dict(contacts=(0.0, 0.0)),
               dict(hotspots=torch.tensor([0, 19]), clash_distance=0.0, contacts=(1, 2), hotspot_contacts=0.0, hotspot_weight=0.0)):
        with pytest.raises(capi.GenieError, match='no CPU path'):
            BinderPotential(40, abar, y, device='cpu', **kw)
    with pytest.raises(capi.GenieError, match='no CPU path'):
        BinderPotential(40, abar, y.double().numpy(), hotspots=[2], device='cpu')
    doc = BinderPotential.__doc__
    assert 'design choices' in doc and 'unmeasured' in doc


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

def test_parsers_constants_and_the_no_term_message():
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    import genie.sample_unconditional_shape as mirror
    assert mirror.add_binder_arguments is Sh.add_binder_arguments and mirror.binder_potential is Sh.binder_potential
    base = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']
    defaults = dict(target_pdb=None, target_chains=None, hotspots=None, hotspot_contacts=1.0, hotspot_weight=1.0, contact_distance=8.0,
                    contacts_min=None, contacts_max=None, contacts_weight=1.0, target_clash_distance=None, target_clash_weight=1.0,
                    target_standoff=None, binder_tausq=1.0, write_binder=False, write_complex=False)
    given = ['--target_pdb', TARGET, '--target_chains', 'A', '--hotspots', 'A10,A11,A12', '--hotspot_contacts', '2', '--hotspot_weight', '0.5',
             '--contact_distance', '9', '--contacts_min', '20', '--contacts_max', '60', '--contacts_weight', '0.25', '--target_clash_distance',
             '4', '--target_clash_weight', '3', '--target_standoff', '12', '--binder_tausq', '4', '--write_binder', '--write_complex']
    values = dict(target_pdb=TARGET, target_chains='A', hotspots='A10,A11,A12', hotspot_contacts=2.0, hotspot_weight=0.5, contact_distance=9.0,
                  contacts_min=20.0, contacts_max=60.0, contacts_weight=0.25, target_clash_distance=4.0, target_clash_weight=3.0,
                  target_standoff=12.0, binder_tausq=4.0, write_binder=True, write_complex=True)
    for parser, more in ((Sh.build_parser(), []), (M.build_parser(), ['--motif_file', MOTIF])):
        a = vars(parser.parse_args(base + more))
        assert {k: a[k] for k in defaults} == defaults
        # (the flags that were there keep their defaults)
        assert a['rog_max'] is None and a['clash_distance'] is None and a['symmetry'] is None and a['clash_weight'] == 1.0
        a = vars(parser.parse_args(base + more + given))
        assert {k: a[k] for k in values} == values

    # constants: a binder term is enough on its own for the shape CLI; the target arrives read, placed and picklable
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base + given)))
    assert {k: c[k] for k in values} == values and Sh.has_binder_terms(c) and c['contacts'] == (20.0, 60.0)
    assert not Sh.has_shape_terms(c) and not Sh.has_secstruct_terms(c) and not Sh.has_sheet_terms(c) and not Sh.has_symmetry_terms(c)
    t = c['target']
    assert t['hotspots'] == [9, 10, 11] and t['chain_lengths'] == [100] and t['labels'][9] == ('A', 10) and Sh.hotspot_names(t) == ['A10', 'A11', 'A12']
    assert isinstance(t['xyz'], np.ndarray) and t['xyz'].dtype == np.float64 and t['xyz'].shape == (100, 3) and t['aatype'].shape == (100,)
    assert float(np.linalg.norm(t['xyz'][[9, 10, 11]].mean(axis=0))) == pytest.approx(12.0, abs=1e-9)
    import pickle
    assert pickle.loads(pickle.dumps(t))['hotspots'] == [9, 10, 11]
    for flags, want in ((['--contacts_min', '5'], (5.0, math.inf)), (['--contacts_max', '7'], (0.0, 7.0))):
        c = Sh.binder_constants(vars(Sh.build_parser().parse_args(base + ['--target_pdb', TARGET] + flags)))
        assert c['contacts'] == want and c['target']['hotspots'] == []
        from genie2_amd.smc import load_target
        assert np.array_equal(c['target']['xyz'], load_target(TARGET)[0].numpy())                # no standoff: the file's frame
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF] + given)))
    assert {k: c[k] for k in values} == values and c['tausq'] == 0.012 and Sh.has_binder_terms(c)
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF])))
    assert {k: c[k] for k in defaults} == defaults and c['target'] is None and not Sh.has_binder_terms(c)
    assert Sh.binder_potential(c, 60, None, 'cuda') is None                                    # no term: no potential, no device

    # a binder flag without --target_pdb says so, in both CLIs; a target without a term, and one that does not hold up, end the run too
    for flags in (['--hotspots', 'A10'], ['--contacts_min', '5'], ['--target_clash_distance', '4'], ['--write_binder'], ['--write_complex'],
                  ['--target_standoff', '10'], ['--binder_tausq', '2'], ['--target_chains', 'A'], ['--hotspot_weight', '2']):
        with pytest.raises(SystemExit, match='needs --target_pdb'):
            Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base + flags)))
        with pytest.raises(SystemExit, match='needs --target_pdb'):
            M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + ['--motif_file', MOTIF] + flags)))
    for flags in ([], ['--write_binder'], ['--hotspots', 'A101'], ['--hotspots', 'A10', '--target_chains', 'B'],
                  ['--contacts_min', '5', '--target_standoff', '10'], ['--hotspots', 'A10', '--target_standoff', '-1']):
        with pytest.raises(SystemExit):
            Sh.binder_constants(vars(Sh.build_parser().parse_args(base + ['--target_pdb', TARGET] + flags)))
    with pytest.raises(SystemExit):
        Sh.binder_constants(vars(Sh.build_parser().parse_args(base + ['--target_pdb', 'no_such_file.pdb', '--hotspots', 'A10'])))
    # the message of a run with no term names the binder flags, and still ends as tests/test_symmetry_host.py reads it
    with pytest.raises(SystemExit, match='no shape term.*--symmetry$') as info:
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(base)))
    assert '--target_pdb' in str(info.value) and '--hotspots' in str(info.value)


def test_report_and_complex_writers(tmp_path):
    from genie2_amd import capi
    from genie2_amd import sample_unconditional_shape as Sh
    from genie2_amd.features import parse_pdb
    base = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']
    c = Sh.binder_constants(vars(Sh.build_parser().parse_args(base + ['--target_pdb', TARGET, '--hotspots', 'A12,A10', '--target_standoff', '12'])))
    merged = {'rog': torch.tensor([12.3, 9.0]), 'contacts': torch.tensor([41.23456, 0.0]), 'n_contacts': torch.tensor([37, 0]),
              'n_interface': torch.tensor([12, 0]), 'target_min_distance': torch.tensor([4.56789, 73.2]), 'n_target_clash': torch.tensor([1, 0]),
              'n_hotspots_contacted': torch.tensor([2, 0]), 'e_target_clash': torch.tensor([0.0004, 0.0]), 'e_contact': torch.tensor([1234.5678, 25.0]),
              'e_hotspot': torch.tensor([0.0, 2.0])}
    assert list(Sh.report_fields(merged, capi.BINDER_REPORT)) == list(capi.BINDER_REPORT)
    Sh.write_binder_report(torch.tensor([[0.87349, 1.5], [0.0, 1e-7]]), Sh.hotspot_names(c['target']), Sh.report_fields(merged, capi.BINDER_REPORT),
                           str(tmp_path / 'binder'), 40, 4)
    assert sorted(os.listdir(tmp_path / 'binder')) == ['40_4.txt', '40_5.txt']
    assert (tmp_path / 'binder' / '40_4.txt').read_text() == (
        'hotspot A10 0.873\nhotspot A12 1.500\ncontacts 41.235\nn_contacts 37\nn_interface 12\ntarget_min_distance 4.568\nn_target_clash 1\n'
        'n_hotspots_contacted 2\ne_target_clash 0.000\ne_contact 1234.568\ne_hotspot 0.000\n')
    assert (tmp_path / 'binder' / '40_5.txt').read_text().splitlines()[:3] == ['hotspot A10 0.000', 'hotspot A12 0.000', 'contacts 0.000']
    # no hotspots: the report alone
    Sh.write_binder_report(torch.zeros(2, 0), [], Sh.report_fields(merged, capi.BINDER_REPORT), str(tmp_path / 'plain'), 40, 0)
    assert (tmp_path / 'plain' / '40_0.txt').read_text().splitlines()[0] == 'contacts 41.235'

    # the complex: the target's chain, then the design as the last chain; centred as a whole, relative placement kept
    designs = Bd.designs(2, 40) + torch.tensor([0.0, 3.0, -2.0])
    Sh.write_complex(designs.numpy(), c['target'], str(tmp_path / 'complex'), 40, 4)
    assert sorted(os.listdir(tmp_path / 'complex')) == ['40_4.pdb', '40_5.pdb']
    for i in range(2):
        path = str(tmp_path / 'complex' / ('40_%d.pdb' % (4 + i)))
        lines = [ln for ln in open(path) if ln.startswith('ATOM')]
        assert [ln[21] for ln in lines] == ['A'] * 100 + ['B'] * 40
        assert [int(ln[22:26]) for ln in lines] == list(range(1, 101)) + list(range(1, 41))
        seqs, coords = parse_pdb(path)
        assert seqs[0] == parse_pdb(TARGET)[0][0] and seqs[1] == [0] * 40
        got = np.concatenate(coords)
        want = np.concatenate([c['target']['xyz'], designs[i].double().numpy()])
        assert np.abs(got.mean(axis=0)).max() < 1e-3
        assert np.abs(got - (want - want.mean(axis=0))).max() <= 5e-4 + 1e-9                   # (the file rounds to 1e-3)
    # two target chains: the design is chain C
    target = dict(c['target'], chain_lengths=[60, 40])
    Sh.write_complex(designs[:1].numpy(), target, str(tmp_path / 'two'), 40, 0)
    assert [ln[21] for ln in open(tmp_path / 'two' / '40_0.pdb')] == ['A'] * 60 + ['B'] * 40 + ['C'] * 40
