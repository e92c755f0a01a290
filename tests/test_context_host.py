"""The context potential without a device: the float64 oracle of tests/_context.py against its own loop gradient, its invariance under
rigid motion and the balance of its gradient; csrc/horn.h's four-eigenpair fit and its adjoint as a stand-alone host program under the
address and undefined-behaviour sanitizers; the C entry's symbols, work sizes and refusals (genie_context_potential,
include/genie_hip.h); ContextPotential's host side; the motif command line's parser, constants and writers.

What holds the kernel to the oracle is tests/test_context_gpu.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import _context as Cx
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')
TARGET = os.path.join(GOLDEN, 'dataset_100_0.pdb')       # 100 residues, chain A, numbered from 1
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', Cx.CASES[:3], ids=Cx.case_id)
def test_oracle_gradient_matches_the_looped_analytic_gradient(case):
    """Autograd through torch.linalg.eigh against the header's formula written with loops -- pair forces, their sum and moment, the
    adjoint of the fit through the three other eigenpairs, the anchors' shares -- to 1e-12 of the largest entry, for both terms
    together and each alone; the anchors carry gradient, so a formula without the part through the rotation would not pass."""
    x, idx, t, y, cfg = Cx.inputs(case)
    x, var = x.double(), 0.8
    ref = Cx.reference(x, idx, t, y, cfg, var)
    scale = float(ref['grad'].abs().max())
    assert float((ref['grad'] - Cx.analytic_gradient(x, idx, t, y, cfg, var)).abs().max()) <= 1e-12 * scale
    assert torch.allclose(ref['logp'], -(ref['e_context_clash'] + ref['e_context_contact']) / (2 * var), rtol=1e-13, atol=0)
    for term in ('clash', 'contacts'):
        one = Cx.only(cfg, term)
        part = Cx.reference(x, idx, t, y, one, var)
        assert float((part['grad'] - Cx.analytic_gradient(x, idx, t, y, one, var)).abs().max()) <= 1e-12 * scale, term
        assert float(part['grad'].abs().max()) > 0, term
    on_anchor = torch.gather(ref['grad'].abs().amax(dim=2), 1, idx).amax(dim=1)
    assert float((on_anchor / ref['grad'].abs().amax(dim=(1, 2))).max()) >= 1e-2
    # the float32 restatement is the same function to float32 rounding (the fit amplifies by 1 / gap, at least 0.1 here)
    r32 = Cx.restatement32(x, idx, t, y, cfg, var)
    assert torch.allclose(r32['logp'].double(), ref['logp'], rtol=1e-4) and float((r32['grad'].double() - ref['grad']).abs().max()) <= 1e-3 * scale


@pytest.mark.parametrize('case', [Cx.CASES[1], Cx.CASES[4]], ids=Cx.case_id)
def test_oracle_is_invariant_and_its_gradient_balanced(case):
    """logp does not change under a rigid motion of x (the context follows), and the gradient has no net force and no net torque:
    to 1e-12 of the scale of each."""
    x, idx, t, y, cfg = Cx.inputs(case)
    x = x.double()
    ref = Cx.reference(x, idx, t, y, cfg, 1.0)
    Q, shift = Cx.random_rotation(3), torch.tensor([5.0, -40.0, 17.0], dtype=torch.float64)
    moved = Cx.reference(x @ Q.T + shift, idx, t, y, cfg, 1.0)
    assert torch.allclose(moved['logp'], ref['logp'], rtol=1e-12, atol=0)
    assert torch.allclose(moved['grad'], ref['grad'] @ Q.T, rtol=0, atol=1e-12 * float(ref['grad'].abs().max()))
    assert torch.allclose(moved['placed'], ref['placed'] @ Q.T + shift, rtol=0, atol=1e-10)
    g = ref['grad']
    N, size, scale = x.shape[1], float(x.abs().max()), float(g.abs().max())
    assert float(g.sum(dim=1).abs().max()) <= 1e-12 * N * scale
    assert float(torch.cross(x, g, dim=2).sum(dim=1).abs().max()) <= 1e-12 * N * size * scale


def test_oracle_inputs_report_and_limits():
    """Every parity input passes the oracle's own conditions; the report's fields are what their definitions say on a hand-made
    input whose fit is exact; contacts_max = inf has no upper hinge; a weight of 0 removes energy and force."""
    for case in Cx.CASES + [Cx.LDS_CASE]:
        x, idx, t, y, cfg = Cx.inputs(case)
        assert Cx.margins(x, idx, t, y, cfg) >= 1e-4 and tuple(idx.shape) == (case[0], case[2]) and tuple(y.shape) == (case[3], 3)
    assert Cx.anchor_runs(65, 12)[-4:] == [61, 62, 63, 64] and Cx.anchor_runs(4, 3) == [0, 1, 3]
    # the motif is the design's anchors turned a quarter about z and shifted: the fit undoes exactly that
    x = torch.tensor([[[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 0.0, 5.0], [10.0, 0.0, 0.0], [50.0, 0.0, 0.0]]])
    idx = torch.tensor([[0, 1, 2, 3]])
    Q = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    shift = torch.tensor([7.0, -2.0, 1.0])
    t = x[0, :4] @ Q.T + shift
    y = torch.tensor([[10.0, 3.0, 0.0], [10.0, 7.0, 0.0], [100.0, 0.0, 0.0]]) @ Q.T + shift
    cfg = Cx.config(clash_distance=4.0, clash_weight=2.0, contacts_min=5.0, contacts_max=6.0, contacts_weight=0.5)
    r = Cx.reference(x, idx, t, y, cfg, 1.0)
    assert float(r['anchor_rmsd']) < 1e-6 and torch.allclose(r['R'][0], Q.T.double(), atol=1e-6)
    assert torch.allclose(r['placed'][0], torch.tensor([[10.0, 3.0, 0.0], [10.0, 7.0, 0.0], [100.0, 0.0, 0.0]], dtype=torch.float64), atol=1e-5)
    assert int(r['n_context_contacts']) == 2 and int(r['n_context_interface']) == 1 and int(r['n_context_clash']) == 1
    assert float(r['context_min_distance']) == pytest.approx(3.0, abs=1e-5) and float(r['e_context_clash']) == pytest.approx(2.0, abs=1e-4)
    s = lambda d: 1.0 / (1.0 + (d / 8.0) ** 6)      # noqa: E731
    total = sum(s(v) for v in (3.0, 7.0, 90.0, math.hypot(40, 3), math.hypot(40, 7), 50.0))      # residues 4 and 5: the anchors sit out
    assert float(r['context_contacts']) == pytest.approx(total, rel=1e-6)
    assert float(r['e_context_contact']) == pytest.approx(0.5 * (5.0 - total) ** 2, rel=1e-6)
    above = Cx.reference(x, idx, t, y, dict(cfg, contacts_min=0.0, contacts_max=1.0), 1.0)
    assert float(above['e_context_contact']) == pytest.approx(0.5 * (total - 1.0) ** 2, rel=1e-6)
    assert float(Cx.reference(x, idx, t, y, dict(cfg, contacts_min=0.0, contacts_max=math.inf), 1.0)['e_context_contact']) == 0.0
    off = Cx.reference(x, idx, t, y, dict(cfg, clash_weight=0.0, contacts_weight=0.0), 1.0)
    assert float(off['logp']) == 0.0 and bool((off['grad'] == 0).all())


# ---- the fit and its adjoint, stand-alone ----------------------------------------------------------------------------------------

def test_fit_and_adjoint_on_the_host_under_sanitizers(tmp_path):
    """tests/context_fit_check.cpp: mr_eigen and mr_fit_adjoint of csrc/horn.h compiled for the host alone into a program of its own,
    with the address and undefined-behaviour sanitizers, against a float64 Jacobi and central differences (its bounds are derived in
    the file).  Nothing of it is loaded into this process."""
    from genie2_amd import build
    exe = str(tmp_path / 'context_fit_check')
    sanitize = ['-Xarch_host', '-fsanitize=address', '-Xarch_host', '-fsanitize=undefined', '-Xarch_host', '-fno-sanitize-recover=undefined']
    cmd = [build.HIPCC, '-x', 'hip', '--cuda-host-only', '-O1', '-g', '-std=c++17'] + sanitize + [os.path.join(HERE, 'context_fit_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), (r.stdout, r.stderr)


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_load(lib):
    from genie2_amd import build, capi
    assert 'context_kernels.hip' in build.SOURCES and os.path.exists(os.path.join(os.path.dirname(build.__file__), 'csrc', 'context_kernels.hip'))
    assert len(capi.SYMBOLS['genie_context_potential'][1]) == 22 and capi.SYMBOLS['genie_context_potential'][0] is C.c_int
    assert capi.SYMBOLS['genie_context_potential_work_bytes'] == (C.c_size_t, [C.c_int, C.c_int])
    assert lib.genie_context_potential is not None and lib.genie_context_potential_work_bytes is not None
    assert capi.CONTEXT_REPORT == Cx.REPORT and len(capi.CONTEXT_REPORT) == 8 and capi.CONTEXT_COUNTS == Cx.COUNTS
    assert not set(capi.CONTEXT_REPORT) & set(capi.BINDER_REPORT) and not set(capi.CONTEXT_REPORT) & set(capi.SHAPE_REPORT)
    header = open(os.path.join(os.path.dirname(build.__file__), '..', 'include', 'genie_hip.h')).read()
    assert '#define GENIE_CONTEXT_REPORT 8' in header and '#define GENIE_CONTEXT_MAX_ATOMS %d' % capi.CONTEXT_MAX_ATOMS in header
    assert len(capi.SYMBOLS['genie_binder_potential'][1]) == 23                                # (the neighbours keep their arguments)
    horn = open(os.path.join(os.path.dirname(build.__file__), 'csrc', 'horn.h')).read()
    assert 'MrEigen mr_eigen(' in horn and 'MrMat mr_fit_adjoint(' in horn and 'MR_GAP_FLOOR = 1e-6f' in horn
    # 4 B (40 + 7 N + 32 ceil(N / 64)) bytes; 0 for sizes the entry refuses
    wb = lib.genie_context_potential_work_bytes
    for B, N in ((1, 3), (3, 64), (3, 65), (2, 129), (128, 256), (65535, 4)):
        assert wb(B, N) == 4 * B * (40 + 7 * N + 32 * ((N + 63) // 64)), (B, N)
    assert all(wb(*a) == 0 for a in ((0, 5), (1, 0), (-1, 5)))


def test_entry_refuses_before_the_device_is_touched(lib):
    """Every refusal returns GENIE_E_ARG without a device, and genie_last_error(NULL) names the entry and the argument."""
    from genie2_amd import capi
    d = C.c_void_p(64)                                           # never dereferenced: every call below fails its checks
    inf, nan = math.inf, math.nan
    floats = dict(clash_distance=4.0, clash_weight=1.0, contact_distance=8.0, contacts_min=1.0, contacts_max=inf, contacts_weight=1.0)

    def call(B=2, N=60, x0=d, A=13, anchor_index=d, anchor_xyz=d, Cn=100, context=d, var=d, logp=d, grad=d, report=d, pose=d, work=d,
             work_bytes=1 << 30, **kw):
        f = dict(floats, **kw)
        rc = lib.genie_context_potential(None, B, N, x0, A, anchor_index, anchor_xyz, Cn, context, *(f[k] for k in floats), var, logp, grad,
                                         report, pose, work, work_bytes)
        return rc, lib.genie_last_error(None)

    cases = [(dict(B=0), b'B'), (dict(B=65536), b'B'), (dict(N=0), b'N'), (dict(N=-3), b'N'), (dict(A=2), b'A outside'), (dict(A=61), b'A outside'),
             (dict(A=-1), b'A outside'), (dict(Cn=0), b'C below'), (dict(Cn=-1), b'C below'), (dict(x0=None), b'x0'),
             (dict(anchor_index=None), b'anchor_index'), (dict(anchor_xyz=None), b'anchor_xyz'), (dict(context=None), b'context'),
             (dict(var=None), b'var'), (dict(logp=None, grad=None, report=None, pose=None), b'no output'),
             (dict(logp=None), b'logp_out and grad_out'), (dict(grad=None), b'logp_out and grad_out'),
             (dict(contacts_min=3.0, contacts_max=2.0), b'contacts_max'), (dict(contacts_max=nan), b'contacts_max'),
             (dict(contacts_max=-1.0), b'contacts_max'), (dict(contacts_min=inf), b'contacts_min'), (dict(contact_distance=0.0), b'contact_distance'),
             (dict(work=None), b'work'), (dict(work_bytes=16), b'work'), (dict(work=C.c_void_p(66)), b'aligned'),
             (dict(Cn=capi.CONTEXT_MAX_ATOMS + 1), b'LDS'), (dict(Cn=1000000), b'LDS')]
    for k in floats:
        if k != 'contacts_max':
            cases += [(dict([(k, v)]), k.encode()) for v in (-1.0, nan)] + ([(dict([(k, inf)]), k.encode())] if k != 'contacts_min' else [])
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b'genie_context_potential: ') and word in msg, (kw, rc, msg)
    # what is allowed passes every check (and then fails on the device instead, with another code)
    if not torch.cuda.is_available():
        need = lib.genie_context_potential_work_bytes(2, 60)
        for kw in (dict(), dict(logp=None, grad=None), dict(report=None, pose=None), dict(logp=None, grad=None, report=None),
                   dict(clash_weight=0.0, contacts_weight=0.0), dict(clash_distance=0.0), dict(contacts_min=0.0, contacts_max=0.0),
                   dict(contacts_max=5.0), dict(work_bytes=need), dict(N=3, A=3, Cn=1), dict(A=60), dict(Cn=capi.CONTEXT_MAX_ATOMS), dict(Cn=5500),
                   dict(B=65535, work_bytes=1 << 40)):
            assert call(**kw)[0] != -1, kw
        assert call(work_bytes=need - 1)[0] == -1


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------

def test_constructor_validates_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import ContextPotential, check_anchor_index
    import genie.sampler.context as mirror
    assert mirror.ContextPotential is ContextPotential
    abar = torch.linspace(0.999, 0.001, 13)
    t, y = Cx.walk(5, 1), Cx.walk(20, 2)
    idx = [3, 4, 5, 20, 21]
    inf, nan = math.inf, math.nan
    ok = dict(anchor_index=idx, clash_distance=4.0)
    for kw in (dict(anchor_index=idx), dict(clash_distance=4.0), dict(ok, motif=object()), dict(ok, segments=[0]), dict(ok, anchor_index=idx[:4]),
               dict(ok, anchor_index=[3, 4, 5, 20, 40]), dict(ok, anchor_index=[-1, 4, 5, 20, 21]), dict(ok, anchor_index=[3, 3, 5, 20, 21]),
               dict(ok, anchor_index=[3.0, 4, 5, 20, 21]), dict(ok, anchor_index=[True, 4, 5, 20, 21]), dict(ok, anchor_index=7),
               dict(ok, anchor_index=[idx, idx[:4]]), dict(clash_distance=4.0, motif=object()), dict(ok, clash_distance=-1.0), dict(ok, clash_distance=nan),
               dict(ok, clash_distance=inf), dict(ok, clash_weight=-1.0), dict(ok, contact_distance=0.0), dict(ok, contact_distance=None),
               dict(ok, contact_distance=inf), dict(ok, contacts=(3.0, 2.0)), dict(ok, contacts=(-1.0, 2.0)), dict(ok, contacts=(inf, inf)),
               dict(ok, contacts=(1.0, nan)), dict(ok, contacts=5.0), dict(ok, contacts=(1.0,)), dict(ok, contacts=('a', 'b')),
               dict(ok, contacts=(1.0, 2.0), contacts_weight=nan), dict(ok, tausq=0.0), dict(ok, tausq=inf)):
        with pytest.raises(ValueError):
            ContextPotential(40, abar, t, y, device='cpu', **kw)        # (before the device: a CPU potential is a GenieError)
    with pytest.raises(ValueError, match='no term enabled'):
        ContextPotential(40, abar, t, y, anchor_index=idx, device='cpu')
    with pytest.raises(ValueError, match='exactly one of anchor_index and motif'):
        ContextPotential(40, abar, t, y, clash_distance=4.0, device='cpu')
    for n_res in (0, -5, 40.0, True, 4):                                # (4: fewer residues than anchors)
        with pytest.raises(ValueError):
            ContextPotential(n_res, abar, t, y, anchor_index=[0, 1, 2, 3, 4], clash_distance=4.0, device='cpu')
    bad = y.clone()
    bad[3, 1] = nan
    for context in (y[:, :2], y[:0], y.reshape(-1), bad, torch.zeros(capi.CONTEXT_MAX_ATOMS + 1, 3), 'file.pdb', None):
        with pytest.raises(ValueError, match='context'):
            ContextPotential(40, abar, t, context, device='cpu', **ok)
    line = torch.arange(5.0)[:, None] * torch.tensor([1.0, 2.0, -1.0])
    for anchors in (t[:, :2], t[:2], bad[:5], line, None):
        with pytest.raises(ValueError, match='anchor_xyz'):
            ContextPotential(40, abar, anchors, y, anchor_index=idx[:len(anchors) if anchors is not None else 5], clash_distance=4.0, device='cpu')
    for kw in (ok, dict(anchor_index=idx, contacts=(5.0, inf)), dict(anchor_index=idx, contacts=(0.0, 0.0)),
               dict(anchor_index=torch.tensor([idx, idx[::-1]]), clash_distance=0.0, contacts=(1, 2)),
               dict(anchor_index=np.array(idx).tolist(), clash_distance=4.0, clash_weight=0.0)):
        with pytest.raises(capi.GenieError, match='no CPU path'):
            ContextPotential(40, abar, t, y, device='cpu', **kw)
    with pytest.raises(capi.GenieError, match='no CPU path'):
        ContextPotential(40, abar, t.double().numpy(), y.double().numpy(), device='cpu', **ok)
    rows = check_anchor_index(torch.tensor([idx, idx[::-1]]), 5, 40)
    assert rows.dtype == torch.int32 and rows.tolist() == [idx, idx[::-1]] and check_anchor_index(idx, 5, 40).tolist() == [idx]
    doc = ContextPotential.__doc__
    assert 'design choices' in doc and 'unmeasured' in doc and 'held fixed' in doc


# ---- the command line ----------------------------------------------------------------------------------------------------------------

def test_parser_constants_and_refusals(tmp_path):
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    base = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']
    motif = ['--motif_file', MOTIF]
    defaults = dict(context_pdb=None, context_chains=None, context_clash_distance=None, context_clash_weight=1.0, context_contact_distance=8.0,
                    context_contacts_min=None, context_contacts_max=None, context_contacts_weight=1.0, context_group=None, context_tausq=1.0,
                    write_context=False, write_context_complex=False)
    assert Sh.CONTEXT_DEFAULTS == defaults
    given = ['--context_pdb', TARGET, '--context_chains', 'A', '--context_clash_distance', '4', '--context_clash_weight', '3',
             '--context_contact_distance', '9', '--context_contacts_min', '20', '--context_contacts_max', '60', '--context_contacts_weight', '0.25',
             '--context_tausq', '4', '--write_context', '--write_context_complex']
    values = dict(context_pdb=TARGET, context_chains='A', context_clash_distance=4.0, context_clash_weight=3.0, context_contact_distance=9.0,
                  context_contacts_min=20.0, context_contacts_max=60.0, context_contacts_weight=0.25, context_group=None, context_tausq=4.0,
                  write_context=True, write_context_complex=True)
    a = vars(M.build_parser().parse_args(base + motif))
    assert {k: a[k] for k in defaults} == defaults and a['target_pdb'] is None and a['align'] == 'translation'      # (the others keep theirs)
    a = vars(M.build_parser().parse_args(base + motif + given))
    assert {k: a[k] for k in values} == values
    # the shape CLI does not take the flags: a context needs a motif
    with pytest.raises(SystemExit):
        Sh.build_parser().parse_args(base + ['--rog_max', '8', '--context_pdb', TARGET])
    assert not any(k.startswith('context') for k in vars(Sh.build_parser().parse_args(base + ['--rog_max', '8'])))

    # a run without context flags builds the motif potential alone, and its constants say so without looking at a device
    c = M.MotifRunner().create_constants(a0 := vars(M.build_parser().parse_args(base + motif)))
    assert a0['context_pdb'] is None and c['context'] is None and c['context_segments'] is None and not Sh.has_context_terms(c)
    assert not c['write_context'] and not c['write_context_complex']
    made = []

    class FakeMotif:
        def __init__(self, *args, **kw):
            made.append((args, kw))
    import genie2_amd.smc as smc
    real = smc.MotifPotential
    smc.MotifPotential = FakeMotif
    try:
        runner = M.MotifRunner()
        pots = runner.batch_potentials(c, 60, None, 'cuda')
    finally:
        smc.MotifPotential = real
    assert len(pots) == 1 and isinstance(pots[0], FakeMotif) and runner.context is None and len(made) == 1

    # with them: the file read in its own frame, picklable; the contact range completed as the binder's is
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + motif + given)))
    assert {k: c[k] for k in values} == values and Sh.has_context_terms(c) and c['context_contacts'] == (20.0, 60.0) and c['context_segments'] == [0, 1]
    from genie2_amd.smc import load_target
    t = c['context']
    assert isinstance(t['xyz'], np.ndarray) and t['xyz'].dtype == np.float64 and np.array_equal(t['xyz'], load_target(TARGET)[0].numpy())
    assert t['chain_lengths'] == [100] and t['labels'][9] == ('A', 10) and t['aatype'].shape == (100,)
    import pickle
    assert pickle.loads(pickle.dumps(t))['chain_lengths'] == [100]
    for flags, want in ((['--context_contacts_min', '5'], (5.0, math.inf)), (['--context_contacts_max', '7'], (0.0, 7.0))):
        assert Sh.context_constants(vars(M.build_parser().parse_args(base + motif + ['--context_pdb', TARGET] + flags)))['context_contacts'] == want
    # motif groups: the context is tied to one of them
    grouped = base + motif + ['--motif_groups', 'file', '--context_pdb', TARGET, '--context_clash_distance', '4']
    assert M.MotifRunner().create_constants(vars(M.build_parser().parse_args(grouped + ['--context_group', 'A'])))['context_segments'] == [0]
    assert M.MotifRunner().create_constants(vars(M.build_parser().parse_args(grouped + ['--context_group', 'B'])))['context_segments'] == [1]
    with pytest.raises(SystemExit, match='needs --context_group'):
        M.MotifRunner().create_constants(vars(M.build_parser().parse_args(grouped)))
    with pytest.raises(SystemExit, match='--context_group Z'):
        M.MotifRunner().create_constants(vars(M.build_parser().parse_args(grouped + ['--context_group', 'Z'])))
    with pytest.raises(SystemExit, match='needs --motif_groups file'):
        M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + motif + ['--context_pdb', TARGET, '--context_clash_distance', '4',
                                                                                             '--context_group', 'A'])))

    # a context flag without --context_pdb says so; a context without a term, and a file or chain that does not hold up, end the run too
    for flags in (['--context_clash_distance', '4'], ['--context_contacts_min', '5'], ['--write_context'], ['--write_context_complex'],
                  ['--context_tausq', '2'], ['--context_chains', 'A'], ['--context_clash_weight', '2'], ['--context_group', 'A'],
                  ['--context_contact_distance', '9']):
        with pytest.raises(SystemExit, match='needs --context_pdb'):
            M.MotifRunner().create_constants(vars(M.build_parser().parse_args(base + motif + flags)))
    for flags in ([], ['--write_context'], ['--context_clash_distance', '4', '--context_chains', 'B']):
        with pytest.raises(SystemExit):
            Sh.context_constants(vars(M.build_parser().parse_args(base + motif + ['--context_pdb', TARGET] + flags)))
    with pytest.raises(SystemExit):
        Sh.context_constants(vars(M.build_parser().parse_args(base + motif + ['--context_pdb', 'no_such_file.pdb', '--context_clash_distance', '4'])))
    assert 'unmeasured' in open(Sh.__file__).read().split('CONTEXT_DEFAULTS = ')[0][-400:]


def test_report_and_complex_writers(tmp_path):
    from genie2_amd import capi
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    from genie2_amd.features import parse_pdb
    base = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o', '--motif_file', MOTIF]
    c = Sh.context_constants(vars(M.build_parser().parse_args(base + ['--context_pdb', TARGET, '--context_clash_distance', '4'])))
    merged = {'rog': torch.tensor([12.3, 9.0]), 'context_contacts': torch.tensor([41.23456, 0.0]), 'n_context_contacts': torch.tensor([37, 0]),
              'n_context_interface': torch.tensor([12, 0]), 'context_min_distance': torch.tensor([4.56789, 73.2]),
              'n_context_clash': torch.tensor([1, 0]), 'anchor_rmsd': torch.tensor([0.87349, 1.5]), 'e_context_clash': torch.tensor([0.0004, 0.0]),
              'e_context_contact': torch.tensor([1234.5678, 25.0])}
    Sh.write_context_report(Sh.report_fields(merged, capi.CONTEXT_REPORT), str(tmp_path / 'context'), 40, 4)
    assert sorted(os.listdir(tmp_path / 'context')) == ['40_4.txt', '40_5.txt']
    assert (tmp_path / 'context' / '40_4.txt').read_text() == (
        'context_contacts 41.235\nn_context_contacts 37\nn_context_interface 12\ncontext_min_distance 4.568\nn_context_clash 1\n'
        'anchor_rmsd 0.873\ne_context_clash 0.000\ne_context_contact 1234.568\n')
    # the complex: the context's chain as placed for each design, then the design as the last chain; centred as a whole
    designs = Cx.designs(2, 40) + torch.tensor([0.0, 3.0, -2.0])
    placed = np.stack([c['context']['xyz'] + 1.0, c['context']['xyz'][:, [1, 2, 0]] - 2.0])
    Sh.write_context_complex(designs.numpy(), placed, c['context'], str(tmp_path / 'complex'), 40, 4)
    assert sorted(os.listdir(tmp_path / 'complex')) == ['40_4.pdb', '40_5.pdb']
    for i in range(2):
        path = str(tmp_path / 'complex' / ('40_%d.pdb' % (4 + i)))
        lines = [ln for ln in open(path) if ln.startswith('ATOM')]
        assert [ln[21] for ln in lines] == ['A'] * 100 + ['B'] * 40
        seqs, coords = parse_pdb(path)
        assert seqs[0] == parse_pdb(TARGET)[0][0] and seqs[1] == [0] * 40
        got = np.concatenate(coords)
        want = np.concatenate([placed[i], designs[i].double().numpy()])
        assert np.abs(got - (want - want.mean(axis=0))).max() <= 5e-4 + 1e-9                   # (the file rounds to 1e-3)
