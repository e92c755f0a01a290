"""The superposed (rotation-invariant) motif potential, genie_motif_potential_rigid (csrc/smc_kernels.hip), MotifPotential(align='rigid')
and MotifPotential.locate in genie2_amd/smc.py, TwistedSampler.last_fit and the CLI's --align / --write_motif_locations, against the
float64 oracle of tests/_motif_rigid.py (Kabsch by SVD, torch autograd).

Bounds, those the translation kernel is held to (tests/test_motif_potential.py): logp within 1e-5 max(1, |logp|); gradient within 1e-5
of the particle's largest gradient entry; rmsd within 1e-5 relative + 1e-4 A.  The planted fit alone compares its gradient to
1e-5 (max|g_b| + max|t_c| / var): there the gradient is the difference of two terms of size |t_c| / var, and float32 resolves it
against that scale."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _motif import (_abar, _ca_coordinates, _check, _fix_var, _lds_cap, _pot, _run, _tiny_model, _var500, all_starts as _all_starts,
                    segments_6e6r as _segments, top_two_gap, walk as _walk)
from _motif_rigid import fit_rmsd, logp_only, rigid_oracle
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')
_ORACLE = {}


def _target():
    t = torch.cat(_segments())
    return t - t.mean(dim=0, keepdim=True)


def _oracle(key, x0, starts, lens, target, var, **kw):
    """One float64 reference per (case, var), shared by the tests that need it."""
    k = (key, float(var), tuple(sorted(kw.items())))
    if k not in _ORACLE:
        _ORACLE[k] = rigid_oracle(x0, starts, lens, target, var, **kw)
    return _ORACLE[k]


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

def test_oracle_gradient_matches_central_differences_and_the_detached_rotation():
    segs = _segments()
    lens = [len(s) for s in segs]
    starts = _all_starts(20, lens)
    assert starts.shape == (36, 2)
    x0, tgt, var = _walk(2, 20, 3), _target(), 0.5
    ref = rigid_oracle(x0, starts, lens, tgt, var)
    det = rigid_oracle(x0, starts, lens, tgt, var, detach_rotation=True)
    gmax = float(ref['grad'].abs().max())
    d_det = float((ref['grad'] - det['grad']).abs().max())
    print('autograd through the SVD against R detached: %.2e of the largest entry' % (d_det / gmax))
    assert d_det <= 1e-12 * gmax and torch.equal(ref['logp'], det['logp'])
    x, h = x0.double(), 1e-5
    fd = torch.zeros_like(x)
    for i in range(x.numel()):
        e = torch.zeros(x.numel(), dtype=torch.float64)
        e[i] = h
        e = e.reshape(x.shape)
        fd.view(-1)[i] = (logp_only(x + e, starts, lens, tgt, var) - logp_only(x - e, starts, lens, tgt, var)) / (2 * h)
    d_fd = float((ref['grad'] - fd).abs().max())
    print('oracle gradient against central differences: %.2e of the largest entry' % (d_fd / gmax))
    assert d_fd <= 1e-6 * gmax


def test_rigid_entry_rejects_impossible_shapes():
    """The C entry validates its shape before it touches the device (so this runs without one), and says how much work it needs."""
    from genie2_amd import build, capi
    build.build()
    lib = capi.load_library()
    assert lib.genie_motif_potential_rigid_work_bytes(8, 1000) == 0
    assert lib.genie_motif_potential_rigid_work_bytes(8, 20000) >= 8 * 20000 * 32
    need = lib.genie_motif_potential_rigid_work_bytes(2, 20000)
    d = C.c_void_p(64)                                           # never dereferenced: every call below fails its shape check

    def call(B=2, N=60, P=10, S=2, M=13, x0=d, logp=d, grad=d, best=d, rmsd=d, work=None, work_bytes=0):
        return lib.genie_motif_potential_rigid(None, B, N, x0, P, S, M, d, d, d, d, logp, grad, best, rmsd, work, work_bytes)

    assert call(M=2) == -1 and call(M=2, S=1) == -1 and call(M=0) == -1
    assert call(P=0) == -1 and call(S=0) == -1 and call(B=0) == -1 and call(N=0) == -1
    assert call(M=61) == -1 and call(S=14) == -1
    assert call(P=20000) == -1                                   # large P needs work
    assert call(P=20000, work=d, work_bytes=need - 1) == -1
    assert call(grad=d, logp=None) == -1 and call(logp=d, grad=None) == -1
    assert call(logp=None, grad=None, best=None, rmsd=None) == -1
    assert call(x0=None) == -1


def test_motif_cli_parser_has_the_alignment_and_location_flags():
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    base = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o', '--motif_file', MOTIF]
    a = build_parser().parse_args(base)
    assert a.align == 'translation' and a.write_motif_locations is False
    c = MotifRunner().create_constants(vars(a))
    assert c['align'] == 'translation' and c['write_motif_locations'] is False
    a = build_parser().parse_args(base + ['--align', 'rigid', '--write_motif_locations'])
    assert a.align == 'rigid' and a.write_motif_locations is True
    c = MotifRunner().create_constants(vars(a))
    assert c['align'] == 'rigid' and c['write_motif_locations'] is True
    assert build_parser().parse_args(base + ['--align', 'translation']).align == 'translation'
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ['--align', 'sideways'])


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _check_fit(fit, ref, what, need_gap=True):
    gap = top_two_gap(ref['score']) if ref['score'].shape[1] > 1 else torch.ones(ref['score'].shape[0])
    best, rmsd = fit['best'].cpu().long(), fit['rmsd'].double().cpu()
    print(what, 'top-two gap', gap.tolist(), 'best', best.tolist(), ref['best'].tolist(), 'rmsd', rmsd.tolist(), ref['rmsd'].tolist())
    if need_gap:
        assert bool((gap > 1e-4).all()), (what, gap)                 # the argmax is the oracle's to decide
        assert torch.equal(best, ref['best']), (what, best, ref['best'])
    assert bool(((rmsd - ref['rmsd']).abs() <= 1e-5 * ref['rmsd'] + 1e-4).all()), (what, rmsd, ref['rmsd'])


@pytest.mark.gpu
def test_rigid_potential_matches_the_float64_oracle_small_shapes():
    abar = _abar()
    segs = _segments()
    lens = [len(s) for s in segs]
    var = _var500(abar)

    # one placement of one segment
    one = [torch.randn(5, 3, generator=torch.Generator().manual_seed(1)) * 4]
    pot = _pot(one, 5, abar, align='rigid')
    assert pot.P == 1 and pot.S == 1
    x0 = _walk(2, 5, 2)
    ref = _oracle('one', x0, pot.starts.cpu(), pot.seg_len, pot.target, var)
    _check(*_run(pot, x0), ref, 'one placement')
    _check_fit(pot.locate(x0.cuda()), ref, 'one placement')

    pot = _pot(segs, 20, abar, align='rigid')
    assert pot.P == 36
    x0 = _walk(2, 20, 3)
    ref = _oracle('n20', x0, pot.starts.cpu(), lens, pot.target, var)
    _check(*_run(pot, x0), ref, 'N=20')
    _check_fit(pot.locate(x0.cuda()), ref, 'N=20')


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 3])
def test_rigid_potential_matches_the_float64_oracle_every_placement_of_n60(B):
    abar = _abar()
    segs = _segments()
    lens = [len(s) for s in segs]
    pot = _pot(segs, 60, abar, align='rigid')
    assert pot.P == 1176
    x0 = _walk(B, 60, 10 + B)
    # var of schedule step 500, then one / a few / all placements carrying weight
    for v in (None, 1e-4, 1.0, 30.0, 1e4):
        pot = _pot(segs, 60, abar, align='rigid')
        var = _var500(abar) if v is None else _fix_var(pot, v)
        ref = _oracle('n60b%d' % B, x0, pot.starts.cpu(), lens, pot.target, var)
        w = torch.softmax(ref['score'], dim=1)
        print('var %g: placements with weight > 1e-3: %s' % (var, (w > 1e-3).sum(dim=1).tolist()))
        _check(*_run(pot, x0), ref, 'N=60 B=%d var=%g' % (B, var))
    _check_fit(pot.locate(x0.cuda()), ref, 'N=60 B=%d' % B)


@pytest.mark.gpu
def test_rigid_potential_matches_the_float64_oracle_n256():
    abar = _abar()
    segs = _segments()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    pot = _pot(segs, 256, abar, P=1000, seed=21, align='rigid')
    assert pot.P == 1000 and pot.lib.genie_motif_potential_rigid_work_bytes(8, 1000) == 0
    x0 = _walk(8, 256, 21)
    ref = _oracle('n256', x0, pot.starts.cpu(), lens, pot.target, var)
    _check(*_run(pot, x0), ref, 'N=256 B=8 P=1000')
    _check_fit(pot.locate(x0.cuda()), ref, 'N=256 B=8 P=1000')


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['cap', 'cap+1', '20000'])
def test_rigid_potential_matches_the_float64_oracle_around_the_lds_cap(which):
    from genie2_amd import capi
    abar = _abar()
    segs = _segments()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    cap = _lds_cap(lambda P: capi.load_library().genie_motif_potential_rigid_work_bytes(2, P))
    P = {'cap': cap, 'cap+1': cap + 1, '20000': 20000}[which]
    pot = _pot(segs, 256, abar, P=P, seed=22, align='rigid')
    assert pot.P == P and (pot.lib.genie_motif_potential_rigid_work_bytes(2, P) > 0) == (which != 'cap')
    x0 = _walk(2, 256, 23)
    ref = _oracle('cap' + which, x0, pot.starts.cpu(), lens, pot.target, var)
    _check(*_run(pot, x0), ref, 'N=256 B=2 P=%d' % P)
    _check_fit(pot.locate(x0.cuda()), ref, 'N=256 B=2 P=%d' % P)


def _entry(pot, x, var, want_potential=True, want_fit=True):
    """The C entry itself with every output, or with one pair NULL."""
    B = x.shape[0]
    need = pot.lib.genie_motif_potential_rigid_work_bytes(B, pot.P)
    work = torch.empty(max(need, 16), dtype=torch.uint8, device='cuda')
    v = torch.tensor([var], dtype=torch.float32, device='cuda')
    logp, grad = torch.full((B,), 7.0, device='cuda'), torch.full_like(x, 7.0)
    best, rmsd = torch.full((B,), -7, dtype=torch.int32, device='cuda'), torch.full((B,), 7.0, device='cuda')
    p = lambda t, on=True: C.c_void_p(t.data_ptr()) if on else None      # noqa: E731
    rc = pot.lib.genie_motif_potential_rigid(C.c_void_p(torch.cuda.current_stream().cuda_stream), B, pot.n_res, p(x), pot.P, pot.S, pot.M,
                                             p(pot.seg_len_t), p(pot.starts), p(pot.target), p(v), p(logp, want_potential),
                                             p(grad, want_potential), p(best, want_fit), p(rmsd, want_fit), p(work, need > 0),
                                             work.numel())
    torch.cuda.synchronize()
    assert rc == 0
    return logp, grad, best, rmsd


@pytest.mark.gpu
@pytest.mark.parametrize('P', [1000, 20000])
def test_rigid_entry_outputs_best_and_rmsd_and_null_pairs_leave_the_rest_alone(P):
    abar = _abar()
    segs = _segments()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    pot = _pot(segs, 256, abar, P=P, seed=31, align='rigid')
    x0 = _walk(3, 256, 32)
    x = x0.cuda().contiguous()
    ref = _oracle('entry%d' % P, x0, pot.starts.cpu(), lens, pot.target, var)
    logp, grad, best, rmsd = _entry(pot, x, var)
    _check(logp, grad, ref, 'entry P=%d' % P)
    _check_fit({'best': best, 'rmsd': rmsd}, ref, 'entry P=%d' % P)
    lp2, g2, b2, r2 = _entry(pot, x, var, want_fit=False)
    assert torch.equal(lp2, logp) and torch.equal(g2, grad) and bool((b2 == -7).all()) and bool((r2 == 7.0).all())
    lp3, g3, b3, r3 = _entry(pot, x, var, want_potential=False)
    assert torch.equal(b3, best) and torch.equal(r3, rmsd) and bool((lp3 == 7.0).all()) and bool((g3 == 7.0).all())
    # locate() is this entry with var = 1, and the potential's forward / backward are its first pair
    fit = pot.locate(x)
    assert torch.equal(fit['best'], best.long()) and torch.equal(fit['starts'], pot.starts[best.long()].long())
    assert torch.equal(fit['ends'], fit['starts'] + torch.tensor(lens, device='cuda')[None] - 1)
    lp4, g4 = _run(pot, x0)
    assert torch.equal(lp4, logp) and torch.equal(g4, grad)


def _plant(x0, starts_row, lens, motif, seed, mirror=False):
    """A randomly rotated and translated copy of the centred motif (its mirror image: z negated first) plus N(0, 0.1^2) noise, written
    into particle 0 at one placement."""
    g = torch.Generator().manual_seed(seed)
    m = motif.double().clone()
    if mirror:
        m[:, 2] = -m[:, 2]
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    pos = (m @ q.T + 10.0 * torch.randn(1, 3, generator=g, dtype=torch.float64)
           + 0.1 * torch.randn(m.shape, generator=g, dtype=torch.float64)).float()
    x = x0.clone()
    at = 0
    for st, n in zip(starts_row, lens):
        x[0, st:st + n] = pos[at:at + n]
        at += n
    return x


@pytest.mark.gpu
def test_planted_fit_is_found_and_its_mirror_image_is_not():
    abar = _abar()
    segs = _segments()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    pot = _pot(segs, 60, abar, align='rigid')
    assert pot.P == 1176
    row = pot.starts[700].tolist()
    tc = pot.target.cpu()

    x0 = _plant(_walk(2, 60, 41), row, lens, tc, 42)
    ref = _oracle('planted', x0, pot.starts.cpu(), lens, tc, var)
    assert int(ref['best'][0]) == 700 and 0.1 < float(ref['rmsd'][0]) < 0.3
    _check(*_run(pot, x0), ref, 'planted fit', grad_floor=float(tc.abs().max()) / var)
    fit = pot.locate(x0.cuda())
    _check_fit(fit, ref, 'planted fit')
    assert int(fit['best'][0]) == 700

    # the mirror image: a proper rotation cannot fit it, an improper one would reach the noise level
    xm = _plant(_walk(2, 60, 41), row, lens, tc, 42, mirror=True)
    refm = _oracle('mirror', xm, pot.starts.cpu(), lens, tc, var)
    q700 = float(refm['q'][0, 700])
    assert np.sqrt(q700 / 13) > 3.0
    _check_fit(pot.locate(xm.cuda()), refm, 'mirror image, every placement')
    pot.starts, pot.P = pot.starts[700:701].contiguous(), 1               # that placement alone: rmsd reports its q
    r = float(pot.locate(xm.cuda())['rmsd'][0])
    print('mirror image at the planted placement: rmsd %.4f, oracle %.4f' % (r, np.sqrt(q700 / 13)))
    assert abs(r - np.sqrt(q700 / 13)) <= 1e-5 * np.sqrt(q700 / 13) + 1e-4


@pytest.mark.gpu
def test_collinear_coordinates_give_finite_outputs_and_the_right_logp():
    abar = _abar()
    segs = _segments()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    pot = _pot(segs, 60, abar, align='rigid')
    along = torch.tensor([[1.0, 2.0, -0.5], [0.0, 0.0, 3.8]])
    x0 = torch.arange(60.0)[None, :, None] * along[:, None, :] + torch.tensor([4.0, -3.0, 9.0])
    ref = _oracle('line', x0, pot.starts.cpu(), lens, pot.target, var, want_grad=False)
    lp, g = _run(pot, x0)
    fit = pot.locate(x0.cuda())
    assert all(bool(torch.isfinite(t).all()) for t in (lp, g, fit['rmsd']))
    assert bool(((fit['best'] >= 0) & (fit['best'] < pot.P)).all())
    tol = 1e-5 * ref['logp'].abs().clamp(min=1.0)
    print('collinear: logp', lp.tolist(), ref['logp'].tolist())
    assert bool(((lp.double().cpu() - ref['logp']).abs() <= tol).all())
    # every point the same: the correlation is zero
    lp, g = _run(pot, torch.full((1, 60, 3), 2.5))
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all())


@pytest.mark.gpu
def test_rigid_gradient_is_zero_where_no_placement_reaches():
    # the max_offsets=1 case of tests/test_motif_potential.py, with a motif that is not collinear (the rigid form refuses one that is)
    abar = _abar()
    pot = _pot([torch.tensor([[0.0, 0.0, 0.0], [3.8, 0.0, 0.0], [5.0, 3.6, 0.0]])], 10, abar, P=1, seed=0, align='rigid')
    assert pot.P == 1
    st = int(pot.starts[0, 0])
    lp, g = _run(pot, _walk(2, 10, 3), 400)
    outside = torch.ones(10, dtype=torch.bool)
    outside[st:st + 3] = False
    assert bool((g[:, outside] == 0).all()) and bool((g[:, ~outside] != 0).any())


@pytest.mark.gpu
@pytest.mark.parametrize('P', [1000, 20000])
def test_rigid_potential_is_deterministic_and_never_synchronises(P):
    abar = _abar()
    pot = _pot(_segments(), 256, abar, P=P, seed=P, align='rigid')
    x0 = _walk(8, 256, 7).cuda()
    a = _run(pot, x0, 400)
    b = _run(pot, x0, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), P
    x = x0.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(x, 400)
        g, = torch.autograd.grad(lp.mean(), x)
        fit = pot.locate(x0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.equal(g, a[1] * 0.125)          # (the backward scales by grad_output = 1/8)
    assert bool((fit['rmsd'] > 0).all())


@pytest.mark.gpu
def test_align_translation_is_todays_potential_and_rigid_validates_its_motif():
    from genie2_amd.smc import MotifPotential
    abar = _abar()
    segs = _segments()
    x0 = _walk(3, 60, 51)
    np.random.seed(5)
    a = _run(MotifPotential(segs, 60, abar, device='cuda'), x0)
    np.random.seed(5)
    pot = MotifPotential(segs, 60, abar, device='cuda', align='translation')
    b = _run(pot, x0)
    assert pot.align == 'translation' and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        MotifPotential(segs, 60, abar, device='cuda', align='sideways')
    with pytest.raises(ValueError):
        MotifPotential([torch.tensor([[0.0, 0.0, 0.0], [3.8, 0.0, 0.0]])], 10, abar, device='cuda', align='rigid')
    with pytest.raises(ValueError):
        MotifPotential([torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]]), torch.tensor([[3.0, 6.0, 9.0]])], 10, abar, device='cuda',
                       align='rigid')
    # the same motifs are fine for today's potential
    MotifPotential([torch.tensor([[0.0, 0.0, 0.0], [3.8, 0.0, 0.0]])], 10, abar, device='cuda')


@pytest.mark.gpu
def test_rigid_guidance_pulls_the_motif_in_and_the_sampler_reports_where(tmp_path, base_weights):
    from genie2_amd import pack
    from genie2_amd.smc import TwistedSampler
    B, N, T = 4, 40, 12
    model = _tiny_model(base_weights, T)
    segs = _segments()
    lens = [len(s) for s in segs]
    abar = pack.schedule_tensors(T)['alphas_cumprod'].cuda()
    noise = torch.randn(T, B, N, 3, generator=torch.Generator().manual_seed(4))
    base = {'length': N, 'scale': 0.6, 'num_samples': B, 'outdir': str(tmp_path), 'prefix': 'x', 'offset': 0, 'noise': noise,
            'last_unguided_steps': 0, 'guidance_alpha': 0.05, 'ess_threshold': 0.0}
    tw = TwistedSampler(model)
    pot = _pot(segs, N, abar, tausq=0.5, align='rigid')
    assert pot.P == 406

    out = tw._sample(dict(base, twisting_function=pot))
    xyz = torch.from_numpy(np.stack([r['atom_positions'] for r in out]))
    fit = tw.last_fit
    assert bool(torch.isfinite(xyz).all()) and tw.resampled_at == []
    assert all(not t.is_cuda for t in fit.values()) and fit['best'].shape == (B,) and fit['starts'].shape == (B, 2)
    ref = rigid_oracle(xyz, pot.starts.cpu(), lens, pot.target, 1.0, want_grad=False)
    _check_fit(fit, ref, 'last_fit')
    assert torch.equal(fit['starts'], pot.starts.cpu()[fit['best']].long())
    assert torch.equal(fit['ends'], fit['starts'] + torch.tensor(lens)[None] - 1)

    # the same noise without guidance: a potential that does not depend on x0 (and has no locate)
    free = tw._sample(dict(base, twisting_function=lambda x0, step: (x0 * 0).sum(dim=(1, 2))))
    assert tw.last_fit is None
    xyz_free = torch.from_numpy(np.stack([r['atom_positions'] for r in free]))
    rmsd_free = pot.locate(xyz_free.cuda())['rmsd'].cpu()
    print('superposed motif RMSD: guided %s (mean %.3f), unguided %s (mean %.3f)'
          % (fit['rmsd'].tolist(), float(fit['rmsd'].mean()), rmsd_free.tolist(), float(rmsd_free.mean())))
    assert float(fit['rmsd'].mean()) <= 0.5 * float(rmsd_free.mean())


@pytest.mark.gpu
def test_motif_cli_writes_one_location_file_per_sample(tmp_path, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    root = str(tmp_path / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    out = str(tmp_path / 'out')
    common = ['--name', 'base', '--epoch', '7', '--rootdir', root, '--scale', '0.6', '--motif_file', MOTIF, '--last_unguided_steps', '0']
    args = build_parser().parse_args(common + ['--outdir', out, '--min_length', '40', '--max_length', '56', '--length_step', '16',
                                               '--batch_size', '3', '--num_samples', '4', '--align', 'rigid', '--write_motif_locations'])
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    names = sorted('{}_{}'.format(n, i) for n in (56, 40) for i in range(4))
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == [n + '.pdb' for n in names]
    assert sorted(os.listdir(os.path.join(out, 'motif_locations'))) == [n + '.txt' for n in names]
    assert sorted(os.listdir(out)) == ['motif_locations', 'pdbs']
    segs = _segments()
    lens = [len(s) for s in segs]
    for name in names:
        n = int(name.split('_')[0])
        lines = open(os.path.join(out, 'motif_locations', name + '.txt')).read().splitlines()
        assert len(lines) == 3 and lines[2].startswith('# rmsd '), (name, lines)
        spans = [tuple(int(v) for v in line.split('\t')) for line in lines[:2]]
        assert [e - s + 1 for s, e in spans] == lens and spans[0][0] >= 0 and spans[0][1] < spans[1][0] and spans[1][1] <= n - 1, spans
        assert len(lines[2].split()[2].split('.')[1]) == 3
        xyz = _ca_coordinates(os.path.join(out, 'pdbs', name + '.pdb'))
        assert xyz.shape == (n, 3) and np.isfinite(xyz).all()
        want = fit_rmsd(xyz, [s for s, _ in spans], lens, torch.cat(segs))
        print(name, spans, lines[2], 'oracle on the PDB: %.4f' % want)
        assert abs(float(lines[2].split()[2]) - want) <= 2e-3, (name, lines[2], want)

    # without the flag nothing new is written
    out2 = str(tmp_path / 'out2')
    args = build_parser().parse_args(common + ['--outdir', out2, '--min_length', '40', '--max_length', '40', '--batch_size', '2',
                                               '--num_samples', '2', '--align', 'rigid'])
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    assert sorted(os.listdir(out2)) == ['pdbs'] and sorted(os.listdir(os.path.join(out2, 'pdbs'))) == ['40_0.pdb', '40_1.pdb']
