"""Motif-guided SMC sampling: the fused motif placement potential (genie_motif_potential, csrc/smc_kernels.hip; MotifPotential in
genie2_amd/smc.py) against the PyTorch restatement of unconditional_smc.py:303-345 (motif_twisting_function) with torch autograd in
float64, its placement encoding against the mask layout, TwistedSampler with either potential, and the motif sampling CLI
(the fork's genie/sample_unconditional_motif.py).

Bounds of the fused potential: logp within 1e-5 max(1, |logp|); gradient within 1e-5 of the particle's largest gradient entry."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _motif import _abar, _tiny_model, segments_6e6r as _segments, walk as _walk
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')


def _masks_from_starts(starts, seg_len, n_res):
    m = torch.zeros(starts.shape[0], n_res, dtype=torch.bool)
    for p, row in enumerate(starts.tolist()):
        for st, n in zip(row, seg_len):
            m[p, st:st + n] = True
    return m


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

def test_placement_starts_describe_the_placement_masks():
    from genie2_amd.smc import generate_motif_index_mask, get_all_motif_locations, placement_masks, placement_starts
    st = placement_starts(get_all_motif_locations(5, [2, 1]))
    assert st.dtype == torch.int32 and st.tolist() == [[0, 2], [0, 3], [0, 4], [1, 3], [1, 4], [2, 4]]
    assert placement_starts(get_all_motif_locations(4, [4])).tolist() == [[0]]
    assert placement_starts([]).shape == (0, 0)
    segs = _segments()
    lens = [len(s) for s in segs]
    for n_res, max_offsets, count in ((60, 10 ** 6, 1176), (60, 1000, 1000), (256, 10 ** 6, 29890), (256, 1000, 1000)):
        np.random.seed(11)
        starts = placement_starts(get_all_motif_locations(n_res, lens, max_offsets))
        after_starts = np.random.rand()
        np.random.seed(11)
        masks = placement_masks(generate_motif_index_mask(segs, n_res, max_offsets))
        after_masks = np.random.rand()
        assert starts.shape == (count, 2), (n_res, max_offsets)
        assert torch.equal(_masks_from_starts(starts, lens, n_res), masks), (n_res, max_offsets)
        assert after_starts == after_masks                       # one choice() draw each, or none
    # a thinned draw keeps the reference's (unsorted) order of the choice() result
    np.random.seed(3)
    few = placement_starts(get_all_motif_locations(256, lens, 1000))
    assert not bool((few[1:, 0] >= few[:-1, 0]).all())


def test_motif_potential_entry_rejects_impossible_shapes():
    """The C entry validates its shape before it touches the device (so this runs without one), and says how much work it needs."""
    from genie2_amd import build, capi
    build.build()
    lib = capi.load_library()
    assert lib.genie_motif_potential_work_bytes(8, 1000) == 0
    assert lib.genie_motif_potential_work_bytes(8, 20000) == 8 * 20000 * 16
    assert lib.genie_motif_potential_work_bytes(64, 32768) == 64 * 32768 * 16
    d = C.c_void_p(64)                                           # never dereferenced: every call below fails its shape check

    def call(B=2, N=60, P=10, S=2, M=13, work=None, work_bytes=0):
        return lib.genie_motif_potential(None, B, N, d, P, S, M, d, d, d, d, d, d, work, work_bytes)

    assert call(P=0) == -1 and call(S=0) == -1 and call(M=0) == -1 and call(B=0) == -1 and call(N=0) == -1
    assert call(M=61) == -1 and call(S=14) == -1
    assert call(P=20000) == -1                                   # large P needs work
    assert call(P=20000, work=d, work_bytes=2 * 20000 * 16 - 1) == -1
    assert lib.genie_motif_potential(None, 2, 60, None, 10, 2, 13, d, d, d, d, d, d, None, 0) == -1


def test_motif_cli_parser_segments_and_tasks(capsys):
    from genie2_amd import features as F
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser, load_motif_segments
    a = build_parser().parse_args(['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o', '--motif_file', MOTIF])
    assert (a.num_samples, a.batch_size, a.min_length, a.max_length, a.length_step, a.num_devices) == (5, 4, 50, 256, 1, 1)
    assert a.sequential_order is False and a.resume is False and a.rootdir == 'results'
    assert (a.tausq, a.guidance_alpha, a.ess_threshold, a.last_unguided_steps, a.max_offsets) == (0.012, 0.012, 0.5, 50, 1000)
    a = build_parser().parse_args(['--name', 'b', '--epoch', '1', '--rootdir', 'r', '--scale', '1', '--outdir', 'o', '--num_samples', '3',
                                   '--batch_size', '2', '--min_length', '40', '--max_length', '56', '--length_step', '16',
                                   '--num_devices', '2', '--sequential_order', '--motif_file', MOTIF, '--tausq', '0.5',
                                   '--guidance_alpha', '0.1', '--ess_threshold', '0', '--last_unguided_steps', '3',
                                   '--max_offsets', '20', '--resume'])
    assert (a.num_devices, a.sequential_order, a.tausq, a.ess_threshold, a.max_offsets, a.resume) == (2, True, 0.5, 0.0, 20, True)
    with pytest.raises(SystemExit):
        build_parser().parse_args(['--name', 'b', '--epoch', '1', '--scale', '1', '--outdir', 'o'])       # --motif_file is required
    help_text = ' '.join(build_parser().format_help().split())
    assert help_text.count('(not in the reference CLI)') == 7

    segs = load_motif_segments(MOTIF)
    assert [len(s) for s in segs] == [6, 7]
    _, coords = F.parse_pdb(MOTIF)
    assert np.array_equal(np.array(segs[0] + segs[1]), np.array(coords[0]))

    tasks = MotifRunner().create_tasks(dict(min_length=5, max_length=20, length_step=1, motif_file=MOTIF))
    assert [t['length'] for t in tasks] == list(range(20, 12, -1))
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and '12' in out[0] and '5' in out[0]
    c = MotifRunner().create_constants(vars(a))
    assert c['segments'] == segs and c['max_offsets'] == 20 and c['tausq'] == 0.5 and c['resume'] is True


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _reference(x0, starts, seg_len, target, var):
    """float64 restatement of motif_twisting_function for a given var, vectorised over placements (its equality with
    motif_twisting_function itself is checked below), with the gradient from torch autograd."""
    x = x0.detach().double().cpu().requires_grad_(True)
    idx = torch.cat([starts[:, s:s + 1].long() + torch.arange(n) for s, n in enumerate(seg_len)], dim=1)     # [P, M]
    sel = x[:, idx]                                                                                        # [B, P, M, 3]
    sel = sel - sel.mean(dim=-2, keepdim=True)
    score = -((sel - target.double().cpu()[None, None]) ** 2).sum(dim=(2, 3)) / (2 * var)
    logp = torch.logsumexp(score, dim=1) - np.log(score.shape[1])
    grad, = torch.autograd.grad(logp.sum(), x)
    return logp.detach(), grad


def _check(logp, grad, ref_logp, ref_grad, what):
    lp, g = logp.double().cpu(), grad.double().cpu()
    tol = 1e-5 * ref_logp.abs().clamp(min=1.0)
    assert bool(((lp - ref_logp).abs() <= tol).all()), (what, lp, ref_logp)
    for b in range(g.shape[0]):
        d = float((g[b] - ref_grad[b]).abs().max())
        bound = 1e-5 * float(ref_grad[b].abs().max())
        assert d <= bound, (what, b, d, bound)


def pot_var(abar, step, tausq=0.012):
    from genie2_amd.smc import xstart_variance
    return xstart_variance(abar[step], tausq).to(torch.float32)


def _run(pot, x0, step):
    x = x0.cuda().requires_grad_(True)
    lp = pot(x, step)
    g, = torch.autograd.grad(lp.sum(), x)
    return lp.detach(), g


@pytest.mark.gpu
def test_fused_potential_matches_torch_autograd_in_float64():
    from genie2_amd.smc import MotifPotential, generate_motif_index_mask, motif_twisting_function, placement_masks, xstart_variance
    abar = _abar()
    segs = _segments()
    lens = [len(s) for s in segs]
    step = 500
    var = float(pot_var(abar, step))                 # the f32 value the kernel reads
    var64 = float(xstart_variance(abar[step].double().cpu(), 0.012))

    # one placement of one segment
    g = torch.Generator().manual_seed(1)
    one = [torch.randn(5, 3, generator=g) * 4]
    pot = MotifPotential(one, 5, abar, device='cuda')
    assert pot.P == 1 and pot.S == 1
    x0 = _walk(2, 5, 2)
    _check(*_run(pot, x0, step), *_reference(x0, pot.starts.cpu(), pot.seg_len, pot.target, var), 'one placement')

    # 6E6R at N = 60, every placement; here the vectorised reference is also tied to motif_twisting_function itself
    for B in (1, 3):
        np.random.seed(0)
        pot = MotifPotential(segs, 60, abar, max_offsets=10 ** 6, device='cuda')
        assert pot.P == 1176
        x0 = _walk(B, 60, 10 + B)
        ref_lp, ref_g = _reference(x0, pot.starts.cpu(), lens, pot.target, var)
        tie_lp, tie_g = _reference(x0, pot.starts.cpu(), lens, pot.target, var64)
        np.random.seed(0)
        pm = placement_masks(generate_motif_index_mask(segs, 60, 10 ** 6))
        x = x0.double().requires_grad_(True)
        lp_t = motif_twisting_function(x, pm, pot.target.double().cpu(), abar[step].double().cpu(), 0.012)
        g_t, = torch.autograd.grad(lp_t.sum(), x)
        # (atol: motif_twisting_function takes log P of a float32 tensor)
        assert torch.allclose(lp_t.detach(), tie_lp, rtol=1e-12, atol=1e-6) and torch.allclose(g_t, tie_g, rtol=1e-9, atol=1e-12)
        _check(*_run(pot, x0, step), ref_lp, ref_g, '6E6R N=60 B=%d' % B)

    # N = 256, B = 8, the default 1000 placements; and 20 000, past what LDS holds: the work path
    for P, seed in ((1000, 21), (20000, 22)):
        np.random.seed(seed)
        pot = MotifPotential(segs, 256, abar, max_offsets=P, device='cuda')
        assert pot.P == P
        assert (pot.lib.genie_motif_potential_work_bytes(8, P) > 0) == (P > 2048)
        x0 = _walk(8, 256, seed)
        _check(*_run(pot, x0, step), *_reference(x0, pot.starts.cpu(), lens, pot.target, var), 'N=256 P=%d' % P)

    # a target that is not centred (the mean-residual term of the gradient), and var far from the schedule's range
    np.random.seed(5)
    pot = MotifPotential(segs, 60, abar, device='cuda')
    pot.target = (pot.target + torch.tensor([3.0, -2.0, 5.0], device='cuda')).contiguous()
    x0 = _walk(3, 60, 31)
    _check(*_run(pot, x0, step), *_reference(x0, pot.starts.cpu(), lens, pot.target, var), 'non-centred target')
    for v in (1e-4, 1e4):
        pot.variance = lambda step, v=v: torch.tensor([v], dtype=torch.float32, device='cuda')
        _check(*_run(pot, x0, step), *_reference(x0, pot.starts.cpu(), lens, pot.target, float(np.float32(v))), 'var=%g' % v)


@pytest.mark.gpu
def test_fused_potential_is_deterministic_and_never_synchronises():
    from genie2_amd.smc import MotifPotential
    abar = _abar()
    segs = _segments()
    for P in (1000, 20000):
        np.random.seed(P)
        pot = MotifPotential(segs, 256, abar, max_offsets=P, device='cuda')
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
        finally:
            torch.cuda.set_sync_debug_mode('default')
        assert torch.equal(lp, a[0]) and torch.equal(g, a[1] * 0.125)          # (the backward scales by grad_output = 1/8)
    # residues no placement covers have exactly zero gradient
    pot = MotifPotential([torch.zeros(3, 3) + torch.arange(3.0)[:, None]], 10, abar, max_offsets=1, rng=np.random.RandomState(0),
                         device='cuda')
    st = int(pot.starts[0, 0])
    lp, g = _run(pot, _walk(2, 10, 3), 400)
    outside = torch.ones(10, dtype=torch.bool)
    outside[st:st + 3] = False
    assert bool((g[:, outside] == 0).all()) and bool((g[:, ~outside] != 0).any())


@pytest.mark.gpu
def test_twisted_sampler_with_the_fused_potential_follows_the_torch_path(tmp_path, base_weights):
    from genie2_amd import pack
    from genie2_amd.smc import MotifPotential, TwistedSampler
    B, N, T = 4, 40, 12
    model = _tiny_model(base_weights, T)
    segs = _segments()
    abar = pack.schedule_tensors(T)['alphas_cumprod'].cuda()
    noise = torch.randn(T, B, N, 3, generator=torch.Generator().manual_seed(4))
    base = {'length': N, 'scale': 0.6, 'num_samples': B, 'outdir': str(tmp_path), 'prefix': 'x', 'offset': 0, 'noise': noise,
            'last_unguided_steps': 0, 'guidance_alpha': 0.05}

    def both(extra):
        tw = TwistedSampler(model)
        np.random.seed(7)
        a = tw._sample(dict(base, motif_target=[s.numpy() for s in segs], **extra))
        ra = list(tw.resampled_at)
        np.random.seed(7)
        b = tw._sample(dict(base, twisting_function=MotifPotential(segs, N, abar, device='cuda'), **extra))
        rb = list(tw.resampled_at)
        return np.stack([r['atom_positions'] for r in a]), np.stack([r['atom_positions'] for r in b]), ra, rb

    a, b, ra, rb = both({'ess_threshold': 0.0})
    rms = float(np.sqrt((a ** 2).mean()))
    d = float(np.abs(a - b).max())
    print(f'no resampling: max |d| = {d:.3e}, coordinate RMS = {rms:.2f}')
    assert np.isfinite(b).all() and ra == rb == [] and d <= 1e-3 * rms
    a, b, ra, rb = both({'ess_threshold': 0.5, 'resample_u': [0.37] * T})
    print('resampled at', ra, rb)
    assert ra == rb and len(ra) > 0 and np.isfinite(b).all()


@pytest.mark.gpu
def test_motif_cli_end_to_end(tmp_path, base_weights):
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
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', root, '--scale', '0.6', '--outdir', out,
                                      '--motif_file', MOTIF, '--min_length', '40', '--max_length', '56', '--length_step', '16',
                                      '--batch_size', '3', '--num_samples', '4', '--last_unguided_steps', '0'])
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    files = sorted(os.listdir(os.path.join(out, 'pdbs')))
    assert files == sorted('{}_{}.pdb'.format(n, i) for n in (56, 40) for i in range(4))
    for name in files:
        n = int(name.split('_')[0])
        ca = [line for line in open(os.path.join(out, 'pdbs', name)) if line.startswith('ATOM') and line[13:15].strip() == 'CA']
        assert len(ca) == n, name
        xyz = np.array([[float(line[30:38]), float(line[38:46]), float(line[46:54])] for line in ca])
        assert np.isfinite(xyz).all(), name
