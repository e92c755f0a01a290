"""Independent particle systems on the GPU: genie_smc_reweight against the float64 oracle of tests/_smc_particles.py, and
TwistedSampler's params['num_particles'] against today's one-system sampler, against itself run one system at a time, and through
the CLI.

Measured on an MI355X against float64 (the bar is twice what smc.py's float32 torch lines make on the same inputs, on the GPU):
    case (S, K, N, sigma)   max |log w|   log_w_acc error: entry / torch float32   ESS error: entry / torch float32
    (1, 1, 2, 0.2)           0.1          0 / 0                                     0 / 0
    (1, 2, 2, 0.2)           0.4          1.1e-8 / 1.9e-8                           3.8e-8 / 8.2e-8
    (3, 5, 40, 0.2)          6.8          1.8e-8 / 4.9e-6                           1.7e-7 / 5.6e-6
    (2, 64, 40, 0.2)        12.8          5.1e-8 / 9.3e-6                           3.7e-7 / 1.5e-5
    (4, 8, 257, 0.02)       41.6          1.8e-8 / 3.8e-4                           1.5e-7 / 5.9e-4
The entry's own error is the rounding of its float64 result to the float32 it stores."""
import os

import numpy as np
import pytest
import torch

import _smc_particles as P
from _motif import MOTIF, _ca_coordinates, _pot, _tiny_model, segments_6e6r

pytestmark = pytest.mark.gpu


def _call(S, K, N, inp, ess_fraction=P.ESS_FRACTION):
    """One genie_smc_reweight call on the case's inputs: dict of its outputs on the CPU."""
    from genie2_amd.smc import SmcReweight
    d = {k: v.cuda() for k, v in inp.items()}
    rw = SmcReweight(S, K, N, 'cuda')
    x_out, index = rw(d['x_new'], d['mean_tw'], d['mean_un'], d['sigma'], d['log_prob'], d['u'], ess_fraction, d['log_proposal'],
                      d['log_w_acc'])
    return dict(x_out=x_out.cpu(), index=index.cpu().long(), ess=rw.ess.cpu(), resampled=rw.resampled.cpu(),
                log_proposal=d['log_proposal'].cpu(), log_w_acc=d['log_w_acc'].cpu())


@pytest.mark.parametrize('S,K,N,sigma,seed', P.CASES)
def test_reweight_matches_the_float64_oracle(S, K, N, sigma, seed):
    inp = P.make_inputs(S, K, N, sigma, seed)
    ref = P.oracle(S, K, inp)
    ess_margin, point_margin = P.margins(S, K, ref)
    assert ess_margin >= 0.05 and point_margin >= 1e-3, (ess_margin, point_margin)       # the discrete outputs are unambiguous
    got = _call(S, K, N, inp)
    again = _call(S, K, N, inp)
    assert all(torch.equal(got[k], again[k]) for k in got)                                # bitwise reproducible
    assert torch.equal(got['index'], ref['index']) and torch.equal(got['resampled'].bool(), ref['resampled'])
    assert torch.equal(got['x_out'].view(torch.int32), inp['x_new'][got['index']].view(torch.int32))
    assert torch.equal(got['log_proposal'].view(torch.int32), inp['log_prob'][got['index']].view(torch.int32))
    stays = (~ref['resampled']).repeat_interleave(K)
    assert bool((got['log_w_acc'][~stays] == 0).all())
    # accuracy: at most twice the error of smc.py's own float32 lines, run on the GPU one system at a time on the same inputs
    torch_ess, torch_acc = zip(*(P.torch_float32_lines(K, inp, s, 'cuda') for s in range(S)))
    torch_ess, torch_acc = torch.stack(torch_ess), torch.cat(torch_acc)
    err = lambda a, b, sel: float((a.double() - b)[sel].abs().max()) if bool(sel.any()) else 0.0      # noqa: E731
    every = torch.ones(S, dtype=torch.bool)
    e_acc, bar_acc = err(got['log_w_acc'], ref['log_w_acc'], stays), err(torch_acc, ref['log_w_acc'], stays)
    e_ess, bar_ess = err(got['ess'], ref['ess'], every), err(torch_ess, ref['ess'], every)
    print('case %s max|log w| %.1f: log_w_acc error %.3e (torch float32 %.3e), ESS error %.3e (torch float32 %.3e)'
          % ((S, K, N, sigma), float(ref['log_w'].abs().max()), e_acc, bar_acc, e_ess, bar_ess))
    assert e_acc <= 2 * bar_acc and e_ess <= 2 * bar_ess


def test_reweight_edge_values():
    """A particle of weight exactly 0 is no one's ancestor; a system of NaN stays in place and does not disturb its neighbour."""
    S, K, N = 2, 4, 2
    inp = P.make_inputs(S, K, N, 0.2, 0)
    inp['log_prob'][K + 2] = float('-inf')
    ref = P.oracle(S, K, inp, 0.99)
    assert bool(ref['resampled'][1])                                                       # system 1 resamples
    got = _call(S, K, N, inp, 0.99)
    assert int(got['resampled'][1]) == 1 and K + 2 not in got['index'].tolist()
    assert torch.equal(got['index'], ref['index']) and bool(torch.isfinite(got['log_proposal'][K:]).all())
    bad = {k: v.clone() for k, v in inp.items()}
    bad['log_prob'][:K] = float('nan')
    nan = _call(S, K, N, bad, 0.99)
    assert nan['index'][:K].tolist() == list(range(K)) and int(nan['resampled'][0]) == 0
    assert torch.equal(nan['x_out'][:K], inp['x_new'][:K])
    for k in ('x_out', 'index', 'log_proposal', 'log_w_acc'):
        assert torch.equal(nan[k][K:], got[k][K:]), k
    assert int(nan['resampled'][1]) == 1 and torch.equal(nan['ess'][1], got['ess'][1])


def test_reweight_refusals_leave_the_entry_usable():
    from genie2_amd import capi
    lib = capi.load_library()
    S, K, N = 2, 4, 2
    inp = P.make_inputs(S, K, N, 0.2, 0)
    d = {k: v.cuda() for k, v in inp.items()}
    d.update(x_out=torch.zeros_like(d['x_new']), index_out=torch.zeros(S * K, dtype=torch.int32, device='cuda'),
             ess_out=torch.zeros(S, device='cuda'), resampled_out=torch.zeros(S, dtype=torch.int32, device='cuda'))
    keep = {k: v.clone() for k, v in d.items()}
    ptrs = {k: v.data_ptr() for k, v in d.items()}
    need = lib.genie_smc_reweight_work_bytes(S, K, N)
    work = torch.zeros(need + 65 * 8, dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    for kw in (dict(ptrs=dict(ptrs, x_out=ptrs['x_new'])), dict(K=65), dict(work_bytes=need - 1)):
        args = dict(S=S, K=K, N=N, ptrs=ptrs, work=work.data_ptr(), work_bytes=need, stream=stream)
        args.update(kw)
        assert P.raw_call(lib, **args) == -1 and b'genie_smc_reweight' in lib.genie_last_error(None), kw
    torch.cuda.synchronize()
    assert all(torch.equal(d[k], keep[k]) for k in d)                                     # nothing was launched
    got = _call(S, K, N, inp)
    assert torch.equal(got['index'], P.oracle(S, K, inp)['index'])


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N = 12, 40


@pytest.fixture(scope='module')
def ctx(base_weights):
    from genie2_amd import pack
    from genie2_amd.smc import TwistedSampler
    model = _tiny_model(base_weights, T)
    abar = pack.schedule_tensors(T)['alphas_cumprod'].cuda()
    sampler, pot = TwistedSampler(model), _pot(segments_6e6r(), N, abar)
    cache = {}

    def run(noise, outdir, **extra):
        """(coordinates [B, N, 3], resampled_at, ess_trace, sampler attributes) of one _sample call."""
        out = sampler._sample(dict({'length': N, 'scale': 0.6, 'outdir': str(outdir), 'prefix': 'x', 'offset': 0, 'noise': noise,
                                    'last_unguided_steps': 0, 'guidance_alpha': 0.05, 'twisting_function': pot}, **extra))
        attrs = {k: getattr(sampler, k, None) for k in ('last_log_weights', 'last_choice', 'last_fit')}
        return np.stack([r['atom_positions'] for r in out]), sampler.resampled_at, sampler.ess_trace, attrs

    return dict(run=run, cache=cache)


def _noise(steps, B, seed):
    return torch.randn(steps, B, N, 3, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('num_steps', [None, 5])
def test_one_system_is_todays_sampler(ctx, tmp_path, num_steps):
    run, K = ctx['run'], 4
    steps = T if num_steps is None else num_steps
    noise, more = _noise(steps, K, 4), ({} if num_steps is None else {'num_steps': num_steps})
    a, ra, _, _ = run(noise, tmp_path, num_samples=K, ess_threshold=0.0, **more)
    b, rb, ess, _ = run(noise, tmp_path, num_samples=1, num_particles=K, ess_threshold=0.0, **more)
    rms, d = float(np.sqrt((a ** 2).mean())), float(np.abs(a - b).max())
    print('num_steps %s, no resampling: max |d| = %.3e, coordinate RMS = %.2f' % (num_steps, d, rms))
    assert np.isfinite(b).all() and ra == [] and rb == [[]] and d <= 1e-3 * rms
    assert tuple(ess.shape) == (steps - 1, 1) and ess.device.type == 'cpu'
    u = [0.37] * T
    a, ra, ess_a, _ = run(noise, tmp_path, num_samples=K, ess_threshold=0.5, resample_u=u, **more)
    gap = min(abs(e - 0.5 * K) / (0.5 * K) for e in ess_a)
    assert gap >= 1e-3, 'the ESS of today\'s run comes within %.1e of the threshold: take another noise seed' % gap
    b, rb, ess_b, _ = run(noise, tmp_path, num_samples=1, num_particles=K, ess_threshold=0.5, resample_u=u, **more)
    print('num_steps %s: resampled at' % num_steps, ra, rb, 'ESS', ess_a, ess_b[:, 0].tolist())
    assert rb[0] == ra and len(ra) > 0 and np.isfinite(b).all()


def _three_systems(ctx, tmp_path):
    if 'three' not in ctx['cache']:
        S, K = 3, 4
        noise = _noise(T, S * K, 11)
        us = [[0.05, 0.11, 0.21]] * T
        ctx['cache']['three'] = (noise, us, ctx['run'](noise, tmp_path, num_samples=S, num_particles=K, ess_threshold=0.5, resample_u=us))
    return ctx['cache']['three']


def test_systems_are_independent(ctx, tmp_path):
    K = 4
    noise, us, (x, resampled_at, ess, attrs) = _three_systems(ctx, tmp_path)
    assert tuple(ess.shape) == (T - 1, 3) and len(resampled_at) == 3 and tuple(attrs['last_log_weights'].shape) == (3, K)
    solo, solo_at, solo_ess, _ = ctx['run'](noise[:, K:2 * K], tmp_path, num_samples=1, num_particles=K, ess_threshold=0.5,
                                            resample_u=[row[1] for row in us])
    rms, d = float(np.sqrt((solo ** 2).mean())), float(np.abs(x[K:2 * K] - solo).max())
    print('system 1 in a batch of 3 against alone: max |d| = %.3e, coordinate RMS = %.2f; resampled at' % (d, rms), resampled_at, solo_at)
    assert solo_at[0] == resampled_at[1] and d <= 1e-3 * rms
    assert any(len(r) > 0 for r in resampled_at)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert resampled_at[i] != resampled_at[j] or float(np.abs(x[i * K:(i + 1) * K] - x[j * K:(j + 1) * K]).max()) > 1e-3 * rms


def test_best_particle_of_every_system(ctx, tmp_path):
    S, K = 3, 4
    noise, us, (x, _, _, _) = _three_systems(ctx, tmp_path)
    best, _, _, attrs = ctx['run'](noise, tmp_path, num_samples=S, num_particles=K, ess_threshold=0.5, resample_u=us,
                                   return_particles='best')
    choice, lw = attrs['last_choice'], attrs['last_log_weights']
    assert tuple(best.shape) == (S, N, 3) and tuple(choice.shape) == (S,) and tuple(lw.shape) == (S, K)
    assert choice.tolist() == [int(np.flatnonzero(row == row.max())[0]) for row in lw.numpy()]
    rms = float(np.sqrt((x ** 2).mean()))
    for s in range(S):
        assert float(np.abs(best[s] - x[s * K + int(choice[s])]).max()) <= 1e-3 * rms, s
    assert tuple(attrs['last_fit']['rmsd'].shape) == (S,) and tuple(attrs['last_fit']['starts'].shape)[0] == S


def test_cli_writes_one_design_per_system(tmp_path, base_weights):
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
                                      '--motif_file', MOTIF, '--min_length', '40', '--max_length', '40', '--batch_size', '2',
                                      '--num_samples', '3', '--num_particles', '3', '--last_unguided_steps', '0',
                                      '--write_motif_locations'])
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == ['40_%d.pdb' % i for i in range(3)]
    assert sorted(os.listdir(os.path.join(out, 'motif_locations'))) == ['40_%d.txt' % i for i in range(3)]
    for i in range(3):
        xyz = _ca_coordinates(os.path.join(out, 'pdbs', '40_%d.pdb' % i))
        assert xyz.shape == (40, 3) and np.isfinite(xyz).all(), i
