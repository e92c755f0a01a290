"""Few-step sampling on the GPU: the reverse step in coefficient form (genie_reverse_step, mode 2 of k_p_sample_frenet), the strided
loop (genie_sample_loop_steps) and the samplers' `num_steps`, against float64 restatements of the formulas over the oracle's denoiser
(tests/_fewstep.py).

Bars, all taken from the tests of the consecutive loop: one step |dx| <= 2e-6 max(1, |x|_inf) and frames 5e-6
(test_p_sample_matches_oracle); a trajectory max|dx| <= 1e-4 coordinate RMS (test_sampler_api_end_to_end); the twisted sampler under a
constant potential 2e-3 RMS (test_twisted_sampler_constant_potential_is_the_ancestral_sampler_and_guidance_pulls)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _fewstep as R
from oracle import genie_oracle as O

pytestmark = pytest.mark.gpu

T20, STEPS5, SCALE = 20, [20, 15, 10, 6, 1], 0.6
SAMPLERS = {'ancestral': ('ancestral', 0.0), 'ddim0': ('ddim', 0.0), 'ddim1': ('ddim', 1.0)}
BATCHES = {'ragged': [30, 23], 'n24': [24, 24]}


def mdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _noise(lengths, K=5):
    return torch.randn(K, len(lengths), max(lengths), 3, generator=torch.Generator().manual_seed(8 + max(lengths)))


@pytest.fixture(scope='module')
def genie20(base_weights):
    from genie.config import Config
    from genie2_amd.diffusion import Genie
    cfg = Config()
    cfg.diffusion['n_timestep'] = T20
    model = Genie(cfg)
    model.model.load_state_dict(base_weights)
    model = model.eval().to('cuda:0')
    model._test_weights = base_weights
    yield model
    model.model._drop_engine()


@functools.lru_cache(maxsize=None)
def _oracle_states(batch, sampler):
    """The strided loop over the oracle, once per (batch, sampler): [5,B,N,3] states after every iteration."""
    sd = O.synthetic_state_dict(O.BASE_DIMS, seed=0)           # (conftest.base_weights, whose fixture checked the stream)
    name, eta = SAMPLERS[sampler]
    rows = R.coefficient_rows(T20, STEPS5, name, eta)
    return R.strided_loop(sd, dict(O.BASE_DIMS, n_timestep=T20), O.empty_features(BATCHES[batch]), _noise(BATCHES[batch]), SCALE,
                          STEPS5, rows)


# --------------------------------------------------------------- 1. one step
@pytest.mark.parametrize('sampler,eta', [('ancestral', 0.0), ('ddim', 0.5)])
def test_reverse_step_matches_the_float64_formula(base_engine, sampler, eta):
    from genie2_amd import pack
    f = O.empty_features([33, 21])
    fr = O.prepare_features(f)
    g = torch.Generator().manual_seed(5)
    x, z, e = (torch.randn(2, 33, 3, generator=g) * s for s in (5.0, 1.0, 1.0))
    base_engine.bind_features(f)
    for steps, eps in (([1000, 990], e), ([500, 250], e), ([11, 1], e), ([1], None)):
        row = pack.reverse_coefficients(1000, steps, sampler, eta)[0]
        ref = R.reverse_step(R.coefficient_rows(1000, steps, sampler, eta)[0], SCALE, x, z, eps, fr['residue_mask'])
        ref_rots = O.compute_frenet_frames(ref.float(), fr['chain_index'], fr['residue_mask'])
        xg = x.clone().cuda()
        rg = base_engine.reverse_step(row, SCALE, xg, z.cuda(), eps.cuda() if eps is not None else None)
        bar = 2e-6 * max(1.0, float(ref.abs().max()))
        print('one step %s eta %g %s: |dx| %.2e of %.2e, frames %.2e of 5e-6' % (sampler, eta, steps, mdiff(xg, ref), bar, mdiff(rg, ref_rots)))
        assert mdiff(xg, ref) <= bar, steps
        assert mdiff(rg, ref_rots) < 5e-6, steps
        assert float(xg[1, 21:].abs().max()) == 0.0           # masked residues are exactly 0


# --------------------------------------------------------------- 2. consecutive steps are today's loop
def test_consecutive_steps_equal_the_schedule_table_loop(genie20):
    from genie2_amd import pack
    eng = genie20.model.engine()
    eng.bind_features(O.empty_features([30, 30]))
    noise = torch.randn(T20, 2, 30, 3, generator=torch.Generator().manual_seed(8))
    ref, _, ref_rec = eng.sample_loop(noise, SCALE, record=True)
    steps = pack.respaced_steps(T20, T20)
    got, _, rec = eng.sample_loop_steps(noise, SCALE, steps, pack.reverse_coefficients(T20, steps), record=True)
    rms = float(ref.pow(2).mean().sqrt())
    print('K = T against sample_loop: worst |dx| / (1e-4 rms) = %.3f' % (mdiff(rec, ref_rec) / (1e-4 * rms)))
    assert mdiff(got, ref) <= 1e-4 * rms and mdiff(rec, ref_rec) <= 1e-4 * rms


# --------------------------------------------------------------- 3. strided loop against the oracle
@pytest.mark.parametrize('batch', list(BATCHES))
@pytest.mark.parametrize('sampler', list(SAMPLERS))
def test_strided_loop_matches_oracle(genie20, sampler, batch):
    from genie2_amd import pack
    name, eta = SAMPLERS[sampler]
    lengths = BATCHES[batch]
    eng = genie20.model.engine()
    eng.bind_features(O.empty_features(lengths))
    noise = _noise(lengths)
    coef = pack.reverse_coefficients(T20, STEPS5, name, eta)
    final, rots, rec = eng.sample_loop_steps(noise, SCALE, STEPS5, coef, record=True)
    ref = _oracle_states(batch, sampler)
    m = O.empty_features(lengths)['residue_mask'].unsqueeze(-1).float()
    rms = float(ref[-1].pow(2).mean().sqrt())
    per_it = [mdiff(rec[i].cpu() * m, ref[i] * m) / (1e-4 * rms) for i in range(5)]
    print('strided %s %s: |dx| / (1e-4 rms) per iteration %s' % (sampler, batch, ['%.3f' % v for v in per_it]))
    assert max(per_it) <= 1.0, per_it
    assert torch.equal(rec[-1], final)                                         # record holds the per-iteration states
    assert float((final.cpu() * (1 - m)).abs().max()) == 0.0
    # resumed after two iterations from the recorded state: the tails of steps, coef and noise; noise[2] is not read again
    state = (rec[1].clone(), eng.frenet(rec[1]))
    f2, r2, rec2 = eng.sample_loop_steps(noise[2:], SCALE, STEPS5[2:], coef[2:], state=state, record=True)
    assert f2 is state[0] and torch.equal(f2, final) and torch.equal(r2, rots) and torch.equal(rec2, rec[2:])


# --------------------------------------------------------------- 4. refusals
def test_refusals_name_the_entry_and_leave_the_handle_usable(base_engine):
    from genie2_amd import capi, pack
    f = O.empty_features([20, 17])
    base_engine.bind_features(f)
    noise = torch.randn(3, 2, 20, 3, generator=torch.Generator().manual_seed(1)).cuda()
    good = pack.reverse_coefficients(1000, [1000, 500, 1])
    nan = good.clone()
    nan[1, 1] = float('nan')
    inf = good.clone()
    inf[2, 0] = float('inf')
    for steps, coef, word in (([1, 500, 1000], good, 'steps not strictly decreasing'), ([1000, 500, 500], good, 'steps not strictly decreasing'),
                              ([1000, 500, 0], good, r'steps\[2\] = 0 outside 1..1000'), ([1001, 500, 1], good, r'steps\[0\] = 1001 outside'),
                              ([1000, 500, 1], nan, r'non-finite coefficient coef\[1\]\[1\]'), ([1000, 500, 1], inf, r'non-finite coefficient coef\[2\]\[0\]')):
        with pytest.raises(capi.GenieError, match=r'genie_sample_loop_steps failed \(rc=-1\): genie_sample_loop_steps: ' + word):
            base_engine.sample_loop_steps(noise, SCALE, steps, coef)
    lib, h, st = base_engine.lib, base_engine._h, base_engine._stream()
    tr, ro = torch.zeros(2, 20, 3, device='cuda'), torch.zeros(2, 20, 3, 3, device='cuda')
    one_step, one_coef = (C.c_int32 * 1)(5), (C.c_float * 3)(1.0, -0.1, 0.0)
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    for args, word in (((0, one_step, one_coef, p(noise), None, 1, p(tr), p(ro), None), b'n_iter = 0'),
                       ((1, None, one_coef, p(noise), None, 1, p(tr), p(ro), None), b'null steps'),
                       ((1, one_step, None, p(noise), None, 1, p(tr), p(ro), None), b'null steps'),
                       ((1, one_step, one_coef, p(noise), None, 1, None, p(ro), None), b'null steps'),
                       ((1, one_step, one_coef, None, None, 1, p(tr), p(ro), None), b'null noise')):
        assert lib.genie_sample_loop_steps(h, st, *args) == -1
        msg = lib.genie_last_error(h)
        assert msg.startswith(b'genie_sample_loop_steps: ') and word in msg, msg
    assert float(tr.abs().max()) == 0.0                         # nothing was launched
    with pytest.raises(capi.GenieError, match=r'genie_reverse_step failed \(rc=-1\): genie_reverse_step: non-finite coefficient'):
        base_engine.reverse_step((1.0, float('nan'), 0.0), SCALE, tr, noise[0], None)
    assert lib.genie_reverse_step(h, st, 1.0, 0.0, 0.0, p(tr), None, p(noise[0]), None) == -1
    assert b'genie_reverse_step: null tensor' in lib.genie_last_error(h)
    # the handle still denoises
    x = noise[0].cpu()
    fr = O.prepare_features(f)
    z = base_engine.denoise(x, O.compute_frenet_frames(x, fr['chain_index'], fr['residue_mask']), torch.full((2,), 7, dtype=torch.int32))['z']
    assert torch.isfinite(z).all() and float(z.abs().max()) > 0


# --------------------------------------------------------------- 5. samplers
def test_unconditional_sampler_num_steps_matches_oracle_and_writes_pdbs(tmp_path, genie20):
    from genie.sampler.unconditional import UnconditionalSampler
    sampler = UnconditionalSampler(genie20)
    noise = _noise(BATCHES['n24'])
    params = {'length': 24, 'scale': SCALE, 'num_samples': 2, 'outdir': str(tmp_path), 'prefix': '24', 'offset': 4, 'noise': noise,
              'num_steps': 5}
    sampler.sample(params)
    assert sorted(p.name for p in (tmp_path / 'pdbs').iterdir()) == ['24_4.pdb', '24_5.pdb']
    lines = (tmp_path / 'pdbs' / '24_4.pdb').read_text().splitlines()
    assert len(lines) == 24 and lines[0].startswith('ATOM      1  CA  ALA A   1')
    for name, key in (('ancestral', 'ancestral'), ('ddim', 'ddim0')):
        got = sampler._sample(dict(params, sampler=name))
        xyz = torch.tensor(np.stack([g['atom_positions'] for g in got]), dtype=torch.float32)
        ref = _oracle_states('n24', key)[-1]
        assert mdiff(xyz, ref) <= 1e-4 * float(ref.pow(2).mean().sqrt()), name
    # default noise: K draws of the device generator, reproducible, and not the T-step path's draws
    del params['noise']
    torch.manual_seed(0)
    a = sampler._sample(params)
    after = torch.randn(1, device='cuda:0')
    torch.manual_seed(0)
    b = sampler._sample(params)
    assert np.array_equal(a[0]['atom_positions'], b[0]['atom_positions'])
    torch.manual_seed(0)
    torch.stack([torch.randn(2, 24, 3, device='cuda:0') for _ in range(5)])
    assert torch.equal(after, torch.randn(1, device='cuda:0'))                  # exactly 5 [B,N,3] draws were taken


def test_twisted_sampler_num_steps(tmp_path, base_weights):
    from genie.config import Config
    from genie2_amd import pack
    from genie2_amd.diffusion import Genie
    from genie2_amd.sampler import UnconditionalSampler
    from genie2_amd.smc import TwistedSampler, motif_twisting_function
    cfg = Config()
    cfg.diffusion['n_timestep'] = 12
    model = Genie(cfg)
    model.model.load_state_dict(base_weights)
    model = model.eval().to('cuda:0')
    B, N, T, K = 4, 24, 12, 5
    noise = torch.randn(K, B, N, 3, generator=torch.Generator().manual_seed(4))
    base = {'length': N, 'scale': SCALE, 'num_samples': B, 'outdir': str(tmp_path), 'prefix': 'x', 'offset': 0, 'noise': noise,
            'num_steps': K}
    ref = UnconditionalSampler(model)._sample(dict(base))
    tw = TwistedSampler(model)
    got = tw._sample(dict(base, twisting_function=lambda x0, step: (x0 * 0).sum(dim=(1, 2)), last_unguided_steps=0, ess_threshold=0.0))
    a = np.stack([r['atom_positions'] for r in ref])
    b = np.stack([r['atom_positions'] for r in got])
    print('twisted, constant potential: |dx| / (2e-3 rms) = %.3f' % (np.abs(a - b).max() / (2e-3 * np.sqrt((a ** 2).mean()))))
    assert np.abs(a - b).max() <= 2e-3 * np.sqrt((a ** 2).mean())
    assert len(tw.ess_trace) == K - 1 == 4 and tw.resampled_at == []
    # the six-residue motif at residues 5..10; the potential reads the timestep value (abar[step]), not the iteration index
    g = torch.Generator().manual_seed(9)
    target = torch.randn(6, 3, generator=g) * 3
    target = (target - target.mean(0, keepdim=True)).cuda()
    mask = torch.zeros(1, N, dtype=torch.bool)
    mask[0, 5:11] = True
    abar = pack.schedule_tensors(T)['alphas_cumprod'].cuda()
    seen = []

    def twist(x0, step):
        seen.append(step)
        return motif_twisting_function(x0, mask.cuda(), target, abar[step], tausq=0.5)

    guided = tw._sample(dict(base, twisting_function=twist, last_unguided_steps=0, guidance_alpha=0.05, ess_threshold=0.0))
    assert seen == pack.respaced_steps(T, K)

    def motif_rmsd(items):
        out = []
        for it in items:
            x = torch.tensor(it['atom_positions'][5:11], dtype=torch.float32)
            out.append(float(((x - x.mean(0, keepdim=True) - target.cpu()) ** 2).sum(-1).mean().sqrt()))
        return float(np.mean(out))

    print('motif RMSD guided %.3f, unguided %.3f' % (motif_rmsd(guided), motif_rmsd(ref)))
    assert all(np.isfinite(it['atom_positions']).all() for it in guided)
    assert motif_rmsd(guided) < motif_rmsd(ref)
    model.model._drop_engine()
