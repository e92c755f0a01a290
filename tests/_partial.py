"""Helpers of the partial-diffusion tests: a CPU stand-in for the sampling side of GenieEngine over the oracle (so a sampler's host
logic -- which rows of the noise it hands to which loop -- runs without a GPU), stand-in models, and the tail-equivalence case both
the host and the GPU test run."""
import types

import torch

from oracle import genie_oracle as O


class OracleEngine:
    """The calls the samplers make on a bound GenieEngine, over the oracle in float32 on the CPU.  `sample_loop` indexes its noise
    the way include/genie_hip.h states it for genie_sample_loop: by the timestep (row T - t + 1 for the landing of step t, row 0
    only when entered at T), with `noise_first` the row noise[0] stands for; a row outside `noise` is an IndexError here."""
    device = torch.device('cpu')

    def __init__(self, sd, dims):
        self.sd, self.dims = sd, dict(dims)
        self.sched = O.setup_schedule(self.dims['n_timestep'])
        self.rows_read = []

    def bind_features(self, features):
        self.f = O.prepare_features(features)
        self.B, self.N = self.f['residue_mask'].shape

    def frenet(self, trans):
        return O.compute_frenet_frames(trans.float(), self.f['chain_index'], self.f['residue_mask'])

    def q_sample(self, x0, z, c0, c1):
        trans = c0.view(-1, 1, 1) * x0.float() + c1.view(-1, 1, 1) * z.float()
        return trans, self.frenet(trans)

    def denoise(self, trans, rots, timesteps, quat_codes=None, taps=()):
        with torch.no_grad():
            return {'z': O.denoiser_forward(self.sd, self.dims, rots, trans, timesteps.int(), self.f, 'closed', quat_codes)['z']}

    def p_sample(self, step, scale, trans, z, eps):
        new, rots = O.p_sample_step(self.sched, step, scale, trans, z, eps, self.f)
        trans.copy_(new)
        return rots

    def _step(self, trans, rots, step):
        return self.denoise(trans, rots, torch.full((self.B,), step, dtype=torch.int32))['z']

    def sample_loop(self, noise, scale, quat_codes=None, first_step=None, last_step=1, state=None, record=False, noise_first=0):
        T = self.dims['n_timestep']
        first_step = T if first_step is None else first_step

        def row(r):
            if not 0 <= r - noise_first < noise.shape[0]:
                raise IndexError('genie_sample_loop would read row %d; noise holds rows %d..%d' % (r, noise_first, noise_first + noise.shape[0] - 1))
            self.rows_read.append(r - noise_first)
            return noise[r - noise_first].float()

        if first_step == T:
            trans = row(0).clone()
            rots = self.frenet(trans)
        else:
            trans, rots = state
        rec = []
        for step in range(first_step, last_step - 1, -1):
            z = self._step(trans, rots, step)
            rots = self.p_sample(step, scale, trans, z, None if step == 1 else row(T - step + 1))
            rec.append(trans.clone())
        return trans, rots, (torch.stack(rec) if record else None)

    def sample_loop_steps(self, noise, scale, steps, coef, quat_codes=None, state=None, record=False):
        import _fewstep as R
        assert noise.shape[0] == len(steps) == len(coef)
        if state is None:
            trans = noise[0].float().clone()
            rots = self.frenet(trans)
        else:
            trans, rots = state
        rec = []
        for it, step in enumerate(steps):
            z = self._step(trans, rots, step)
            eps = None if it == len(steps) - 1 else noise[it + 1]
            trans.copy_(R.reverse_step(tuple(float(v) for v in coef[it]), scale, trans, z, eps, self.f['residue_mask']).float())
            rots = self.frenet(trans)
            rec.append(trans.clone())
        return trans, rots, (torch.stack(rec) if record else None)


def oracle_model(n_timestep=20, seed=2):
    """(model stand-in on the CPU whose Denoiser.bind returns an OracleEngine, that engine): reduced depth, synthetic weights."""
    from genie2_amd.config import Config
    dims = O.small_dims(n_timestep=n_timestep)
    eng = OracleEngine(O.synthetic_state_dict(dims, seed=seed), dims)
    cfg = Config()
    cfg.diffusion['n_timestep'] = n_timestep

    def bind(features):
        eng.bind_features(features)
        return eng

    model = types.SimpleNamespace(model=types.SimpleNamespace(bind=bind, dims=dims), config=cfg, device=torch.device('cpu'),
                                  setup_schedule=lambda: None)
    return model, eng


def host_model(n_timestep=10):
    """A real Denoiser on torch.device('cpu') behind the samplers' model interface (as test_triatt_host._tri_model, without the
    triangular attention): its bind() raises, so a test that passes through it has reached the library."""
    from genie2_amd.config import Config
    from genie2_amd.model import Denoiser
    cfg = Config()
    cfg.model.update(n_pair_transform_layer=1, n_structure_layer=1)
    cfg.diffusion['n_timestep'] = n_timestep
    m = Denoiser(**cfg.model, n_timestep=n_timestep, max_n_res=64, max_n_chain=1)
    return types.SimpleNamespace(model=m, config=cfg, device=torch.device('cpu'), setup_schedule=lambda: None)


def tail_case(eng, sampler, T, t0, Z, rec, scale, B, N):
    """Tail equivalence at t0: the state the full loop held on entering step t0 (`rec` = its record, `Z` its noise) is reproduced by
    the sampler's own noising of init_structure = 0 with noise[0] = x_t0 / c1[t0]; noise[1:] is the matching tail of Z.  Returns
    the sampler's final coordinates [B,N,3] (float32, CPU)."""
    import numpy as np
    from genie2_amd import pack
    x_t0 = (Z[0] if t0 == T else rec[T - t0 - 1]).detach().cpu().float()
    c1 = pack.schedule_tensors(T)['sqrt_one_minus_alphas_cumprod'][t0].float()
    noise = torch.cat([(x_t0 / c1).unsqueeze(0), Z[T - t0 + 1:].cpu().float()])
    assert noise.shape[0] == t0
    got = sampler._sample({'length': N, 'scale': scale, 'num_samples': B, 'init_structure': torch.zeros(N, 3), 'start_step': t0,
                           'noise': noise})
    return torch.tensor(np.stack([g['atom_positions'] for g in got]), dtype=torch.float32)
