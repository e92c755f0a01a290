"""Samplers with the reference's API (genie/sampler/base.py, unconditional.py).

`BaseSampler._sample` keeps the reference's contract -- features from
`create_np_features`, T-step ancestral sampling, the same Gaussian draw order
(1 initial + one per step except the last, each [B,N,3] from the default
generator of the model's device) -- but the loop body never returns to the
host: all T steps are enqueued through `genie_sample_loop`.

Optional params 'num_steps' = K, 'sampler' ('ancestral' | 'ddim') and 'eta'
(DDIM only) run the reverse process on K of the T timesteps instead
(pack.respaced_steps / reverse_coefficients, `genie_sample_loop_steps`); not in
the reference.  Without them the path above is taken unchanged.

Partial diffusion (not in the reference): optional params 'init_structure' and 'start_step' = t0, given together, start the
reverse process from a backbone the caller already has, noised to step t0 <= T, instead of from pure noise at step T.

  init_structure  float [N, 3] (every sample starts from it) or [B, N, 3] (one per sample), C-alpha, Angstrom, N the padded
                  length the sampler's features give.  Training items are centred on their valid residues
                  (features.create_np_features_from_pdb), so it is centred the same way here: per sample, over the residue
                  mask, on the host; padded rows become 0.  The centring acts on init_structure alone, never on the noised state.
  start_step      an integer in 1..T.
  the start state `eng.q_sample(x_in, noise[0] * mask, c0, c1)`: x_t0 = c0 x_in + c1 noise[0] with c0 = sqrt_alphas_cumprod[t0],
                  c1 = sqrt_one_minus_alphas_cumprod[t0] of pack.schedule_tensors(T) as float32 [B] (what GenieTrainer.training_step
                  passes) and q_sample's own frames; formed on the device, no host round trip.
  the noise       mirrors sample_loop_steps: with n iterations 'noise' is [n, B, N, 3], noise[0] the forward-noising draw and
                  noise[k] the draw of the landing of iteration k - 1; without 'noise' the n draws come from torch.randn on the
                  device in that order.  'quat_codes' [n, B, N, N], where passed, belong to iteration k in the same way.
  the steps       without 'num_steps': t0, t0 - 1, ..., 1 (n = t0) through genie_sample_loop(first_step = t0, state), the T-step
                  loop's own arithmetic.  That entry indexes its noise by the timestep (row T - t + 1 for the landing of step t),
                  so it is handed the caller's rows positioned at row T - t0 (GenieEngine.sample_loop's noise_first); at t0 = T,
                  where the entry would start from noise[0] itself, step T is run by genie_denoise + genie_p_sample and the loop
                  entered at T - 1.  With 'num_steps' = K: pack.partial_steps(T, t0, K), the rows of reverse_coefficients for them
                  and genie_sample_loop_steps carrying the state in (it skips noise[0]); 'sampler' and 'eta' as from noise.

After a partial run `last_start_rmsd` holds the C-alpha RMSD [B] of every result to its (centred) start after optimal
superposition (start_rmsd below: float64 on the host, once per batch); None after a run from noise.
"""
import math
import numbers
import os
from abc import ABC, abstractmethod

import numpy as np
import torch

from . import features as F
from . import pack


def start_rmsd(x, start, mask):
    """C-alpha RMSD [B] (float64, host) of x [B,N,3] to start [B,N,3] after optimal superposition over the residues with
    mask [B,N] != 0: Kabsch with a proper rotation (a mirror image does not fit), padded rows ignored.  A report, not a hot path."""
    x, y, m = (torch.as_tensor(v if torch.is_tensor(v) else np.asarray(v)).detach().cpu().double() for v in (x, start, mask))
    m = (m != 0).double().unsqueeze(-1)
    n = m.sum(dim=1, keepdim=True).clamp(min=1.0)
    xc = (x - (x * m).sum(dim=1, keepdim=True) / n) * m
    yc = (y - (y * m).sum(dim=1, keepdim=True) / n) * m
    u, _, vh = torch.linalg.svd(xc.transpose(1, 2) @ yc)                 # H = sum_i x_i y_i^T = U S V^T;  R = V diag(1, 1, d) U^T
    v = vh.transpose(1, 2)
    d = torch.where(torch.linalg.det(v @ u.transpose(1, 2)) < 0, -1.0, 1.0).double()
    rot = (v * torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=1).unsqueeze(1)) @ u.transpose(1, 2)
    diff = (xc @ rot.transpose(1, 2) - yc) * m
    return torch.sqrt(diff.pow(2).sum(dim=(1, 2)) / n.view(-1))


def prepare_init_structure(x, residue_mask):
    """'init_structure' [N, 3] or [B, N, 3] for a batch with residue_mask [B, N] -> float32 [B, N, 3] on the host, every sample
    centred on its valid residues (in float64) and its padded rows 0.  A wrong shape or a non-finite value is a ValueError."""
    mask = torch.as_tensor(np.asarray(residue_mask)) != 0
    B, N = mask.shape
    try:
        x = (x.detach().cpu() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float64))).double()
    except (TypeError, ValueError) as e:
        raise ValueError('init_structure must be a float tensor or array [%d, 3] or [%d, %d, 3]: %s' % (N, B, N, e))
    if tuple(x.shape) not in ((N, 3), (B, N, 3)):
        raise ValueError('init_structure must be [%d, 3] or [%d, %d, 3], got %s' % (N, B, N, tuple(x.shape)))
    if not bool(torch.isfinite(x).all()):
        raise ValueError('init_structure has a non-finite value')
    x = x.expand(B, N, 3)
    m = mask.unsqueeze(-1)
    x = torch.where(m, x, torch.zeros((), dtype=torch.float64))
    centre = x.sum(dim=1, keepdim=True) / m.sum(dim=1, keepdim=True).clamp(min=1)
    return torch.where(m, x - centre, torch.zeros((), dtype=torch.float64)).float()


def check_start_step(start_step, n_timestep):
    """'start_step' as an int in 1..T; a bool, a fraction, 0 or T + 1 is a ValueError."""
    ok = not isinstance(start_step, bool) and isinstance(start_step, numbers.Real) and math.isfinite(start_step)
    if not ok or int(start_step) != start_step or not 1 <= int(start_step) <= n_timestep:
        raise ValueError('start_step must be an integer in 1..%d, got %r' % (n_timestep, start_step))
    return int(start_step)


class BaseSampler(ABC):
    last_start_rmsd = None

    def __init__(self, model):
        """model: a `genie2_amd.diffusion.Genie` (or anything with .device,
        .config, .model = Denoiser and .setup_schedule())."""
        self.model = model
        self.device = model.device
        self.required = ['scale', 'outdir', 'num_samples', 'prefix', 'offset']
        self.model.setup_schedule()
        self.setup()

    @abstractmethod
    def setup(self):
        raise NotImplementedError

    @abstractmethod
    def on_sample_start(self, params):
        raise NotImplementedError

    @abstractmethod
    def create_np_features(self, params):
        raise NotImplementedError

    @abstractmethod
    def on_sample_end(self, params, list_np_features):
        raise NotImplementedError

    def sample(self, params):
        self.validate_parameters(params)          # like the reference, the result is not acted upon (base.py:164)
        self.on_sample_start(params)
        list_np_features = self._sample(params)
        self.on_sample_end(params, list_np_features)

    def draw_noise(self, B, N, T):
        """The reference's draws (base.py:227,269), in its order, on its device."""
        return torch.stack([torch.randn(B, N, 3, device=self.device) for _ in range(T)])

    def init_structure(self, params):
        """The backbone a partial run starts from, as the caller gave it ([N, 3] or [B, N, 3]), or None."""
        return params.get('init_structure')

    def partial_start(self, params):
        """None without the partial-diffusion params (the run starts from noise at step T); else t0 = 'start_step', checked.
        'init_structure' and 'start_step' come together: one alone is a ValueError naming the missing one.  Host only."""
        x, t0 = self.init_structure(params), params.get('start_step')
        if x is None and t0 is None:
            return None
        if x is None:
            raise ValueError('start_step=%r needs init_structure (the backbone to start from); it is missing' % (t0,))
        if t0 is None:
            raise ValueError('init_structure needs start_step (the timestep it is noised to); it is missing')
        return check_start_step(t0, self.model.config.diffusion['n_timestep'])

    def few_step_plan(self, params):
        """None without 'num_steps' (the reference's T-step loop, or its last t0 steps in a partial run); else (steps, float64
        coefficient rows) of the strided process: pack.respaced_steps from noise, pack.partial_steps below 'start_step'.
        Host only: every bad value raises ValueError here, before the device is touched."""
        num_steps, sampler, eta = params.get('num_steps'), params.get('sampler'), params.get('eta')
        t0 = self.partial_start(params)
        noise = params.get('noise')
        if num_steps is None:
            if sampler not in (None, 'ancestral') or eta is not None:
                raise ValueError('sampler=%r / eta=%r need num_steps' % (sampler, eta))
            if t0 is not None and noise is not None and (noise.dim() != 4 or noise.shape[0] != t0):
                raise ValueError('noise must be [n, B, N, 3] = [%d, B, N, 3] with start_step=%d, got %s' % (t0, t0, tuple(noise.shape)))
            return None
        T = self.model.config.diffusion['n_timestep']
        sampler = 'ancestral' if sampler is None else sampler
        eta = pack.check_sampler(sampler, eta)
        steps = pack.respaced_steps(T, num_steps) if t0 is None else pack.partial_steps(T, t0, num_steps)
        if noise is not None and (noise.dim() != 4 or noise.shape[0] != len(steps)):
            if t0 is not None:
                raise ValueError('noise must be [n, B, N, 3] = [%d, B, N, 3] with start_step=%d and num_steps=%d, got %s'
                                 % (len(steps), t0, len(steps), tuple(noise.shape)))
            raise ValueError('noise must be [%d, B, N, 3] with num_steps=%d, got %s' % (len(steps), len(steps), tuple(noise.shape)))
        return steps, pack.reverse_coefficients(T, steps, sampler, eta)

    def partial_inputs(self, params, np_features, n):
        """Host half of a partial run for the batched numpy features: None from noise; else (t0, x_in): the centred start
        float32 [B, N, 3].  Checks 'init_structure' and the whole shape of 'noise' ([n, B, N, 3]) before the device is touched."""
        t0 = self.partial_start(params)
        if t0 is None:
            return None
        B, N = np_features['residue_mask'].shape
        x_in = prepare_init_structure(self.init_structure(params), np_features['residue_mask'])
        noise = params.get('noise')
        if noise is not None and tuple(noise.shape) != (n, B, N, 3):
            raise ValueError('noise must be [n, B, N, 3] = [%d, %d, %d, 3] with start_step=%d, got %s' % (n, B, N, t0, tuple(noise.shape)))
        return t0, x_in

    def start_state(self, eng, x_in, z0, t0):
        """(trans, rots) at step t0 on the device: genie_q_sample of the centred start and the masked forward draw z0."""
        sched = pack.schedule_tensors(self.model.config.diffusion['n_timestep'])
        B = x_in.shape[0]
        c0 = sched['sqrt_alphas_cumprod'][t0].float().repeat(B)
        c1 = sched['sqrt_one_minus_alphas_cumprod'][t0].float().repeat(B)
        return eng.q_sample(x_in, z0, c0, c1)

    def _partial_loop(self, eng, params, plan, t0, x_in, noise, mask):
        """The reverse process from step t0 (the module docstring): the final trans."""
        T = self.model.config.diffusion['n_timestep']
        noise = noise.to(device=self.device, dtype=torch.float32).contiguous()
        codes, scale = params.get('quat_codes'), params['scale']
        trans, rots = self.start_state(eng, x_in, noise[0] * mask, t0)
        if plan is not None:        # noise[0] is not read again: the loop carries the state in
            return eng.sample_loop_steps(noise, scale, plan[0], plan[1], quat_codes=codes, state=(trans, rots))[0]
        if t0 == T:                 # genie_sample_loop entered at T would start from noise[0]: step T by its two halves
            ts = torch.full((trans.shape[0],), T, dtype=torch.int32, device=self.device)
            z = eng.denoise(trans, rots, ts, None if codes is None else codes[0])['z']
            rots = eng.p_sample(T, scale, trans, z, noise[1] if T > 1 else None)
            if T == 1:
                return trans
            codes, t0 = (None if codes is None else codes[1:]), T - 1
        # the caller's row k is the entry's row T - n + k (n rows, the landing of step t draws row T - t + 1 there)
        return eng.sample_loop(noise, scale, quat_codes=codes, first_step=t0, state=(trans, rots), noise_first=T - noise.shape[0])[0]

    def _sample(self, params):
        plan = self.few_step_plan(params)
        np_feats = F.batchify_np_features([self.create_np_features(params) for _ in range(params['num_samples'])])
        T = self.model.config.diffusion['n_timestep']
        partial = self.partial_inputs(params, np_feats, (self.partial_start(params) or T) if plan is None else len(plan[0]))
        feats = F.convert_np_features_to_tensor(np_feats, self.device)
        B, N = feats['residue_mask'].shape
        noise = params.get('noise')
        if noise is None:
            noise = self.draw_noise(B, N, (T if partial is None else partial[0]) if plan is None else len(plan[0]))
        denoiser = self.model.model
        eng = denoiser.bind(feats)
        self.last_start_rmsd = None
        if partial is not None:
            trans = self._partial_loop(eng, params, plan, partial[0], partial[1], noise, feats['residue_mask'].unsqueeze(-1).float())
            self.last_start_rmsd = start_rmsd(trans, partial[1], feats['residue_mask'])
        elif plan is None:
            trans, _, _ = eng.sample_loop(noise, params['scale'], quat_codes=params.get('quat_codes'))
        else:
            trans, _, _ = eng.sample_loop_steps(noise, params['scale'], plan[0], plan[1], quat_codes=params.get('quat_codes'))
        feats['atom_positions'] = trans.detach().cpu()
        return F.debatchify_np_features(F.convert_tensor_features_to_numpy(feats))

    def add_required_parameter(self, name):
        self.required.append(name)

    def validate_parameters(self, params):
        return all(name in params for name in self.required)


class UnconditionalSampler(BaseSampler):
    """genie/sampler/unconditional.py:12-137."""

    def setup(self):
        self.add_required_parameter('length')

    def on_sample_start(self, params):
        os.makedirs(os.path.join(params['outdir'], 'pdbs'), exist_ok=True)

    def create_np_features(self, params):
        """One chain of params['length'] residues, or (not in the reference's sampler; its features and the denoiser have them) the
        chains of params['chain_lengths']: positive integers that sum to the length, at most as many as the engine's chain table has
        rows.  SymmetryPotential.chain_lengths() gives the units of a symmetric design."""
        chains = params.get('chain_lengths')
        if chains is None:
            return F.create_empty_np_features([params['length']])
        chains = list(chains)
        if not chains or any(isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1 for n in chains):
            raise ValueError('chain_lengths must be positive integers, got %r' % (chains,))
        if sum(chains) != params['length']:
            raise ValueError('chain_lengths %r sum to %d, the length is %d' % (chains, sum(chains), params['length']))
        rows = pack.chain_table_rows(self.model.model.dims)
        if len(chains) > rows:
            raise ValueError('%d chains, the engine\'s chain table holds %d' % (len(chains), rows))
        return F.create_empty_np_features(chains)

    def on_sample_end(self, params, list_np_features):
        for i, np_features in enumerate(list_np_features):
            name = '{}_{}'.format(params['prefix'], params['offset'] + i)
            F.save_np_features_to_pdb(np_features, os.path.join(params['outdir'], 'pdbs', name + '.pdb'))


class ScaffoldSampler(BaseSampler):
    """genie/sampler/scaffold.py:12-169: motif scaffolding.  Conditioning enters only through
    the features (aatype, atom_positions, fixed_* masks); scaffold lengths are drawn per sample,
    so batches are ragged and the residue mask matters."""

    def setup(self):
        self.add_required_parameter('filepath')

    def on_sample_start(self, params):
        for sub in ('pdbs', 'motif_pdbs'):
            os.makedirs(os.path.join(params['outdir'], sub), exist_ok=True)

    def _design(self, params):
        """(design_filepath, motif_filepath) of a re-scaffolding run, or None; one without the other is a ValueError."""
        design, motif = params.get('design_filepath'), params.get('motif_filepath')
        if design is None and motif is None:
            return None
        if design is None or motif is None:
            raise ValueError('design_filepath and motif_filepath come together: %s is missing'
                             % ('design_filepath' if design is None else 'motif_filepath'))
        if params.get('init_structure') is not None:
            raise ValueError('init_structure and design_filepath both name a start: give one')
        return design, motif

    def init_structure(self, params):
        """With 'design_filepath' (a previous run's pdbs/{name}.pdb) and 'motif_filepath' (its motif_pdbs/{name}.pdb) the start is
        the design's C-alpha coordinates and the features are the ones that design was generated with
        (features.create_np_features_from_design: no random draw); 'start_step' goes with them.  'filepath', the problem file,
        stays required: on_sample_end re-indexes its motif records."""
        files = self._design(params)
        if files is None:
            return params.get('init_structure')
        _, coords = F.parse_pdb(files[0])
        return np.concatenate(coords).astype(float)

    def create_np_features(self, params):
        files = self._design(params)
        if files is not None:
            return F.create_np_features_from_design(*files)
        return F.create_np_features_from_motif_pdb(params['filepath'])

    def on_sample_end(self, params, list_np_features):
        from .motif import save_motif_pdb
        for i, np_features in enumerate(list_np_features):
            name = '{}_{}'.format(params['prefix'], params['offset'] + i)
            F.save_np_features_to_pdb(np_features, os.path.join(params['outdir'], 'pdbs', name + '.pdb'))
            save_motif_pdb(params['filepath'], np_features['fixed_sequence_mask'],
                           os.path.join(params['outdir'], 'motif_pdbs', name + '.pdb'))
