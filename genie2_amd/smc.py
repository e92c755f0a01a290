"""Twisted-diffusion / SMC sampling with gradients through the denoiser: the algorithm of the fork's
`genie/sampler/unconditional_smc.py` (:25-43 weight helpers, :233-288 systematic resampling, :303-345 the motif twisting
function, :465-576 the loop) without its wandb / file logging.  The gradient torch.autograd takes there through the whole
Denoiser is `GenieEngine.denoise_vjp` here (HIP backward kernels, frames held fixed exactly as `T(rots.detach(), trans.detach())`
does); the reference's potential acts on a [B, N, 3] tensor and stays in PyTorch here (motif_twisting_function), with
MotifPotential (appended below) as its one-pass HIP form (csrc/smc_kernels.hip).  ShapePotential (csrc/shape_kernels.hip: radius of
gyration, clashes, distance restraints; not in the reference) is the second built-in potential, SecStructPotential
(csrc/secstruct_kernels.hip: helix / extended content and a blueprint; the reference's sampler/secstruct.py runs P-SEA on the host and
is not differentiable) the third, SheetPotential (csrc/sheet_kernels.hip: antiparallel / parallel strand pairing and a ladder of listed
rungs; not in the reference) the fourth, SymmetryPotential (csrc/symmetry_kernels.hip: cyclic, dihedral and repeat symmetry by
superposing units under the group's generators; not in the reference) the fifth, BinderPotential (csrc/binder_kernels.hip: contacts,
hotspot coverage and clashes against a fixed target that is not sampled; not in the reference) the sixth, FoldPotential and
AlignedFoldPotential (csrc/fold_kernels.hip, fold_align_kernels.hip: TM-score ranges to fixed backbones) and DiversityPotential
(csrc/diversity_kernels.hip: the particles of a batch repel each other) follow, and SumPotential adds potentials.

The reference module imports wandb / Bio, which are not installed here, so it could not be run: parity of this file is
UNPINNED by reference outputs; what is tested is (a) the helpers against restatements of the quoted lines, (b) that a constant
potential reproduces the ancestral sampler, (c) that the guided gradient equals torch autograd through the oracle."""
import ctypes as C
import numbers
import types

import torch

from . import capi
from . import features as F
from . import pack
from .sampler import UnconditionalSampler, start_rmsd


def normalize_log_weights(log_weights, dim):
    log_weights = log_weights - log_weights.max(dim=dim, keepdims=True)[0]
    return log_weights - torch.logsumexp(log_weights, dim=dim, keepdims=True)


def normalize_weights(log_weights, dim=0):
    return torch.exp(normalize_log_weights(log_weights, dim=dim))


def compute_ess(w, dim=0):
    return (w.sum(dim=dim)) ** 2 / torch.sum(w ** 2, dim=dim)


def compute_ess_from_log_w(log_w, dim=0):
    return compute_ess(normalize_weights(log_w, dim=dim), dim=dim)


def log_normal_density(sample, mean, var):
    return torch.distributions.normal.Normal(loc=mean, scale=torch.sqrt(var)).log_prob(sample)


def systematic_resampling(particles, weights, u=None):
    """unconditional_smc.py:237-288: one uniform draw u in [0, 1/N), points u + i/N, particle j is taken for every point in
    (cumsum_j, cumsum_{j+1}].  Returns (resampled particles, new log-weights = 0, indices)."""
    n = len(weights)
    weights = weights / torch.sum(weights)
    cumsum = torch.cumsum(weights, dim=0)
    if u is None:
        u = torch.distributions.Uniform(low=0.0, high=1.0 / n).sample()
    points = (torch.as_tensor(u, dtype=cumsum.dtype) + torch.arange(n, dtype=cumsum.dtype) / n).to(cumsum.device)
    # the reference walks j up while points[i] > cumsum[j + 1]: the number of cumulative sums strictly below the point
    indexes = torch.searchsorted(cumsum, points, right=False).clamp_(max=n - 1)
    return particles[indexes], torch.zeros(n, device=particles.device), indexes


def xstart_variance(alphas_cumprod_t, tausq=0.012):
    """unconditional_smc.py:290-302, var_type 6: sigma^2 tau^2 / (sigma^2 + tau^2), sigma^2 = (1 - abar) / abar."""
    sigmasq = (1 - alphas_cumprod_t) / alphas_cumprod_t
    return (sigmasq * tausq) / (sigmasq + tausq)


def motif_twisting_function(x0, motif_index_mask, motif_target, alphas_cumprod_t, tausq=0.012):
    """unconditional_smc.py:303-345: log of the mean over candidate placements of a Gaussian likelihood of the (centred) motif
    coordinates.  x0 [B,N,3]; motif_index_mask [n_placement, N] bool (one segment set per placement, equal counts);
    motif_target [n_motif_res, 3] centred.  Returns [B]."""
    var = xstart_variance(alphas_cumprod_t, tausq)
    scores = []
    for mask in motif_index_mask:
        sel = x0[:, mask]                                           # [B, n_motif_res, 3]
        sel = sel - sel.mean(dim=-2, keepdim=True)
        scores.append(-torch.sum((sel - motif_target[None]) ** 2, dim=(1, 2)) / (2 * var))
    score = torch.stack(scores)                                     # [n_placement, B]
    return torch.logsumexp(score, dim=0) - torch.log(torch.tensor(float(score.shape[0]), device=x0.device))


def get_all_motif_locations(L, segment_lengths, max_offsets=1000, rng=None):
    """unconditional_smc.py:173-215: every placement of the segments, in order and without overlap, inside 0..L-1, as
    [(start, end), ...] per placement (end inclusive), in the reference's order -- ascending in the first start, then the second,
    ...  More than `max_offsets` placements are thinned with one `choice(n, max_offsets, replace=False)` draw (numpy's global
    generator there; `rng` here, default the same global one)."""
    import numpy as np
    k, total = len(segment_lengths), sum(segment_lengths)
    out = []
    starts = [0] * k

    def place(seg, first_free):
        # the segments from `seg` on need this much room; the last admissible start leaves exactly that
        need = sum(segment_lengths[seg:])
        for st in range(first_free, L - need + 1):
            starts[seg] = st
            if seg + 1 == k:
                out.append([(s, s + n - 1) for s, n in zip(starts, segment_lengths)])
            else:
                place(seg + 1, st + segment_lengths[seg])

    if k and total <= L:
        place(0, 0)
    if len(out) > max_offsets:
        pick = (rng if rng is not None else np.random).choice(len(out), max_offsets, replace=False)
        out = [out[i] for i in pick]
    return out


def generate_motif_index_mask(motif_target, n_res, max_offsets=1000, rng=None, device=None):
    """unconditional_smc.py:172-232: bool [n_placement, n_segment, n_res, 3], True over the residues segment j occupies in
    placement i.  `motif_target`: one entry per segment (anything with a length: its residues)."""
    locs = get_all_motif_locations(n_res, [len(seg) for seg in motif_target], max_offsets, rng)
    mask = torch.zeros(len(locs), len(motif_target), n_res, 3, dtype=torch.bool)
    for i, placement in enumerate(locs):
        for j, (st, end) in enumerate(placement):
            mask[i, j, st:end + 1] = True
    return mask.to(device) if device is not None else mask


def placement_masks(motif_index_mask):
    """[n_placement, n_segment, N, 3] -> [n_placement, N]: the residues any segment covers (what motif_twisting_function takes)."""
    return motif_index_mask[..., 0].any(dim=1)


class TwistedSampler(UnconditionalSampler):
    """params: the UnconditionalSampler's + 'twisting_function': callable (x0_pred [B,N,3] requiring grad, step) -> log p(y | x_t) [B];
    or, instead, 'motif_target' (list of [n_i, 3] segments: the placements are enumerated with generate_motif_index_mask and the
    potential is motif_twisting_function over all of them, unconditional_smc.py:303-345); optional 'tausq' with it;
    optional 'noise' [T,B,N,3] (initial draw + one per step, as BaseSampler), 'resample_u' (list of uniforms, tests),
    'guidance_alpha' (default 0.012), 'ess_threshold' (default 0.5), 'last_unguided_steps' (default 50), 'chain_lengths' (the
    UnconditionalSampler's: the structure as several chains, e.g. SymmetryPotential.chain_lengths()).
    After _sample, `last_fit` holds what the twisting function's `locate` says of the final coordinates (MotifPotential.locate: 'best',
    'rmsd', 'starts', 'ends' as CPU tensors, one row per returned sample; with motif groups also 'group_rmsd' and the 'groups' labels),
    or None when it has no `locate`; `last_shape` what its `describe` says of them (ShapePotential.describe: 'rog', 'min_distance',
    'n_clash', 'e_rog', 'e_clash', 'e_restraint', 'n_violated', 'max_violation' as CPU tensors, one row per returned sample; with a
    SecStructPotential its eight fields, with a SheetPotential its nine, with a SymmetryPotential its eight, and with a SumPotential
    every member's; with a BinderPotential its nine), or None when it has no `describe`; `last_secstruct` what its `assign` says of them (SecStructPotential.assign: int8 [rows, N] on the CPU, 0 C, 1 H, 2 E), or None when it has no
    `assign`; `last_pairs` what its `pairs` says of them (SheetPotential.pairs: int32 [rows, N, 2] on the CPU, every residue's
    antiparallel and parallel partner, -1 for none), or None when it has no `pairs`; `last_positions` the returned coordinates
    themselves in the sampler's frame, a CPU float32 [rows, N, 3] tensor (the written PDBs are centred per design, so this is what
    puts a design next to a BinderPotential's target).
    Optional 'num_steps' = K (not in the reference) visits the K timesteps of pack.respaced_steps with the ancestral kernel between
    them (pack.twisted_coefficients): `ess_trace` then has K - 1 entries, the last visited step takes the role of step 1, and
    `last_unguided_steps` and the potential keep reading the timestep itself.  'sampler': 'ddim' is refused (ValueError): the
    weights are ratios of the Gaussian transition densities of the ancestral kernel.
    A model with triangular attention is refused at construction: the guidance needs the denoiser's VJP, which is not built for it.

    One loop serves every variant: _setup builds the run's state, guided_step (below the class) is the guided half of an iteration,
    _host_update or one SmcReweight call its SMC bookkeeping, _finish the reports.

    Optional 'num_particles' = K in 1..64 (not in the reference; the fork's latest sampler has the layout) makes 'num_samples' = S
    independent particle systems of K particles each in one device batch of S K, system-major (particle b belongs to system b // K):
    weights, ESS, resampling and the gradient-norm cap are per system, and the SMC bookkeeping of a step is one genie_smc_reweight
    call (csrc/smc_step_kernels.hip) with no host read inside the loop.  'noise' is then [T, S K, N, 3]; entry `it` of 'resample_u'
    is a scalar for every system or S values; `ess_trace` is a CPU tensor [steps - 1, S], `resampled_at` a list of S lists of steps,
    `last_log_weights` [S, K] the accumulated log-weights after the last weight update and `last_choice` [S] their argmax (the lowest
    index of equal ones).  'return_particles': 'all' (default) returns the S K structures, 'best' particle last_choice[s] of every
    system (S structures, `last_fit` with S rows).  Without 'num_particles' nothing of this applies: one system of num_samples.

    Partial diffusion ('init_structure' + 'start_step' = t0, the sampler module's docstring; not in the reference): the particles
    start at x_t0 = c0 x_in + c1 noise[0] (genie_q_sample, its frames) and visit t0, ..., 1, or pack.partial_steps(T, t0, K) with
    pack.twisted_coefficients; 'noise' is [n, B, N, 3] for n visited steps, noise[0] the forward draw.  With particle systems an
    [N, 3] start is shared by all particles of all systems and an [S K, N, 3] start is system-major like everything else.
    The initial log_proposal is log_normal_density(noise[0], 0, 1).sum(dim=(1, 2)): the density of the actual proposal
    q(x_t0 | x_in) = N(c0 x_in, c1^2) at x_t0 is that of noise[0] under N(0, 1) minus 3 N log c1, a constant that is equal for all
    particles and cancels in every normalisation the loop performs (softmax, normalize_log_weights, the ESS).  With t0 = T it is
    today's expression to within c0 ~ 1.6e-3.  `ess_trace` (n - 1 entries), `resampled_at`, `last_unguided_steps` and the
    potential's `step` argument stay defined on the timestep itself.  'sampler': 'ddim' stays refused.  `last_start_rmsd` [B] is
    set as in BaseSampler (every returned structure against the start of its own batch slot, whichever ancestor it was resampled from)."""

    def __init__(self, model):
        if getattr(model.model, 'dims', {}).get('n_head_tri', 0):       # before any device work
            raise NotImplementedError('triangular attention: sampling only (the twisted sampler needs the denoiser VJP through it)')
        super().__init__(model)

    def few_step_plan(self, params):
        if params.get('sampler') not in (None, 'ancestral'):
            pack.check_sampler(params['sampler'])                       # (an unknown name is its own error)
            raise ValueError('the twisted sampler has the ancestral kernel only, got sampler=%r' % (params['sampler'],))
        plan = super().few_step_plan(params)
        return None if plan is None else (plan[0], pack.twisted_coefficients(self.model.config.diffusion['n_timestep'], plan[0]))

    def _setup(self, params, steps, coef, B, S=None):
        """The state of a run over `steps` (`coef`: their rows of pack.twisted_coefficients on the host, or None) with a device
        batch of B, as S systems (None: one system, the whole batch): what guided_step reads, and the start of the loop --
        trans, rots, log_proposal, log_w_acc."""
        m = self.model
        np_feats = F.batchify_np_features([self.create_np_features(params) for _ in range(B)])
        partial = self.partial_inputs(params, np_feats, len(steps))
        feats = F.convert_np_features_to_tensor(np_feats, self.device)
        N = feats['residue_mask'].shape[1]
        tw_coef = None if coef is None else coef.to(device=self.device, dtype=torch.float32)
        sched = {k: v.to(self.device) for k, v in pack.schedule_tensors(m.config.diffusion['n_timestep']).items()}
        abar = sched['alphas_cumprod']
        noise = params.get('noise')
        draw = (lambda k: noise[k].to(self.device)) if noise is not None else (lambda k: torch.randn(B, N, 3, device=self.device))
        twist = params.get('twisting_function')
        if twist is None:       # the reference's own potential: every placement of the motif segments (:172-232, 303-345)
            segs = [torch.as_tensor(x, dtype=torch.float32) for x in params['motif_target']]
            pm = placement_masks(generate_motif_index_mask(segs, N)).to(self.device)
            tgt = torch.cat(segs).to(self.device)
            tgt = tgt - tgt.mean(dim=0, keepdim=True)
            tausq = float(params.get('tausq', 0.012))
            twist = lambda x0, step: motif_twisting_function(x0, pm, tgt, abar[step], tausq)      # noqa: E731
        eng = m.model.bind(feats)
        w = pack.flatten_state_dict(m.model.state_dict(), m.model.dims).to(self.device)
        mask = feats['residue_mask'].unsqueeze(-1).float()
        trans = draw(0)
        log_proposal = log_normal_density(trans, torch.tensor(0., device=self.device), torch.tensor(1., device=self.device)).sum(dim=(1, 2))
        if partial is None:
            rots = eng.frenet(trans)
        else:           # trans was the forward draw noise[0]: log_proposal is its density (the class docstring), the state q_sample's
            trans, rots = self.start_state(eng, partial[1], trans.float() * mask, partial[0])
        return types.SimpleNamespace(
            steps=steps, tw_coef=tw_coef, sched=sched, feats=feats, partial=partial, draw=draw, twist=twist, eng=eng, w=w, mask=mask,
            S=S, alpha=float(params.get('guidance_alpha', 0.012)), unguided=int(params.get('last_unguided_steps', 50)),
            ess_fraction=float(params.get('ess_threshold', 0.5)), trans=trans, rots=rots, log_proposal=log_proposal,
            log_w_acc=torch.zeros(B, device=self.device))

    def _host_update(self, st, step, new, mean_t, mean_u, sigma, log_prob, us):
        """The SMC bookkeeping of one system of B = the whole batch, in torch with one host read (the ESS): the weight update, then
        systematic resampling (its uniform from `us`, else drawn on the host) or the renormalisation.  Returns the next particles."""
        B = new.shape[0]
        log_rev = log_normal_density(new, mean_u, sigma ** 2).sum(dim=(1, 2))
        log_tw = log_normal_density(new, mean_t, sigma ** 2).sum(dim=(1, 2))
        log_w = (log_rev + log_prob - log_tw) - st.log_proposal
        st.log_proposal = log_prob
        st.log_w_acc = log_w + st.log_w_acc
        ess = compute_ess_from_log_w(st.log_w_acc)
        self.ess_trace.append(float(ess))
        if ess < st.ess_fraction * B:
            new, st.log_w_acc, idx = systematic_resampling(new, torch.softmax(st.log_w_acc, dim=0), us.pop(0) if us else None)
            st.log_proposal = st.log_proposal[idx.to(self.device)]
            self.resampled_at.append(step)
        else:
            st.log_w_acc = normalize_log_weights(st.log_w_acc, dim=0) + torch.log(torch.tensor(float(B), device=self.device))
        return new

    def _finish(self, st, trans, feats, start):
        """The reports on the returned coordinates `trans` (MotifPotential.locate: the best placement of every sample and its
        superposed RMSD; describe; assign; the RMSD to `start`; the coordinates themselves as last_positions) and the features to write."""
        twist = st.twist
        self.last_fit = None
        if hasattr(twist, 'locate') and getattr(twist, 'has_fit', True):
            self.last_fit = {k: v.cpu() if torch.is_tensor(v) else v for k, v in twist.locate(trans).items()}
        self.last_shape = {k: v.cpu() for k, v in twist.describe(trans).items()} if hasattr(twist, 'describe') else None
        self.last_secstruct = twist.assign(trans).cpu() if hasattr(twist, 'assign') else None
        self.last_pairs = twist.pairs(trans).cpu() if hasattr(twist, 'pairs') else None
        feats['atom_positions'] = trans.cpu()
        self.last_positions = feats['atom_positions'].detach().to(torch.float32)
        self.last_start_rmsd = None if start is None else start_rmsd(feats['atom_positions'], start, feats['residue_mask'])
        return F.debatchify_np_features(F.convert_tensor_features_to_numpy(feats))

    def _sample(self, params):
        K, S = params.get('num_particles'), None
        if K is not None or params.get('return_particles') is not None:       # S = num_samples systems of K particles (the class docstring)
            keep = params.get('return_particles', 'all')
            if K is None:
                raise ValueError("return_particles=%r needs num_particles" % (keep,))
            if isinstance(K, bool) or not isinstance(K, numbers.Integral) or not 1 <= K <= SMC_MAX_PARTICLES:
                raise ValueError('num_particles must be an integer in 1..%d, got %r' % (SMC_MAX_PARTICLES, K))
            if keep not in ('all', 'best'):
                raise ValueError("return_particles must be 'all' or 'best', got %r" % (keep,))
            K, S = int(K), params['num_samples']
        plan = self.few_step_plan(params)
        steps = list(range(self.partial_start(params) or self.model.config.diffusion['n_timestep'], 0, -1)) if plan is None else plan[0]
        us = list(params.get('resample_u', []))
        if S is not None:
            noise = params.get('noise')
            if noise is not None and (noise.dim() != 4 or noise.shape[0] != len(steps) or noise.shape[1] != S * K):
                raise ValueError('noise must be [%d, %d, N, 3] with num_samples=%d and num_particles=%d, got %s'
                                 % (len(steps), S * K, S, K, tuple(noise.shape)))
            us = [[float(e)] * S if _is_scalar(e) else [float(v) for v in e] for e in us]
            if any(len(e) != S for e in us):
                raise ValueError('an entry of resample_u is a scalar or %d values, one per system' % S)
        st = self._setup(params, steps, None if plan is None else plan[1], params['num_samples'] if S is None else S * K, S)
        feats, trans, rots = st.feats, st.trans, st.rots
        B, N = feats['residue_mask'].shape
        if S is None:
            self.ess_trace, self.resampled_at = [], []
        else:
            reweight = SmcReweight(S, K, N, self.device)
            ess_dev = torch.zeros(max(len(steps) - 1, 0), S, dtype=torch.float32, device=self.device)
            resampled_dev = torch.zeros(max(len(steps) - 1, 0), S, dtype=torch.int32, device=self.device)
        for it, step in enumerate(steps):
            mean_t, mean_u, sigma, log_prob = guided_step(st, it, step, trans, rots)
            if it == len(steps) - 1:
                trans = mean_t
                break
            new = (mean_t + params['scale'] * sigma * st.draw(it + 1)) * st.mask
            if S is None:
                trans = self._host_update(st, step, new, mean_t, mean_u, sigma, log_prob, us)
            else:       # the same bookkeeping per system as one genie_smc_reweight call, no host read
                if it < len(us):
                    u = torch.tensor(us[it], dtype=torch.float32).to(self.device)
                else:
                    u = torch.rand(S, device=self.device) / K
                trans, _ = reweight(new, mean_t, mean_u, sigma, log_prob, u, st.ess_fraction, st.log_proposal, st.log_w_acc,
                                    ess_out=ess_dev[it], resampled_out=resampled_dev[it])
            rots = st.eng.frenet(trans)
        trans = trans.detach()
        start = None if st.partial is None else st.partial[1]
        if S is not None:
            # the one host read of the run
            self.ess_trace = ess_dev.cpu()
            flags = resampled_dev.cpu()
            self.resampled_at = [[steps[it] for it in range(flags.shape[0]) if int(flags[it, s])] for s in range(S)]
            self.last_log_weights = st.log_w_acc.detach().cpu().view(S, K)
            top = self.last_log_weights == self.last_log_weights.max(dim=1, keepdim=True).values
            first = torch.where(top, torch.arange(K).expand(S, K), torch.full((S, K), K)).min(dim=1).values
            self.last_choice = torch.where(first < K, first, torch.zeros_like(first))       # (no entry equals a NaN max: particle 0)
            if keep == 'best':
                pick = (torch.arange(S) * K + self.last_choice).to(self.device)
                trans = trans[pick]
                start = None if start is None else start[pick.cpu()]
                feats = {k: (v[pick] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B else v) for k, v in feats.items()}
        return self._finish(st, trans, feats, start)


def guided_step(state, it, step, trans, rots):
    """The guided half of iteration `it` of TwistedSampler's loop, at timestep `step`: the denoiser's E[x_0 | x_t], the potential and
    its gradient through the denoiser, capped in norm, and the posterior between `step` and the next visited one.  Returns
    (mean_t, mean_u, sigma, log_prob): the twisted and the unguided mean, the posterior's standard deviation, log p(y | x_t) [B]
    detached.  `state` holds eng, w, sched, tw_coef, twist, alpha, unguided and S (TwistedSampler._setup); with S systems the cap is
    over a system's own particles, with S = None over the whole batch."""
    st, B = state, trans.shape[0]
    abar, betas = st.sched['alphas_cumprod'], st.sched['betas']
    ts = torch.full((B,), step, dtype=torch.int32, device=trans.device)
    c0, c1 = torch.sqrt(abar[step]), torch.sqrt(1 - abar[step])
    z = st.eng.denoise(trans, rots, ts)['z']
    x0 = ((trans - c1 * z) / c0).detach().requires_grad_(True)          # E[x_0 | x_t] (:474)
    log_prob = st.twist(x0, step)
    g = torch.autograd.grad(log_prob.mean(), x0)[0] * B                   # (:480-482, "rescale mean back")
    # chain rule through x0(trans) = (trans - c1 z(trans)) / c0 with the frames fixed: the part through z is the HIP VJP
    _, dz_part = st.eng.denoise_vjp(st.w, trans, rots, ts, (-c1 / c0) * g)
    grad = g / c0 + dz_part
    if st.S is None:
        norm = grad.double().norm().float()                               # (f64: the f32 sum of squares overflows before the cap below acts)
    else:       # over a system's own particles: a system's step must not depend on its batch neighbours
        norm = grad.double().view(st.S, -1).norm(dim=1).float().view(st.S, 1, 1, 1)
        grad = grad.view(st.S, B // st.S, *grad.shape[1:])
    grad = (grad * st.alpha * norm / (st.alpha + norm)).view(x0.shape)   # (:483-488)
    x0u = x0.detach()
    x0t = x0u + grad if step >= st.unguided else x0u
    if st.tw_coef is None:
        coef1 = torch.sqrt(abar[step - 1]) * betas[step] / (1 - abar[step])
        coef2 = st.sched['sqrt_alphas'][step] * (1.0 - abar[step - 1]) / (1 - abar[step])
        sigma = st.sched['sqrt_betas'][step]
    else:           # the same posterior between step and the next visited one (float64 on the host, pack.twisted_coefficients)
        coef1, coef2, sigma = st.tw_coef[it]
    return coef1 * x0t + coef2 * trans, coef1 * x0u + coef2 * trans, sigma, log_prob.detach()


SMC_MAX_PARTICLES = 64          # K of genie_smc_reweight: one wave holds a system


def _is_scalar(x):
    return isinstance(x, numbers.Real) or (torch.is_tensor(x) and x.dim() == 0)


def _ptr(t):
    """A tensor's data pointer as a C entry takes it; NULL for None."""
    return C.c_void_p(t.data_ptr() if t is not None else 0)


class _HipEntry:
    """What a class that launches libgenie_hip entries holds: the library, its GPU device and the checked call."""

    def _bind(self, device, name):
        """Load the library and normalise `device`, which must be a GPU (`name` is who says so): its index is filled in."""
        self.lib = capi.load_library()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise capi.GenieError('%s runs on the GPU (libgenie_hip); there is no CPU path' % name)
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, *args):
        """Run the entry `name` with the device current; a non-zero return is a GenieError with the library's message."""
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(*args)
        if rc != 0:
            msg = self.lib.genie_last_error(None)
            raise capi.GenieError('%s failed (%d): %s' % (name, rc, msg.decode() if msg else '?'))


class SmcReweight(_HipEntry):
    """genie_smc_reweight (include/genie_hip.h) for S systems of K particles of N residues on `device`: one call does, per system,
    what smc.py's loop does after the draw -- the weight update, the ESS, systematic resampling below `ess_fraction` K or the
    renormalisation above it -- on torch's current stream, without a host read.  `log_proposal` and `log_w_acc` [S K] are updated in
    place; returns (x_out [S K, N, 3], index [S K] int32: every particle's ancestor as a batch index) and leaves the ESS and the 0 / 1
    resampling flag of every system in `ess_out` / `resampled_out` [S] (its own `ess`, `resampled` when none are given)."""

    def __init__(self, S, K, N, device='cuda'):
        self.S, self.K, self.N = int(S), int(K), int(N)
        self._bind(device, 'genie_smc_reweight')
        need = self.lib.genie_smc_reweight_work_bytes(self.S, self.K, self.N)
        if need == 0:
            raise ValueError('S = %d, K = %d, N = %d: needs S, N >= 1 and K in 1..%d' % (self.S, self.K, self.N, SMC_MAX_PARTICLES))
        self.work = torch.empty(need // 8, dtype=torch.float64, device=self.device)
        self.ess = torch.zeros(self.S, dtype=torch.float32, device=self.device)
        self.resampled = torch.zeros(self.S, dtype=torch.int32, device=self.device)

    def __call__(self, x_new, mean_tw, mean_un, sigma, log_prob, u, ess_fraction, log_proposal, log_w_acc, ess_out=None,
                 resampled_out=None, x_out=None, work_bytes=None):
        B, f32 = self.S * self.K, torch.float32
        ess_out = self.ess if ess_out is None else ess_out
        resampled_out = self.resampled if resampled_out is None else resampled_out
        ins = [t.detach().to(f32).contiguous() for t in (x_new, mean_tw, mean_un)]
        sigma = sigma.detach().to(f32).reshape(1).contiguous()
        log_prob, u = log_prob.detach().to(f32).contiguous(), u.detach().to(f32).contiguous()
        for t, shape, dtype in ((ins[0], (B, self.N, 3), f32), (ins[1], (B, self.N, 3), f32), (ins[2], (B, self.N, 3), f32),
                                (log_prob, (B,), f32), (u, (self.S,), f32), (log_proposal, (B,), f32), (log_w_acc, (B,), f32),
                                (ess_out, (self.S,), f32), (resampled_out, (self.S,), torch.int32)):
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                raise ValueError('genie_smc_reweight: expected a contiguous %s %s on %s, got %s %s on %s'
                                 % (dtype, shape, self.device, t.dtype, tuple(t.shape), t.device))
        x_out = torch.empty_like(ins[0]) if x_out is None else x_out
        index = torch.empty(B, dtype=torch.int32, device=self.device)
        self._call('genie_smc_reweight', self._stream(), self.S, self.K, self.N, *(_ptr(t) for t in ins), _ptr(sigma), _ptr(log_prob),
                   _ptr(u), float(ess_fraction), _ptr(log_proposal), _ptr(log_w_acc), _ptr(x_out), _ptr(index), _ptr(ess_out),
                   _ptr(resampled_out), _ptr(self.work), self.work.numel() * 8 if work_bytes is None else work_bytes)
        return x_out, index


def placement_starts(locs):
    """get_all_motif_locations' output ([(start, end), ...] per placement) -> int32 [P, S], the start residue of every segment in
    every placement, in the same order: what genie_motif_potential takes instead of the [P, N] masks of placement_masks."""
    if not locs:
        return torch.zeros(0, 0, dtype=torch.int32)
    return torch.tensor([[st for st, _ in pl] for pl in locs], dtype=torch.int32)


def canonical_groups(groups, n_segments):
    """One hashable label per segment -> (labels in order of first appearance, group index of every segment): B, A, B gives
    ([B, A], [0, 1, 0])."""
    groups = list(groups)
    if len(groups) != n_segments:
        raise ValueError('groups needs one label per segment: %d labels for %d segments' % (len(groups), n_segments))
    labels = []
    for g in groups:
        if g not in labels:
            labels.append(g)
    return labels, [labels.index(g) for g in groups]


def _check_superposable(xyz, what):
    """A superposed fit of these residues [n, 3] has a unique rotation: three at least, not on one line."""
    xyz = xyz.double()
    if len(xyz) < 3:
        raise ValueError('a superposed fit needs at least 3 motif residues, got %d%s' % (len(xyz), what))
    sv = torch.linalg.svdvals(xyz - xyz.mean(dim=0, keepdim=True))
    if float(sv[1]) < 1e-3 * float(sv[0]):
        raise ValueError('the motif residues%s are collinear: their superposition has no unique rotation' % what)


def _check_starts(starts, seg_len, n_res):
    """The contract of genie_motif_potential, checked once on the host: segments in order, without overlap, inside 0..n_res-1."""
    lens = torch.as_tensor(seg_len, dtype=torch.int64)
    st = starts.to(torch.int64)
    if st.dim() != 2 or st.shape[0] < 1 or st.shape[1] != len(lens):
        raise ValueError('starts must be [P >= 1, %d], got %s' % (len(lens), tuple(starts.shape)))
    ends = st + lens[None]                                          # one past each segment
    if bool((st[:, 0] < 0).any()) or bool((ends[:, -1] > n_res).any()) or bool((ends[:, :-1] > st[:, 1:]).any()):
        raise ValueError('a placement leaves 0..%d or puts its segments out of order' % (n_res - 1))


class _PotentialFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, pot, var):
        logp, grad = pot._launch(pot._checked(x0), var)
        ctx.save_for_backward(grad)
        return logp

    @staticmethod
    def backward(ctx, grad_output):
        grad, = ctx.saved_tensors
        return grad_output[:, None, None] * grad, None, None


class _HipPotential(_HipEntry):
    """What the built-in potentials share: `pot(x0 [B,N,3], step) -> log p [B]` through the subclass's `_launch(x, var)`, which
    returns (logp, grad) of one C entry; the forward keeps that gradient and the backward scales it.  A subclass validates its
    arguments on the host and then calls this constructor, which is the first to look at the device.  (No `locate`, `describe`,
    `assign` or `has_fit` here: TwistedSampler and SumPotential take a potential to report what it has a method for.)"""

    def __init__(self, n_res, alphas_cumprod, tausq, device):
        self._bind(device, type(self).__name__)
        self.n_res, self.tausq = int(n_res), float(tausq)
        self.abar = torch.as_tensor(alphas_cumprod).to(self.device)
        self._work = torch.zeros(0, dtype=torch.uint8, device=self.device)
        self._one = torch.ones(1, dtype=torch.float32, device=self.device)

    def variance(self, step):
        return xstart_variance(self.abar[step], self.tausq).to(torch.float32).reshape(1).contiguous()

    def __call__(self, x0, step):
        return _PotentialFn.apply(x0, self, self.variance(step))

    def _checked(self, x0):
        if x0.dim() != 3 or x0.shape[1] != self.n_res or x0.shape[2] != 3:
            raise ValueError('x0 must be [B, %d, 3], got %s' % (self.n_res, tuple(x0.shape)))
        if x0.device != self.device:
            raise ValueError('x0 is on %s, the potential on %s' % (x0.device, self.device))
        return x0.detach().to(torch.float32).contiguous()

    def _workspace(self, need):
        """The entry's `work` arguments (pointer, bytes): a device buffer of at least `need` bytes, grown on demand; NULL for 0."""
        if need > self._work.numel():
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        return _ptr(self._work if need else None), self._work.numel()


def _decode_report(report, names, count_names):
    """A [B, len(names)] report of a C entry as {name: [B]}: int64 for the `count_names`, a copy of the column otherwise."""
    return {k: report[:, i].round().long() if k in count_names else report[:, i].clone() for i, k in enumerate(names)}


class MotifPotential(_HipPotential):
    """The motif twisting function of unconditional_smc.py:303-345 (motif_twisting_function above) as one HIP pass over every
    placement: `pot(x0 [B,N,3], step) -> log p(y | x0) [B]`, differentiable in x0, a drop-in `twisting_function` for TwistedSampler.

    The placements are enumerated (and thinned to `max_offsets` with one choice() draw of `rng`, numpy's global generator by default)
    exactly as generate_motif_index_mask does, the concatenated target is centred as TwistedSampler centres it, and both are uploaded
    once.  The forward launches genie_motif_potential on torch's current stream and keeps the gradient it computes; the backward
    scales it.  Nothing on the per-step path reads device memory from the host: var = xstart_variance(alphas_cumprod[step], tausq)
    stays on the device.

    `align='rigid'` guides with the superposed form instead (genie_motif_potential_rigid): every placement is compared to the motif
    in its best-fitting orientation (a proper rotation), so the orientation the motif file is written in no longer matters.  It needs
    at least 3 motif residues that are not collinear.  `locate(x)` reports, for either `align`, the best placement of every sample
    and its motif RMSD after optimal superposition.

    `groups` (one hashable label per segment, e.g. load_motif_groups of the problem file) makes it a multi-motif problem: the segments
    of one group keep their relative pose, different groups are independent bodies.  With two or more distinct labels every group is
    translated or superposed on its own (genie_motif_potential_grouped) while the placements stay joint; `locate` then also returns
    'group_rmsd' [B, G] and 'groups' (the labels, by first appearance).  `None` or one label is the single rigid motif above, the same
    entries and the same results."""

    def __init__(self, segments, n_res, alphas_cumprod, tausq=0.012, max_offsets=1000, rng=None, device='cuda', align='translation',
                 groups=None):
        if align not in ('translation', 'rigid'):
            raise ValueError("align must be 'translation' or 'rigid', got %r" % (align,))
        self.align = align
        segs = [torch.as_tensor(x, dtype=torch.float32).reshape(-1, 3) for x in segments]
        self.seg_len = [len(x) for x in segs]
        if not segs or min(self.seg_len) < 1:
            raise ValueError('the motif needs at least one segment of at least one residue')
        # the motif is validated on the host, once, before the device is looked at and before any placement is drawn
        self.groups = self.seg_group = None                              # (set for two or more groups)
        if groups is not None:
            labels, index = canonical_groups(groups, len(segs))
            if len(labels) > capi.MOTIF_MAX_GROUPS:
                raise ValueError('%d motif groups, at most %d are supported' % (len(labels), capi.MOTIF_MAX_GROUPS))
            if len(labels) > 1:
                self.groups, self.seg_group = labels, index
        if align == 'rigid' and self.groups is None:
            _check_superposable(torch.cat(segs), '')
        elif align == 'rigid':
            for g, label in enumerate(self.groups):
                _check_superposable(torch.cat([x for x, i in zip(segs, self.seg_group) if i == g]), ' in group %r' % (label,))
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.locs = get_all_motif_locations(self.n_res, self.seg_len, max_offsets, rng)
        if not self.locs:
            raise ValueError('a motif of %d residues does not fit in %d' % (sum(self.seg_len), self.n_res))
        starts = placement_starts(self.locs)
        _check_starts(starts, self.seg_len, self.n_res)
        self.P, self.S, self.M = starts.shape[0], starts.shape[1], sum(self.seg_len)
        self.starts = starts.to(self.device)
        self.seg_len_t = torch.tensor(self.seg_len, dtype=torch.int32, device=self.device)
        tgt = torch.cat(segs).to(self.device)
        self.target = (tgt - tgt.mean(dim=0, keepdim=True)).contiguous()      # (as TwistedSampler, smc.py:133-140)
        self.has_fit = self.M >= 3                                    # locate() superposes: three residues at least
        if self.groups is not None:
            self.G = len(self.groups)
            self.seg_group_t = torch.tensor(self.seg_group, dtype=torch.int32, device=self.device)
            self.has_fit = min(sum(n for n, g in zip(self.seg_len, self.seg_group) if g == k) for k in range(self.G)) >= 3

    def locate(self, x):
        """Where the motif is in x [B,N,3]: {'best' [B]: the placement that fits best after optimal superposition (the lowest
        index of equal ones), 'rmsd' [B]: its motif RMSD, 'starts', 'ends' [B,S]: the residues its segments occupy, 0-based, end
        inclusive (what the reference writes to motif_location.txt, unconditional_smc.py:334-343)}.  Always the superposed fit,
        whatever `align` guides with; tensors on the potential's device.  With motif groups every group is superposed on its own:
        'rmsd' is over all motif residues, and 'group_rmsd' [B, G] and 'groups' (the labels, in that order) are added."""
        if not self.has_fit:
            if self.groups is not None:
                raise ValueError('a superposed fit needs at least 3 motif residues in every group')
            raise ValueError('a superposed fit needs at least 3 motif residues, got %d' % self.M)
        best, rmsd, *group_rmsd = self._launch(self._checked(x), self._one, fit=True)      # (argmax of -q/2: var plays no part)
        starts = self.starts[best.long()].long()
        fit = {'best': best.long(), 'rmsd': rmsd, 'starts': starts, 'ends': starts + self.seg_len_t.long()[None] - 1}
        if self.groups is not None:
            fit.update(group_rmsd=group_rmsd[0], groups=list(self.groups))
        return fit

    def _entry(self, x, var, fit):
        """The C entry that (`groups`, `align`, `fit`) select, for x (f32, contiguous): (its name, the `work` bytes it needs, its
        arguments up to `work`, its outputs).  The outputs are freshly allocated, in the entry's order logp, grad, best, rmsd
        [, group_rmsd]: the fit when `fit` (always superposed), else the potential; the other half is None and passed as NULL."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        rigid = fit or self.align == 'rigid'
        head = (self._stream(), B, self.n_res, _ptr(x), self.P, self.S, self.M)
        tail = (_ptr(self.starts), _ptr(self.target), _ptr(var))
        if self.groups is not None:
            name, n_out = 'genie_motif_potential_grouped', 5
            need = self.lib.genie_motif_potential_grouped_work_bytes(B, self.P, self.G, int(rigid))
            args = head + (self.G, _ptr(self.seg_len_t), _ptr(self.seg_group_t)) + tail + (int(rigid),)
        elif rigid:
            name, n_out = 'genie_motif_potential_rigid', 4
            need = self.lib.genie_motif_potential_rigid_work_bytes(B, self.P)
            args = head + (_ptr(self.seg_len_t),) + tail
        else:
            name, n_out = 'genie_motif_potential', 2
            need = self.lib.genie_motif_potential_work_bytes(B, self.P)
            args = head + (_ptr(self.seg_len_t),) + tail
        if fit:
            outs = [None, None, torch.empty(B, dtype=torch.int32, device=x.device), torch.empty(B, **f32)]
            outs += [torch.empty(B, self.G, **f32)] if n_out == 5 else []
        else:
            outs = [torch.empty(B, **f32), torch.empty_like(x)] + [None] * (n_out - 2)
        return name, need, args + tuple(_ptr(t) for t in outs), outs

    def _launch(self, x, var, fit=False):
        """One call of the C entry on x (f32, contiguous): (best, rmsd[, group_rmsd]) when `fit`, else (logp, grad)."""
        name, need, args, outs = self._entry(x, var, fit)
        self._call(name, *args, *self._workspace(need))
        return tuple(t for t in outs if t is not None)


def load_restraints(path):
    """A restraint file -> [(i, j, lo, hi, weight), ...] for ShapePotential: one restraint per line, `i j lo hi [weight]`, residues
    0-based like the motif_locations files, distances in Angstrom, `inf` allowed for hi, weight 1 when omitted; `#` starts a comment,
    blank lines are ignored.  A bad line raises ValueError('<path>:<line number>: ...')."""
    out = []
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            fields = line.split('#', 1)[0].split()
            if not fields:
                continue
            if len(fields) not in (4, 5):
                raise ValueError('%s:%d: expected `i j lo hi [weight]`, got %d fields' % (path, number, len(fields)))
            try:
                i, j = int(fields[0]), int(fields[1])
                lo, hi = float(fields[2]), float(fields[3])
                weight = float(fields[4]) if len(fields) == 5 else 1.0
            except ValueError:
                raise ValueError('%s:%d: residues are integers, lo, hi and weight numbers: %r' % (path, number, line.strip())) from None
            out.append((i, j, lo, hi, weight))
    return out


def check_restraints(restraints, n_res):
    """The restraints of ShapePotential, validated on the host: [(i, j, lo, hi, weight), ...] with i != j, both in 0..n_res-1,
    0 <= lo <= hi (hi may be inf), weight finite and >= 0 (1 when omitted), no pair listed twice in either order."""
    import math
    out, seen = [], set()
    for k, r in enumerate(restraints):
        r = tuple(r)
        if len(r) not in (4, 5):
            raise ValueError('restraint %d: expected (i, j, lo, hi[, weight]), got %r' % (k, r))
        i, j = r[0], r[1]
        if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in (i, j)):
            raise ValueError('restraint %d: residues must be integers, got %r and %r' % (k, i, j))
        i, j, lo, hi, weight = int(i), int(j), float(r[2]), float(r[3]), float(r[4]) if len(r) == 5 else 1.0
        if i == j:
            raise ValueError('restraint %d: residue %d is restrained to itself' % (k, i))
        if not (0 <= i < n_res and 0 <= j < n_res):
            raise ValueError('restraint %d: residues %d and %d must lie in 0..%d' % (k, i, j, n_res - 1))
        if not (0 <= lo <= hi) or math.isinf(lo):
            raise ValueError('restraint %d: needs 0 <= lo <= hi with lo finite, got lo = %r, hi = %r' % (k, lo, hi))
        if not (math.isfinite(weight) and weight >= 0):
            raise ValueError('restraint %d: the weight must be finite and >= 0, got %r' % (k, weight))
        if (min(i, j), max(i, j)) in seen:
            raise ValueError('restraint %d: the pair (%d, %d) is listed twice' % (k, i, j))
        seen.add((min(i, j), max(i, j)))
        out.append((i, j, lo, hi, weight))
    return out


def restraint_table(restraints, n_res):
    """The per-residue table genie_shape_potential takes, as CPU tensors (offset int32 [n_res + 1], partner int32 [R2], lo, hi, weight
    f32 [R2]): every restraint at both of its residues, a residue's entries at offset[n] .. offset[n + 1] - 1 with ascending partners."""
    entries = sorted([(i, j, lo, hi, w) for i, j, lo, hi, w in restraints] + [(j, i, lo, hi, w) for i, j, lo, hi, w in restraints])
    offset = [0] * (n_res + 1)
    for e in entries:
        offset[e[0] + 1] += 1
    for n in range(n_res):
        offset[n + 1] += offset[n]
    f32 = lambda k: torch.tensor([e[k] for e in entries], dtype=torch.float32)      # noqa: E731
    return (torch.tensor(offset, dtype=torch.int32), torch.tensor([e[1] for e in entries], dtype=torch.int32), f32(2), f32(3), f32(4))


class ShapePotential(_HipPotential):
    """Shape guidance as one HIP pass (genie_shape_potential, csrc/shape_kernels.hip; include/genie_hip.h states the mathematics):
    `pot(x0 [B,N,3], step) -> log p [B]`, differentiable in x0, a drop-in `twisting_function` for TwistedSampler beside MotifPotential
    (SumPotential adds them).  Three terms, each a squared hinge in Angstrom:
      rog_max          a cap on the radius of gyration (None: off), weighted rog_weight;
      clash_distance   every pair of residues at least clash_separation apart in sequence closer than this (None: off), weighted
                       clash_weight;
      restraints       [(i, j, lo, hi[, weight]), ...], 0-based residues like the motif_locations files: the distance of i and j is
                       kept in lo..hi (hi may be inf, lo may be 0); load_restraints reads them from a file.
    log p = -(E_rog + E_clash + E_rst) / (2 var), var = xstart_variance(alphas_cumprod[step], tausq) computed on the device, so nothing
    on the per-step path reads device memory from the host; the forward keeps the gradient the kernel computes and the backward
    scales it.  The likelihood is unnormalised (the sampler only uses differences and normalised weights).

    The restraints are validated on the host (check_restraints) before the device is looked at; the per-residue table is built and
    uploaded once.  A potential with no term enabled is a ValueError.  `describe(x)` reports every sample of x: 'rog', 'min_distance'
    (over the eligible pairs; inf when there is none), 'n_clash' (int64), 'e_rog', 'e_clash', 'e_restraint' (the weighted energies,
    before the division by 2 var), 'n_violated' (int64), 'max_violation', [B] tensors on the potential's device.

    The defaults (tausq = 1 A^2, separation 2, weights 1) are design choices: no trained checkpoint is in the tree, so their effect on
    sample quality is unmeasured."""

    def __init__(self, n_res, alphas_cumprod, rog_max=None, rog_weight=1.0, clash_distance=None, clash_separation=2, clash_weight=1.0,
                 restraints=None, tausq=1.0, device='cuda'):
        import math
        self.n_res = int(n_res)
        if self.n_res < 1:
            raise ValueError('n_res must be at least 1, got %r' % (n_res,))
        if rog_max is None and clash_distance is None and not restraints:
            raise ValueError('no term enabled: give rog_max, clash_distance or restraints')
        for name, v in (('rog_max', rog_max), ('rog_weight', rog_weight), ('clash_distance', clash_distance), ('clash_weight', clash_weight)):
            if v is not None and not (math.isfinite(float(v)) and float(v) >= 0):
                raise ValueError('%s must be finite and >= 0, got %r' % (name, v))
        if isinstance(clash_separation, bool) or not isinstance(clash_separation, numbers.Integral) or clash_separation < 1:
            raise ValueError('clash_separation must be an integer >= 1, got %r' % (clash_separation,))
        if not (math.isfinite(float(tausq)) and float(tausq) > 0):
            raise ValueError('tausq must be finite and > 0, got %r' % (tausq,))
        # a term that is off is a weight of 0 to the entry
        self.rog_max, self.rog_weight = (0.0, 0.0) if rog_max is None else (float(rog_max), float(rog_weight))
        self.clash_distance, self.clash_weight = (0.0, 0.0) if clash_distance is None else (float(clash_distance), float(clash_weight))
        self.clash_separation = int(clash_separation)
        self.restraints = check_restraints(restraints or [], self.n_res)
        table = restraint_table(self.restraints, self.n_res)
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.R2 = int(table[1].numel())
        self.table = tuple(t.to(self.device) for t in table) if self.R2 else (None,) * 5

    def describe(self, x):
        """The report of every sample of x [B,N,3] (the class docstring), on the potential's device."""
        report, = self._launch(self._checked(x), self._one, report=True)                   # (the energies do not depend on var)
        return _decode_report(report, capi.SHAPE_REPORT, ('n_clash', 'n_violated'))

    def _launch(self, x, var, report=False):
        """One call of the C entry on x (f32, contiguous): (report [B, 8],) when `report`, else (logp, grad)."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        if report:
            outs = [None, None, torch.empty(B, len(capi.SHAPE_REPORT), **f32)]
        else:
            outs = [torch.empty(B, **f32), torch.empty_like(x), None]
        self._call('genie_shape_potential', self._stream(), B, self.n_res, _ptr(x), self.rog_max, self.rog_weight, self.clash_distance,
                   self.clash_separation, self.clash_weight, self.R2, *(_ptr(t) for t in self.table), _ptr(var), *(_ptr(t) for t in outs),
                   *self._workspace(self.lib.genie_shape_potential_work_bytes(B, self.n_res)))
        return tuple(t for t in outs if t is not None)


SS_CODES = {'-': 0, 'H': 1, 'E': 2}      # the int8 codes of genie_secstruct_potential's target
SS_LETTERS = 'CHE'                        # its assignment codes 0, 1, 2 as letters


def load_ss_target(path_or_string):
    """A secondary-structure blueprint for SecStructPotential, as a string over `HE-`: `H` helix, `E` extended, `-` or `C` free.
    The argument is the blueprint itself or the path of a file that holds it; in a file whitespace (line breaks included) is
    ignored and `#` starts a comment.  Anything else raises ValueError."""
    import os
    text, where = str(path_or_string), 'the blueprint'
    if os.path.isfile(text):
        where = text
        with open(text) as fh:
            text = ''.join(''.join(line.split('#', 1)[0].split()) for line in fh)
    else:
        text = ''.join(text.split())
    bad = sorted(set(text) - set('HEC-'))
    if bad:
        raise ValueError('%s: expected H, E and - (or C) only, got %r' % (where, ''.join(bad)))
    if not text:
        raise ValueError('%s is empty' % where)
    return text.replace('C', '-')


def ss_target_windows(target):
    """The number of five-residue windows a blueprint string targets: those whose residues are all H or all E."""
    return sum(1 for i in range(len(target) - 4) if target[i] in 'HE' and target[i:i + 5] == target[i] * 5)


def ss_string(codes):
    """A row of assignment codes (0 C, 1 H, 2 E) as a string over `HEC`."""
    return ''.join(SS_LETTERS[int(c)] for c in codes)


class SecStructPotential(_HipPotential):
    """Secondary-structure guidance as one HIP pass (genie_secstruct_potential, csrc/secstruct_kernels.hip; include/genie_hip.h
    states the mathematics): `pot(x0 [B,N,3], step) -> log p [B]`, differentiable in x0, a drop-in `twisting_function` for
    TwistedSampler beside MotifPotential and ShapePotential (SumPotential adds them).  Every five-residue window is scored against a
    helix and an extended class on its C-alpha distances i..i+2, i..i+3, i..i+4 and a chirality, with a rational score in (0, 1];
    the soft count of a class is the sum of its scores.  Three terms:
      helix     (min, max), fractions of the N - 4 windows: the soft helix count is kept between them by a squared hinge (None: off),
                weighted helix_weight;
      extended  the same for the extended class, weighted extended_weight;
      target    a blueprint string over `HE-` of length n_res (load_ss_target reads one): every window whose five residues are all
                H, or all E, is pulled to that class harmonically, weighted target_weight.
    log p = -(E_helix + E_extended + E_target) / (2 var), var = xstart_variance(alphas_cumprod[step], tausq) computed on the device,
    so nothing on the per-step path reads device memory from the host; the forward keeps the gradient the kernel computes and the
    backward scales it.  The likelihood is unnormalised.  `table` replaces the 16 class constants (capi.SECSTRUCT_TABLE: H mu, H
    sigma, E mu, E sigma over d2, d3, d4, chi).

    Everything is validated on the host before the device is looked at; a potential with no term enabled is a ValueError.
    `describe(x)` reports every sample of x: 'helix_content', 'extended_content' (soft count / windows), 'n_helix', 'n_extended'
    (residues of the hard assignment, int64), 'e_helix', 'e_extended', 'e_target' (the weighted energies, before the division by
    2 var), 'n_target_missed' (blueprint residues whose hard assignment differs, int64), [B] tensors on the potential's device;
    `assign(x)` is the hard assignment, int8 [B, N] with 0 C, 1 H, 2 E.

    "Extended" is local geometry only: there is no strand pairing (P-SEA's inter-strand criteria are out of scope), so it says that a
    stretch is straight and flat like a strand, not that it sits in a sheet: SheetPotential, below, scores pairing.  The defaults
    (the table, weights 1, tausq = 1 A^2, the rational score) are design choices: no trained checkpoint is in the tree, so their
    effect on sample quality is unmeasured."""

    def __init__(self, n_res, alphas_cumprod, helix=None, helix_weight=1.0, extended=None, extended_weight=1.0, target=None,
                 target_weight=1.0, table=None, tausq=1.0, device='cuda'):
        import math
        self.n_res = int(n_res)
        if self.n_res < 5:
            raise ValueError('n_res must be at least 5 (a window covers five residues), got %r' % (n_res,))
        if helix is None and extended is None and target is None:
            raise ValueError('no term enabled: give helix, extended or target')
        for name, v in (('helix_weight', helix_weight), ('extended_weight', extended_weight), ('target_weight', target_weight)):
            if not (math.isfinite(float(v)) and float(v) >= 0):
                raise ValueError('%s must be finite and >= 0, got %r' % (name, v))
        bounds = {}
        for name, v in (('helix', helix), ('extended', extended)):
            if v is None:
                bounds[name] = None
                continue
            try:
                lo, hi = (float(e) for e in v)
            except (TypeError, ValueError):
                raise ValueError('%s must be (min, max), got %r' % (name, v)) from None
            if not 0.0 <= lo <= hi <= 1.0:
                raise ValueError('%s needs 0 <= min <= max <= 1, got %r' % (name, v))
            bounds[name] = (lo, hi)
        if not (math.isfinite(float(tausq)) and float(tausq) > 0):
            raise ValueError('tausq must be finite and > 0, got %r' % (tausq,))
        table = capi.SECSTRUCT_TABLE if table is None else tuple(float(v) for v in (table.reshape(-1).tolist() if torch.is_tensor(table) else table))
        if len(table) != 16 or not all(math.isfinite(v) for v in table):
            raise ValueError('table must hold 16 finite numbers (H mu, H sigma, E mu, E sigma over d2, d3, d4, chi), got %r' % (table,))
        if min(table[4:8] + table[12:16]) <= 0:
            raise ValueError('every sigma of the table must be > 0, got %r' % (table[4:8] + table[12:16],))
        if target is not None:
            if not isinstance(target, str):
                raise ValueError('target must be a string over H, E and -, got %r' % (target,))
            if len(target) != self.n_res:
                raise ValueError('the target names %d residues, the potential has %d' % (len(target), self.n_res))
            if set(target) - set(SS_CODES):
                raise ValueError('target must hold H, E and - only, got %r' % ''.join(sorted(set(target) - set(SS_CODES))))
            if ss_target_windows(target) == 0:
                raise ValueError('the target has no run of five equal H or E residues: it targets no window')
        # a term that is off is a weight of 0 to the entry
        self.helix, self.helix_weight = ((0.0, 1.0), 0.0) if bounds['helix'] is None else (bounds['helix'], float(helix_weight))
        self.extended, self.extended_weight = ((0.0, 1.0), 0.0) if bounds['extended'] is None else (bounds['extended'], float(extended_weight))
        self.target, self.target_weight = target, (0.0 if target is None else float(target_weight))
        self.table = table
        self._table = (C.c_float * 16)(*table)
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.target_t = None if target is None else torch.tensor([SS_CODES[c] for c in target], dtype=torch.int8).to(self.device)

    def describe(self, x):
        """The report of every sample of x [B,N,3] (the class docstring), on the potential's device."""
        report, _ = self._launch(self._checked(x), self._one, report=True)                 # (the energies do not depend on var)
        return _decode_report(report, capi.SECSTRUCT_REPORT, ('n_helix', 'n_extended', 'n_target_missed'))

    def assign(self, x):
        """The hard assignment of every sample of x [B,N,3]: int8 [B, N], 0 C, 1 H, 2 E, on the potential's device."""
        return self._launch(self._checked(x), self._one, report=True)[1]

    def _launch(self, x, var, report=False):
        """One call of the C entry on x (f32, contiguous): (report [B, 8], assignment [B, N]) when `report`, else (logp, grad)."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        if report:
            outs = [None, None, torch.empty(B, len(capi.SECSTRUCT_REPORT), **f32), torch.empty(B, self.n_res, dtype=torch.int8, device=x.device)]
        else:
            outs = [torch.empty(B, **f32), torch.empty_like(x), None, None]
        self._call('genie_secstruct_potential', self._stream(), B, self.n_res, _ptr(x), self._table, self.helix[0], self.helix[1],
                   self.helix_weight, self.extended[0], self.extended[1], self.extended_weight, _ptr(self.target_t), self.target_weight,
                   _ptr(var), *(_ptr(t) for t in outs))
        return tuple(t for t in outs if t is not None)


def load_ladder(path):
    """A ladder file -> [(i, j, len, cls, weight), ...] for SheetPotential: one ladder per line, `i j len A|P [weight]`, residues
    0-based like the motif_locations files: class A pairs residue i + k with j - k, class P pairs i + k with j + k, k = 0..len-1;
    weight 1 when omitted; `#` starts a comment, blank lines are ignored.  A bad line raises ValueError('<path>:<line number>: ...')."""
    out = []
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            fields = line.split('#', 1)[0].split()
            if not fields:
                continue
            if len(fields) not in (4, 5):
                raise ValueError('%s:%d: expected `i j len A|P [weight]`, got %d fields' % (path, number, len(fields)))
            try:
                i, j, n = int(fields[0]), int(fields[1]), int(fields[2])
                weight = float(fields[4]) if len(fields) == 5 else 1.0
            except ValueError:
                raise ValueError('%s:%d: residues and len are integers, weight a number: %r' % (path, number, line.strip())) from None
            if fields[3] not in ('A', 'P'):
                raise ValueError('%s:%d: the class is A or P, got %r' % (path, number, fields[3]))
            out.append((i, j, n, fields[3], weight))
    return out


def check_ladder(ladder, n_res):
    """The ladder of SheetPotential, validated on the host: [(i, j, len, 'A'|'P'[, weight]), ...] -> its rungs [(i, j, cls, weight),
    ...] with i < j, in the order given.  Every rung's two centres lie in 1..n_res-2 and at least 3 apart, len >= 1, weight finite and
    >= 0 (1 when omitted), no rung listed twice in one class."""
    import math
    out, seen = [], set()
    for k, e in enumerate(ladder):
        e = tuple(e)
        if len(e) not in (4, 5):
            raise ValueError("ladder %d: expected (i, j, len, 'A'|'P'[, weight]), got %r" % (k, e))
        if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in e[:3]):
            raise ValueError('ladder %d: residues and len must be integers, got %r' % (k, e[:3]))
        i, j, n, cls, weight = int(e[0]), int(e[1]), int(e[2]), e[3], float(e[4]) if len(e) == 5 else 1.0
        if cls not in ('A', 'P'):
            raise ValueError("ladder %d: the class must be 'A' or 'P', got %r" % (k, cls))
        if n < 1:
            raise ValueError('ladder %d: len must be at least 1, got %d' % (k, n))
        if not (math.isfinite(weight) and weight >= 0):
            raise ValueError('ladder %d: the weight must be finite and >= 0, got %r' % (k, weight))
        for step in range(n):
            a, b = i + step, (j - step if cls == 'A' else j + step)
            a, b = min(a, b), max(a, b)
            if not (1 <= a and b <= n_res - 2):
                raise ValueError('ladder %d: the rung (%d, %d) needs both residues in 1..%d' % (k, a, b, n_res - 2))
            if b - a < 3:
                raise ValueError('ladder %d: the residues of the rung (%d, %d) are less than 3 apart' % (k, a, b))
            if (a, b, cls) in seen:
                raise ValueError('ladder %d: the rung (%d, %d) is listed twice in class %s' % (k, a, b, cls))
            seen.add((a, b, cls))
            out.append((a, b, cls, weight))
    return out


def ladder_table(rungs, n_res, table=None):
    """The per-residue table genie_sheet_potential takes, as CPU tensors (offset int32 [n_res + 1], partner int32 [L2], mu, coef f32
    [L2]), from check_ladder's rungs and the class table (mu_A, sigma_A, mu_P, sigma_P; capi.SHEET_TABLE by default): a rung's u is
    a third of three squared deviations, so every rung gives three harmonic terms coef (d - mu)^2 with coef = weight / (3 sigma^2);
    the terms of one class on one distance are merged; every term is listed at both of its residues, a residue's entries at
    offset[n] .. offset[n + 1] - 1 with ascending partners (class A before P on one partner).  A partner word carries
    capi.SHEET_PARALLEL for class P and capi.SHEET_RUNG where the term is the d0 of a listed rung."""
    table = capi.SHEET_TABLE if table is None else table
    terms = {}                                                      # (p, q, class index) -> [coef, is the d0 of a rung]
    for i, j, cls, w in rungs:
        c = 'AP'.index(cls)
        ends = ((i, j), (i - 1, j + 1), (i + 1, j - 1)) if c == 0 else ((i, j), (i - 1, j - 1), (i + 1, j + 1))
        for f, (p, q) in enumerate(ends):
            t = terms.setdefault((p, q, c), [0.0, False])
            t[0] += w / (3.0 * table[2 * c + 1] ** 2)
            t[1] = t[1] or f == 0
    entries = sorted([(p, q, c, v[0], v[1]) for (p, q, c), v in terms.items()] + [(q, p, c, v[0], v[1]) for (p, q, c), v in terms.items()])
    offset = [0] * (n_res + 1)
    for e in entries:
        offset[e[0] + 1] += 1
    for n in range(n_res):
        offset[n + 1] += offset[n]
    words = [e[1] | (capi.SHEET_PARALLEL if e[2] else 0) | (capi.SHEET_RUNG if e[4] else 0) for e in entries]
    f32 = lambda values: torch.tensor(values, dtype=torch.float32)      # noqa: E731
    return (torch.tensor(offset, dtype=torch.int32), torch.tensor(words, dtype=torch.int32), f32([table[2 * e[2]] for e in entries]),
            f32([e[3] for e in entries]))


class SheetPotential(_HipPotential):
    """Sheet guidance as one HIP pass (genie_sheet_potential, csrc/sheet_kernels.hip; include/genie_hip.h states the mathematics):
    `pot(x0 [B,N,3], step) -> log p [B]`, differentiable in x0, a drop-in `twisting_function` for TwistedSampler beside MotifPotential,
    ShapePotential and SecStructPotential (SumPotential adds them).  It is the strand pairing SecStructPotential's "extended" class
    does not have.  Every pair of interior residues at least `separation` apart is scored as an antiparallel and as a parallel rung
    on three C-alpha distances (the pair and its two neighbouring pairs) with a squared-rational score in (0, 1]; the soft rung count
    of a class is the sum of its scores.  Three terms:
      antiparallel  (min, max) in rungs per residue (an interior strand of a large sheet approaches 1; max may be inf): the soft
                    antiparallel count is kept between N min and N max by a squared hinge (None: off), weighted antiparallel_weight;
      parallel      the same for the parallel class, weighted parallel_weight;
      ladder        [(i, j, len, 'A'|'P'[, weight]), ...] (load_ladder reads them from a file): the listed rungs -- i + k with j - k
                    for A, with j + k for P, k = 0..len-1 -- are pulled to their class harmonically, weighted ladder_weight.
    log p = -(E_antiparallel + E_parallel + E_ladder) / (2 var), var = xstart_variance(alphas_cumprod[step], tausq) computed on the
    device, so nothing on the per-step path reads device memory from the host; the forward keeps the gradient the kernel computes and
    the backward scales it.  The likelihood is unnormalised.  `table` replaces the four class constants (capi.SHEET_TABLE: mu_A,
    sigma_A, mu_P, sigma_P), `separation` the smallest j - i of an antiparallel and of a parallel rung (both at least 3; the default
    5 for parallel keeps the (i, i+3) pairs of a helix out, which look parallel by C-alpha distance alone).

    Everything is validated on the host before the device is looked at; a potential with no term enabled is a ValueError.
    `describe(x)` reports every sample of x: 'antiparallel_content', 'parallel_content' (soft count / N), 'n_antiparallel',
    'n_parallel' (formed rungs: all three distances within one sigma, int64), 'n_paired' (residues in a formed rung, int64),
    'e_antiparallel', 'e_parallel', 'e_ladder' (the weighted energies, before the division by 2 var), 'n_ladder_missed' (listed rungs
    that are not formed, int64), [B] tensors on the potential's device; `pairs(x)` is int32 [B, N, 2]: every residue's partner in its
    best formed antiparallel (column 0) and parallel (column 1) rung, -1 for none.

    The defaults (the table, the separations, weights 1, tausq = 1 A^2, the squared-rational score) are design choices from ideal
    pleated-sheet geometry: no trained checkpoint is in the tree, so their effect on sample quality is unmeasured."""

    def __init__(self, n_res, alphas_cumprod, antiparallel=None, antiparallel_weight=1.0, parallel=None, parallel_weight=1.0, ladder=None,
                 ladder_weight=1.0, table=None, separation=(3, 5), tausq=1.0, device='cuda'):
        import math
        self.n_res = int(n_res)
        if self.n_res < 1:
            raise ValueError('n_res must be at least 1, got %r' % (n_res,))
        if antiparallel is None and parallel is None and not ladder:
            raise ValueError('no term enabled: give antiparallel, parallel or ladder')
        weights = dict(antiparallel_weight=antiparallel_weight, parallel_weight=parallel_weight, ladder_weight=ladder_weight)
        for name, v in weights.items():
            if not (math.isfinite(float(v)) and float(v) >= 0):
                raise ValueError('%s must be finite and >= 0, got %r' % (name, v))
        bounds = {}
        for name, v in (('antiparallel', antiparallel), ('parallel', parallel)):
            if v is None:
                bounds[name] = None
                continue
            try:
                lo, hi = (float(e) for e in v)
            except (TypeError, ValueError):
                raise ValueError('%s must be (min, max), got %r' % (name, v)) from None
            if not 0.0 <= lo <= hi or math.isinf(lo):
                raise ValueError('%s needs 0 <= min <= max with min finite, got %r' % (name, v))
            bounds[name] = (lo, hi)
        try:
            sep = tuple(separation)
        except TypeError:
            sep = ()
        if len(sep) != 2 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 3 for v in sep):
            raise ValueError('separation must be two integers >= 3 (antiparallel, parallel), got %r' % (separation,))
        if not (math.isfinite(float(tausq)) and float(tausq) > 0):
            raise ValueError('tausq must be finite and > 0, got %r' % (tausq,))
        if table is None:
            table = capi.SHEET_TABLE
        table = tuple(float(v) for v in (table.reshape(-1).tolist() if torch.is_tensor(table) else table))
        if len(table) != 4 or not all(math.isfinite(v) for v in table):
            raise ValueError('table must hold 4 finite numbers (mu_A, sigma_A, mu_P, sigma_P), got %r' % (table,))
        if min(table[1], table[3]) <= 0:
            raise ValueError('every sigma of the table must be > 0, got %r' % ((table[1], table[3]),))
        self.rungs = check_ladder(ladder or [], self.n_res)
        # a term that is off is a weight of 0 to the entry
        self.antiparallel, self.antiparallel_weight = \
            ((0.0, math.inf), 0.0) if bounds['antiparallel'] is None else (bounds['antiparallel'], float(antiparallel_weight))
        self.parallel, self.parallel_weight = \
            ((0.0, math.inf), 0.0) if bounds['parallel'] is None else (bounds['parallel'], float(parallel_weight))
        self.ladder_weight = float(ladder_weight) if self.rungs else 0.0
        self.table, self.separation = table, (int(sep[0]), int(sep[1]))
        lad = ladder_table(self.rungs, self.n_res, table)
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.L2 = int(lad[1].numel())
        self.ladder = tuple(t.to(self.device) for t in lad) if self.L2 else (None,) * 4

    def describe(self, x):
        """The report of every sample of x [B,N,3] (the class docstring), on the potential's device."""
        report, = self._launch(self._checked(x), self._one, want='report')                 # (the energies do not depend on var)
        return _decode_report(report, capi.SHEET_REPORT, capi.SHEET_COUNTS)

    def pairs(self, x):
        """Every residue's partners in every sample of x [B,N,3]: int32 [B, N, 2] (antiparallel, parallel; -1: none), on the
        potential's device."""
        return self._launch(self._checked(x), self._one, want='pairs')[0]

    def _launch(self, x, var, want='logp'):
        """One call of the C entry on x (f32, contiguous) for the outputs `want` names, the others passed as NULL: 'logp' gives (logp,
        grad), 'report' (report [B, 9],), 'pairs' (pairs [B, N, 2],)."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        outs = [None, None, None, None]
        if want == 'logp':
            outs[:2] = torch.empty(B, **f32), torch.empty_like(x)
        elif want == 'report':
            outs[2] = torch.empty(B, len(capi.SHEET_REPORT), **f32)
        else:
            outs[3] = torch.empty(B, self.n_res, 2, dtype=torch.int32, device=x.device)
        self._call('genie_sheet_potential', self._stream(), B, self.n_res, _ptr(x), *self.table, *self.separation, self.antiparallel[0],
                   self.antiparallel[1], self.antiparallel_weight, self.parallel[0], self.parallel[1], self.parallel_weight, self.L2,
                   *(_ptr(t) for t in self.ladder), self.ladder_weight, _ptr(var), *(_ptr(t) for t in outs),
                   *self._workspace(self.lib.genie_sheet_potential_work_bytes(B, self.n_res)))
        return tuple(t for t in outs if t is not None)


def parse_symmetry(symmetry):
    """A symmetry symbol -> (kind, n, units): 'C3' is ('C', 3, 3), 'D2' ('D', 2, 4), 'R4' ('R', 4, 4); n >= 2.  Anything else is a
    ValueError."""
    text = symmetry.strip().upper() if isinstance(symmetry, str) else ''
    if len(text) < 2 or text[0] not in 'CDR' or not text[1:].isdigit() or int(text[1:]) < 2:
        raise ValueError("symmetry must be C<n>, D<n> or R<n> with n >= 2 (a cyclic or dihedral group, n repeats), got %r" % (symmetry,))
    n = int(text[1:])
    return text[0], n, 2 * n if text[0] == 'D' else n


def symmetry_layout(symmetry, n_res, unit_length=None, linker=0, offset=0):
    """The units of a symmetric chain of n_res residues, validated on the host: (units U, unit length m).  Unit k starts at
    offset + k (m + linker) and offset + U m + (U - 1) linker <= n_res; `unit_length=None` divides what is left of n_res evenly among
    the units, or is a ValueError when that leaves a remainder.  Every generator of the symbol needs at least 3 pairs."""
    kind, n, units = parse_symmetry(symmetry)
    for name, v in (('n_res', n_res), ('linker', linker), ('offset', offset)) + ((('unit_length', unit_length),) if unit_length is not None else ()):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError('%s must be an integer, got %r' % (name, v))
    if n_res < 1 or linker < 0 or offset < 0:
        raise ValueError('needs n_res >= 1, linker >= 0 and offset >= 0, got %d, %d and %d' % (n_res, linker, offset))
    if unit_length is None:
        left = n_res - offset - (units - 1) * linker
        if left < units or left % units:
            raise ValueError('%d residues with offset %d and linker %d do not divide into %d equal units: give unit_length'
                             % (n_res, offset, linker, units))
        unit_length = left // units
    if unit_length < 1:
        raise ValueError('unit_length must be at least 1, got %d' % unit_length)
    if offset + units * unit_length + (units - 1) * linker > n_res:
        raise ValueError('%s with %d units of %d residues, linker %d and offset %d needs %d residues, the chain has %d'
                         % (symmetry, units, unit_length, linker, offset, offset + units * unit_length + (units - 1) * linker, n_res))
    pairs = (n - 1) * unit_length if kind == 'R' else units * unit_length
    if pairs < 3:
        raise ValueError('%s with units of %d residues has a generator of %d pairs: a superposition needs 3' % (symmetry, unit_length, pairs))
    return units, int(unit_length)


def symmetry_generators(symmetry, unit_length, n_res, linker=0, offset=0):
    """The generators of a symmetric layout (include/genie_hip.h states them) as [(src, dst), ...] lists of residue indices, one pair
    of lists per generator: one for C<n> (unit k onto k + 1 mod n) and R<n> (unit k onto k + 1, k = 0..n-2), two for D<n> (the n-fold,
    which turns the second ring the other way, and the two-fold that swaps the rings).  The layout is validated by symmetry_layout."""
    kind, n, _ = parse_symmetry(symmetry)
    units, m = symmetry_layout(symmetry, n_res, unit_length, linker, offset)
    res = lambda k, a: offset + k * (m + linker) + a      # noqa: E731
    if kind == 'R':
        maps = [[(k, k + 1) for k in range(n - 1)]]
    elif kind == 'C':
        maps = [[(k, (k + 1) % n) for k in range(n)]]
    else:
        maps = [[(k, (k + 1) % n) for k in range(n)] + [(n + k, n + (k - 1) % n) for k in range(n)],
                [(k, n + k) for k in range(n)] + [(n + k, k) for k in range(n)]]
    return [([res(k, a) for k, _ in mp for a in range(m)], [res(j, a) for _, j in mp for a in range(m)]) for mp in maps]


def check_generators(generators, n_res):
    """The generators of SymmetryPotential, validated on the host: 1..capi.SYMMETRY_MAX_GENERATORS of them, each (src, dst) with two
    lists of L >= 3 integers in 0..n_res-1, src_i != dst_i, no residue a source twice and none a destination twice.  Returns them as
    [(src, dst), ...] lists of ints."""
    try:
        generators = [tuple(g) for g in generators]
    except TypeError:
        raise ValueError('generators must be a list of (src, dst) pairs of index lists, got %r' % (generators,)) from None
    if not 1 <= len(generators) <= capi.SYMMETRY_MAX_GENERATORS:
        raise ValueError('needs 1..%d generators, got %d' % (capi.SYMMETRY_MAX_GENERATORS, len(generators)))
    out = []
    for k, g in enumerate(generators):
        if len(g) != 2:
            raise ValueError('generator %d: expected (src, dst), got %d entries' % (k, len(g)))
        src, dst = (v.tolist() if torch.is_tensor(v) else list(v) for v in g)
        if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in src + dst):
            raise ValueError('generator %d: residues must be integers' % k)
        if len(src) != len(dst) or len(src) < 3:
            raise ValueError('generator %d: needs as many sources as destinations and at least 3 pairs, got %d and %d' % (k, len(src), len(dst)))
        if not all(0 <= v < n_res for v in src + dst):
            raise ValueError('generator %d: residues must lie in 0..%d' % (k, n_res - 1))
        if any(a == b for a, b in zip(src, dst)):
            raise ValueError('generator %d: a residue is mapped to itself' % k)
        if len(set(src)) != len(src) or len(set(dst)) != len(dst):
            raise ValueError('generator %d: a residue is a source twice or a destination twice' % k)
        out.append(([int(v) for v in src], [int(v) for v in dst]))
    return out


def partner_table(generators, n_res):
    """The per-residue table genie_symmetry_potential takes, a CPU tensor int32 [G, 2, n_res]: [g][0][i] the residue i maps to as a
    source of generator g, [g][1][i] the residue that maps to i, -1 for none."""
    table = torch.full((len(generators), 2, n_res), -1, dtype=torch.int32)
    for g, (src, dst) in enumerate(generators):
        table[g, 0, src] = torch.tensor(dst, dtype=torch.int32)
        table[g, 1, dst] = torch.tensor(src, dtype=torch.int32)
    return table


class SymmetryPotential(_HipPotential):
    """Symmetry guidance as one HIP pass (genie_symmetry_potential, csrc/symmetry_kernels.hip; include/genie_hip.h states the
    mathematics): `pot(x0 [B,N,3], step) -> log p [B]`, differentiable in x0, a drop-in `twisting_function` for TwistedSampler beside
    the other built-in potentials (SumPotential adds them).  The chain holds U units of `unit_length` residues, unit k starting at
    offset + k (unit_length + linker); `symmetry` names how they repeat:
      'C<n>'  n units related by an n-fold axis: a cyclic oligomer, or a closed single-chain toroid;
      'D<n>'  2 n units, two rings of n related by a two-fold: a dihedral oligomer;
      'R<n>'  n units that follow one another by one screw motion: an open repeat protein.
    Every generator of the symbol maps units onto units; its energy is the squared deviation left after the best proper rotation and
    translation superposes the sources on their destinations.  log p = -weight sum_g w_g E_g / (2 var), var =
    xstart_variance(alphas_cumprod[step], tausq) computed on the device, so nothing on the per-step path reads device memory from the
    host; the forward keeps the gradient the kernel computes and the backward scales it.  The likelihood is unnormalised.  Residues in
    no unit (before `offset`, in a linker, after the last unit) are free: their gradient is exactly 0.
    `unit_length=None` divides what is left of n_res evenly (a ValueError when it does not divide).  `generators=[(src, dst), ...]`
    takes explicit index lists instead of a symbol (check_generators' rules); `generator_weights` the w_g (1 each by default).

    Everything is validated on the host before the device is looked at.  `describe(x)` reports every sample of x with the names of
    capi.SYMMETRY_REPORT: 'e_symmetry' (the weighted energy, before the division by 2 var), 'symmetry_rmsd' (over all pairs of all
    generators), and per generator slot 'rmsd_g', 'angle_g' (degrees, 0..180; 360 / n for a closed C<n>, the twist of a repeat) and
    'rise_g' (Angstrom along the axis; 0 for a closed ring, the rise of a repeat), zeros for an unused slot: [B] tensors on the
    potential's device.  `chain_lengths()` is [unit_length] * U, what UnconditionalSampler takes as params['chain_lengths'] to emit
    the units as separate chains; it needs a symbol with linker 0, offset 0 and U unit_length = n_res.

    The defaults (tausq = 1 A^2, weights 1) are design choices: no trained checkpoint is in the tree, so their effect on sample quality
    is unmeasured.  Units can satisfy the term by lying on top of each other, which a ShapePotential's clash_distance prevents; its
    rog_max over the assembly keeps separate chains together."""

    def __init__(self, n_res, alphas_cumprod, symmetry=None, unit_length=None, linker=0, offset=0, generators=None, weight=1.0,
                 generator_weights=None, tausq=1.0, device='cuda'):
        import math
        if isinstance(n_res, bool) or not isinstance(n_res, numbers.Integral) or n_res < 1:
            raise ValueError('n_res must be an integer >= 1, got %r' % (n_res,))
        if (symmetry is None) == (generators is None):
            raise ValueError('give either symmetry (C<n>, D<n>, R<n>) or generators')
        self.symmetry = self.units = self.unit_length = None
        self.linker, self.offset = linker, offset
        if symmetry is not None:
            self.units, self.unit_length = symmetry_layout(symmetry, n_res, unit_length, linker, offset)
            self.symmetry = symmetry.strip().upper()
            generators = symmetry_generators(symmetry, self.unit_length, n_res, linker, offset)
        elif unit_length is not None or linker != 0 or offset != 0:
            raise ValueError('unit_length, linker and offset describe the layout of a symmetry symbol, not of explicit generators')
        self.generators = check_generators(generators, int(n_res))
        G = len(self.generators)
        if not (math.isfinite(float(weight)) and float(weight) >= 0):
            raise ValueError('weight must be finite and >= 0, got %r' % (weight,))
        try:
            gw = [1.0] * G if generator_weights is None else [float(v) for v in generator_weights]
        except (TypeError, ValueError):
            raise ValueError('generator_weights must hold %d numbers, got %r' % (G, generator_weights)) from None
        if len(gw) != G or not all(math.isfinite(v) and v >= 0 for v in gw):
            raise ValueError('generator_weights must hold %d finite numbers >= 0, got %r' % (G, generator_weights))
        if not (math.isfinite(float(tausq)) and float(tausq) > 0):
            raise ValueError('tausq must be finite and > 0, got %r' % (tausq,))
        self.weight, self.generator_weights = float(weight), tuple(gw)
        table = partner_table(self.generators, int(n_res))
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.G = G
        self.partner = table.to(self.device).contiguous()

    def chain_lengths(self):
        """[unit_length] * U: the units as the chains of params['chain_lengths'].  A layout with a linker, an offset or residues after
        the last unit has residues in no chain, and explicit generators have no units: a ValueError."""
        if self.symmetry is None:
            raise ValueError('explicit generators have no units to emit as chains')
        if self.linker != 0 or self.offset != 0 or self.units * self.unit_length != self.n_res:
            raise ValueError('the units are chains only with linker 0, offset 0 and units * unit_length = n_res: %d units of %d, linker %d, '
                             'offset %d in %d residues' % (self.units, self.unit_length, self.linker, self.offset, self.n_res))
        return [self.unit_length] * self.units

    def describe(self, x):
        """The report of every sample of x [B,N,3] (the class docstring), on the potential's device."""
        report, = self._launch(self._checked(x), self._one, report=True)                   # (the energies do not depend on var)
        return _decode_report(report, capi.SYMMETRY_REPORT, ())

    def _launch(self, x, var, report=False):
        """One call of the C entry on x (f32, contiguous): (report [B, 8],) when `report`, else (logp, grad)."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        if report:
            outs = [None, None, torch.empty(B, len(capi.SYMMETRY_REPORT), **f32)]
        else:
            outs = [torch.empty(B, **f32), torch.empty_like(x), None]
        w = [self.weight * v for v in self.generator_weights] + [0.0]
        self._call('genie_symmetry_potential', self._stream(), B, self.n_res, _ptr(x), self.G, _ptr(self.partner), w[0], w[1], _ptr(var),
                   *(_ptr(t) for t in outs), *self._workspace(self.lib.genie_symmetry_potential_work_bytes(B, self.n_res)))
        return tuple(t for t in outs if t is not None)


def load_target(path, chains=None):
    """The fixed target of a BinderPotential from a PDB file (plain or .gz): the C-alpha atoms of the chains named in `chains` (a
    string of chain letters such as 'AB'; None: every chain), in file order, as (xyz float64 [M, 3] in the file's frame, labels
    [(chain, resseq), ...] one per residue, chain_lengths [one per run of a chain letter], aatype int64 [M] residue-type indices in
    features.RESTYPES' order, 0 (ALA) for a residue name outside the twenty).  features.parse_pdb drops the residue numbers a hotspot
    is named by, so this is a reader of its own over the same columns.  A file with no C-alpha atom of the chosen chains, and a chosen
    chain the file does not have, are ValueErrors."""
    import gzip
    from .features import RESTYPE_ORDER, _RESTYPE_3_TO_1
    if chains is not None and (not isinstance(chains, str) or not chains or len(set(chains)) != len(chains)):
        raise ValueError('chains must be a string of distinct chain letters such as "AB", got %r' % (chains,))
    xyz, labels, lengths, aatype, current, seen = [], [], [], [], None, set()
    with (gzip.open(path, 'rt') if str(path).endswith('.gz') else open(path, 'r')) as fh:
        for line in fh:
            if not (line.startswith('ATOM') and line[13:15].strip() == 'CA'):
                continue
            chain = line[21]
            seen.add(chain)
            if chains is not None and chain not in chains:
                current = None
                continue
            if chain != current:
                lengths.append(0)
                current = chain
            lengths[-1] += 1
            labels.append((chain, int(line[22:26])))
            aatype.append(RESTYPE_ORDER.get(_RESTYPE_3_TO_1.get(line[17:20], 'A'), 0))
            xyz.append([float(line[30:38]), float(line[38:46]), float(line[46:54])])
    missing = [c for c in (chains or '') if c not in seen]
    if missing:
        raise ValueError('%s has no C-alpha atom of chain(s) %s (it has %s)' % (path, ', '.join(missing), ', '.join(sorted(seen)) or 'none'))
    if not xyz:
        raise ValueError('%s has no C-alpha ATOM record' % (path,))
    return torch.tensor(xyz, dtype=torch.float64), labels, lengths, torch.tensor(aatype, dtype=torch.int64)


def parse_hotspots(spec, labels):
    """Hotspot residues named by chain letter and residue number, `A45,A46,B12` (commas or whitespace between tokens), or a file of
    such tokens in which `#` starts a comment -> their sorted distinct indices into `labels` (load_target's).  A token that names no
    residue of the target, that names more than one, that does not parse or that is given twice is a ValueError naming it; so are
    more than capi.BINDER_MAX_HOTSPOTS of them."""
    import os
    import re
    if not isinstance(spec, str):
        raise ValueError('hotspots must be a string such as "A45,A46" or a file of such tokens, got %r' % (spec,))
    if os.path.isfile(spec):
        with open(spec) as fh:
            spec = ' '.join(line.split('#', 1)[0] for line in fh)
    index, out = {}, []
    for i, label in enumerate(labels):
        index.setdefault((label[0], int(label[1])), []).append(i)
    for token in [t for t in re.split(r'[,\s]+', spec) if t]:
        m = re.fullmatch(r'(\S)(-?\d+)', token)
        if m is None:
            raise ValueError('hotspot %r is not a chain letter followed by a residue number' % token)
        found = index.get((m.group(1), int(m.group(2))), [])
        if len(found) != 1:
            raise ValueError('hotspot %r names %s residue of the target' % (token, 'no' if not found else 'more than one'))
        if found[0] in out:
            raise ValueError('hotspot %r is given twice' % token)
        out.append(found[0])
    if len(out) > capi.BINDER_MAX_HOTSPOTS:
        raise ValueError('at most %d hotspots, got %d' % (capi.BINDER_MAX_HOTSPOTS, len(out)))
    return sorted(out)


def place_target(xyz, hotspots, standoff):
    """The target moved, by a pure translation, so that the sampler's origin -- where designs are born -- lies `standoff` Angstrom
    outside the hotspot patch: with t the target's centroid, h the hotspots' and u = (h - t) / |h - t|, every atom moves by
    -(h + standoff u).  The hotspot centroid then sits at -standoff u and the target's behind it on the same ray.  No rotation.
    `standoff=None` leaves the file's frame alone (a float64 copy).  No hotspots, |h - t| < 1e-3 A (no direction to step out in) and a
    negative or non-finite standoff are ValueErrors."""
    import math
    xyz = torch.as_tensor(xyz, dtype=torch.float64).clone()
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError('the target must be [M, 3] with M >= 1, got %s' % (tuple(xyz.shape),))
    if standoff is None:
        return xyz
    if not (math.isfinite(float(standoff)) and float(standoff) >= 0):
        raise ValueError('standoff must be finite and >= 0, got %r' % (standoff,))
    hotspots = list(hotspots) if hotspots is not None else []
    if not hotspots:
        raise ValueError('a standoff needs hotspots: they say on which side of the target the design starts')
    t, h = xyz.mean(dim=0), xyz[hotspots].mean(dim=0)
    gap = float((h - t).norm())
    if gap < 1e-3:
        raise ValueError('the hotspot centroid is %.1e A from the target centroid: no direction to step out in' % gap)
    return xyz - (h + float(standoff) * (h - t) / gap)


def check_hotspots(hotspots, n_target):
    """Hotspot indices as a sorted list of distinct integers in 0..n_target-1, at most capi.BINDER_MAX_HOTSPOTS of them; a ValueError
    otherwise."""
    try:
        out = [h for h in (hotspots.tolist() if torch.is_tensor(hotspots) else list(hotspots if hotspots is not None else []))]
    except TypeError:
        raise ValueError('hotspots must be a list of target indices, got %r' % (hotspots,)) from None
    for h in out:
        if isinstance(h, bool) or not isinstance(h, numbers.Integral) or not 0 <= h < n_target:
            raise ValueError('hotspot %r is not an integer in 0..%d' % (h, n_target - 1))
    if len(set(out)) != len(out):
        raise ValueError('a hotspot is listed twice: %r' % (out,))
    if len(out) > capi.BINDER_MAX_HOTSPOTS:
        raise ValueError('at most %d hotspots, got %d' % (capi.BINDER_MAX_HOTSPOTS, len(out)))
    return sorted(int(h) for h in out)


BINDER_MAX_TARGET = 12714       # the longest target whose staging fits in the kernel's 160 KiB of LDS (include/genie_hip.h)


class BinderPotential(_HipPotential):
    """Binder guidance as one HIP pass (genie_binder_potential, csrc/binder_kernels.hip; include/genie_hip.h states the mathematics):
    `pot(x0 [B,N,3], step) -> log p [B]`, differentiable in x0, a drop-in `twisting_function` for TwistedSampler beside the other
    built-in potentials (SumPotential adds them).  It is the one potential that looks at something that is not being sampled:
    `target` [M, 3], fixed C-alpha coordinates in the frame the sampler works in (load_target reads them from a file, place_target
    moves them so that the origin, where designs are born, faces the hotspots).  Three terms, each a squared hinge:
      clash_distance   every design-target pair closer than this many Angstrom (None: off), weighted clash_weight;
      contacts         (min, max): the soft number of contacts C = sum over pairs of 1 / (1 + (d / contact_distance)^6) is kept in
                       that range (None: off; max may be inf), weighted contacts_weight;
      hotspots         target indices (None or empty: off): each hotspot's own soft contacts c_h, summed over the design, are kept
                       at or above hotspot_contacts, weighted hotspot_weight.
    log p = -(E_clash + E_contact + E_hot) / (2 var), var = xstart_variance(alphas_cumprod[step], tausq) computed on the device, so
    nothing on the per-step path reads device memory from the host; the forward keeps the gradient the kernel computes and the
    backward scales it.  The likelihood is unnormalised.

    Everything is validated on the host before the device is looked at; a potential with no term enabled is a ValueError.  The target
    and the hotspot list are uploaded once.  `describe(x)` reports every sample of x with the names of capi.BINDER_REPORT: 'contacts'
    (C), 'n_contacts' (pairs closer than contact_distance), 'n_interface' (design residues in such a pair), 'target_min_distance',
    'n_target_clash' (pairs closer than clash_distance), 'n_hotspots_contacted' (int64 counts), 'e_target_clash', 'e_contact',
    'e_hotspot' (the weighted energies, before the division by 2 var): [B] tensors on the potential's device.
    `hotspot_contacts_of(x)` is [B, H], the c_h in the order of `hotspots` (ascending target index).

    The defaults (tausq = 1 A^2, contact_distance 8 A, one soft contact per hotspot, weights 1) are design choices: no trained
    checkpoint is in the tree, so their effect on sample quality is unmeasured.  The target does not rotate, no design residue is
    exempt from or singled out for the interface, only C-alpha atoms are seen, and the denoiser never sees the target."""

    def __init__(self, n_res, alphas_cumprod, target, hotspots=None, clash_distance=None, clash_weight=1.0, contact_distance=8.0,
                 contacts=None, contacts_weight=1.0, hotspot_contacts=1.0, hotspot_weight=1.0, tausq=1.0, device='cuda'):
        import math
        if isinstance(n_res, bool) or not isinstance(n_res, numbers.Integral) or n_res < 1:
            raise ValueError('n_res must be an integer >= 1, got %r' % (n_res,))
        try:
            y = torch.as_tensor(target).detach().to(dtype=torch.float32, device='cpu')
        except (TypeError, ValueError, RuntimeError):
            raise ValueError('target must be [M, 3] coordinates, got %r' % (type(target),)) from None
        if y.dim() != 2 or y.shape[1] != 3 or y.shape[0] < 1:
            raise ValueError('target must be [M, 3] with M >= 1, got %s' % (tuple(y.shape),))
        if y.shape[0] > BINDER_MAX_TARGET:
            raise ValueError('target has %d residues, at most %d fit in the LDS of the kernel' % (y.shape[0], BINDER_MAX_TARGET))
        if not bool(torch.isfinite(y).all()):
            raise ValueError('target has a coordinate that is not finite')
        self.hotspots = check_hotspots(hotspots, int(y.shape[0]))
        for name, v in (('clash_distance', clash_distance), ('clash_weight', clash_weight), ('contact_distance', contact_distance),
                        ('contacts_weight', contacts_weight), ('hotspot_contacts', hotspot_contacts), ('hotspot_weight', hotspot_weight)):
            if v is not None and not (_is_scalar(v) and math.isfinite(float(v)) and float(v) >= 0):
                raise ValueError('%s must be finite and >= 0, got %r' % (name, v))
        if contact_distance is None or not float(contact_distance) > 0:
            raise ValueError('contact_distance must be > 0, got %r' % (contact_distance,))
        if contacts is not None:
            try:
                lo, hi = (float(v) for v in contacts)
            except (TypeError, ValueError):
                raise ValueError('contacts must be (min, max), got %r' % (contacts,)) from None
            if not (math.isfinite(lo) and lo >= 0 and hi >= lo):
                raise ValueError('contacts must be (min, max) with 0 <= min <= max, min finite, got %r' % (contacts,))
        if not (_is_scalar(tausq) and math.isfinite(float(tausq)) and float(tausq) > 0):
            raise ValueError('tausq must be finite and > 0, got %r' % (tausq,))
        if clash_distance is None and contacts is None and not self.hotspots:
            raise ValueError('no term enabled: give clash_distance, contacts or hotspots')
        # a term that is off is a weight of 0 to the entry
        self.clash_distance, self.clash_weight = (0.0, 0.0) if clash_distance is None else (float(clash_distance), float(clash_weight))
        self.contact_distance = float(contact_distance)
        self.contacts, self.contacts_weight = ((0.0, math.inf), 0.0) if contacts is None else ((lo, hi), float(contacts_weight))
        self.hotspot_contacts, self.hotspot_weight = float(hotspot_contacts), float(hotspot_weight) if self.hotspots else 0.0
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.M, self.H = int(y.shape[0]), len(self.hotspots)
        self.target = y.contiguous().to(self.device)
        self.hotspot_index = torch.tensor(self.hotspots, dtype=torch.int32).to(self.device) if self.H else None

    def describe(self, x):
        """The report of every sample of x [B,N,3] (the class docstring), on the potential's device."""
        report, = self._launch(self._checked(x), self._one, want='report')               # (the energies do not depend on var)
        return _decode_report(report, capi.BINDER_REPORT, capi.BINDER_COUNTS)

    def hotspot_contacts_of(self, x):
        """[B, H] float32 on the potential's device: every hotspot's soft contacts c_h with every sample of x [B,N,3]."""
        x = self._checked(x)
        if not self.H:
            return torch.zeros(x.shape[0], 0, dtype=torch.float32, device=x.device)
        return self._launch(x, self._one, want='hotspots')[0]

    def _launch(self, x, var, want='logp'):
        """One call of the C entry on x (f32, contiguous): (logp, grad), (report [B, 9],) or (hotspot_out [B, H],) as `want` says."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        outs = {'logp': lambda: [torch.empty(B, **f32), torch.empty_like(x), None, None],
                'report': lambda: [None, None, torch.empty(B, len(capi.BINDER_REPORT), **f32), None],
                'hotspots': lambda: [None, None, None, torch.empty(B, self.H, **f32)]}[want]()
        self._call('genie_binder_potential', self._stream(), B, self.n_res, _ptr(x), self.M, _ptr(self.target), self.H,
                   _ptr(self.hotspot_index), self.clash_distance, self.clash_weight, self.contact_distance, self.contacts[0],
                   self.contacts[1], self.contacts_weight, self.hotspot_contacts, self.hotspot_weight, _ptr(var),
                   *(_ptr(t) for t in outs), *self._workspace(self.lib.genie_binder_potential_work_bytes(B, self.n_res, self.H)))
        return tuple(t for t in outs if t is not None)


def check_anchor_index(anchor_index, n_anchors, n_res):
    """Anchor residues as an int32 tensor [rows, n_anchors] -- one row for every particle, or [n_anchors] for one row that serves all
    -- of integers in 0..n_res-1, distinct within a row; a ValueError otherwise."""
    try:
        rows = anchor_index.tolist() if torch.is_tensor(anchor_index) else list(anchor_index)
        rows = [list(r) for r in rows] if rows and isinstance(rows[0], (list, tuple)) else [list(rows)]
    except TypeError:
        raise ValueError('anchor_index must be a list of design residue indices, got %r' % (anchor_index,)) from None
    for row in rows:
        if len(row) != n_anchors:
            raise ValueError('anchor_index has %d residues in a row, anchor_xyz has %d' % (len(row), n_anchors))
        for i in row:
            if isinstance(i, bool) or not isinstance(i, numbers.Integral) or not 0 <= i < n_res:
                raise ValueError('anchor_index %r is not an integer in 0..%d' % (i, n_res - 1))
        if len(set(row)) != len(row):
            raise ValueError('anchor_index lists a residue twice: %r' % (row,))
    return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), n_anchors)


class ContextPotential(_HipPotential):
    """Context guidance as one HIP entry (genie_context_potential, csrc/context_kernels.hip; include/genie_hip.h states the
    mathematics): `pot(x0 [B,N,3], step) -> log p [B]`, differentiable in x0, a drop-in `twisting_function` for TwistedSampler beside
    the other built-in potentials (SumPotential adds them).  A context is the binding partner of a motif: `context` [C, 3], C-alpha
    coordinates in the same frame as `anchor_xyz` [A, 3], the motif residues it is tied to (the motif file's frame; this class keeps
    its own copies and does not depend on how MotifPotential centres its target).  For every particle the anchors are superposed on
    the design residues that hold them, the fitted rigid motion places the context, and the placed context is scored against the rest
    of the design -- the anchors sit out -- with BinderPotential's clash and contact terms:
      clash_distance   every design-context pair closer than this many Angstrom (None: off), weighted clash_weight;
      contacts         (min, max): the soft number of contacts sum 1 / (1 + (d / contact_distance)^6) is kept in that range (None:
                       off; max may be inf), weighted contacts_weight.
    log p = -(E_clash + E_contact) / (2 var), var = xstart_variance(alphas_cumprod[step], tausq) computed on the device.  The gradient
    is exact, the part that flows through the fitted rotation included: the partner is a long lever on a small motif.

    Exactly one of two arguments says where the anchors are:
      anchor_index     A design residues (or one row of A per particle, [B, A]): a known placement;
      motif            a MotifPotential, with `segments`, the indices of its segments that `anchor_xyz` lists, in order (None: all of
                       them; with motif groups, the segments of exactly one group).  Every call first runs the motif's superposed fit
                       (MotifPotential.locate's) and takes the anchors from each particle's best placement, with device tensor
                       operations.  Which placement that is is held fixed within a call: the function is piecewise in x across a
                       change of best placement, as AlignedFoldPotential is across a change of alignment.
    Nothing on the per-step path reads device memory from the host.

    Everything is validated on the host before the device is looked at; a potential with no term enabled and collinear anchors are
    ValueErrors.  `describe(x)` reports every sample of x with the names of capi.CONTEXT_REPORT: 'context_contacts',
    'n_context_contacts', 'n_context_interface', 'context_min_distance', 'n_context_clash' (int64 counts), 'anchor_rmsd' (of the
    superposition), 'e_context_clash', 'e_context_contact' (the weighted energies, before the division by 2 var).  `pose_of(x)` is
    (R [B,3,3], t [B,3]) with placed = R y + t, `placed_context(x)` the placed context [B, C, 3].

    The defaults (tausq = 1 A^2, contact_distance 8 A, weights 1) are design choices: no trained checkpoint is in the tree, so their
    effect on sample quality is unmeasured.  Only C-alpha atoms are seen, and the denoiser never sees the context."""

    def __init__(self, n_res, alphas_cumprod, anchor_xyz, context, anchor_index=None, motif=None, segments=None, clash_distance=None,
                 clash_weight=1.0, contact_distance=8.0, contacts=None, contacts_weight=1.0, tausq=1.0, device='cuda'):
        import math
        if isinstance(n_res, bool) or not isinstance(n_res, numbers.Integral) or n_res < 1:
            raise ValueError('n_res must be an integer >= 1, got %r' % (n_res,))
        coords = {}
        for name, v, low in (('anchor_xyz', anchor_xyz, 3), ('context', context, 1)):
            try:
                c = torch.as_tensor(v).detach().to(dtype=torch.float32, device='cpu')
            except (TypeError, ValueError, RuntimeError):
                raise ValueError('%s must be [n, 3] coordinates, got %r' % (name, type(v))) from None
            if c.dim() != 2 or c.shape[1] != 3 or c.shape[0] < low:
                raise ValueError('%s must be [n, 3] with n >= %d, got %s' % (name, low, tuple(c.shape)))
            if not bool(torch.isfinite(c).all()):
                raise ValueError('%s has a coordinate that is not finite' % name)
            coords[name] = c.contiguous()
        t, y = coords['anchor_xyz'], coords['context']
        if t.shape[0] > n_res:
            raise ValueError('anchor_xyz has %d residues, the design %d' % (t.shape[0], n_res))
        if y.shape[0] > capi.CONTEXT_MAX_ATOMS:
            raise ValueError('context has %d atoms, at most %d fit in the LDS of the kernel' % (y.shape[0], capi.CONTEXT_MAX_ATOMS))
        try:
            _check_superposable(t, ' of anchor_xyz')
        except ValueError as e:
            raise ValueError('anchor_xyz: %s' % e) from None
        if (anchor_index is None) == (motif is None):
            raise ValueError('give exactly one of anchor_index and motif')
        if motif is None and segments is not None:
            raise ValueError('segments goes with motif')
        self.motif = motif
        if motif is None:
            rows = check_anchor_index(anchor_index, int(t.shape[0]), n_res)
        else:
            if not isinstance(motif, MotifPotential):
                raise ValueError('motif must be a MotifPotential, got %r' % (type(motif),))
            if motif.n_res != n_res:
                raise ValueError('motif places its segments in %d residues, n_res is %d' % (motif.n_res, n_res))
            if not motif.has_fit:
                raise ValueError('motif has no superposed fit (3 motif residues at least, in every group)')
            try:
                segs = list(range(motif.S)) if segments is None else [s for s in segments]
            except TypeError:
                raise ValueError('segments must be a list of segment indices of motif, got %r' % (segments,)) from None
            for s in segs:
                if isinstance(s, bool) or not isinstance(s, numbers.Integral) or not 0 <= s < motif.S:
                    raise ValueError('segments: %r is not an integer in 0..%d' % (s, motif.S - 1))
            if not segs or len(set(segs)) != len(segs):
                raise ValueError('segments must be distinct and at least one, got %r' % (segs,))
            if motif.groups is not None:
                of = sorted({motif.seg_group[s] for s in segs})
                if len(of) != 1 or sorted(segs) != [s for s, g in enumerate(motif.seg_group) if g == of[0]]:
                    raise ValueError('segments must be the segments of exactly one motif group (motif has groups %r), got %r'
                                     % (motif.groups, segs))
            if sum(motif.seg_len[s] for s in segs) != t.shape[0]:
                raise ValueError('anchor_xyz has %d residues, segments %r of motif have %d'
                                 % (t.shape[0], segs, sum(motif.seg_len[s] for s in segs)))
            self.segments = [int(s) for s in segs]
        for name, v in (('clash_distance', clash_distance), ('clash_weight', clash_weight), ('contact_distance', contact_distance),
                        ('contacts_weight', contacts_weight)):
            if v is not None and not (_is_scalar(v) and math.isfinite(float(v)) and float(v) >= 0):
                raise ValueError('%s must be finite and >= 0, got %r' % (name, v))
        if contact_distance is None or not float(contact_distance) > 0:
            raise ValueError('contact_distance must be > 0, got %r' % (contact_distance,))
        if contacts is not None:
            try:
                lo, hi = (float(v) for v in contacts)
            except (TypeError, ValueError):
                raise ValueError('contacts must be (min, max), got %r' % (contacts,)) from None
            if not (math.isfinite(lo) and lo >= 0 and hi >= lo):
                raise ValueError('contacts must be (min, max) with 0 <= min <= max, min finite, got %r' % (contacts,))
        if not (_is_scalar(tausq) and math.isfinite(float(tausq)) and float(tausq) > 0):
            raise ValueError('tausq must be finite and > 0, got %r' % (tausq,))
        if clash_distance is None and contacts is None:
            raise ValueError('no term enabled: give clash_distance or contacts')
        # a term that is off is a weight of 0 to the entry
        self.clash_distance, self.clash_weight = (0.0, 0.0) if clash_distance is None else (float(clash_distance), float(clash_weight))
        self.contact_distance = float(contact_distance)
        self.contacts, self.contacts_weight = ((0.0, math.inf), 0.0) if contacts is None else ((lo, hi), float(contacts_weight))
        super().__init__(n_res, alphas_cumprod, tausq, device)
        if motif is not None and motif.device != self.device:
            raise ValueError('motif is on %s, the potential on %s' % (motif.device, self.device))
        self.A, self.C = int(t.shape[0]), int(y.shape[0])
        self.anchor_xyz, self.context = t.to(self.device), y.to(self.device)
        if motif is None:
            self.anchor_index = rows.to(self.device)
        else:                                                           # anchor k is residue _anchor_offset[k] of segment _anchor_segment[k]
            self._anchor_segment = torch.tensor([s for s in self.segments for _ in range(motif.seg_len[s])], dtype=torch.int64, device=self.device)
            self._anchor_offset = torch.tensor([i for s in self.segments for i in range(motif.seg_len[s])], dtype=torch.int32, device=self.device)

    def anchors_of(self, x):
        """[B, A] int32 on the potential's device: the design residues that hold the anchors in every sample of x (f32, contiguous,
        checked) -- the given ones, or those of the motif's best placement after optimal superposition.  No host read."""
        B = x.shape[0]
        if self.motif is None:
            if self.anchor_index.shape[0] not in (1, B):
                raise ValueError('anchor_index has %d rows, x0 %d particles' % (self.anchor_index.shape[0], B))
            return self.anchor_index.expand(B, self.A).contiguous()
        best = self.motif._launch(x, self.motif._one, fit=True)[0]
        starts = self.motif.starts.index_select(0, best.long())         # [B, S]
        return (starts.index_select(1, self._anchor_segment) + self._anchor_offset[None]).contiguous()

    def describe(self, x):
        """The report of every sample of x [B,N,3] (the class docstring), on the potential's device."""
        report, = self._launch(self._checked(x), self._one, want='report')               # (the energies do not depend on var)
        return _decode_report(report, capi.CONTEXT_REPORT, capi.CONTEXT_COUNTS)

    def pose_of(self, x):
        """(R [B,3,3], t [B,3]) float32 on the potential's device: the fitted motion of every sample of x [B,N,3], placed = R y + t."""
        pose, = self._launch(self._checked(x), self._one, want='pose')
        return pose[:, :9].reshape(-1, 3, 3).clone(), pose[:, 9:].clone()

    def placed_context(self, x):
        """[B, C, 3] float32 on the potential's device: the context as placed for every sample of x [B,N,3]."""
        R, t = self.pose_of(x)
        return torch.einsum('bij,cj->bci', R, self.context) + t[:, None]

    def _launch(self, x, var, want='logp'):
        """One call of the C entry on x (f32, contiguous): (logp, grad), (report [B, 8],) or (pose [B, 12],) as `want` says."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        outs = {'logp': lambda: [torch.empty(B, **f32), torch.empty_like(x), None, None],
                'report': lambda: [None, None, torch.empty(B, len(capi.CONTEXT_REPORT), **f32), None],
                'pose': lambda: [None, None, None, torch.empty(B, 12, **f32)]}[want]()
        index = self.anchors_of(x)
        self._call('genie_context_potential', self._stream(), B, self.n_res, _ptr(x), self.A, _ptr(index), _ptr(self.anchor_xyz), self.C,
                   _ptr(self.context), self.clash_distance, self.clash_weight, self.contact_distance, self.contacts[0], self.contacts[1],
                   self.contacts_weight, _ptr(var), *(_ptr(t) for t in outs),
                   *self._workspace(self.lib.genie_context_potential_work_bytes(B, self.n_res)))
        return tuple(t for t in outs if t is not None)


def check_fold_bounds(bounds, n_refs):
    """Per-reference rows (lo, hi, weight) -- or (lo, hi): weight 1 -- as a float64 tensor [n_refs, 3]: TM-scores to stay between,
    0 <= lo <= hi, lo finite, hi possibly inf, weight finite and >= 0; a ValueError otherwise."""
    import math
    try:
        rows = [[float(v) for v in row] for row in (bounds.tolist() if torch.is_tensor(bounds) else bounds)]
    except (TypeError, ValueError):
        raise ValueError('bounds must hold one (lo, hi[, weight]) row per reference, got %r' % (bounds,)) from None
    if len(rows) != n_refs or any(len(row) not in (2, 3) for row in rows):
        raise ValueError('bounds must hold one (lo, hi[, weight]) row per reference: %d rows for %d references' % (len(rows), n_refs))
    rows = [row + [1.0] if len(row) == 2 else row for row in rows]
    for r, (lo, hi, weight) in enumerate(rows):
        if not (math.isfinite(lo) and lo >= 0 and hi >= lo):
            raise ValueError('bounds of reference %d must be (lo, hi) with 0 <= lo <= hi, lo finite, got (%r, %r)' % (r, lo, hi))
        if not (math.isfinite(weight) and weight >= 0):
            raise ValueError('weight of reference %d must be finite and >= 0, got %r' % (r, weight))
    return torch.tensor(rows, dtype=torch.float64).reshape(n_refs, 3)


class FoldPotential(_HipPotential):
    """Fold guidance as one HIP entry (genie_fold_potential, csrc/fold_kernels.hip; include/genie_hip.h states the mathematics):
    `pot(x0 [B,N,3], step) -> log p [B]`, differentiable in x0, a drop-in `twisting_function` for TwistedSampler beside the other
    built-in potentials (SumPotential adds them).  It is the score of similarity.PairwiseTM used while sampling: `references` [R, N, 3]
    are fixed C-alpha backbones of the design's own length, and `bounds` one row (lo, hi[, weight]) per reference, the range its
    TM-score to every particle is kept in -- (0.6, inf) samples around a template, (0, 0.5) stays away from a known fold.  With n_r the
    soft number of superposed residues of the seeded ascent (`n_iter` iterations per seed, the particle moving, gapless, offset 0),
      E = sum_r weight_r [ max(0, N lo_r - n_r)^2 + max(0, n_r - N hi_r)^2 ],   log p = -E / (2 var),
    var = xstart_variance(alphas_cumprod[step], tausq) computed on the device, so nothing on the per-step path reads device memory
    from the host.  The gradient is taken with every pair's winning rigid transform held fixed (the envelope theorem makes it the
    total derivative at a converged ascent); the forward keeps the gradient the kernel computes and the backward scales it.

    Everything is validated on the host before the device is looked at; a potential whose weights are all 0 is a ValueError.  The
    references and bounds are uploaded once.  `describe(x)` reports every sample of x with the names of capi.FOLD_REPORT:
    'tm_nearest' (the largest TM to a reference), 'nearest' (its index, int64), 'tm_lowest_wanted' (the smallest TM to a reference
    with lo > 0; 0 without one), 'n_fold_violations' (references outside their range, int64), 'e_fold' (E): [B] tensors on the
    potential's device.  `tm_of(x)` is [B, R], every TM-score.

    The defaults (tausq = 1 A^2, weights 1) are design choices: no trained checkpoint is in the tree, so their effect on sample
    quality is unmeasured.  References of another length or with gaps are AlignedFoldPotential's (below), which aligns before it
    scores.  Coupling between the particles of a batch is DiversityPotential's.  Not built: per-residue masks on a reference, a
    best-of-several-templates form."""

    def __init__(self, n_res, alphas_cumprod, references, bounds, n_iter=16, tausq=1.0, device='cuda'):
        import math
        if isinstance(n_res, bool) or not isinstance(n_res, numbers.Integral) or not capi.TM_MIN_LENGTH <= n_res <= capi.TM_MAX_LENGTH:
            raise ValueError('n_res must be an integer in %d..%d, got %r' % (capi.TM_MIN_LENGTH, capi.TM_MAX_LENGTH, n_res))
        try:
            y = torch.as_tensor(references).detach().to(dtype=torch.float32, device='cpu')
        except (TypeError, ValueError, RuntimeError):
            raise ValueError('references must be [R, %d, 3] coordinates, got %r' % (n_res, type(references))) from None
        if y.dim() != 3 or y.shape[1] != n_res or y.shape[2] != 3:
            raise ValueError('references must be [R, %d, 3], got %s' % (n_res, tuple(y.shape)))
        if not 1 <= y.shape[0] <= capi.FOLD_MAX_REFERENCES:
            raise ValueError('references must hold 1..%d backbones, got %d' % (capi.FOLD_MAX_REFERENCES, y.shape[0]))
        if not bool(torch.isfinite(y).all()):
            raise ValueError('references has a coordinate that is not finite')
        table = check_fold_bounds(bounds, int(y.shape[0]))
        if isinstance(n_iter, bool) or not isinstance(n_iter, numbers.Integral) or not 1 <= n_iter <= capi.TM_MAX_ITER:
            raise ValueError('n_iter must be an integer in 1..%d, got %r' % (capi.TM_MAX_ITER, n_iter))
        if not (_is_scalar(tausq) and math.isfinite(float(tausq)) and float(tausq) > 0):
            raise ValueError('tausq must be finite and > 0, got %r' % (tausq,))
        if not bool((table[:, 2] > 0).any()):
            raise ValueError('no term enabled: every reference has weight 0')
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.R, self.n_iter = int(y.shape[0]), int(n_iter)
        self.references = y.contiguous().to(self.device)
        self.bounds = table.to(torch.float32).contiguous().to(self.device)

    def describe(self, x):
        """The report of every sample of x [B,N,3] (the class docstring), on the potential's device."""
        report, = self._launch(self._checked(x), self._one, want='report')               # (the energy does not depend on var)
        return _decode_report(report, capi.FOLD_REPORT, capi.FOLD_COUNTS)

    def tm_of(self, x):
        """[B, R] float32 on the potential's device: the TM-score of every sample of x [B,N,3] to every reference."""
        return self._launch(self._checked(x), self._one, want='tm')[0]

    def _launch(self, x, var, want='logp'):
        """One call of the C entry on x (f32, contiguous): (logp, grad), (report [B, 5],) or (tm_out [B, R],) as `want` says."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        outs = {'logp': lambda: [torch.empty(B, **f32), torch.empty_like(x), None, None],
                'report': lambda: [None, None, torch.empty(B, len(capi.FOLD_REPORT), **f32), None],
                'tm': lambda: [None, None, None, torch.empty(B, self.R, **f32)]}[want]()
        self._call('genie_fold_potential', self._stream(), B, self.n_res, _ptr(x), self.R, _ptr(self.references), _ptr(self.bounds),
                   self.n_iter, _ptr(var), *(_ptr(t) for t in outs),
                   *self._workspace(self.lib.genie_fold_potential_work_bytes(B, self.n_res, self.R)))
        return tuple(t for t in outs if t is not None)


def _check_aligned_references(references, lengths, n_res):
    """AlignedFoldPotential's references as (y float32 [R, Nr, 3] on the CPU, padded with zeros and trimmed to the longest chain, the
    lengths as R ints): a list of [L_r, 3] arrays, or a padded [R, Nr, 3] tensor with `lengths`; a ValueError otherwise."""
    lo, hi, cells = capi.TM_MIN_LENGTH, capi.TMALIGN_MAX_LENGTH, capi.TMALIGN_MAX_CELLS
    if lengths is None:
        try:
            chains = [torch.as_tensor(c).detach().to(dtype=torch.float32, device='cpu') for c in references]
        except (TypeError, ValueError, RuntimeError):
            raise ValueError('references must be a list of [L, 3] coordinates, or [R, Nr, 3] with lengths=, got %r' % type(references)) from None
        for r, c in enumerate(chains):
            if c.dim() != 2 or c.shape[1] != 3:
                raise ValueError('reference %d must be [L, 3], got %s' % (r, tuple(c.shape)))
        lengths = [int(c.shape[0]) for c in chains]
    else:
        try:
            padded = torch.as_tensor(references).detach().to(dtype=torch.float32, device='cpu')
        except (TypeError, ValueError, RuntimeError):
            raise ValueError('references must be a list of [L, 3] coordinates, or [R, Nr, 3] with lengths=, got %r' % type(references)) from None
        if padded.dim() != 3 or padded.shape[2] != 3:
            raise ValueError('references must be [R, Nr, 3] where lengths is given, got %s' % (tuple(padded.shape),))
        lengths = lengths.tolist() if torch.is_tensor(lengths) else list(lengths)
        if len(lengths) != padded.shape[0] or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in lengths):
            raise ValueError('lengths must hold one integer per reference: %d entries for %d references' % (len(lengths), padded.shape[0]))
        lengths = [int(v) for v in lengths]
        if any(v > padded.shape[1] for v in lengths):
            raise ValueError('lengths holds %d, references has %d rows per chain' % (max(lengths), padded.shape[1]))
        chains = [padded[r, :max(v, 0)] for r, v in enumerate(lengths)]
    if not 1 <= len(chains) <= capi.FOLD_ALIGN_MAX_REFERENCES:
        raise ValueError('references must hold 1..%d backbones, got %d' % (capi.FOLD_ALIGN_MAX_REFERENCES, len(chains)))
    for r, v in enumerate(lengths):
        if not lo <= v <= hi:
            raise ValueError('reference %d has %d residues, the gapped alignment takes %d..%d' % (r, v, lo, hi))
        if n_res * v > cells:
            raise ValueError('reference %d has %d residues: n_res (%d) times that is above %d cells' % (r, v, n_res, cells))
    y = torch.zeros(len(chains), max(lengths), 3, dtype=torch.float32)
    for r, c in enumerate(chains):
        if not bool(torch.isfinite(c).all()):
            raise ValueError('reference %d has a coordinate that is not finite' % r)
        y[r, :lengths[r]] = c
    return y, lengths


class AlignedFoldPotential(_HipPotential):
    """Fold guidance under gapped alignment as one HIP entry (genie_fold_align_potential, csrc/fold_align_kernels.hip;
    include/genie_hip.h states the mathematics): FoldPotential for references of any length.  `pot(x0 [B,N,3], step) -> log p [B]`,
    differentiable in x0, a drop-in `twisting_function` for TwistedSampler beside the other built-in potentials (SumPotential adds
    them).  `references` is a list of [L_r, 3] C-alpha backbones of 4..1024 residues each, n_res L_r at most 131072 -- or a padded
    tensor [R, Nr, 3] with `lengths=` -- and `bounds` one row (lo, hi[, weight]) per reference, as FoldPotential takes them.  Every
    particle is aligned to every reference exactly as similarity.TMAlign aligns a query to a reference (`norm`, `n_iter`, `n_rounds`,
    `gap_open` are its arguments; `offset_stride` s visits every s-th offset of the gapless stage and always the last), the winning
    fit is polished by `n_iter` more ascent steps over the aligned pairs, and with n_r the soft number of superposed residues and
    Lnorm_r the normalising length
      E = sum_r weight_r [ max(0, Lnorm_r lo_r - n_r)^2 + max(0, n_r - Lnorm_r hi_r)^2 ],   log p = -E / (2 var),
    var = xstart_variance(alphas_cumprod[step], tausq) computed on the device.  The gradient holds every pair's alignment and fit
    fixed: the alignment is piecewise constant in x0, so it is the derivative on the piece the particle lies in (an unaligned residue
    gets 0), and the envelope theorem covers the fit.  The forward keeps the gradient the kernel computes and the backward scales it.

    Everything is validated on the host before the device is looked at; a potential whose weights are all 0 is a ValueError.
    `describe(x)` is FoldPotential's report (capi.FOLD_REPORT); `tm_of(x)` is [B, R], every polished TM-score, at least TMAlign's in
    exact arithmetic; `alignment_of(x)` is a dict of 'map' [B,R,N] int32 (per particle residue the matched reference residue, or -1),
    'n_aligned' [B,R] int32, 'rot' [B,R,3,3] and 'trans' [B,R,3] (the polished fit, rot x + trans ~ reference), 'rot0' and 'trans0'
    (the search's fit before the polish) and 'tm' [B,R].

    The defaults (TMAlign's, stride 1, tausq = 1 A^2, weights 1) are design choices: no trained checkpoint is in the tree, so their
    effect on sample quality is unmeasured.  Not built: gradients across a change of alignment, warm-starting the search from the
    previous step, tables above 131072 cells, per-residue masks, a best-of-several-templates form."""

    def __init__(self, n_res, alphas_cumprod, references, bounds, norm='query', n_iter=16, n_rounds=8, gap_open=-0.6, offset_stride=1,
                 tausq=1.0, device='cuda', lengths=None):
        import math
        if isinstance(n_res, bool) or not isinstance(n_res, numbers.Integral) or not capi.TM_MIN_LENGTH <= n_res <= capi.TMALIGN_MAX_LENGTH:
            raise ValueError('n_res must be an integer in %d..%d, got %r' % (capi.TM_MIN_LENGTH, capi.TMALIGN_MAX_LENGTH, n_res))
        y, lengths = _check_aligned_references(references, lengths, int(n_res))
        table = check_fold_bounds(bounds, int(y.shape[0]))
        if norm not in capi.TMALIGN_NORMS:
            raise ValueError('norm must be one of %s, got %r' % (capi.TMALIGN_NORMS, norm))
        if isinstance(n_iter, bool) or not isinstance(n_iter, numbers.Integral) or not 1 <= n_iter <= capi.TM_MAX_ITER:
            raise ValueError('n_iter must be an integer in 1..%d, got %r' % (capi.TM_MAX_ITER, n_iter))
        if isinstance(n_rounds, bool) or not isinstance(n_rounds, numbers.Integral) or not 0 <= n_rounds <= capi.TMALIGN_MAX_ROUNDS:
            raise ValueError('n_rounds must be an integer in 0..%d, got %r' % (capi.TMALIGN_MAX_ROUNDS, n_rounds))
        if isinstance(gap_open, bool) or not isinstance(gap_open, numbers.Real) or not -10.0 <= gap_open <= 0.0:       # (NaN fails both)
            raise ValueError('gap_open must be a number in -10..0, got %r' % (gap_open,))
        if (isinstance(offset_stride, bool) or not isinstance(offset_stride, numbers.Integral)
                or not 1 <= offset_stride <= capi.FOLD_ALIGN_MAX_STRIDE):
            raise ValueError('offset_stride must be an integer in 1..%d, got %r' % (capi.FOLD_ALIGN_MAX_STRIDE, offset_stride))
        if not (_is_scalar(tausq) and math.isfinite(float(tausq)) and float(tausq) > 0):
            raise ValueError('tausq must be finite and > 0, got %r' % (tausq,))
        if not bool((table[:, 2] > 0).any()):
            raise ValueError('no term enabled: every reference has weight 0')
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.R, self.Nr, self.lengths = int(y.shape[0]), int(y.shape[1]), list(lengths)
        self.norm, self.n_iter, self.n_rounds = norm, int(n_iter), int(n_rounds)
        self.gap_open, self.offset_stride = float(gap_open), int(offset_stride)
        self.references = y.contiguous().to(self.device)
        self.lr = torch.tensor(lengths, dtype=torch.int32).to(self.device)
        self.bounds = table.to(torch.float32).contiguous().to(self.device)

    def describe(self, x):
        """The report of every sample of x [B,N,3] (FoldPotential's), on the potential's device."""
        return _decode_report(self._launch(self._checked(x), self._one, want='report')['report'], capi.FOLD_REPORT, capi.FOLD_COUNTS)

    def tm_of(self, x):
        """[B, R] float32 on the potential's device: the polished TM-score of every sample of x [B,N,3] to every reference."""
        return self._launch(self._checked(x), self._one, want='tm')['tm']

    def alignment_of(self, x):
        """The alignment of every sample of x [B,N,3] to every reference (the class docstring names the keys), on the potential's device."""
        return self._launch(self._checked(x), self._one, want='alignment')

    def _launch(self, x, var, want='logp'):
        """One call of the C entry on x (f32, contiguous): (logp, grad) for 'logp', else a dict of the outputs `want` names."""
        B, N, R = x.shape[0], self.n_res, self.R
        f32, i32 = dict(dtype=torch.float32, device=x.device), dict(dtype=torch.int32, device=x.device)
        names = ('logp', 'grad', 'report', 'tm', 'n_aligned', 'map', 'rot', 'trans', 'rot0', 'trans0')
        make = {'logp': lambda: torch.empty(B, **f32), 'grad': lambda: torch.empty_like(x),
                'report': lambda: torch.empty(B, len(capi.FOLD_REPORT), **f32), 'tm': lambda: torch.empty(B, R, **f32),
                'n_aligned': lambda: torch.empty(B, R, **i32), 'map': lambda: torch.empty(B, R, N, **i32),
                'rot': lambda: torch.empty(B, R, 3, 3, **f32), 'trans': lambda: torch.empty(B, R, 3, **f32),
                'rot0': lambda: torch.empty(B, R, 3, 3, **f32), 'trans0': lambda: torch.empty(B, R, 3, **f32)}
        asked = {'logp': ('logp', 'grad'), 'report': ('report',), 'tm': ('tm',),
                 'alignment': ('tm', 'n_aligned', 'map', 'rot', 'trans', 'rot0', 'trans0')}[want]
        out = {k: make[k]() for k in asked}
        self._call('genie_fold_align_potential', self._stream(), B, N, _ptr(x), R, self.Nr, _ptr(self.references), _ptr(self.lr),
                   _ptr(self.bounds), capi.TMALIGN_NORMS.index(self.norm), self.n_iter, self.n_rounds, self.gap_open, self.offset_stride,
                   _ptr(var), *(_ptr(out.get(k)) for k in names),
                   *self._workspace(self.lib.genie_fold_align_potential_work_bytes(B, N, R)))
        return (out['logp'], out['grad']) if want == 'logp' else out


class DiversityPotential(_HipPotential):
    """Diversity guidance as one HIP entry (genie_diversity_potential, csrc/diversity_kernels.hip; include/genie_hip.h states the
    mathematics): `pot(x0 [B,N,3], step) -> log p [B]`, differentiable in x0, a drop-in `twisting_function` for TwistedSampler beside
    the other built-in potentials (SumPotential adds them).  The particles of one device batch repel each other: the batch is
    S = B / num_particles particle systems, system-major as TwistedSampler lays them out (particle b belongs to system
    b // num_particles), and every pair of particles of DIFFERENT systems is scored once with FoldPotential's score (the particle of
    the lower index moving, `n_iter` iterations per seed).  With n_bj the soft number of superposed residues of particles b and j,
      E_b = (weight / num_particles) sum_{j in other systems} max(0, n_bj - N tm_max)^2,   log p_b = -E_b / (2 var),
    var = xstart_variance(alphas_cumprod[step], tausq) computed on the device, so nothing on the per-step path reads device memory
    from the host.  The gradient of log p_b is taken in x_b alone, every other particle and every pair's fit held fixed: each
    particle's own twisting function, with its neighbours as parameters.  Particles of one system are resampled copies of each other
    and do not repel.

    A system's step now depends on its batch neighbours, on purpose: that is what the term is for, and it is the one built-in
    potential of which this is true (weights, resampling and the gradient cap stay per system).  The coupling is within one device
    batch only; across batches and runs, avoid the earlier outputs with a FoldPotential.  The potential is meant for `num_particles`
    runs (TwistedSampler's 'num_particles', 1 included: single coupled trajectories): without them the whole batch is one system,
    and one system spanning the whole batch has nothing to repel -- log p and the gradient are exactly 0.

    Everything is validated on the host before the device is looked at.  `pot(x0, step)` takes B a multiple of `num_particles`
    (ValueError otherwise).  `describe(x)` and `tm_of(x)` score EVERY ROW OF x AS A DESIGN OF ITS OWN (one particle per system),
    which is what TwistedSampler's reports call them on -- the returned structures, be they every system's best particle or all of
    them: `describe` gives the names of capi.DIVERSITY_REPORT, 'tm_nearest_design' (the largest TM to another design; 0 for a single
    row), 'nearest_design' (its row, int64; -1 for a single row), 'tm_mean_design', 'n_similar' (designs above tm_max, int64),
    'e_diversity' (E with num_particles = 1): [B] tensors on the potential's device; `tm_of` is [B, B], symmetric, 0 on the diagonal.

    The defaults (tm_max 0.5, weight 1, tausq = 1 A^2) are design choices: no trained checkpoint is in the tree, so their effect on
    sample quality is unmeasured.  Not built: gapped alignment between particles, coupling across batches or devices, weighting
    partners by their SMC weights, a lower hinge."""

    def __init__(self, n_res, alphas_cumprod, num_particles, tm_max=0.5, weight=1.0, n_iter=16, tausq=1.0, device='cuda'):
        import math
        if isinstance(n_res, bool) or not isinstance(n_res, numbers.Integral) or not capi.TM_MIN_LENGTH <= n_res <= capi.TM_MAX_LENGTH:
            raise ValueError('n_res must be an integer in %d..%d, got %r' % (capi.TM_MIN_LENGTH, capi.TM_MAX_LENGTH, n_res))
        if isinstance(num_particles, bool) or not isinstance(num_particles, numbers.Integral) or not 1 <= num_particles <= SMC_MAX_PARTICLES:
            raise ValueError('num_particles must be an integer in 1..%d, got %r' % (SMC_MAX_PARTICLES, num_particles))
        if not (_is_scalar(tm_max) and 0 < float(tm_max) <= 1):
            raise ValueError('tm_max must be in (0, 1], got %r' % (tm_max,))
        if not (_is_scalar(weight) and math.isfinite(float(weight)) and float(weight) > 0):
            raise ValueError('weight must be finite and > 0, got %r' % (weight,))
        if isinstance(n_iter, bool) or not isinstance(n_iter, numbers.Integral) or not 1 <= n_iter <= capi.TM_MAX_ITER:
            raise ValueError('n_iter must be an integer in 1..%d, got %r' % (capi.TM_MAX_ITER, n_iter))
        if not (_is_scalar(tausq) and math.isfinite(float(tausq)) and float(tausq) > 0):
            raise ValueError('tausq must be finite and > 0, got %r' % (tausq,))
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.K, self.tm_max, self.weight, self.n_iter = int(num_particles), float(tm_max), float(weight), int(n_iter)

    def _checked(self, x0, K=None):
        x = super()._checked(x0)
        K = self.K if K is None else K
        if x.shape[0] < 1 or x.shape[0] % K:
            raise ValueError('x0 must hold a multiple of num_particles = %d rows, got %d' % (K, x.shape[0]))
        if x.shape[0] > capi.DIVERSITY_MAX_BATCH:
            raise ValueError('x0 must hold at most %d rows, got %d' % (capi.DIVERSITY_MAX_BATCH, x.shape[0]))
        return x

    def describe(self, x):
        """The report of every row of x [B,N,3] as a design of its own (the class docstring), on the potential's device."""
        report, = self._launch(self._checked(x, 1), self._one, want='report', K=1)         # (the energy does not depend on var)
        return _decode_report(report, capi.DIVERSITY_REPORT, capi.DIVERSITY_COUNTS)

    def tm_of(self, x):
        """[B, B] float32 on the potential's device: the TM-score of every row of x [B,N,3] to every other, 0 on the diagonal."""
        return self._launch(self._checked(x, 1), self._one, want='tm', K=1)[0]

    def _launch(self, x, var, want='logp', K=None):
        """One call of the C entry on x (f32, contiguous) as systems of K (default: num_particles): (logp, grad), (report [B, 5],)
        or (tm_out [B, B],) as `want` says."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        K = self.K if K is None else K
        outs = {'logp': lambda: [torch.empty(B, **f32), torch.empty_like(x), None, None],
                'report': lambda: [None, None, torch.empty(B, len(capi.DIVERSITY_REPORT), **f32), None],
                'tm': lambda: [None, None, None, torch.empty(B, B, **f32)]}[want]()
        self._call('genie_diversity_potential', self._stream(), B, K, self.n_res, _ptr(x), self.tm_max, self.weight, self.n_iter,
                   _ptr(var), *(_ptr(t) for t in outs), *self._workspace(self.lib.genie_diversity_potential_work_bytes(B, K, self.n_res)))
        return tuple(t for t in outs if t is not None)


def load_burial_targets(path):
    """A burial file -> [(i, lo, hi, weight), ...] for BurialPotential: one residue per line, `i lo hi [weight]`, residues 0-based
    like the motif_locations files, lo and hi soft half-sphere counts, `inf` allowed for hi, weight 1 when omitted; `#` starts a
    comment, blank lines are ignored.  A bad line raises ValueError('<path>:<line number>: ...')."""
    out = []
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            fields = line.split('#', 1)[0].split()
            if not fields:
                continue
            if len(fields) not in (3, 4):
                raise ValueError('%s:%d: expected `i lo hi [weight]`, got %d fields' % (path, number, len(fields)))
            try:
                i = int(fields[0])
                lo, hi = float(fields[1]), float(fields[2])
                weight = float(fields[3]) if len(fields) == 4 else 1.0
            except ValueError:
                raise ValueError('%s:%d: the residue is an integer, lo, hi and weight numbers: %r' % (path, number, line.strip())) from None
            out.append((i, lo, hi, weight))
    return out


def check_burial_targets(targets, n_res):
    """The targets of BurialPotential, validated on the host: [(i, lo, hi, weight), ...] with i in 0..n_res-1, 0 <= lo <= hi (hi may
    be inf), weight finite and >= 0 (1 when omitted), no residue listed twice; returned sorted by residue."""
    import math
    out, seen = [], set()
    for k, t in enumerate(targets):
        try:
            t = tuple(t)
        except TypeError:
            raise ValueError('burial target %d: expected (i, lo, hi[, weight]), got %r' % (k, t)) from None
        if len(t) not in (3, 4):
            raise ValueError('burial target %d: expected (i, lo, hi[, weight]), got %r' % (k, t))
        i = t[0]
        if isinstance(i, bool) or not isinstance(i, numbers.Integral):
            raise ValueError('burial target %d: the residue must be an integer, got %r' % (k, i))
        try:
            i, lo, hi, weight = int(i), float(t[1]), float(t[2]), float(t[3]) if len(t) == 4 else 1.0
        except (TypeError, ValueError):
            raise ValueError('burial target %d: lo, hi and weight must be numbers, got %r' % (k, t)) from None
        if not 0 <= i < n_res:
            raise ValueError('burial target %d: residue %d must lie in 0..%d' % (k, i, n_res - 1))
        if not (0 <= lo <= hi) or math.isinf(lo):
            raise ValueError('burial target %d: needs 0 <= lo <= hi with lo finite, got lo = %r, hi = %r' % (k, lo, hi))
        if not (math.isfinite(weight) and weight >= 0):
            raise ValueError('burial target %d: the weight must be finite and >= 0, got %r' % (k, weight))
        if i in seen:
            raise ValueError('burial target %d: residue %d is listed twice' % (k, i))
        seen.add(i)
        out.append((i, lo, hi, weight))
    return sorted(out)


def parse_residue_ranges(spec):
    """'3,10-20,35' -> [3, 10, 11, ..., 20, 35]: 0-based residues and inclusive ranges, comma-separated, ascending, each once; a
    ValueError for anything else (a reversed range, a residue named twice, a negative number, an empty item)."""
    out = []
    for item in str(spec).split(','):
        item = item.strip()
        ends = item.split('-')
        if not 1 <= len(ends) <= 2 or not all(e.strip().isdigit() for e in ends):
            raise ValueError('residue ranges look like 3,10-20,35 (0-based, inclusive), got %r' % (spec,))
        first, last = int(ends[0]), int(ends[-1])
        if last < first:
            raise ValueError('the range %r runs backwards' % item)
        out.extend(range(first, last + 1))
    if len(set(out)) != len(out):
        raise ValueError('a residue is named twice in %r' % (spec,))
    return sorted(out)


BURIAL_MAX_LENGTH = capi.BURIAL_MAX_LENGTH      # the longest chain whose staging fits in the kernel's 64 KiB of LDS (include/genie_hip.h)


class BurialPotential(_HipPotential):
    """Burial guidance as one HIP entry (genie_burial_potential, csrc/burial_kernels.hip; include/genie_hip.h states the mathematics):
    `pot(x0 [B,N,3], step) -> log p [B]`, differentiable in x0, a drop-in `twisting_function` for TwistedSampler beside the other
    built-in potentials (SumPotential adds them).  It is the one potential that tells inside from outside, by the half-sphere
    exposure of a C-alpha chain (HSE-alpha).  In words:
      the count         residue n points where its side chain would: along 2 x_n - x_{n-1} - x_{n+1}, made a unit vector with
                        a floor of eps = 0.1 A on its length (the two ends have no direction).  Its burial c_n is the soft number
                        of residues at least `separation` away in sequence that lie within `radius` of it (the binder potential's
                        rational switch, 1/2 at `radius`) and on that side of it (a soft half-space of `width` Angstrom: 1/2 on the
                        plane through the residue); an end counts half of its whole sphere.
      targets           [(i, lo, hi[, weight]), ...], 0-based residues like the motif_locations files: c_i is kept in lo..hi by a
                        squared hinge (hi may be inf: "bury"; lo may be 0: "expose"); load_burial_targets reads them from a file.
      mean              (min, max): the mean of c_n over the chain is kept in that range by a squared hinge weighted mean_weight
                        (max may be inf): a design with a core, not just a small one.
    log p = -(E_targets + E_mean) / (2 var), var = xstart_variance(alphas_cumprod[step], tausq) computed on the device, so nothing on
    the per-step path reads device memory from the host; the forward keeps the gradient the kernel computes and the backward scales
    it.  The likelihood is unnormalised.

    Everything is validated on the host (check_burial_targets) before the device is looked at; the per-residue table is built and
    uploaded once.  A potential with no term enabled (no targets, and no mean or a mean_weight of 0) is a ValueError.  `describe(x)`
    reports every sample of x with the names of capi.BURIAL_REPORT: 'burial_mean', 'burial_min', 'burial_max', 'n_burial_violated'
    (targeted residues outside their range, int64), 'max_burial_violation', 'e_burial_target', 'e_burial_mean' (the weighted
    energies, before the division by 2 var): [B] tensors on the potential's device.  `burial_of(x)` is [B, N], the c_n.

    The defaults (radius 10 A, width 2 A, separation 3, eps 0.1 A, weights 1, tausq = 1 A^2) are design choices: no trained
    checkpoint is in the tree, so their effect on sample quality is unmeasured.  Not built: tying targets to a motif's placement,
    which moves per particle; chain breaks under --unit_chains (the direction stencil crosses them); a full-atom or C-beta model;
    counting a binder target's atoms as neighbours."""

    def __init__(self, n_res, alphas_cumprod, targets=None, mean=None, mean_weight=1.0, radius=10.0, width=2.0, separation=3, tausq=1.0,
                 device='cuda'):
        import math
        if isinstance(n_res, bool) or not isinstance(n_res, numbers.Integral) or not 1 <= n_res <= BURIAL_MAX_LENGTH:
            raise ValueError('n_res must be an integer in 1..%d, got %r' % (BURIAL_MAX_LENGTH, n_res))
        for name, v in (('radius', radius), ('width', width), ('tausq', tausq)):
            if not (_is_scalar(v) and math.isfinite(float(v)) and float(v) > 0):
                raise ValueError('%s must be finite and > 0, got %r' % (name, v))
        if not (_is_scalar(mean_weight) and math.isfinite(float(mean_weight)) and float(mean_weight) >= 0):
            raise ValueError('mean_weight must be finite and >= 0, got %r' % (mean_weight,))
        if isinstance(separation, bool) or not isinstance(separation, numbers.Integral) or separation < 1:
            raise ValueError('separation must be an integer >= 1, got %r' % (separation,))
        if mean is not None:
            try:
                lo, hi = (float(v) for v in mean)
            except (TypeError, ValueError):
                raise ValueError('mean must be (min, max), got %r' % (mean,)) from None
            if not (math.isfinite(lo) and lo >= 0 and hi >= lo):
                raise ValueError('mean must be (min, max) with 0 <= min <= max, min finite, got %r' % (mean,))
        self.targets = check_burial_targets(targets if targets is not None else [], int(n_res))
        if not self.targets and (mean is None or float(mean_weight) == 0):
            raise ValueError('no term enabled: give targets or mean (with a mean_weight above 0)')
        # a term that is off is a weight of 0 (the mean) or no table (the targets) to the entry
        self.mean, self.mean_weight = ((0.0, math.inf), 0.0) if mean is None else ((lo, hi), float(mean_weight))
        self.radius, self.width, self.separation = float(radius), float(width), int(separation)
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.table = (None, None, None)
        if self.targets:
            rows = torch.zeros(3, self.n_res, dtype=torch.float32)
            rows[1] = math.inf
            for i, a, b, weight in self.targets:
                rows[0, i], rows[1, i], rows[2, i] = a, b, weight
            rows = rows.to(self.device)
            self.table = (rows[0], rows[1], rows[2])

    def describe(self, x):
        """The report of every sample of x [B,N,3] (the class docstring), on the potential's device."""
        report, = self._launch(self._checked(x), self._one, want='report')               # (the energies do not depend on var)
        return _decode_report(report, capi.BURIAL_REPORT, capi.BURIAL_COUNTS)

    def burial_of(self, x):
        """[B, N] float32 on the potential's device: the soft half-sphere count c_n of every residue of every sample of x [B,N,3]."""
        return self._launch(self._checked(x), self._one, want='burial')[0]

    def _launch(self, x, var, want='logp'):
        """One call of the C entry on x (f32, contiguous): (logp, grad), (report [B, 7],) or (burial_out [B, N],) as `want` says."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        outs = {'logp': lambda: [torch.empty(B, **f32), torch.empty_like(x), None, None],
                'report': lambda: [None, None, torch.empty(B, len(capi.BURIAL_REPORT), **f32), None],
                'burial': lambda: [None, None, None, torch.empty(B, self.n_res, **f32)]}[want]()
        self._call('genie_burial_potential', self._stream(), B, self.n_res, _ptr(x), self.radius, self.width, self.separation,
                   *(_ptr(t) for t in self.table), self.mean[0], self.mean[1], self.mean_weight, _ptr(var), *(_ptr(t) for t in outs),
                   *self._workspace(self.lib.genie_burial_potential_work_bytes(B, self.n_res)))
        return tuple(t for t in outs if t is not None)


ENVELOPE_MAX_LENGTH, ENVELOPE_MAX_POINTS = capi.ENVELOPE_MAX_LENGTH, capi.ENVELOPE_MAX_POINTS      # include/genie_hip.h says what sets them


def load_envelope(path):
    """An envelope file -> (points [M, 3], weights [M]) float64 tensors for EnvelopePotential.  A `.pdb` file gives the coordinates of
    every ATOM / HETATM record (columns 31-54), weights 1: a C-alpha trace, a full-atom model and a pseudo-atom file from a map tool
    all work.  Any other file is text, one point per line, `x y z [weight]` in Angstrom, weight 1 when omitted; `#` starts a comment,
    blank lines are ignored.  A bad line raises ValueError('<path>:<line number>: ...'), a file without a point ValueError('<path>:
    ...')."""
    points, weights = [], []
    pdb = str(path).lower().endswith('.pdb')
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            if pdb:
                if not line.startswith(('ATOM', 'HETATM')):
                    continue
                try:
                    row = [float(line[30:38]), float(line[38:46]), float(line[46:54]), 1.0]
                except ValueError:
                    raise ValueError('%s:%d: no coordinates in columns 31-54: %r' % (path, number, line.rstrip())) from None
            else:
                fields = line.split('#', 1)[0].split()
                if not fields:
                    continue
                if len(fields) not in (3, 4):
                    raise ValueError('%s:%d: expected `x y z [weight]`, got %d fields' % (path, number, len(fields)))
                try:
                    row = [float(f) for f in fields] + [1.0] * (4 - len(fields))
                except ValueError:
                    raise ValueError('%s:%d: x, y, z and weight are numbers: %r' % (path, number, line.strip())) from None
            points.append(row[:3])
            weights.append(row[3])
    if not points:
        raise ValueError('%s: no envelope point (%s)' % (path, 'no ATOM or HETATM record' if pdb else 'no `x y z [weight]` line'))
    return torch.tensor(points, dtype=torch.float64), torch.tensor(weights, dtype=torch.float64)


ENVELOPE_SHAPES = {'sphere': ('R',), 'ellipsoid': ('A', 'B', 'C'), 'cylinder': ('R', 'L'), 'torus': ('R', 'r'), 'box': ('A', 'B', 'C')}


def envelope_shape_points(spec, spacing):
    """The points of a solid for EnvelopePotential, [M, 3] float64, centred on the origin: `sphere:R`, `ellipsoid:A,B,C` (semi-axes
    along x, y, z), `cylinder:R,L` (radius and full length, axis z), `torus:R,r` (ring radius and tube radius, axis z) and `box:A,B,C`
    (full edge lengths), in Angstrom.  They are the points (i, j, k) spacing of the integer lattice, the origin included, that satisfy
    the solid's closed inequality, in ascending (i, j, k) order: deterministic, host only.  A ValueError for a specification that does
    not parse, a size or spacing that is not finite and positive, a solid that holds no lattice point (a torus may miss them all) and
    one with more than ENVELOPE_MAX_POINTS points (use a larger spacing)."""
    import math
    name, _, tail = str(spec).partition(':')
    name = name.strip().lower()
    if name not in ENVELOPE_SHAPES:
        raise ValueError('an envelope shape is one of %s, got %r' % (', '.join('%s:%s' % (k, ','.join(v)) for k, v in ENVELOPE_SHAPES.items()), spec))
    try:
        sizes = [float(v) for v in tail.split(',')]
    except ValueError:
        sizes = []
    if len(sizes) != len(ENVELOPE_SHAPES[name]) or not all(math.isfinite(v) and v > 0 for v in sizes):
        raise ValueError('%s takes %d finite sizes above 0, %s:%s, got %r' % (name, len(ENVELOPE_SHAPES[name]), name, ','.join(ENVELOPE_SHAPES[name]), spec))
    if not (_is_scalar(spacing) and math.isfinite(float(spacing)) and float(spacing) > 0):
        raise ValueError('spacing must be finite and > 0, got %r' % (spacing,))
    h = float(spacing)
    if name == 'sphere':
        sizes = sizes * 3
    if name in ('sphere', 'ellipsoid'):
        half = sizes
        inside = lambda x, y, z: (x / sizes[0]) ** 2 + (y / sizes[1]) ** 2 + (z / sizes[2]) ** 2 <= 1.0      # noqa: E731
    elif name == 'cylinder':
        half = [sizes[0], sizes[0], sizes[1] / 2]
        inside = lambda x, y, z: (x * x + y * y <= sizes[0] ** 2) & (z.abs() <= sizes[1] / 2)      # noqa: E731
    elif name == 'torus':
        half = [sizes[0] + sizes[1], sizes[0] + sizes[1], sizes[1]]
        inside = lambda x, y, z: (torch.sqrt(x * x + y * y) - sizes[0]) ** 2 + z * z <= sizes[1] ** 2      # noqa: E731
    else:
        half = [v / 2 for v in sizes]
        inside = lambda x, y, z: (x.abs() <= sizes[0] / 2) & (y.abs() <= sizes[1] / 2) & (z.abs() <= sizes[2] / 2)      # noqa: E731
    reach = [int(math.floor(v / h)) for v in half]
    cells = 1
    for r in reach:
        cells *= 2 * r + 1
    if cells > 64 * ENVELOPE_MAX_POINTS:                                # (the bounding box alone says so, before anything is allocated)
        raise ValueError('%s at spacing %g has more than %d points: use a larger spacing' % (spec, h, ENVELOPE_MAX_POINTS))
    axes = [torch.arange(-r, r + 1, dtype=torch.float64) * h for r in reach]
    x, y, z = torch.meshgrid(*axes, indexing='ij')                      # ascending (i, j, k): k fastest
    pts = torch.stack([x, y, z], dim=-1)[inside(x, y, z)]
    if len(pts) == 0:
        raise ValueError('%s at spacing %g holds no lattice point: use a smaller spacing' % (spec, h))
    if len(pts) > ENVELOPE_MAX_POINTS:
        raise ValueError('%s at spacing %g has %d points, more than %d: use a larger spacing' % (spec, h, len(pts), ENVELOPE_MAX_POINTS))
    return pts


class EnvelopePotential(_HipPotential):
    """Envelope guidance as one HIP entry (genie_envelope_potential, csrc/envelope_kernels.hip; include/genie_hip.h states the
    mathematics): `pot(x0 [B,N,3], step) -> log p [B]`, differentiable in x0, a drop-in `twisting_function` for TwistedSampler beside
    the other built-in potentials (SumPotential adds them).  It is the one potential that says what shape the design should have:
    `points` [M, 3] with `weights` [M] (None: all 1) are the envelope -- the lattice points of a solid (envelope_shape_points), the
    atoms of an existing protein or the pseudo-atoms of a low-resolution map (load_envelope) -- in the frame the sampler works in.
    Designs are born around the origin, so with `center` (the default) the envelope's weighted centroid is moved there; center=False
    keeps the frame of the points (with a binder target, say).  Two terms, each a squared hinge over a soft minimum of squared
    distances with softness `softness` (tau, A^2):
      stay inside      every residue's soft distance a_n to the nearest points is kept at or below inside_distance (weight
                       inside_weight);
      fill it          every point's soft distance c_m to the nearest residues is kept at or below cover_distance (weight
                       cover_weight, times N / sum v so that the two terms stay comparable at any point count).
    A weight of 0 switches a term off; both 0 is a ValueError.  log p = -(E_inside + E_cover) / (2 var), var =
    xstart_variance(alphas_cumprod[step], tausq) computed on the device, so nothing on the per-step path reads device memory from the
    host; the forward keeps the gradient the kernel computes and the backward scales it.  The likelihood is unnormalised.

    Everything is validated on the host before the device is looked at; points and weights are uploaded once (`points`, `weights` as
    placed).  `describe(x)` reports every sample of x with the names of capi.ENVELOPE_REPORT: 'n_outside', 'n_uncovered' (int64),
    'max_outside', 'max_uncovered' (Angstrom beyond the two distances), 'e_envelope_inside', 'e_envelope_cover' (the weighted
    energies, before the division by 2 var): [B] tensors on the potential's device.  `distance_of(x)` is [B, N], the a_n;
    `gap_of(x)` is [B, M], the c_m.

    The defaults (inside 3 A, cover 5 A, softness 4 A^2, weights 1, tausq = 1 A^2) are design choices: no trained checkpoint is in
    the tree, so their effect on sample quality is unmeasured.  Not built: rotating or fitting the envelope to the design, assigning
    regions of it to residues, envelopes that follow a motif's placement, density-map file formats."""

    def __init__(self, n_res, alphas_cumprod, points, weights=None, inside_distance=3.0, inside_weight=1.0, cover_distance=5.0,
                 cover_weight=1.0, softness=4.0, tausq=1.0, center=True, device='cuda'):
        import math
        if isinstance(n_res, bool) or not isinstance(n_res, numbers.Integral) or not 1 <= n_res <= ENVELOPE_MAX_LENGTH:
            raise ValueError('n_res must be an integer in 1..%d, got %r' % (ENVELOPE_MAX_LENGTH, n_res))
        try:
            y = torch.as_tensor(points).detach().to(dtype=torch.float64, device='cpu')
        except (TypeError, ValueError, RuntimeError):
            raise ValueError('points must be [M, 3] coordinates, got %r' % (type(points),)) from None
        if y.dim() != 2 or y.shape[1] != 3 or not 1 <= y.shape[0] <= ENVELOPE_MAX_POINTS:
            raise ValueError('points must be [M, 3] with M in 1..%d, got %s' % (ENVELOPE_MAX_POINTS, tuple(y.shape)))
        if not bool(torch.isfinite(y).all()):
            raise ValueError('points has a coordinate that is not finite')
        v = None
        if weights is not None:
            try:
                v = torch.as_tensor(weights).detach().to(dtype=torch.float64, device='cpu')
            except (TypeError, ValueError, RuntimeError):
                raise ValueError('weights must be [M] numbers, got %r' % (type(weights),)) from None
            if tuple(v.shape) != (y.shape[0],):
                raise ValueError('weights must be [%d], one per point, got %s' % (y.shape[0], tuple(v.shape)))
            if not bool((torch.isfinite(v) & (v > 0)).all()):
                raise ValueError('every weight must be finite and > 0')
        for name, d in (('inside_distance', inside_distance), ('cover_distance', cover_distance)):
            if not (_is_scalar(d) and math.isfinite(float(d)) and float(d) > capi.ENVELOPE_EPS):
                raise ValueError('%s must be finite and above eps = %g A, got %r' % (name, capi.ENVELOPE_EPS, d))
        for name, d in (('inside_weight', inside_weight), ('cover_weight', cover_weight)):
            if not (_is_scalar(d) and math.isfinite(float(d)) and float(d) >= 0):
                raise ValueError('%s must be finite and >= 0, got %r' % (name, d))
        for name, d in (('softness', softness), ('tausq', tausq)):
            if not (_is_scalar(d) and math.isfinite(float(d)) and float(d) > 0):
                raise ValueError('%s must be finite and > 0, got %r' % (name, d))
        if float(inside_weight) == 0 and float(cover_weight) == 0:
            raise ValueError('no term enabled: inside_weight and cover_weight are both 0')
        if center:
            u = torch.ones(len(y), dtype=torch.float64) if v is None else v
            y = y - (u[:, None] * y).sum(dim=0, keepdim=True) / u.sum()
        self.inside_distance, self.inside_weight = float(inside_distance), float(inside_weight)
        self.cover_distance, self.cover_weight = float(cover_distance), float(cover_weight)
        self.softness, self.center = float(softness), bool(center)
        super().__init__(n_res, alphas_cumprod, tausq, device)
        self.M = int(y.shape[0])
        self.points = y.to(torch.float32).contiguous().to(self.device)
        self.weights = None if v is None else v.to(torch.float32).contiguous().to(self.device)

    def describe(self, x):
        """The report of every sample of x [B,N,3] (the class docstring), on the potential's device."""
        report, = self._launch(self._checked(x), self._one, want='report')               # (the energies do not depend on var)
        return _decode_report(report, capi.ENVELOPE_REPORT, capi.ENVELOPE_COUNTS)

    def distance_of(self, x):
        """[B, N] float32 on the potential's device: the soft distance a_n of every residue of every sample of x [B,N,3] to the envelope."""
        return self._launch(self._checked(x), self._one, want='distance')[0]

    def gap_of(self, x):
        """[B, M] float32 on the potential's device: the soft distance c_m of every envelope point to every sample of x [B,N,3]."""
        return self._launch(self._checked(x), self._one, want='gap')[0]

    def _launch(self, x, var, want='logp'):
        """One call of the C entry on x (f32, contiguous): (logp, grad), (report [B, 6],), (distance_out [B, N],) or (gap_out [B, M],)
        as `want` says."""
        B, f32 = x.shape[0], dict(dtype=torch.float32, device=x.device)
        outs = {'logp': lambda: [torch.empty(B, **f32), torch.empty_like(x), None, None, None],
                'report': lambda: [None, None, torch.empty(B, len(capi.ENVELOPE_REPORT), **f32), None, None],
                'distance': lambda: [None, None, None, torch.empty(B, self.n_res, **f32), None],
                'gap': lambda: [None, None, None, None, torch.empty(B, self.M, **f32)]}[want]()
        self._call('genie_envelope_potential', self._stream(), B, self.n_res, _ptr(x), self.M, _ptr(self.points), _ptr(self.weights),
                   self.softness, self.inside_distance, self.inside_weight, self.cover_distance, self.cover_weight, _ptr(var),
                   *(_ptr(t) for t in outs), *self._workspace(self.lib.genie_envelope_potential_work_bytes(B, self.n_res, self.M)))
        return tuple(t for t in outs if t is not None)


class SumPotential:
    """The sum of twisting functions: `SumPotential(a, b, ...)(x0, step) = a(x0, step) + b(x0, step) + ...`, added in that order.
    `locate` and `has_fit` are those of the first member that has a `locate` (MotifPotential); `describe` is the merge of the reports
    of every member that has one (ShapePotential, SecStructPotential), in member order, the first member winning on a key two of them
    report; `assign` is that of the first member that has one (SecStructPotential), `pairs` likewise (SheetPotential).  An attribute no
    member has is absent, so TwistedSampler's hasattr checks see through the sum."""

    def __init__(self, *potentials):
        if not potentials:
            raise ValueError('SumPotential needs at least one potential')
        self.potentials = tuple(potentials)
        for m in self.potentials:
            if hasattr(m, 'locate'):
                self.locate, self.has_fit = m.locate, getattr(m, 'has_fit', True)
                break
        if any(hasattr(m, 'describe') for m in self.potentials):
            self.describe = self._describe
        for name in ('assign', 'pairs'):
            for m in self.potentials:
                if hasattr(m, name):
                    setattr(self, name, getattr(m, name))
                    break

    def _describe(self, x):
        out = {}
        for m in self.potentials:
            if hasattr(m, 'describe'):
                for k, v in m.describe(x).items():
                    out.setdefault(k, v)
        return out

    def __call__(self, x0, step):
        total = self.potentials[0](x0, step)
        for m in self.potentials[1:]:
            total = total + m(x0, step)
        return total
