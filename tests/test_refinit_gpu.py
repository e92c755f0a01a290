"""The HIP training kernels and both sampling arithmetics AT THE REFERENCE'S OWN INITIALISATION (pack.reference_state_dict): all-zero
'final' matrices and gate matrices, every bias exactly 0 or 1, drawn matrices of size 1e-4 .. 1e-3 -- operands none of the other
GPU tests reach (they run on 'everything live' synthetic weights).  Against the reference's own autograd
(tests/golden/train_grads_refinit_n16_b2.npz) and against torch autograd over the oracle, which test_refinit_host.py pins to the
reference at this init.

Every tolerance is one the project already uses: 5e-3 of a gradient tensor's largest entry (floor 1e-5 of the largest gradient of
all), 2e-4 on z, 1e-4 on the loss, 1e-4 * max(1, |ref|) on the sampling taps.  The float32 oracle itself differs from the float64
oracle by at most 4.8e-5 of a tensor's largest entry at this init (N = 16), a factor 100 under the gradient bar.  New here: a
gradient that the reference (or both the float32 and the float64 oracle) has EXACTLY zero must be exactly zero on the device.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import genie_oracle as O

pytestmark = pytest.mark.gpu


def t(x):
    return torch.from_numpy(np.asarray(x))


def flat(sd, dims):
    from genie2_amd import pack
    return pack.flatten_state_dict(sd, dims)


def split(blob, dims):
    from genie2_amd import pack
    out, o = {}, 0
    for k, shp in pack.weight_layout(dims):
        n = int(np.prod(shp))
        out[k] = blob[o:o + n].reshape(shp)
        o += n
    assert o == blob.numel()
    return out


def _as64(x):
    return x.double() if torch.is_tensor(x) and x.is_floating_point() else x


def oracle_grads(sd, dims, rots, trans, ts, f, z, w, double=False):
    """(z, losses, {key: gradient}) of torch autograd over the oracle; float64 arithmetic on the same float32 values when `double`.
    A parameter the loss does not reach has a zero gradient."""
    cast = _as64 if double else (lambda x: x)
    sdg = {k: cast(v.detach().cpu()).clone().requires_grad_(True) for k, v in sd.items()}
    o = O.denoiser_forward(sdg, dims, cast(rots.cpu()), cast(trans.cpu()), ts.cpu().int(), f, 'closed')
    lo = O.training_loss(o['z'], cast(z.cpu()), O.prepare_features(f), w)
    lo['weighted_loss'].backward()
    return o['z'].detach(), lo, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sdg.items()}


def is_zero(x):
    return bool((x == 0).all())


def check_grads(got, ref, zero=(), tol=5e-3):
    """tests/test_training.py's rule: per tensor max |difference| <= tol x the tensor's largest magnitude, floored at 1e-5 of the
    largest gradient of all; and every tensor named in `zero` exactly zero.  Returns (worst ratio, its key)."""
    worst = (0.0, None)
    floor = 1e-5 * max(float(r.abs().max()) for r in ref.values())
    for k, r in ref.items():
        assert torch.isfinite(got[k]).all(), k
        scale = max(float(r.abs().max()), floor)
        d = float((got[k].cpu().double() - r.double()).abs().max()) / scale
        if d > worst[0]:
            worst = (d, k)
        assert d <= tol, (k, d, scale)
        if k in zero:
            assert is_zero(got[k]), (k, float(got[k].abs().max()))
    return worst


def both_zero(g32, g64):
    return {k for k in g32 if is_zero(g32[k]) and is_zero(g64[k])}


def _case(seed, lengths, motif=True):
    """tests/test_training.py's recipe: ragged batch, sample 0 with a four-residue motif"""
    g = torch.Generator().manual_seed(seed)
    f = O.empty_features(lengths)
    B, N = f['residue_mask'].shape
    if motif:
        O.add_motif(f, 0, torch.randn(4, 3, generator=g) * 4, [1, 2, 3, 9])
    x0 = torch.randn(B, N, 3, generator=g) * 4 * f['residue_mask'].unsqueeze(-1)
    f['atom_positions'] = torch.where(f['fixed_sequence_mask'].unsqueeze(-1), f['atom_positions'] + 0.0, x0)
    z = torch.randn(B, N, 3, generator=g) * f['residue_mask'].unsqueeze(-1)
    return f, z


def _golden_case():
    g = load_golden('train_grads_refinit_n16_b2')
    f = O.empty_features([int(x) for x in g['lengths']])
    for k in ('residue_mask', 'chain_index', 'residue_index', 'fixed_sequence_mask', 'num_residues'):
        f[k] = t(g[k])
    f['atom_positions'] = t(g['atom_positions'])
    return g, f


@pytest.fixture(scope='module')
def init0():
    """the reference's seed-0 initialisation of the base model"""
    from genie2_amd import pack
    return pack.reference_state_dict(dict(O.BASE_DIMS), 0)


@pytest.fixture(scope='module')
def init0_engine(init0):
    from genie2_amd.engine import GenieEngine
    eng = GenieEngine(dict(O.BASE_DIMS), init0, 'cuda:0')
    yield eng
    eng.close()


def test_gradients_at_the_reference_init_match_reference_autograd_golden(init0_engine, init0):
    """all 396 gradients against the reference Denoiser's own autograd at its own seed-0 init: |max|, norm and 8 probes within 5e-3 of
    the tensor's scale, z within 2e-4, the loss within 1e-4; the 315 gradients the reference has exactly zero are exactly zero."""
    g, f = _golden_case()
    dims = dict(O.BASE_DIMS)
    eng = init0_engine
    eng.bind_features(f)
    out = eng.train_forward_backward(flat(init0, dims).cuda(), t(g['trans_s']), t(g['rots_s']), t(g['s']).int(), t(g['z']),
                                     float(g['condition_loss_weight']), quat_codes=t(g['quat_codes']), train_mode=False, fast_math=0)
    m = t(g['residue_mask']).unsqueeze(-1).float()
    dz = float(((out['z'].cpu() - t(g['z_pred'])) * m).abs().max())
    dl = abs(float(out['weighted_loss']) - float(g['loss'])) / max(1.0, abs(float(g['loss'])))
    assert torch.isfinite(out['grads']).all() and torch.isfinite(out['z']).all()
    gr = split(out['grads'].cpu(), dims)
    keys = [str(k) for k in g['keys']]
    assert keys == list(gr.keys())
    zero = [k for i, k in enumerate(keys) if g['grad_is_zero'][i]]
    assert len(zero) >= 300
    worst, not_zero = (0.0, None), []
    for i, k in enumerate(keys):
        scale = max(float(g['grad_abs_max'][i]), 1e-6)
        n = min(8, gr[k].numel())
        errs = (abs(float(gr[k].abs().max()) - float(g['grad_abs_max'][i])) / scale,
                abs(float(gr[k].norm()) - float(g['grad_norm'][i])) / max(float(g['grad_norm'][i]), 1e-6),
                float((gr[k].reshape(-1)[:n] - t(g['grad_probe'][i][:n])).abs().max()) / scale)
        if max(errs) > worst[0]:
            worst = (max(errs), k)
        if g['grad_is_zero'][i] and not is_zero(gr[k]):
            not_zero.append((k, float(gr[k].abs().max())))
    print('reference init, N = 16: |dz| %.2e, relative loss difference %.2e, worst relative gradient difference %.2e (%s), '
          '%d of %d gradients exactly zero' % (dz, dl, worst[0], worst[1], sum(is_zero(v) for v in gr.values()), len(keys)))
    assert dz < 2e-4 and dl < 1e-4
    assert worst[0] <= 5e-3, worst
    assert not not_zero, not_zero[:8]


def test_gradients_at_the_reference_init_base_model_n128(init0_engine, init0):
    """the big-GEMM sizes (lengths [128, 101], a motif: the 128 x 128-tile GEMM, split-K with the bias sums riding along) on all-zero
    and 1e-4-sized operands: every gradient against torch autograd over the oracle, exact zeros where the float32 and the float64
    oracle both have them"""
    dims = dict(O.BASE_DIMS)
    f, z = _case(11, [128, 101])
    sched = O.training_schedule(dims['n_timestep'])
    s = torch.tensor([412, 77])
    fr = O.prepare_features(f)
    trans, rots = O.q_sample(f['atom_positions'], s, z, fr['chain_index'], fr['residue_mask'], sched)
    zo, lo, g32 = oracle_grads(init0, dims, rots, trans, s, f, z, 1.0)
    _, _, g64 = oracle_grads(init0, dims, rots, trans, s, f, z, 1.0, double=True)
    zero = both_zero(g32, g64)
    spread = max(float((g32[k].double() - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-30) for k in g32 if k not in zero)
    eng = init0_engine
    eng.bind_features(f)
    out = eng.train_forward_backward(flat(init0, dims).cuda(), trans, rots, s.int(), z, 1.0, train_mode=False, fast_math=0)
    m = fr['residue_mask'].unsqueeze(-1).float()
    dz = float(((out['z'].cpu() - zo) * m).abs().max())
    dl = abs(float(out['weighted_loss']) - float(lo['weighted_loss'].detach())) / float(lo['weighted_loss'].detach())
    print('reference init, N = 128: |dz| %.2e, relative loss difference %.2e, %d gradients zero in both oracles, float32 vs float64 oracle %.2e'
          % (dz, dl, len(zero), spread))
    assert len(zero) >= 300
    assert dz <= 2e-4 * max(1.0, float(zo.abs().max())) and dl <= 1e-4
    worst = check_grads(split(out['grads'].cpu(), dims), g32, zero)
    print('reference init, N = 128: worst relative gradient difference %.2e (%s)' % worst)


def _motif_batch(lengths, pad, seed):
    """a DataLoader-style batch: ragged, sample 0 conditioned on a four-residue motif (sequence mask and structure block)"""
    from genie2_amd import features as F
    g = torch.Generator().manual_seed(seed)
    feats = []
    for n in lengths:
        ff = F.create_empty_np_features([n])
        ff['atom_positions'] = (torch.randn(n, 3, generator=g) * 5).numpy()
        feats.append(F.pad_np_features(ff, 1, pad))
    batch = {k: torch.as_tensor(np.stack([ff[k] for ff in feats])) for k in feats[0]}
    idx = torch.tensor([2, 3, 4, 11])
    batch['fixed_sequence_mask'][0, idx] = True
    batch['fixed_structure_mask'][0, idx.unsqueeze(1), idx.unsqueeze(0)] = True
    batch['fixed_group'][0, idx] = 1
    batch['aatype'][0, idx, 3] = 1
    return batch


def test_four_adam_steps_from_the_reference_init_follow_the_oracle():
    """The cascade.  GenieTrainer on the small configuration from the reference's init (seed 3): ragged batch with a motif, eval-mode
    forward, lr 1e-3, four Adam steps.  At every step the gradient the trainer is about to use equals the oracle's AT THE TRAINER'S
    OWN WEIGHTS (trajectories are not compared weight for weight: Adam's first step is lr * sign(g)), with exact zeros where both
    oracles have them; and the number of non-zero gradient tensors grows after step 1 -- the pair stack wakes up once linear_out
    has moved."""
    from _oracle_backend import small_config, unflatten
    from genie2_amd import features as F
    from genie2_amd.diffusion import Genie
    from genie2_amd.training import GenieTrainer
    cfg = small_config()
    genie = Genie(cfg)
    genie.model.init_reference_(3)
    genie = genie.to('cuda:0')
    tr = GenieTrainer(genie, train_mode=False, seed=77)
    tr.lr = 1e-3
    dims = genie.model.dims
    batch = _motif_batch((24, 19), 24, 3)
    fo = dict(F.prepare_tensor_features(batch))
    rec = {}
    orig = tr.backend.forward_backward

    def spy(w, gbuf, trans, rots, s, z, cond_w, seed, opts, event):
        rec.update(w=w.clone(), trans=trans.clone(), rots=rots.clone(), s=s.clone(), z=z.clone())
        return orig(w, gbuf, trans, rots, s, z, cond_w, seed, opts, event)

    tr.backend.forward_backward = spy
    torch.manual_seed(1234)                     # the steps' draws of s and z come from the global generator (genie.py:72-79)
    cw = float(cfg.training['condition_loss_weight'])
    counts, worst_all = [], (0.0, None, None)
    for step in range(4):
        loss = float(tr.training_step(batch))
        assert np.isfinite(loss)
        sd = unflatten(rec['w'].cpu(), dims)
        args = (sd, dims, rec['rots'].cpu(), rec['trans'].cpu(), rec['s'].cpu(), fo, rec['z'].cpu(), cw)
        zo, lo, g32 = oracle_grads(*args)
        _, _, g64 = oracle_grads(*args, double=True)
        got = split(tr.g.cpu(), dims)
        assert abs(loss - float(lo['weighted_loss'].detach())) <= 1e-4 * loss
        zero = both_zero(g32, g64)
        worst = check_grads(got, g32, zero)
        counts.append(sum(not is_zero(v) for v in got.values()))
        print('cascade step %d: loss %.5f, %d of %d gradient tensors non-zero (oracle: %d), worst relative gradient difference %.2e (%s)'
              % (step + 1, loss, counts[-1], len(got), len(got) - len(zero), worst[0], worst[1]))
        if worst[0] > worst_all[0]:
            worst_all = (worst[0], worst[1], step + 1)
        tr.optimizer_step()
        assert torch.isfinite(tr.w).all()
    print('cascade: non-zero gradient tensors per step', counts, 'worst', worst_all)
    assert counts[1] > counts[0]


def test_narrower_arithmetics_at_the_reference_init(init0_engine, init0):
    """fast_math 1 (plain bf16 operands) and 2 (two bf16 pieces) on the N = 16 case: finite, the same exact zeros, and the whole
    gradient vector pointing where mode 0's does (the cosines, relative differences and loss bounds tests/test_training.py asks of
    the two modes)"""
    g, f = _golden_case()
    dims = dict(O.BASE_DIMS)
    eng = init0_engine
    eng.bind_features(f)
    w = flat(init0, dims).cuda()
    args = (w, t(g['trans_s']), t(g['rots_s']), t(g['s']).int(), t(g['z']), float(g['condition_loss_weight']))
    ref = eng.train_forward_backward(*args, quat_codes=t(g['quat_codes']), train_mode=False, fast_math=0)
    gr = ref['grads'].double().clone()
    keys = [str(k) for k in g['keys']]
    zero = [k for i, k in enumerate(keys) if g['grad_is_zero'][i]]
    for mode, cos_min, rel_max, loss_tol in ((2, 0.99999, 5e-3, 1e-4), (1, 0.995, 0.1, 2e-2)):
        o = eng.train_forward_backward(*args, quat_codes=t(g['quat_codes']), train_mode=False, fast_math=mode)
        assert torch.isfinite(o['grads']).all() and torch.isfinite(o['z']).all() and np.isfinite(float(o['weighted_loss']))
        gm = o['grads'].double()
        cos = float((gm * gr).sum() / (gm.norm() * gr.norm()))
        print('reference init, fast_math %d: cosine against mode 0 %.7f, relative difference %.2e, loss %.6f (mode 0 %.6f)'
              % (mode, cos, float((gm - gr).norm() / gr.norm()), float(o['weighted_loss']), float(ref['weighted_loss'])))
        parts = split(o['grads'].cpu(), dims)
        assert [k for k in zero if not is_zero(parts[k])] == []
        assert cos >= cos_min and float((gm - gr).norm() / gr.norm()) <= rel_max, (mode, cos)
        assert abs(float(o['weighted_loss']) - float(ref['weighted_loss'])) <= loss_tol * float(ref['weighted_loss'])


@pytest.mark.parametrize('lengths', [[24, 19], [256, 231]], ids=['n24', 'n256'])
def test_sampling_arithmetics_at_the_reference_init(lengths, init0_engine, init0):
    """engine.denoise in hx and f32 at the reference's init -- weights of 1e-4 and all-zero rows through the hx power-of-two
    scales -- z, states and p (and p_init) against the oracle at the project's bar, 1e-4 * max(1, |ref|)"""
    from _parity import MATH_MODES, compare_taps, failures, oracle_taps, seeded_inputs, worst
    dims = dict(O.BASE_DIMS)
    f = O.empty_features(lengths)
    if lengths[0] < 256:
        gm = torch.Generator().manual_seed(5)
        O.add_motif(f, 0, torch.randn(4, 3, generator=gm) * 4, [1, 2, 3, 9])
    trans, ts = seeded_inputs(f, dims['n_timestep'], 17)
    fr = O.prepare_features(f)
    rots = O.compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask'])
    ref = oracle_taps(init0, dims, f, rots, trans, ts)
    eng = init0_engine
    eng.bind_features(f)
    before = eng.math
    bad = []
    try:
        for mode in MATH_MODES:
            eng.set_math(mode)
            out = eng.denoise(trans, rots, ts, taps=('states', 'p_init', 'p'))
            res = compare_taps(out, ref, fr['residue_mask'])
            print('reference init, denoise N = %d, %s: worst tap %s at %.3f of its bound; |z| %.3f'
                  % (lengths[0], mode, *worst(res), float(ref['z'].abs().max())))
            bad += failures(mode, res)
    finally:
        eng.set_math(before)
    assert not bad, bad


def test_from_scratch_training_starts_at_the_reference_init(tmp_path, capsys):
    """what `python -m genie2_amd.train` does without a checkpoint: train.build_model -> device -> GenieTrainer; a checkpoint written
    before the first step holds pack.reference_state_dict(dims, seed) bit for bit; two steps (train mode, dropout on) give finite
    losses and finite weights"""
    from genie2_amd import pack, train
    from genie2_amd.config import Config
    from genie2_amd.diffusion import load_model, save_checkpoint
    from genie2_amd.training import GenieTrainer
    root = tmp_path / 'runs'
    (root / 'tiny').mkdir(parents=True)
    text = '\n'.join(['name tiny', 'rootDirectory ' + str(root), 'numPairTransformLayers 1', 'numStructureLayers 2', 'numTimesteps 50',
                      'maximumNumResidues 32', 'seed 21', 'learningRate 0.001']) + '\n'
    (root / 'tiny' / 'configuration').write_text(text)
    cfgp = tmp_path / 'train.config'
    cfgp.write_text(text)
    cfg = Config(str(cfgp))
    model = train.build_model(cfg, False).to('cuda:0')
    assert 'seed 21' in capsys.readouterr().out
    tr = GenieTrainer(model)
    ref = pack.reference_state_dict(model.model.dims, 21)
    save_checkpoint(model, str(root / 'tiny' / 'version_0' / 'checkpoints' / 'epoch=0.ckpt'), epoch=0, global_step=0, trainer=tr)
    back = load_model(str(root), 'tiny').model.state_dict()
    assert list(back) == list(ref) and all(torch.equal(back[k], ref[k]) for k in ref)
    batch = _motif_batch((24, 19), 24, 9)
    torch.manual_seed(5)
    losses = []
    for _ in range(2):
        losses.append(float(tr.training_step(batch)))
        tr.optimizer_step()
    print('from scratch at the reference init: losses', losses)
    assert all(np.isfinite(x) for x in losses) and torch.isfinite(tr.w).all() and torch.isfinite(tr.g).all()
    assert not torch.equal(tr.w.cpu(), flat(ref, model.model.dims))
