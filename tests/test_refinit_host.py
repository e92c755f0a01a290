"""The reference's parameter initialisation (pack.reference_state_dict, Denoiser.init_reference_, train.build_model) on the host:
against tests/golden/init_reference.npz (tools/make_refinit_golden.py: the reference's own Denoiser built right after seeding
random / numpy / torch) and by its own properties; and the oracle's autograd at that init against the reference's
(tests/golden/train_grads_refinit_n16_b2.npz), which is what the GPU tests of test_refinit_gpu.py lean on.  CPU only."""
import hashlib
import math
import random

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import genie_oracle as O

SEEDS = (0, 1, 1234)
CONFIGS = ('base', 'small', 'triatt')
TRUNC_STD = 0.87962566103423978          # std of a unit normal truncated to +-2 (scipy.stats.truncnorm.std(-2, 2))


def t(x):
    return torch.from_numpy(np.asarray(x))


def _config(name):
    from _oracle_backend import small_config
    from genie2_amd.config import Config
    if name == 'small':
        return small_config()
    cfg = Config()
    if name == 'triatt':
        cfg.model['include_tri_att'] = True
    return cfg


def _dims(name):
    from genie2_amd.diffusion import Genie
    return Genie(_config(name)).model.dims


def _sha(v):
    return hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest()


@pytest.fixture(scope='module')
def base_init7():
    from genie2_amd import pack
    return pack.reference_state_dict(dict(pack.BASE_DIMS), 7)


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('name', CONFIGS)
def test_reference_state_dict_equals_the_reference_fixture(name, seed):
    """key order, zero flags and every tensor of the reference Denoiser's state_dict for this seed: bit for bit (SHA-256 of the
    float32 bytes) under the numpy / scipy / torch versions the fixture was made with, otherwise the 8 probes and |max| to 1e-6 of
    |max|."""
    import scipy
    from genie2_amd import pack
    g = load_golden('init_reference')
    assert [int(s) for s in g['seeds']] == list(SEEDS) and [str(c) for c in g['configs']] == list(CONFIGS)
    recorded = tuple(str(g[k]) for k in ('numpy_version', 'scipy_version', 'torch_version'))
    exact = recorded == (np.__version__, scipy.__version__, torch.__version__)
    sd = pack.reference_state_dict(_dims(name), seed)
    pfx = f'{name}_s{seed}_'
    assert list(sd) == [str(k) for k in g[pfx + 'keys']]
    assert [k for k, _ in pack.weight_layout(_dims(name))] == list(sd)
    if not exact:
        print('library versions differ from the recorded', recorded, ': comparing probes and |max| to 1e-6 instead of hashes')
    for i, (k, v) in enumerate(sd.items()):
        assert v.dtype == torch.float32 and v.is_contiguous(), k
        assert bool((v == 0).all()) == bool(g[pfx + 'is_zero'][i]), k
        if exact:
            assert _sha(v) == str(g[pfx + 'sha256'][i]), k
        else:
            amax = float(g[pfx + 'abs_max'][i])
            n = min(8, v.numel())
            assert abs(float(v.abs().max()) - amax) <= 1e-6 * amax, k
            assert float((v.reshape(-1)[:n] - t(g[pfx + 'first8'][i][:n])).abs().max()) <= 1e-6 * amax, k


def test_modes_gates_finals_norms_and_truncated_normals(base_init7):
    """without the fixture, seed 7, base dims: gating is W = 0 / b = 1, final is all zero, LayerNorm 1 / 0, head_weights the constant;
    every truncated-normal tensor within +-2 std / 0.8796 with std = sqrt(scale / (out * in * out)) (the reference's fan as written),
    its sample std within 5 % of std from 10^4 entries on; 222 of the 396 tensors are zero."""
    from genie2_amd import pack
    sd = base_init7
    assert len(sd) == 396
    seen = {}
    for k, v in sd.items():
        mode = pack.reference_init_mode(k)
        seen[mode] = seen.get(mode, 0) + 1
        is_w = k.endswith('.weight')
        if mode == 'gating':
            assert bool((v == (0.0 if is_w else 1.0)).all()), k
        elif mode == 'final':
            assert bool((v == 0).all()), k
        elif mode == 'norm':
            assert bool((v == (1.0 if is_w else 0.0)).all()), k
        elif mode == 'head_weights':
            assert bool((v == torch.tensor(0.541324854612918, dtype=torch.float32)).all()), k
        elif mode in ('lecun', 'relu'):
            if not is_w:
                assert bool((v == 0).all()), k
                continue
            o, i = v.shape
            std = math.sqrt((2.0 if mode == 'relu' else 1.0) / (o * i * o))
            assert float(v.abs().max()) <= 2 * std / TRUNC_STD * (1 + 1e-6), k
            assert float(v.abs().max()) > 0, k
            if v.numel() >= 10 ** 4:
                assert abs(float(v.double().std()) - std) <= 0.05 * std, (k, float(v.std()), std)
        else:
            assert mode == 'torch' and is_w, k
            bound = 1 / math.sqrt(v.shape[1])               # kaiming_uniform_(a = sqrt 5): U(-1 / sqrt(in), 1 / sqrt(in))
            assert 0 < float(v.abs().max()) <= bound, k
    # tensors per mode, from the module lists of 5 pair layers and 8 structure layers (weight + bias, or weight + bias of a norm)
    assert seen == {'torch': 6, 'lecun': 2 * (5 * 4 + 8 * 6), 'relu': 2 * (5 + 16), 'gating': 2 * 30, 'final': 2 * 31, 'norm': 2 * 41, 'head_weights': 8}
    assert sum(bool((v == 0).all()) for v in sd.values()) == 222
    # a 128 x 128 lecun matrix comes out with std 6.9e-4: a thousand times smaller than 1 / sqrt(in)
    assert abs(float(sd['pair_transform_net.net.0.tri_mul_out.linear_a_p.weight'].std()) - 6.9e-4) < 0.3e-4


def test_private_generators_leave_the_global_streams_alone():
    from genie2_amd import pack
    dims = _dims('small')

    def states():
        return random.getstate(), np.random.get_state(), torch.get_rng_state().clone()

    def same(a, b):
        return (a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]
                and torch.equal(a[2], b[2]))

    keep = states()
    try:
        random.seed(11); np.random.seed(11); torch.manual_seed(11)
        before = states()
        a = pack.reference_state_dict(dims, 5)
        assert same(before, states())
        random.seed(12); np.random.seed(12); torch.manual_seed(12)
        random.random(); np.random.rand(3); torch.randn(3)
        before = states()
        b = pack.reference_state_dict(dims, 5)
        assert same(before, states())
        assert all(torch.equal(a[k], b[k]) for k in a)
    finally:
        random.setstate(keep[0]); np.random.set_state(keep[1]); torch.set_rng_state(keep[2])


def test_two_seeds_differ_in_the_95_drawn_tensors_only(base_init7):
    from genie2_amd import pack
    other = pack.reference_state_dict(dict(pack.BASE_DIMS), 8)
    differ = [k for k in base_init7 if not torch.equal(base_init7[k], other[k])]
    drawn = [k for k in base_init7 if k.endswith('.weight') and pack.reference_init_mode(k) in ('torch', 'lecun', 'relu')]
    assert len(drawn) == 95 and differ == drawn


def test_defaults_are_unchanged(tmp_path, capsys):
    """Denoiser(...) / Genie(cfg) and load_model without a seed still hold pack.random_state_dict(dims, 0); with a seed the
    untrained model carries the reference init; init_reference_ writes in place and drops nothing it should keep."""
    from genie2_amd import pack
    from genie2_amd.diffusion import Genie, load_default_model, load_model
    cfg = _config('small')
    genie = Genie(cfg)
    dims = genie.model.dims
    want = pack.random_state_dict(dims, 0)
    got = genie.model.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    root = tmp_path / 'runs'
    (root / 'tiny').mkdir(parents=True)
    (root / 'tiny' / 'configuration').write_text('name tiny\nnumPairTransformLayers 1\nnumStructureLayers 1\nnumTimesteps 50\nmaximumNumResidues 32\n')
    plain = load_model(str(root), 'tiny').model.state_dict()
    assert all(torch.equal(plain[k], want[k]) for k in want)
    ref = pack.reference_state_dict(dims, 3)
    for seeded in (load_model(str(root), 'tiny', seed=3), load_default_model(str(root), 'tiny', seed=3)):
        sd = seeded.model.state_dict()
        assert list(sd) == list(ref) and all(torch.equal(sd[k], ref[k]) for k in ref)
    params = {k: p for k, p in genie.model.named_parameters()}
    assert genie.model.init_reference_(3) is genie.model
    assert all(p is params[k] and not p.requires_grad and torch.equal(p, ref[k]) for k, p in genie.model.named_parameters())
    capsys.readouterr()


def test_build_model_starts_from_the_reference_init_or_the_checkpoint(tmp_path, capsys):
    from genie2_amd import pack, train
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = tmp_path / 'runs'
    (root / 'tiny').mkdir(parents=True)
    lines = ['name tiny', 'rootDirectory ' + str(root), 'numPairTransformLayers 1', 'numStructureLayers 1', 'numTimesteps 50', 'maximumNumResidues 32']
    cfgs = {}
    for seed in (5, 6):
        p = tmp_path / f'train{seed}.config'
        p.write_text('\n'.join(lines + [f'seed {seed}']) + '\n')
        cfgs[seed] = Config(str(p))
    (root / 'tiny' / 'configuration').write_text('\n'.join(lines) + '\n')
    keep = random.getstate(), np.random.get_state(), torch.get_rng_state().clone()
    m5 = train.build_model(cfgs[5], False)
    assert random.getstate() == keep[0] and torch.equal(torch.get_rng_state(), keep[2]) and np.array_equal(np.random.get_state()[1], keep[1][1])
    said = capsys.readouterr().out
    assert 'reference' in said and 'seed 5' in said
    dims = m5.model.dims
    ref5, sd5 = pack.reference_state_dict(dims, 5), m5.model.state_dict()
    assert list(sd5) == list(ref5) and all(torch.equal(sd5[k], ref5[k]) for k in ref5)
    assert not getattr(m5, 'checkpoint_info', None)
    sd6 = train.build_model(cfgs[6], False).model.state_dict()
    assert any(not torch.equal(sd5[k], sd6[k]) for k in sd5)
    ref6 = pack.reference_state_dict(dims, 6)
    assert all(torch.equal(sd6[k], ref6[k]) for k in ref6)
    # with a checkpoint: its weights, whatever the seed
    trained = Genie(cfgs[5])
    save_checkpoint(trained, str(root / 'tiny' / 'version_0' / 'checkpoints' / 'epoch=0.ckpt'), epoch=0, global_step=4)
    want = pack.random_state_dict(dims, 0)
    capsys.readouterr()
    for seed, weights_only in ((5, False), (6, False), (6, True)):
        m = train.build_model(cfgs[seed], weights_only)
        sd = m.model.state_dict()
        assert all(torch.equal(sd[k], want[k]) for k in want)
        assert (not m.checkpoint_info) if weights_only else (m.checkpoint_info['epoch'] == 0 and m.checkpoint_info['global_step'] == 4)
    assert 'Initialised from scratch' not in capsys.readouterr().out


def _train_features(g):
    f = O.empty_features([int(x) for x in g['lengths']])
    for k in ('residue_mask', 'chain_index', 'residue_index', 'fixed_sequence_mask', 'num_residues'):
        f[k] = t(g[k])
    f['atom_positions'] = t(g['atom_positions'])
    return f


def test_oracle_autograd_at_the_reference_init_matches_the_reference():
    """d weighted_loss / d parameter at the reference's seed-0 init: the oracle under torch autograd against the reference Denoiser's
    own autograd (tests/golden/train_grads_refinit_n16_b2.npz).  The same exactly-zero set (315 of 396: the zero final matrices
    cut the pair stack and every structure layer's attention and transition off the loss), the rest within the bars
    test_oracle_golden.py holds the oracle to on train_grads_n16_b2."""
    from genie2_amd import pack
    g = load_golden('train_grads_refinit_n16_b2')
    f = _train_features(g)
    init = pack.reference_state_dict(dict(O.BASE_DIMS), int(g['init_seed']))
    sd = {k: v.clone().requires_grad_(True) for k, v in init.items()}
    o = O.denoiser_forward(sd, O.BASE_DIMS, t(g['rots_s']), t(g['trans_s']), t(g['s']).int(), f, 'closed', t(g['quat_codes']))
    assert (o['z'].detach() - t(g['z_pred'])).abs().max() < 1e-4
    lo = O.training_loss(o['z'], t(g['z']), f, float(g['condition_loss_weight']))['weighted_loss']
    assert abs(float(lo.detach()) - float(g['loss'])) < 1e-5
    lo.backward()
    keys = [str(k) for k in g['keys']]
    assert keys == list(sd.keys())
    zero = {k for i, k in enumerate(keys) if g['grad_is_zero'][i]}
    assert len(zero) == 315 and all(float(g['grad_abs_max'][i]) == 0.0 for i, k in enumerate(keys) if k in zero)
    for i, k in enumerate(keys):
        gr = sd[k].grad if sd[k].grad is not None else torch.zeros_like(init[k])
        assert bool((gr == 0).all()) == (k in zero), k
        scale = max(float(g['grad_abs_max'][i]), 1e-6)
        assert abs(float(gr.abs().max()) - float(g['grad_abs_max'][i])) <= 5e-3 * scale, k
        assert abs(float(gr.norm()) - float(g['grad_norm'][i])) <= 5e-3 * max(float(g['grad_norm'][i]), 1e-6), k
        n = min(8, gr.numel())
        assert (gr.reshape(-1)[:n] - t(g['grad_probe'][i][:n])).abs().max() <= 5e-3 * scale, k
    # 56 zero-valued weights have a gradient (they wake up at the first step), 149 non-zero weights have none yet
    assert sum(bool((init[k] == 0).all()) and k not in zero for k in keys) == 56
    assert sum(not bool((init[k] == 0).all()) and k in zero for k in keys) == 149
