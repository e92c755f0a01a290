"""Triangular attention, everything that needs no GPU: the torch composition of tests/_triatt.py against the reference's recorded
call (which pins the yardstick of the GPU tests to the reference), the weight layout, the Denoiser's parameters, genie_create's
argument check and the refusals of the training / twisted-sampling wrappers."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from conftest import golden_features, load_golden
from oracle import genie_oracle as O
import _triatt as TA


@pytest.fixture(scope='module')
def golden():
    return load_golden(TA.GOLDEN)


def golden_dims(g):
    return TA.tri_dims(O.small_dims(), int(g['dims_c_hidden_tri_att']), int(g['dims_n_head_tri']))


def test_composition_reproduces_the_reference_call(golden):
    """z, p, states and p after layer 0's tri_att_end of the reference Denoiser(include_tri_att=True), to float32 rounding:
    1e-5 * max(1, |ref|).  (The module alone agrees with the reference's to 4.8e-7.)"""
    g = golden
    dims = golden_dims(g)
    sd = TA.full_state_dict(dims, int(g['seed']))
    f = golden_features(g)
    out = TA.composed_taps(sd, dims, f, torch.from_numpy(g['rots']), torch.from_numpy(g['trans']), torch.from_numpy(g['timesteps']),
                           sign_codes=torch.from_numpy(g['quat_codes']))
    rm = f['residue_mask']
    m3 = rm.unsqueeze(-1).float()
    for name, got, want in (('z', out['z'] * m3, torch.from_numpy(g['z']) * m3), ('p', out['p'], torch.from_numpy(g['p'])),
                            ('states', out['states'] * m3, torch.from_numpy(g['states']) * m3)):
        err, ref = float((got - want).abs().max()), float(want.abs().max())
        print(f'{name}: {err:.2e} at |ref| {ref:.3f}')
        assert err <= 1e-5 * max(1.0, ref), (name, err, ref)
    err, scale = TA.tap_error(out['p_tri_att0'], torch.from_numpy(g['p_tri_att0']), rm)
    print(f'p_tri_att0: {err:.2e} at scale {scale:.3f}')
    assert err <= 1e-5 * scale
    assert torch.isfinite(out['p_tri_att0']).all()


def test_weight_layout_matches_the_reference_state_dict(golden):
    from genie2_amd import capi, pack
    g = golden
    dims = golden_dims(g)
    lay = pack.weight_layout(dims)
    assert [k for k, _ in lay] == [str(k) for k in g['keys']]
    assert [','.join(str(x) for x in s) for _, s in lay] == [str(s) for s in g['shapes']]
    n = sum(int(np.prod(s)) for _, s in lay)
    assert n == int(g['n_param'])
    lib = capi.load_library()
    assert n == lib.genie_weight_count(C.byref(capi.GenieDims(**pack.engine_dims(dims))))
    # one module at the defaults: 82 944 parameters; (16, 8) has the same widths
    base = sum(int(np.prod(s)) for _, s in pack.weight_layout(O.small_dims()))
    assert n - base == 2 * dims['n_pair_transform_layer'] * 82944
    # the default model is untouched, in the layout and in the library
    assert pack.DIM_KEYS == tuple(k for k in pack.DIM_KEYS if k not in pack.TRI_DIM_KEYS) and not set(pack.TRI_DIM_KEYS) & set(pack.BASE_DIMS)
    assert sum(int(np.prod(s)) for _, s in pack.weight_layout(pack.BASE_DIMS)) == 15732080
    assert lib.genie_weight_count(C.byref(capi.GenieDims(**{k: pack.BASE_DIMS[k] for k in pack.DIM_KEYS}))) == 15732080
    full = TA.tri_dims(pack.BASE_DIMS)
    assert lib.genie_weight_count(C.byref(capi.GenieDims(**pack.engine_dims(full)))) == 15732080 + 10 * 82944
    # the recipe's dict flattens, and random_state_dict covers the new keys with live values
    sd = TA.full_state_dict(dims, 0)
    assert pack.flatten_state_dict(sd, dims).numel() == n
    rs = pack.random_state_dict(dims, seed=1)
    assert list(rs) == [k for k, _ in lay]
    assert all(float(rs[k].abs().max()) > 0 for k in rs if 'tri_att' in k)
    assert float(rs['pair_transform_net.net.0.tri_att_end.mha.linear_g.bias'].mean()) > 0.5


def test_denoiser_constructs_from_a_config_with_the_option(golden, tmp_path):
    """Fails without the feature: the constructor used to raise NotImplementedError."""
    from genie2_amd.config import Config
    from genie2_amd.model import Denoiser
    cfg = Config(TA.write_config(str(tmp_path / 'configuration'), numPairTransformLayers=2, numStructureLayers=2, numTimesteps=100))
    assert cfg.model['include_tri_att'] is True and cfg.model['c_hidden_tri_att'] == 32 and cfg.model['n_head_tri'] == 4
    m = Denoiser(**cfg.model, n_timestep=cfg.diffusion['n_timestep'], max_n_res=cfg.io['max_n_res'], max_n_chain=cfg.io['max_n_chain'])
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in golden['keys']]
    assert [','.join(str(x) for x in v.shape) for v in sd.values()] == [str(s) for s in golden['shapes']]
    assert sum(v.numel() for v in sd.values()) == int(golden['n_param'])
    assert m.dims['n_head_tri'] == 4 and m.dims['c_hidden_tri_att'] == 32
    m.load_state_dict(TA.full_state_dict(golden_dims(golden), 0), strict=True)
    # without the option: today's parameters, and a zero tail for the library
    cfg0 = Config()
    m0 = Denoiser(**cfg0.model, n_timestep=10, max_n_res=256, max_n_chain=1)
    assert not any('tri_att' in k for k in m0.state_dict()) and m0.dims['n_head_tri'] == 0 and m0.dims['c_hidden_tri_att'] == 0


def test_create_refuses_unsupported_head_shapes():
    from genie2_amd import capi, pack
    lib = capi.load_library()

    def create(c, H):
        h = C.c_void_p()
        rc = lib.genie_create(C.byref(capi.GenieDims(**pack.engine_dims(TA.tri_dims(pack.BASE_DIMS, c, H)))), 0, C.byref(h))
        return rc, h, lib.genie_last_error(None)

    for (c, H), word in (((32, 3), b'n_head_tri'), ((32, 8), b'n_head_tri'), ((64, 2), b'c_hidden_tri_att'), ((8, 16), b'c_hidden_tri_att'),
                         ((24, 4), b'c_hidden_tri_att'), ((32, -1), b'n_head_tri')):
        rc, h, msg = create(c, H)
        assert rc == -1 and not h.value and word in msg, ((c, H), rc, msg)
    for c, H in ((32, 4), (16, 8), (0, 0), (99, 0)):      # supported, or no attention at all (its width is then ignored)
        rc, h, msg = create(c, H)
        assert rc != -1, ((c, H), msg)
        if rc == 0:
            lib.genie_destroy(h)


def _tri_model():
    from genie2_amd.config import Config
    from genie2_amd.model import Denoiser
    cfg = Config()
    cfg.model.update(include_tri_att=True, n_pair_transform_layer=1, n_structure_layer=1)
    m = Denoiser(**cfg.model, n_timestep=10, max_n_res=64, max_n_chain=1)
    return types.SimpleNamespace(model=m, config=cfg, device=torch.device('cpu'), setup_schedule=lambda: None)


def test_trainer_and_twisted_sampler_refuse_the_option():
    from genie2_amd.smc import TwistedSampler
    from genie2_amd.training import GenieTrainer
    genie = _tri_model()
    with pytest.raises(NotImplementedError, match='triangular attention: sampling only'):
        GenieTrainer(genie)
    with pytest.raises(NotImplementedError, match='triangular attention: sampling only'):
        TwistedSampler(genie)
