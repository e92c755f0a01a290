"""Fixture generator for the triangular-attention tests -- runs on the CPU of a development machine that has the reference
(marvinli00/genie2) checked out; never imported by a test.

    GENIE_REFERENCE=/path/to/genie2 python tools/make_triatt_golden.py

Builds the reference `Denoiser` with include_tri_att=True at the oracle's small depth, loads O.synthetic_state_dict plus the
attention tensors of tests/_triatt.py's seeded recipe, runs one ragged call (B = 2, N = 24, the second entry half padded, one
motif) and writes tests/golden/triatt_call_n24_b2.npz: inputs, recorded quaternion sign codes, the state-dict key / shape lists,
the parameter count, and the outputs z, p, states and p after layer 0's tri_att_end (forward hook; zeroed at padded pairs, where
the value is free).  Only data is written: no weights (the tests rebuild them from the recipe) and no reference source.
The reference is imported as oracle/make_goldens.py does it, with the repository root (whose `genie` package is the
compatibility facade) kept off sys.path.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get('GENIE_REFERENCE')
if not REF:
    sys.exit('set GENIE_REFERENCE to a checkout of marvinli00/genie2')


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


# tests/_triatt.py does `from oracle import genie_oracle`: load both by path, then drop the repository root from sys.path
sys.path.insert(0, ROOT)
from oracle import genie_oracle as O  # noqa: E402
TA = _load('_triatt', os.path.join(ROOT, 'tests', '_triatt.py'))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or '.') != ROOT]
sys.path.insert(0, REF)

from genie.config import Config  # noqa: E402  (reference)
from genie.model.model import Denoiser  # noqa: E402
from genie.utils.affine_utils import T  # noqa: E402
from genie.utils.geo_utils import compute_frenet_frames  # noqa: E402
import genie.model.pair_feature_net as ref_pfn  # noqa: E402


def main():
    dims = TA.tri_dims(O.small_dims())
    seed = TA.GOLDEN_SEED
    cfg = Config(os.path.join(REF, 'results', 'base', 'configuration'))
    cfg.diffusion['n_timestep'] = dims['n_timestep']
    cfg.model.update(include_tri_att=True, c_hidden_tri_att=dims['c_hidden_tri_att'], n_head_tri=dims['n_head_tri'],
                     n_pair_transform_layer=dims['n_pair_transform_layer'], n_structure_layer=dims['n_structure_layer'])
    model = Denoiser(**cfg.model, n_timestep=cfg.diffusion['n_timestep'], max_n_res=cfg.io['max_n_res'],
                     max_n_chain=cfg.io['max_n_chain']).eval()
    sd = TA.full_state_dict(dims, seed)
    ref_sd = model.state_dict()
    keys = list(ref_sd.keys())
    shapes = [tuple(v.shape) for v in ref_sd.values()]
    assert set(keys) == set(sd.keys()), 'recipe and reference disagree on the key set'
    model.load_state_dict(sd, strict=True)
    n_param = sum(v.numel() for v in ref_sd.values())

    B, N = 2, 24
    f = O.empty_features([N, N // 2])
    g = torch.Generator().manual_seed(31)
    ca = 3.0 * torch.randn(5, 3, generator=g)
    O.add_motif(f, 0, ca - ca.mean(0, keepdim=True), [4, 5, 6, 15, 16])
    trans = 2.5 * torch.randn(B, N, 3, generator=g)
    fr = O.prepare_features(f)
    rots = compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask'])
    ts = torch.tensor([37, 80], dtype=torch.int32)

    rec, taps = [], {}
    orig = ref_pfn.rot_to_quat

    def rec_q(r):
        q = orig(r)
        rec.append(q)
        return q

    ref_pfn.rot_to_quat = rec_q
    hook = model.pair_transform_net.net[0].tri_att_end.register_forward_hook(
        lambda m, i, o: taps.__setitem__('p_tri_att0', i[0] + o))          # p + tri_att_end(p): eval-mode dropout is the identity
    try:
        with torch.no_grad():
            out = model(T(rots, trans), ts, fr)
    finally:
        ref_pfn.rot_to_quat = orig
        hook.remove()
    codes = O.quat_sign_codes(rec[0])

    # the restatement against the reference (closed-form quaternions with the recorded signs)
    mine = TA.composed_taps(sd, dims, f, rots, trans, ts, sign_codes=codes)
    rm = fr['residue_mask']
    pm = (rm.unsqueeze(1) * rm.unsqueeze(2)).unsqueeze(-1).float()
    m3 = rm.unsqueeze(-1).float()
    for name, a, b in (('z', out['z'] * m3, mine['z'] * m3), ('p', out['p'], mine['p']),
                       ('states', out['states'] * m3, mine['states'] * m3), ('p_tri_att0', taps['p_tri_att0'] * pm, mine['p_tri_att0'] * pm)):
        err, ref = float((a - b).abs().max()), float(a.abs().max())
        print(f'  {name}: restatement vs reference {err:.2e} at |ref| {ref:.3f}')
        assert err <= 1e-5 * max(1.0, ref), name
    assert torch.isfinite(taps['p_tri_att0']).all()

    path = os.path.join(ROOT, 'tests', 'golden', TA.GOLDEN + '.npz')
    np.savez_compressed(
        path, seed=seed, timesteps=ts.numpy(), trans=trans.numpy(), rots=rots.numpy(), quat_codes=codes.numpy(),
        keys=np.array(keys), shapes=np.array([','.join(str(x) for x in s) for s in shapes]), n_param=n_param,
        dims_c_hidden_tri_att=dims['c_hidden_tri_att'], dims_n_head_tri=dims['n_head_tri'],
        z=out['z'].numpy(), p=out['p'].numpy(), states=out['states'].numpy(), p_tri_att0=(taps['p_tri_att0'] * pm).numpy(),
        **{('f_' + k): v.numpy() for k, v in f.items()})
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB), {n_param} parameters, {len(keys)} tensors')


if __name__ == '__main__':
    main()
