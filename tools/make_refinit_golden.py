"""Fixture generator for the reference-initialisation tests -- runs on the CPU of a development machine that has the reference
(marvinli00/genie2) checked out; never imported by a test.

    GENIE_REFERENCE=/path/to/genie2 python tools/make_refinit_golden.py

Builds the reference `Denoiser` right after `random.seed(s); np.random.seed(s); torch.manual_seed(s)` (what its train.py's
seed_everything + load_default_model amount to) and writes two data-only files under tests/golden/:

  init_reference.npz               seeds {0, 1, 1234} x {base, small (tests/_oracle_backend.small_config), base with triangular
                                   attention}: the state_dict's key list and, per tensor, the SHA-256 of its float32 bytes, its
                                   largest magnitude, its first 8 values and whether it is all zero; the numpy / scipy / torch
                                   versions in use.
  train_grads_refinit_n16_b2.npz   the reference Denoiser's own autograd at its seed-0 init on the inputs recipe of
                                   train_grads_n16_b2.npz (oracle/make_goldens.py: eval mode, eigh signs recorded): loss, z_pred
                                   and per gradient |max|, norm, 8 probes and whether it is exactly zero.

No weights and no reference source are written.  The archives carry a fixed time stamp and the arithmetic runs on one thread, so
a second run reproduces both files byte for byte.  The reference is imported as oracle/make_goldens.py does it, with the
repository root (whose `genie` package is the compatibility facade) kept off sys.path.
"""
import hashlib
import importlib.util
import io
import os
import random
import sys
import zipfile

import numpy as np
import scipy
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get('GENIE_REFERENCE')
if not REF:
    sys.exit('set GENIE_REFERENCE to a checkout of marvinli00/genie2')

_spec = importlib.util.spec_from_file_location('genie_oracle', os.path.join(ROOT, 'oracle', 'genie_oracle.py'))
O = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(O)
sys.path[:] = [p for p in sys.path if os.path.abspath(p or '.') != ROOT]
sys.path.insert(0, REF)

from genie.config import Config  # noqa: E402  (reference)
from genie.model.model import Denoiser  # noqa: E402
from genie.diffusion.schedule import get_betas  # noqa: E402
from genie.utils.affine_utils import T  # noqa: E402
from genie.utils.geo_utils import compute_frenet_frames  # noqa: E402
from genie.utils.loss import mse as ref_mse  # noqa: E402
import genie.model.pair_feature_net as ref_pfn  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
SEEDS = (0, 1, 1234)


def save(name, **arrs):
    """np.savez_compressed with a fixed time stamp in every archive member (numpy stamps the wall clock)."""
    path = os.path.join(OUT, name + '.npz')
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v.numpy() if torch.is_tensor(v) else v), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print(f'  wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)')


def configs():
    def base():
        return Config(os.path.join(REF, 'results', 'base', 'configuration'))

    small = base()                                           # tests/_oracle_backend.small_config()
    small.model['n_pair_transform_layer'] = 1
    small.model['n_structure_layer'] = 1
    small.diffusion['n_timestep'] = 50
    small.io['max_n_res'] = 32
    tri = base()
    tri.model['include_tri_att'] = True
    return {'base': base(), 'small': small, 'triatt': tri}


def seeded_denoiser(cfg, seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return Denoiser(**cfg.model, n_timestep=cfg.diffusion['n_timestep'], max_n_res=cfg.io['max_n_res'],
                    max_n_chain=cfg.io['max_n_chain'])


def first8(t):
    v = t.detach().reshape(-1)[:8].numpy()
    return np.pad(v, (0, 8 - v.size))


def gen_init():
    arrs = dict(seeds=np.array(SEEDS), configs=np.array(list(configs())), numpy_version=np.array(np.__version__),
                scipy_version=np.array(scipy.__version__), torch_version=np.array(torch.__version__))
    for name, cfg in configs().items():
        for seed in SEEDS:
            sd = seeded_denoiser(cfg, seed).state_dict()
            assert all(v.dtype == torch.float32 for v in sd.values())
            pfx = f'{name}_s{seed}_'
            arrs[pfx + 'keys'] = np.array(list(sd.keys()))
            arrs[pfx + 'sha256'] = np.array([hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() for v in sd.values()])
            arrs[pfx + 'abs_max'] = np.array([float(v.abs().max()) for v in sd.values()], dtype=np.float32)
            arrs[pfx + 'first8'] = np.stack([first8(v) for v in sd.values()]).astype(np.float32)
            arrs[pfx + 'is_zero'] = np.array([bool((v == 0).all()) for v in sd.values()])
            print(f'  {name} seed {seed}: {len(sd)} tensors, {int(arrs[pfx + "is_zero"].sum())} all zero')
    save('init_reference', **arrs)


def gen_train_grads():
    """oracle/make_goldens.py gen_train_grads at the reference's own seed-0 init instead of the synthetic weights."""
    cfg = configs()['base']
    model = seeded_denoiser(cfg, 0).eval()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(99)
    f = O.empty_features([16, 11], chains_per_sample=[[16], [5, 6]])
    B, N = f['residue_mask'].shape
    f['fixed_sequence_mask'][0, 2:6] = True
    f['atom_positions'] = torch.randn(B, N, 3, generator=g) * 6 * f['residue_mask'].unsqueeze(-1)
    betas = get_betas(cfg.diffusion['n_timestep'], 'cosine')
    ac = torch.cumprod(1. - betas, 0)
    s = torch.tensor([700, 40])
    z = torch.randn(B, N, 3, generator=g) * f['residue_mask'].unsqueeze(-1)
    trans_s = torch.sqrt(ac)[s].view(-1, 1, 1) * f['atom_positions'] + torch.sqrt(1. - ac)[s].view(-1, 1, 1) * z
    rots_s = compute_frenet_frames(trans_s, f['chain_index'], f['residue_mask'])
    feats = O.prepare_features(f)
    record = []
    orig = ref_pfn.rot_to_quat

    def rec_q(r):
        q = orig(r)
        record.append(q.detach())
        return q

    ref_pfn.rot_to_quat = rec_q
    try:
        out = model(T(rots_s, trans_s), s.int(), feats)
    finally:
        ref_pfn.rot_to_quat = orig
    w = 2.0
    rm, fs = f['residue_mask'], f['fixed_sequence_mask']
    cm, im = rm * fs, rm * ~fs
    cl = ref_mse(out['z'], z, cm, aggregate='sum')
    il = ref_mse(out['z'], z, im, aggregate='sum')
    loss = torch.mean((w * cl + il) / (w * torch.sum(cm, dim=-1) + torch.sum(im, dim=-1)))
    loss.backward()
    ref_grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    keys = list(ref_grads.keys())
    is_zero = np.array([bool((ref_grads[k] == 0).all()) for k in keys])
    # the oracle restatement under autograd, same quaternion signs: the same exact zeros, the rest within the oracle's bar
    codes = O.quat_sign_codes(record[0])
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    o = O.denoiser_forward(sdg, O.BASE_DIMS, rots_s, trans_s, s.int(), f, 'closed', codes)
    lo = O.training_loss(o['z'], z, f, w)['weighted_loss']
    lo.backward()
    worst = 0.0
    for i, k in enumerate(keys):
        mine = sdg[k].grad if sdg[k].grad is not None else torch.zeros_like(sdg[k])
        assert bool((mine == 0).all()) == bool(is_zero[i]), k
        scale = max(float(ref_grads[k].abs().max()), 1e-6)
        worst = max(worst, float((mine - ref_grads[k]).abs().max()) / scale)
    nz = [float(ref_grads[k].abs().max()) for i, k in enumerate(keys) if not is_zero[i]]
    print('  loss ref %.6f oracle %.6f; worst relative gradient difference %.2e over %d tensors, %d exactly zero; '
          'largest entry %.3g, smallest non-zero tensor peaks at %.3g'
          % (float(loss), float(lo), worst, len(keys), int(is_zero.sum()), max(nz), min(nz)))
    assert abs(float(loss) - float(lo)) < 1e-5 and worst < 5e-3
    save('train_grads_refinit_n16_b2', atom_positions=f['atom_positions'], residue_mask=f['residue_mask'],
         chain_index=f['chain_index'], residue_index=f['residue_index'], fixed_sequence_mask=f['fixed_sequence_mask'],
         num_residues=f['num_residues'], lengths=np.array([16, 11]), chain_lengths=np.array([16, 0, 5, 6]), s=s, z=z,
         trans_s=trans_s, rots_s=rots_s, quat_codes=codes, condition_loss_weight=np.float32(w), init_seed=np.int64(0),
         loss=loss.detach(), z_pred=out['z'].detach(), keys=np.array(keys), grad_is_zero=is_zero,
         grad_abs_max=np.array([float(ref_grads[k].abs().max()) for k in keys], dtype=np.float32),
         grad_norm=np.array([float(ref_grads[k].norm()) for k in keys], dtype=np.float32),
         grad_probe=np.stack([first8(ref_grads[k]) for k in keys]).astype(np.float32))


if __name__ == '__main__':
    torch.set_num_threads(1)
    print('init'); gen_init()
    print('train gradients at the seed-0 init'); gen_train_grads()
