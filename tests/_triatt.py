"""Helpers of test_triatt_host.py / test_triatt_gpu.py: the triangular attention of the pair stack restated in torch
(genie/model/modules/triangular_attention.py:30-144 on primitives.py:163-281, eval mode), the seeded recipe of its weights,
and the whole denoiser composed from the oracle's own functions with the two attention modules inserted between the incoming
triangle multiplication and the pair transition (pair_transform_net.py:109-119).  The arithmetic follows the dtype of the
weights, as in the oracle: float64 weights, frames and coordinates give a float64 result."""
import math

import torch
import torch.nn.functional as F

from oracle import genie_oracle as O

TRI_DIM_KEYS = ('c_hidden_tri_att', 'n_head_tri')
MODULES = ('tri_att_start', 'tri_att_end')
GOLDEN = 'triatt_call_n24_b2'
GOLDEN_SEED = 2


def tri_dims(base, c=32, H=4):
    d = dict(base)
    d.update(c_hidden_tri_att=c, n_head_tri=H)
    return d


def tri_module_template(pfx, c_p, c, H):
    """[(key, shape)] of one TriangleAttention module in state_dict order."""
    return [(pfx + 'layer_norm.weight', (c_p,)), (pfx + 'layer_norm.bias', (c_p,)), (pfx + 'linear.weight', (H, c_p)),
            (pfx + 'mha.linear_q.weight', (H * c, c_p)), (pfx + 'mha.linear_k.weight', (H * c, c_p)),
            (pfx + 'mha.linear_v.weight', (H * c, c_p)), (pfx + 'mha.linear_o.weight', (c_p, H * c)),
            (pfx + 'mha.linear_o.bias', (c_p,)), (pfx + 'mha.linear_g.weight', (H * c, c_p)), (pfx + 'mha.linear_g.bias', (H * c,))]


def tri_state_dict(dims, seed):
    """The attention tensors alone, from one generator seeded with 7919 + seed, layer by layer, start before end, keys in
    state_dict order: matrices N(0, 1 / fan_in), LayerNorm gamma 1 + 0.1 randn and beta 0.1 randn, biases 0.1 randn with + 1 on
    linear_g.bias (the reference's gating init); linear_o is NOT zero (its 'final' init would leave the module without effect)."""
    g = torch.Generator().manual_seed(7919 + seed)
    sd = {}
    for l in range(dims['n_pair_transform_layer']):
        for mod in MODULES:
            for key, shape in tri_module_template(f'pair_transform_net.net.{l}.{mod}.', dims['c_p'], dims['c_hidden_tri_att'], dims['n_head_tri']):
                if key.endswith('layer_norm.weight'):
                    t = 1.0 + 0.1 * torch.randn(shape, generator=g)
                elif key.endswith('bias'):
                    t = 0.1 * torch.randn(shape, generator=g) + (1.0 if key.endswith('linear_g.bias') else 0.0)
                else:
                    t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
                sd[key] = t.float().contiguous()
    return sd


def full_state_dict(dims, seed):
    """O.synthetic_state_dict(dims, seed) with the attention tensors at their place in the reference's order (after tri_mul_in.*,
    before pair_transition.* of each layer)."""
    base = O.synthetic_state_dict(dims, seed)
    tri = tri_state_dict(dims, seed)
    out = {}
    for key, val in base.items():
        if '.pair_transition.layer_norm.weight' in key:
            pfx = key[:key.index('pair_transition.')]
            out.update({k: v for k, v in tri.items() if k.startswith(pfx)})
        out[key] = val
    assert len(out) == len(base) + len(tri)
    return out


def triangle_attention(sd, pfx, p, pair_mask, starting, c, H, chunk=32):
    """One TriangleAttention{Starting,Ending}Node, rows in chunks (the logits of a chunk are [B, chunk, H, N, N])."""
    x = p if starting else p.transpose(1, 2)
    m = pair_mask if starting else pair_mask.transpose(1, 2)
    x = O._ln(sd, pfx + 'layer_norm', x)
    B, N = x.shape[:2]
    tb = F.linear(x, sd[pfx + 'linear.weight']).permute(0, 3, 1, 2)                       # [B,H,q,k]
    out = torch.empty_like(x)
    for i0 in range(0, N, chunk):
        xs = x[:, i0:i0 + chunk]
        n = xs.shape[1]
        q = F.linear(xs, sd[pfx + 'mha.linear_q.weight']).view(B, n, N, H, c).permute(0, 1, 3, 2, 4)
        k = F.linear(xs, sd[pfx + 'mha.linear_k.weight']).view(B, n, N, H, c).permute(0, 1, 3, 2, 4)
        v = F.linear(xs, sd[pfx + 'mha.linear_v.weight']).view(B, n, N, H, c).permute(0, 1, 3, 2, 4)
        a = torch.matmul(q, k.transpose(-1, -2)) * (1 / math.sqrt(c))                       # [B,n,H,q,k]
        a = a + (1e9 * (m[:, i0:i0 + chunk] - 1))[:, :, None, None, :]
        a = a + tb[:, None]
        a = torch.softmax(a, dim=-1)
        o = torch.matmul(a, v).permute(0, 1, 3, 2, 4)                                       # [B,n,q,H,c]
        g = torch.sigmoid(F.linear(xs, sd[pfx + 'mha.linear_g.weight'], sd[pfx + 'mha.linear_g.bias'])).view(B, n, N, H, c)
        out[:, i0:i0 + chunk] = F.linear((o * g).reshape(B, n, N, H * c), sd[pfx + 'mha.linear_o.weight'], sd[pfx + 'mha.linear_o.bias'])
    return out if starting else out.transpose(1, 2)


def pair_transform_net(sd, dims, p, features, taps=None):
    """pair_transform_net.py:109-119 in eval mode with include_tri_att."""
    rm = features['residue_mask']
    pm = (rm.unsqueeze(1) * rm.unsqueeze(2)).to(p.dtype)
    c, H = dims['c_hidden_tri_att'], dims['n_head_tri']
    for l in range(dims['n_pair_transform_layer']):
        pfx = f'pair_transform_net.net.{l}.'
        p = p + O.triangle_multiplication(sd, pfx + 'tri_mul_out.', p, pm, True)
        p = p + O.triangle_multiplication(sd, pfx + 'tri_mul_in.', p, pm, False)
        p = p + triangle_attention(sd, pfx + 'tri_att_start.', p, pm, True, c, H)
        p = p + triangle_attention(sd, pfx + 'tri_att_end.', p, pm, False, c, H)
        if taps is not None and l == 0:
            taps['p_tri_att0'] = p
        p = p + O.pair_transition(sd, pfx + 'pair_transition.', p, pm)
        p = p * pm.unsqueeze(-1)
    return p


def denoiser_forward(sd, dims, rots, trans, timesteps, features, quat_mode='closed', sign_codes=None, taps=None):
    """O.denoiser_forward with the pair transform net above."""
    f = O.prepare_features(features)
    f['atom_positions'] = f['atom_positions'].to(trans.dtype)
    trans0 = trans
    trans = trans * dims['rescale']
    N = trans.shape[1]
    s = O.single_feature_net(sd, dims, timesteps, f, N)
    p = O.pair_feature_net(sd, dims, s, rots, trans, f, quat_mode, sign_codes, taps)
    if taps is not None:
        taps['p_init'] = p
    p = pair_transform_net(sd, dims, p, f, taps)
    s_fin, r_out, t_out = O.structure_net(sd, dims, s, p, rots, trans, f, taps)
    t_out = t_out * (1. / dims['rescale'])
    return dict(z=trans0 - t_out, s=s, p=p, s_final=s_fin, rots=r_out, trans=t_out)


def as64(x):
    return x.double() if torch.is_tensor(x) and x.is_floating_point() else x


def composed_taps(sd, dims, features, rots, trans, ts, double=False, sign_codes=None):
    """z, states, p_init, p, p_tri_att0 of the composition (canonical quaternion signs unless codes are given)."""
    cast = as64 if double else (lambda x: x)
    taps = {}
    with torch.no_grad():
        o = denoiser_forward({k: cast(v) for k, v in sd.items()}, dims, cast(rots.cpu()), cast(trans), ts, features, 'closed', sign_codes, taps)
    return dict(z=o['z'], states=taps['states'], p_init=taps['p_init'], p=o['p'], p_tri_att0=taps['p_tri_att0'])


def sample_loop(sd, dims, features, noise, scale):
    """O.sample_loop around the composed denoiser."""
    f = O.prepare_features(features)

    def den(rots, trans, ts):
        with torch.no_grad():
            return denoiser_forward(sd, dims, rots, trans, ts, f, 'closed')['z']
    return O.sample_loop(sd, dims, features, noise, scale, denoiser=den)


def tap_error(got, want, residue_mask):
    """(max |got - want| over VALID pairs, bound scale max(1, |want|_inf over them)) of p_tri_att0: what the attention leaves at
    padded pairs is free (the layer's closing p *= mask removes it), so only valid pairs are compared."""
    m = residue_mask.to(got.device).double()
    pm = (m.unsqueeze(1) * m.unsqueeze(2)).unsqueeze(-1)
    g, w = got.double() * pm, want.to(got.device).double() * pm
    return float((g - w).abs().max()), max(1.0, float(w.abs().max()))


def write_config(path, name='triatt', **extra):
    """A reference-format configuration file with the option on."""
    lines = {'name': name, 'includeTriangularAttention': 'True'}
    lines.update(extra)
    with open(path, 'w') as fh:
        for k, v in lines.items():
            fh.write(f'{k} {v}\n')
    return path
