"""Host-side packing for libgenie_hip.so: the weight blob, the sinusoidal
tables and the diffusion schedule.

Key names / shapes follow the reference `Denoiser.state_dict()`
(genie/model/model.py:76-123 and sub-modules); checkpoint
files prefix them with 'model.' (genie/diffusion/ddpm.py:26,
genie/utils/model_io.py:159-173).
"""
import math

import torch

DIM_KEYS = (
    'c_s', 'c_p', 'c_pos_emb', 'c_chain_emb', 'c_timestep_emb', 'relpos_k', 'template_dist_n_bin',
    'template_dist_min', 'template_dist_step', 'n_pair_transform_layer', 'c_hidden_mul', 'pair_transition_n',
    'n_structure_layer', 'n_structure_block', 'c_hidden_ipa', 'n_head_ipa', 'n_qk_point', 'n_v_point',
    'rescale', 'n_timestep', 'max_n_res', 'max_n_chain')
# Triangular attention (include_tri_att): per-head width and number of heads.  They travel apart from DIM_KEYS, whose contents
# are the frozen dims dict of the oracle; absent or n_head_tri == 0 means "no triangular attention".
TRI_DIM_KEYS = ('c_hidden_tri_att', 'n_head_tri')


def engine_dims(dims):
    """The fields of genie_dims_t from a dims dict: DIM_KEYS as they are, TRI_DIM_KEYS defaulting to 0."""
    out = {k: dims[k] for k in DIM_KEYS}
    out.update({k: int(dims.get(k, 0) or 0) for k in TRI_DIM_KEYS})
    if out['n_head_tri'] == 0:
        out['c_hidden_tri_att'] = 0
    return out


def chain_table_rows(dims):
    """The rows of the chain-embedding table GenieEngine uploads by default: the chains one structure may hold."""
    return max(int(dims['max_n_chain']), 8)


def _linear(out, prefix, o, i, bias=True):
    out.append((prefix + '.weight', (o, i)))
    if bias:
        out.append((prefix + '.bias', (o,)))


def _norm(out, prefix, c):
    out.append((prefix + '.weight', (c,)))
    out.append((prefix + '.bias', (c,)))


def weight_layout(dims):
    """Ordered [(key, shape)] of every Denoiser parameter (with dims['n_head_tri'] > 0: including the two triangular
    attention modules of every pair transform layer, between tri_mul_in.* and pair_transition.* as in the reference)."""
    d = dims
    c_s, c_p, ch = d['c_s'], d['c_p'], d['c_hidden_mul']
    H, C, Pq, Pv = d['n_head_ipa'], d['c_hidden_ipa'], d['n_qk_point'], d['n_v_point']
    nbin = d['template_dist_n_bin']
    lay = []
    _linear(lay, 'single_feature_net.linear', c_s, d['c_pos_emb'] + d['c_chain_emb'] + d['c_timestep_emb'] + 23, False)
    pf = 'pair_feature_net.'
    _linear(lay, pf + 'linear_s_p_i', c_p, c_s, False)
    _linear(lay, pf + 'linear_s_p_j', c_p, c_s, False)
    _linear(lay, pf + 'linear_relpos', c_p, 2 * d['relpos_k'] + 3, False)
    _linear(lay, pf + 'linear_template', c_p, nbin + 6, False)
    _linear(lay, pf + 'linear_motif_template', c_p, nbin + 2, False)
    for layer in range(d['n_pair_transform_layer']):
        base = f'pair_transform_net.net.{layer}.'
        for direction in ('tri_mul_out.', 'tri_mul_in.'):
            t = base + direction
            for name in ('linear_a_p', 'linear_a_g', 'linear_b_p', 'linear_b_g'):
                _linear(lay, t + name, ch, c_p)
            _linear(lay, t + 'linear_g', c_p, c_p)
            _linear(lay, t + 'linear_z', c_p, ch)
            _norm(lay, t + 'layer_norm_in', c_p)
            _norm(lay, t + 'layer_norm_out', ch)
        ht, ct = int(d.get('n_head_tri', 0) or 0), int(d.get('c_hidden_tri_att', 0) or 0)
        for node in (('tri_att_start.', 'tri_att_end.') if ht > 0 else ()):       # triangular_attention.py:57-65, primitives.py:203-217
            t = base + node
            _norm(lay, t + 'layer_norm', c_p)
            _linear(lay, t + 'linear', ht, c_p, False)
            for name in ('linear_q', 'linear_k', 'linear_v'):
                _linear(lay, t + 'mha.' + name, ht * ct, c_p, False)
            _linear(lay, t + 'mha.linear_o', c_p, ht * ct)
            _linear(lay, t + 'mha.linear_g', ht * ct, c_p)
        t = base + 'pair_transition.'
        _norm(lay, t + 'layer_norm', c_p)
        _linear(lay, t + 'linear_1', d['pair_transition_n'] * c_p, c_p)
        _linear(lay, t + 'linear_2', c_p, d['pair_transition_n'] * c_p)
    for layer in range(d['n_structure_layer']):
        base = f'structure_net.net.{layer}.'
        lay.append((base + 'ipa.head_weights', (H,)))
        _linear(lay, base + 'ipa.linear_q', H * C, c_s)
        _linear(lay, base + 'ipa.linear_kv', 2 * H * C, c_s)
        _linear(lay, base + 'ipa.linear_q_points', 3 * H * Pq, c_s)
        _linear(lay, base + 'ipa.linear_kv_points', 3 * H * (Pq + Pv), c_s)
        _linear(lay, base + 'ipa.linear_b', H, c_p)
        _linear(lay, base + 'ipa.linear_out', c_s, H * (c_p + C + 4 * Pv))
        _norm(lay, base + 'ipa_layer_norm', c_s)
        for k in (1, 2, 3):
            _linear(lay, base + f'transition.layers.0.linear_{k}', c_s, c_s)
        _norm(lay, base + 'transition.layer_norm', c_s)
        _linear(lay, base + 'bb_update.linear', 6, c_s)
    return lay


def flatten_state_dict(state_dict, dims):
    """state_dict -> one contiguous fp32 CPU tensor in `weight_layout` order
    (the `blob` argument of genie_load_weights).  Accepts keys with or without
    the checkpoint's 'model.' prefix; refuses missing keys and wrong shapes."""
    parts = []
    for key, shape in weight_layout(dims):
        t = state_dict.get(key)
        if t is None:
            t = state_dict.get('model.' + key)
        if t is None:
            raise KeyError(f'state_dict lacks {key}')
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'{key}: expected shape {tuple(shape)}, got {tuple(t.shape)}')
        parts.append(t.detach().to('cpu', torch.float32).reshape(-1))
    return torch.cat(parts).contiguous()


def sinusoidal_table(n_rows, N, D):
    """Row v = sinusoidal_encoding(v, N, D) for v = 0..n_rows-1, evaluated with
    the same fp32 torch expression as genie/utils/encoding.py:5-25 (even
    columns cos(v*pi / N^(2(k-1)/D)), odd columns sin(v*pi / N^(2k/D)), k 1-based)."""
    v = torch.arange(n_rows, dtype=torch.int32)
    k = torch.arange(1, D + 1)
    arg_sin = v.unsqueeze(-1) * math.pi / (N ** (2 * k / D))
    arg_cos = v.unsqueeze(-1) * math.pi / (N ** (2 * (k - 1) / D))
    tab = torch.sin(arg_sin)
    tab[:, 0::2] = torch.cos(arg_cos)[:, 0::2]
    return tab.float().contiguous()


def cosine_betas(n_timestep):
    """genie/diffusion/schedule.py:27-49: length T+1, beta_0 = 0."""
    steps = n_timestep + 1
    x = torch.linspace(0, n_timestep, steps)
    ac = torch.cos((x / steps) * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    return torch.cat([torch.zeros(1), torch.clip(1 - ac[1:] / ac[:-1], 0, 0.999)])


def schedule_tensors(n_timestep):
    """The DDPM terms BaseSampler reads (genie/diffusion/ddpm.py:40-56)."""
    betas = cosine_betas(n_timestep)
    alphas = 1. - betas
    alphas_cumprod = torch.cumprod(alphas, 0)
    return {
        'betas': betas,
        'alphas': alphas,
        'alphas_cumprod': alphas_cumprod,
        'sqrt_betas': torch.sqrt(betas),
        'sqrt_alphas': torch.sqrt(alphas),
        'sqrt_alphas_cumprod': torch.sqrt(alphas_cumprod),
        'sqrt_one_minus_alphas_cumprod': torch.sqrt(1. - alphas_cumprod),
    }


def schedule_block(sched):
    """[4][T+1] block for genie_set_tables."""
    return torch.stack([sched['alphas'], sched['sqrt_alphas'], sched['sqrt_one_minus_alphas_cumprod'],
                        sched['sqrt_betas']]).float().contiguous()


SAMPLERS = ('ancestral', 'ddim')


def respaced_steps(n_timestep, num_steps):
    """The timesteps a `num_steps`-step reverse process visits, strictly decreasing: rint(linspace(T, 1, K)), [T] for K = 1,
    and T, T-1, ..., 1 for K = T."""
    T, K = int(n_timestep), int(num_steps)
    if K != num_steps or not 1 <= K <= T:
        raise ValueError('num_steps must be an integer in 1..%d, got %r' % (T, num_steps))
    if K == 1:
        return [T]
    return [int(v) for v in torch.round(torch.linspace(T, 1, K, dtype=torch.float64)).tolist()]


def partial_steps(n_timestep, start_step, num_steps):
    """The timesteps a `num_steps`-step reverse process visits when it is entered at `start_step` = t0 instead of T (partial
    diffusion), strictly decreasing: rint(linspace(t0, 1, K)) in float64 exactly as respaced_steps forms its list, [t0] for K = 1,
    t0, t0-1, ..., 1 for K = t0; partial_steps(T, T, K) == respaced_steps(T, K)."""
    T = int(n_timestep)
    if isinstance(start_step, bool) or int(start_step) != start_step or not 1 <= int(start_step) <= T:
        raise ValueError('start_step must be an integer in 1..%d, got %r' % (T, start_step))
    t0 = int(start_step)
    if isinstance(num_steps, bool) or int(num_steps) != num_steps or not 1 <= int(num_steps) <= t0:
        raise ValueError('num_steps must be an integer in 1..%d with start_step=%d, got %r' % (t0, t0, num_steps))
    K = int(num_steps)
    if K == 1:
        return [t0]
    return [int(v) for v in torch.round(torch.linspace(t0, 1, K, dtype=torch.float64)).tolist()]


def check_sampler(sampler, eta=None):
    """The (sampler, eta) pair of the few-step samplers: eta belongs to 'ddim' alone, in [0, 1]; None is its default 0."""
    if sampler not in SAMPLERS:
        raise ValueError('sampler must be one of %s, got %r' % (', '.join(map(repr, SAMPLERS)), sampler))
    if eta is None:
        return 0.0
    if sampler == 'ancestral':
        raise ValueError("eta belongs to the 'ddim' sampler, got eta=%r with 'ancestral'" % (eta,))
    if not 0.0 <= float(eta) <= 1.0:          # (False for NaN)
        raise ValueError('eta must be in [0, 1], got %r' % (eta,))
    return float(eta)


def alphas_cumprod64(n_timestep):
    """abar_0..abar_T in float64 from the float32 betas of schedule_tensors.  The float32 `alphas_cumprod` will not do for a jump
    from t to s: 1 - abar_t / abar_s formed from it is wrong in its third digit at small t."""
    return torch.cumprod(1.0 - cosine_betas(n_timestep).double(), 0)


def _checked_steps(n_timestep, steps):
    steps = [int(s) for s in steps]
    if not steps or steps[0] > n_timestep or steps[-1] < 1 or any(a <= b for a, b in zip(steps, steps[1:])):
        raise ValueError('steps must be strictly decreasing inside 1..%d, got %r' % (n_timestep, steps))
    return steps


def reverse_coefficients(n_timestep, steps, sampler='ancestral', eta=0.0):
    """float64 [len(steps), 3] rows (A, Bz, C): iteration i denoises at t = steps[i] and lands on s = steps[i + 1] (s = 0 with
    abar_0 = 1 after the last) by  x <- ((A x + Bz z) mask + scale C eps) mask.  The last iteration draws no noise; its C is
    returned all the same.
      'ancestral' (the variance choice of base.py:249-270 on the sub-sequence), a' = abar_t / abar_s, b' = 1 - a':
          A = 1 / sqrt(a'),  Bz = -b' / (sqrt(1 - abar_t) sqrt(a')),  C = sqrt(b')
      'ddim', sigma = eta sqrt((1 - abar_s) / (1 - abar_t)) sqrt(1 - abar_t / abar_s):
          A = sqrt(abar_s / abar_t),  Bz = sqrt(max(0, 1 - abar_s - sigma^2)) - A sqrt(1 - abar_t),  C = sigma"""
    if sampler not in SAMPLERS:
        raise ValueError('sampler must be one of %s, got %r' % (', '.join(map(repr, SAMPLERS)), sampler))
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError('eta must be in [0, 1], got %r' % (eta,))
    steps = _checked_steps(n_timestep, steps)
    abar = alphas_cumprod64(n_timestep)
    at, as_ = abar[steps], abar[steps[1:] + [0]]
    if sampler == 'ancestral':
        ap = at / as_
        bp = 1.0 - ap
        return torch.stack([1.0 / torch.sqrt(ap), -bp / (torch.sqrt(1.0 - at) * torch.sqrt(ap)), torch.sqrt(bp)], dim=1)
    sigma = float(eta) * torch.sqrt((1.0 - as_) / (1.0 - at)) * torch.sqrt(1.0 - at / as_)
    a = torch.sqrt(as_ / at)
    return torch.stack([a, torch.sqrt(torch.clamp(1.0 - as_ - sigma ** 2, min=0.0)) - a * torch.sqrt(1.0 - at), sigma], dim=1)


def twisted_coefficients(n_timestep, steps):
    """float64 [len(steps), 3] rows (coef1, coef2, sigma) of the ancestral posterior on the sub-sequence, as the twisted sampler
    uses them: mean = coef1 x0 + coef2 x_t with coef1 = sqrt(abar_s) b' / (1 - abar_t), coef2 = sqrt(a') (1 - abar_s) / (1 - abar_t),
    and sigma = sqrt(b') (a', b', s as in reverse_coefficients)."""
    steps = _checked_steps(n_timestep, steps)
    abar = alphas_cumprod64(n_timestep)
    at, as_ = abar[steps], abar[steps[1:] + [0]]
    ap = at / as_
    bp = 1.0 - ap
    return torch.stack([torch.sqrt(as_) * bp / (1.0 - at), torch.sqrt(ap) * (1.0 - as_) / (1.0 - at), torch.sqrt(bp)], dim=1)


def random_state_dict(dims, seed=0):
    """Random-init weights of the Denoiser architecture for benchmarking
    (trained checkpoints are not available offline).  Unlike the reference's
    default init (primitives.py:76-83,157-158: 'final' layers are zero) every
    matrix is non-zero so that no kernel runs on trivial operands."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in weight_layout(dims):
        if key.endswith('head_weights'):
            t = 0.5413 + 0.3 * torch.randn(shape, generator=g)
        elif 'layer_norm' in key:
            t = (1.0 if key.endswith('weight') else 0.0) + 0.1 * torch.randn(shape, generator=g)
        elif key.endswith('bias'):
            t = 0.1 * torch.randn(shape, generator=g) + (1.0 if ('_g.bias' in key or 'linear_g.bias' in key) else 0.0)
        else:
            t = torch.randn(shape, generator=g) * ((0.1 if 'bb_update' in key else 1.0) / math.sqrt(shape[1]))
        sd[key] = t.float().contiguous()
    return sd


SOFTPLUS_INVERSE_1 = 0.541324854612918          # ipa.head_weights (primitives.py:90-93)


def reference_init_mode(key):
    """How the reference's modules initialise the tensor `key` (primitives.py:96-160,203-217,
    triangular_attention.py:57-65): 'torch' (plain nn.Linear), 'lecun', 'relu', 'glorot', 'normal', 'gating', 'final' for a
    Linear (weight and bias alike), 'norm' for a LayerNorm, 'head_weights'."""
    *path, leaf = key.split('.')
    name = path[-1]
    if leaf == 'head_weights':
        return 'head_weights'
    if 'layer_norm' in name:
        return 'norm'
    if path[0] in ('single_feature_net', 'pair_feature_net'):
        return 'torch'
    if name in ('linear_a_g', 'linear_b_g', 'linear_g'):
        return 'gating'
    if name == 'linear_1' or (name == 'linear_2' and 'transition' in path):       # structure_transition.py:28-29, pair_transition.py:44
        return 'relu'
    if name in ('linear_z', 'linear_2', 'linear_3', 'linear_out', 'linear_o'):
        return 'final'
    if path[-2] == 'mha':                                   # linear_q / linear_k / linear_v of the triangular attention
        return 'glorot'
    if path[-2] in ('tri_att_start', 'tri_att_end'):        # the triangle bias projection
        return 'normal'
    return 'lecun'


def reference_state_dict(dims, seed):
    """The reference's own parameter initialisation: equal bit for bit to `state_dict()` of its `Denoiser(**config.model, ...)`
    built right after `random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)` (genie/train.py:42,51,
    genie/utils/model_io.py:64-77), in `weight_layout` order, float32.

    Two private streams, consumed in the reference's construction order (which is the layout's order; head_weights is a
    constant): `np.random.RandomState(seed)` feeds scipy's truncated normal of the lecun / He matrices (primitives.py:50-69,
    with its fan computation as written: fan = out * in * out), `torch.Generator().manual_seed(seed)` feeds the plain
    nn.Linear's of the two feature nets, the glorot / normal matrices of the triangular attention -- and the default
    nn.Linear init that every primitives.Linear draws and then overwrites (primitives.py:135), replayed here on scratch
    tensors so that later torch draws see the stream where the reference leaves it.  The global random / numpy / torch
    states are neither read nor advanced."""
    try:
        import numpy as np
        from scipy.stats import truncnorm
    except ImportError as e:
        raise ImportError('pack.reference_state_dict needs scipy (the reference draws its truncated normals with '
                          'scipy.stats.truncnorm); install scipy or start from a checkpoint') from e
    from torch.nn import init
    rs = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    trunc_std = truncnorm.std(a=-2, b=2, loc=0, scale=1)
    layout = weight_layout(dims)
    has_bias = {k[:-len('.bias')] for k, _ in layout if k.endswith('.bias')}
    sd = {}
    for key, shape in layout:
        mode = reference_init_mode(key)
        if mode == 'head_weights':
            sd[key] = torch.full(shape, SOFTPLUS_INVERSE_1, dtype=torch.float32)
        elif mode == 'norm':
            sd[key] = torch.ones(shape) if key.endswith('.weight') else torch.zeros(shape)
        elif key.endswith('.bias'):                         # drawn with its weight, below
            sd[key] = torch.full(shape, 1.0 if mode == 'gating' else 0.0, dtype=torch.float32)
        else:
            w = torch.empty(shape, dtype=torch.float32)
            init.kaiming_uniform_(w, a=math.sqrt(5), generator=g)          # nn.Linear.reset_parameters
            if key[:-len('.weight')] in has_bias:
                bound = 1 / math.sqrt(shape[1])
                init.uniform_(torch.empty(shape[0]), -bound, bound, generator=g)
            if mode in ('lecun', 'relu'):
                fan = shape[0] * shape[1] * shape[0]        # _calculate_fan (primitives.py:31-47) on an [out, in] matrix
                std = math.sqrt((2.0 if mode == 'relu' else 1.0) / max(1, fan)) / trunc_std
                samples = truncnorm.rvs(a=-2, b=2, loc=0, scale=std, size=shape[0] * shape[1], random_state=rs)
                w.copy_(torch.tensor(np.reshape(samples, shape)))
            elif mode == 'glorot':
                init.xavier_uniform_(w, gain=1, generator=g)
            elif mode == 'normal':
                init.kaiming_normal_(w, nonlinearity='linear', generator=g)
            elif mode in ('gating', 'final'):
                w.zero_()
            sd[key] = w
        sd[key] = sd[key].contiguous()
    return sd


BASE_DIMS = dict(
    c_s=384, c_p=128, rescale=1.0, c_pos_emb=256, c_chain_emb=64, c_timestep_emb=512,
    relpos_k=32, template_dist_min=2.0, template_dist_step=0.5, template_dist_n_bin=37,
    n_pair_transform_layer=5, c_hidden_mul=128, pair_transition_n=4,
    n_structure_layer=8, n_structure_block=1, c_hidden_ipa=16, n_head_ipa=12, n_qk_point=4, n_v_point=8,
    n_timestep=1000, max_n_res=256, max_n_chain=1)


def sinusoidal_encoding(v, N, D):
    """genie/utils/encoding.py:5-25 for arbitrary index tensors `v` [*] -> [*, D] (the device tables above are
    this function evaluated on 0..n-1)."""
    k = torch.arange(1, D + 1, device=v.device)
    shape = (1,) * v.dim() + (D,)
    sin_enc = torch.sin(v.unsqueeze(-1) * math.pi / (N ** (2 * k / D)).view(shape))
    cos_enc = torch.cos(v.unsqueeze(-1) * math.pi / (N ** (2 * (k - 1) / D)).view(shape))
    enc = sin_enc.clone()
    enc[..., 0::2] = cos_enc[..., 0::2]
    return enc
