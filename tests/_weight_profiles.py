"""Helpers of test_value_range_host.py / test_value_range_gpu.py: weights away from the one point in value space that
O.synthetic_state_dict and TA.full_state_dict draw (matrices N(0, 1 / fan_in), gamma 1 +- 0.1, beta and biases +- 0.1, gate
biases 1 +- 0.1), exact reparametrisations by powers of two, the shared inputs, and the error measures of both files.

The split-f16 arithmetic derives one power-of-two scale per matrix and per bounded activation from the weights at
load time; the profiles move what those scales are derived from: the LayerNorm affine that is folded into the rows, the spread of
row norms under one per-matrix maximum, outliers, biases inside the Cauchy-Schwarz bound, saturated gates and logits, far
coordinates, matrices so small that a reciprocal scale leaves f32.  No tests here."""
import math

import torch

import _parity as P
import _triatt as TA
from oracle import genie_oracle as O

MANDATORY = ('ln_affine', 'row_spread', 'heavy_tail', 'big_bias', 'all')
EXTREME = ('saturated_gates', 'peaked_attention', 'coords_x40', 'tiny_matrices_40', 'tiny_matrices_70', 'beta_dominant')
PROFILES = MANDATORY + EXTREME
E32_CAP = dict([(n, 3e-5) for n in MANDATORY] + [(n, 1e-4) for n in EXTREME])     # of max(1, |ref|_inf), float32 oracle alone
GAMMA_RANGE = {'ln_affine': (0.05, 8.0), 'all': (0.2, 4.0)}
BETA_STD = {'ln_affine': 2.0, 'all': 1.0}
ROW_EXP = {'row_spread': 7, 'all': 4}
# GATE_GAIN is left to the float32 oracle's own error: reduced from 64 until the float32 oracle is within the cap 1e-4 of its
# float64 self on every tap of both models at [40, 33], with a factor to spare for another machine's float32 sums
# (profile_state_dict's docstring has the figures; test_value_range_host.py::test_float32_oracle_is_inside_its_cap holds it there).
GATE_GAIN = 24.0
GATE_BIAS = 30.0
PEAK_GAIN = 8.0
COORD_GAIN = 40.0
DOMINANT_BETA = 24.0
WEIGHT_SEED = {False: 3, True: 1}         # seeds of the plain weights under the profiles: without / with triangular attention
LENGTHS = [40, 33]
MOTIF_INDEX = [3, 4, 5, 20, 21, 22]
LOG2_E_128 = 128.0 * math.log(2.0)        # |pre-activation| beyond which exp2 of the kernels' sigmoid leaves f32 either way


def has_tri(dims):
    return dims.get('n_head_tri', 0) > 0


def model_dims(tri):
    return TA.tri_dims(O.small_dims()) if tri else O.small_dims()


def plain_state_dict(dims, seed):
    return TA.full_state_dict(dims, seed) if has_tri(dims) else O.synthetic_state_dict(dims, seed=seed)


def is_ln(key):
    return 'layer_norm' in key


def is_matrix(key, t):
    return t.dim() == 2 and not is_ln(key)


def is_gate(key):
    """weights and biases of the sigmoid gates: linear_a_g, linear_b_g, linear_g of the triangle multiplications and linear_g of
    the triangular attention"""
    return '_g.' in key


def _signs(shape, g, p_minus):
    return torch.where(torch.rand(shape, generator=g) < p_minus, -1.0, 1.0)


def profile_state_dict(dims, seed, name):
    """The plain weights of `seed` (O.synthetic_state_dict, or TA.full_state_dict when n_head_tri > 0) transformed key by key in
    state_dict order with a generator of its own (1000 + seed).

    trained-like:
      ln_affine   every LayerNorm: gamma log-uniform in [0.05, 8] with 10 % of the entries negated, beta = 2 randn
      row_spread  every 2-D non-LayerNorm matrix: row r times 2^k_r, k_r uniform in -7 .. 7, the matrix times 2^-3.5; then two
                  random rows and two random columns exactly 0
      heavy_tail  every such matrix: entries times exp(0.8 randn), then four random entries times 50
      big_bias    non-LayerNorm biases = 3 randn; gate biases = +-6 + randn
      all         the four together, milder: gamma in [0.2, 4], beta = randn, k_r in -4 .. 4 (the matrix times 2^-2)
    edges:
      saturated_gates   gate weights times GATE_GAIN = 24 and gate biases = +-30: pre-activations up to +-150, beyond +-128 ln 2
                        in both directions.  Worst float32-oracle error (on p) without / with triangular attention: 1.7e-4 /
                        5.4e-4 at 64, 1.3e-4 / 6.4e-5 at 32, 4.8e-5 / 6.3e-5 at 28, 2.6e-5 / 2.3e-5 at 24, 1.1e-5 / 1.2e-5 at 16
                        (where only a handful of pre-activations still pass -128 ln 2): 24 is inside the cap 1e-4 four times over.
      peaked_attention  linear_q, linear_k and the pair-bias `linear` of the triangular attention and linear_q, linear_b of IPA
                        times PEAK_GAIN = 8 (float32 oracle: 4.5e-5 on states with triangular attention, 6.3e-6 without)
      coords_x40        plain weights; profile_inputs multiplies the translations by 40 and leaves the frames
      tiny_matrices_40 / _70   linear_a_p and linear_b_p of both triangle multiplications and the pair transition's linear_1 of
                        layer 0 (weight and bias) times 2^-40 / 2^-70; at 2^-70 the reciprocal 1 / (sa sb) of the operand
                        scales is beyond f32
      beta_dominant     every LayerNorm: beta = 24 randn, gamma as drawn.  W beta then dominates the folded bias, and the bounded
                        activations (a, b, the transition's hidden layer, q, k, v) reach 0.86 of their Cauchy-Schwarz bound
                        (linear_a_p of the first module: 59 of 68) where ln_affine and all leave them at 0.2 to 0.3 of it: a
                        scale a factor 4 too large (a bound from the unfolded weights, a folded bias left out) still fits f16
                        under those (27045 of 65504) and overflows f16 here and nowhere else"""
    assert name in PROFILES, name
    sd = plain_state_dict(dims, seed)
    g = torch.Generator().manual_seed(1000 + seed)
    trained = {'ln_affine': ('ln',), 'row_spread': ('rows',), 'heavy_tail': ('tail',), 'big_bias': ('bias',),
               'all': ('ln', 'rows', 'tail', 'bias')}.get(name, ())
    out = {}
    for k, v in sd.items():
        t = v.clone()
        if 'ln' in trained and is_ln(k):
            if k.endswith('weight'):
                lo, hi = GAMMA_RANGE[name]
                t = torch.exp(torch.empty_like(t).uniform_(math.log(lo), math.log(hi), generator=g))
                t = t * _signs(t.shape, g, 0.1)
            else:
                t = BETA_STD[name] * torch.randn(t.shape, generator=g)
        if 'rows' in trained and is_matrix(k, t):
            e = ROW_EXP[name]
            r = torch.randint(-e, e + 1, (t.shape[0], 1), generator=g).float()
            t = t * torch.exp2(r) * 2.0 ** (-e / 2)
            t[torch.randperm(t.shape[0], generator=g)[:2]] = 0
            t[:, torch.randperm(t.shape[1], generator=g)[:2]] = 0
        if 'tail' in trained and is_matrix(k, t):
            t = t * torch.exp(0.8 * torch.randn(t.shape, generator=g))
            idx = torch.randint(0, t.numel(), (4,), generator=g)
            t.view(-1)[idx] = t.view(-1)[idx] * 50
        if 'bias' in trained and k.endswith('bias') and not is_ln(k):
            if is_gate(k):
                t = 6.0 * _signs(t.shape, g, 0.5) + torch.randn(t.shape, generator=g)
            else:
                t = 3.0 * torch.randn(t.shape, generator=g)
        if name == 'beta_dominant' and is_ln(k) and k.endswith('bias'):
            t = DOMINANT_BETA * torch.randn(t.shape, generator=g)
        if name == 'saturated_gates' and is_gate(k):
            t = t * GATE_GAIN if k.endswith('weight') else GATE_BIAS * _signs(t.shape, g, 0.5)
        if name == 'peaked_attention':
            if '.tri_att_' in k and k.endswith(('mha.linear_q.weight', 'mha.linear_k.weight', '.linear.weight')):
                t = t * PEAK_GAIN
            if k.endswith(('ipa.linear_q.weight', 'ipa.linear_b.weight')):
                t = t * PEAK_GAIN
        if name.startswith('tiny_matrices') and k.startswith('pair_transform_net.net.0.') \
                and ('.linear_a_p.' in k or '.linear_b_p.' in k or '.pair_transition.linear_1.' in k):
            t = t * 2.0 ** -int(name.rsplit('_', 1)[1])
        out[k] = t.float().contiguous()
    return out


def profile_inputs(name, trans):
    """the translations a profile runs on (the frames stay those of the unscaled translations)"""
    return trans * COORD_GAIN if name == 'coords_x40' else trans


def reparametrise(sd, dims, E, seed):
    """A copy of sd with exact rescalings by 2^k, k uniform in -E .. E, that leave the network's function and, the factors being
    powers of two, every float product and sum unchanged:
      (a) pair transition and both ReLU stages of the structure transition: row r of linear_1 (weight and bias) times 2^k,
          column r of the following linear times 2^-k (ReLU commutes with a positive factor);
      (b) both triangle multiplications: row c of linear_a_p (weight and bias) times 2^k, row c of linear_b_p times 2^-k
          (the contraction multiplies channel c of a with channel c of b);
      (c) both triangular attention modules: the rows of head h of linear_q times 2^k, of linear_k times 2^-k.
    Only the kernels' per-matrix scales see it: the largest row sets the maximum and the small rows sit up to 2^2E below it."""
    g = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in sd.items()}

    def pw(n):
        return torch.exp2(torch.randint(-E, E + 1, (n,), generator=g).float())

    def relu_pair(pfx, first, second):
        s = pw(out[pfx + first + '.weight'].shape[0])
        out[pfx + first + '.weight'] *= s[:, None]
        out[pfx + first + '.bias'] *= s
        out[pfx + second + '.weight'] /= s[None, :]

    for k in list(out):
        if k.endswith('pair_transition.linear_1.weight'):
            relu_pair(k[:-len('linear_1.weight')], 'linear_1', 'linear_2')
        if k.endswith('transition.layers.0.linear_1.weight'):
            relu_pair(k[:-len('linear_1.weight')], 'linear_1', 'linear_2')
            relu_pair(k[:-len('linear_1.weight')], 'linear_2', 'linear_3')
        if k.endswith('linear_a_p.weight'):
            b = k[:-len('linear_a_p.weight')]
            s = pw(out[k].shape[0])
            out[k] *= s[:, None]
            out[b + 'linear_a_p.bias'] *= s
            out[b + 'linear_b_p.weight'] /= s[:, None]
            out[b + 'linear_b_p.bias'] /= s
        if has_tri(dims) and k.endswith('mha.linear_q.weight'):
            b = k[:-len('linear_q.weight')]
            s = pw(dims['n_head_tri']).repeat_interleave(dims['c_hidden_tri_att'])
            out[k] *= s[:, None]
            out[b + 'linear_k.weight'] /= s[:, None]
    return out


# ------------------------------------------------------------------ inputs and references
def case_inputs(dims, lengths=LENGTHS, seed=300):
    """(features, residue_mask, frames, translations, timesteps): a ragged batch with a six-residue motif on entry 0,
    P.conditioned_inputs, the oracle's Frenet frames of those translations."""
    f = O.empty_features(list(lengths))
    O.add_motif(f, 0, torch.randn(6, 3, generator=torch.Generator().manual_seed(21)) * 4, MOTIF_INDEX)
    fr = O.prepare_features(f)
    trans, ts = P.conditioned_inputs(f, dims['n_timestep'], seed)
    rots = O.compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask'])
    return f, fr['residue_mask'], rots, trans, ts


def taps_of(dims):
    return P.TAPS + (('p_tri_att0',) if has_tri(dims) else ())


def reference_taps(sd, dims, f, rots, trans, ts, double):
    """the oracle's taps (float64 arithmetic on the same float32 values when `double`): P.oracle_taps, or TA.composed_taps with
    triangular attention"""
    run = TA.composed_taps if has_tri(dims) else P.oracle_taps
    return run(sd, dims, f, rots, trans, ts, double=double)


def masked(tap, x, residue_mask):
    """float64 x with what the bar does not look at zeroed: padded residues of z and states, padded pairs of p_tri_att0"""
    m = residue_mask.to(x.device).double().unsqueeze(-1)
    x = x.double()
    if tap in ('z', 'states'):
        return x * m
    if tap == 'p_tri_att0':
        return x * (m.unsqueeze(1) * m.unsqueeze(2))
    return x


def tap_errors(got, ref, residue_mask):
    """{tap: max |got - ref| / max(1, |ref|_inf)} over the taps of ref, masked as the bar is; nan when got has a non-finite value"""
    out = {}
    for tap, want in ref.items():
        x, y = masked(tap, got[tap], residue_mask), masked(tap, want.to(got[tap].device), residue_mask)
        out[tap] = float((x - y).abs().max()) / max(1.0, float(y.abs().max())) if bool(torch.isfinite(got[tap]).all()) else float('nan')
    return out


def channel_measure(tap, got, want, residue_mask):
    """max over channels c of |got - want|_inf[..., c] / max(|want|_inf[..., c], 1e-3 |want|_inf): under the max norm a small row
    that the per-matrix scale flushed hides behind a large one"""
    x, y = masked(tap, got, residue_mask), masked(tap, want.to(got.device), residue_mask)
    d = (x - y).abs().flatten(0, -2).max(0).values
    s = y.abs().flatten(0, -2).max(0).values
    return float((d / s.clamp_min(max(1e-3 * float(s.max()), 1e-30))).max())


def bounds(e32):
    """max(1e-4, 3 e32) per tap (the factor 3 allows for another summation order)"""
    return {tap: max(P.BAR, 3.0 * e) for tap, e in e32.items()}
