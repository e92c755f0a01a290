"""The weight profiles of tests/_weight_profiles.py judged by the oracle alone (CPU): whether a profile may be used against the
kernels at all is decided here, never by the kernels' result.

A profile is admissible when the float32 oracle is finite and within a cap of the float64 oracle on the same float32 values,
relative to max(1, |ref|_inf) per tap: 3e-5 for the trained-like profiles, 1e-4 for the edges.  The GPU file's bound is
max(1e-4, 3 e32) per tap, so the cap keeps that bound from growing until it hides a failure."""
import math

import pytest
import torch

import _weight_profiles as W

_CASE = {}


def case(name, tri):
    """(dims, weights, residue mask, float32 taps, float64 taps) of a profile on the shared [40, 33] inputs, computed once"""
    if (name, tri) not in _CASE:
        dims = W.model_dims(tri)
        f, rm, rots, trans, ts = W.case_inputs(dims)
        sd = W.profile_state_dict(dims, W.WEIGHT_SEED[tri], name)
        tr = W.profile_inputs(name, trans)
        _CASE[(name, tri)] = (dims, sd, rm, W.reference_taps(sd, dims, f, rots, tr, ts, False), W.reference_taps(sd, dims, f, rots, tr, ts, True))
    return _CASE[(name, tri)]


@pytest.mark.parametrize('tri', [False, True], ids=['plain', 'triatt'])
@pytest.mark.parametrize('name', W.PROFILES)
def test_float32_oracle_is_inside_its_cap(name, tri):
    """Measured here, worst tap: ln_affine 2.4e-6 / 5.9e-6 (without / with triangular attention), row_spread 5.9e-6 / 7.5e-6,
    heavy_tail 1.2e-5 / 7.6e-6, big_bias 2.0e-6 / 2.3e-6, all 1.3e-5 / 1.6e-5; saturated_gates 2.6e-5 / 2.3e-5, peaked_attention
    6.3e-6 / 4.5e-5, coords_x40 2.2e-5 / 2.2e-5 (z), tiny_matrices 4.1e-6 / 3.4e-6, beta_dominant 2.0e-6 / 2.3e-6.  Per channel (p, states), trained-like: at
    most 5.5e-5."""
    dims, sd, rm, r32, r64 = case(name, tri)
    assert set(r64) == set(W.taps_of(dims))
    for tap in r64:
        assert torch.isfinite(r32[tap]).all() and torch.isfinite(r64[tap]).all(), tap
    e32 = W.tap_errors(r32, r64, rm)
    chan = {tap: W.channel_measure(tap, r32[tap], r64[tap], rm) for tap in ('p', 'states')}
    print(name, 'triatt' if tri else 'plain', ' '.join('%s=%.2e' % kv for kv in e32.items()), '| per channel', ' '.join('%s=%.2e' % kv for kv in chan.items()))
    assert all(e <= W.E32_CAP[name] for e in e32.values()), e32


@pytest.mark.parametrize('tri', [False, True], ids=['plain', 'triatt'])
@pytest.mark.parametrize('E', [6, 10])
def test_reparametrisation_leaves_the_oracle_bit_identical(E, tri):
    dims = W.model_dims(tri)
    f, rm, rots, trans, ts = W.case_inputs(dims)
    sd = W.plain_state_dict(dims, W.WEIGHT_SEED[tri])
    rp = W.reparametrise(sd, dims, E, 5)
    changed = [k for k in sd if not torch.equal(sd[k], rp[k])]
    n_layer = dims['n_pair_transform_layer']
    assert len(changed) == n_layer * (2 * 4 + 3 + (4 if tri else 0)) + dims['n_structure_layer'] * 5
    for k in changed:          # every factor an exact power of two within 2^-2E .. 2^2E (a column between two stages carries both)
        nz = sd[k] != 0
        e = torch.log2(rp[k][nz] / sd[k][nz])
        assert torch.equal(e, e.round()) and float(e.abs().max()) <= 2 * E, k
    for double in (False, True):
        a = W.reference_taps(sd, dims, f, rots, trans, ts, double)
        b = W.reference_taps(rp, dims, f, rots, trans, ts, double)
        for tap in W.taps_of(dims):
            assert torch.equal(a[tap], b[tap]), (tap, double)


def _ln_keys(sd, suffix):
    return [k for k in sd if W.is_ln(k) and k.endswith(suffix)]


def _matrices(sd):
    return [k for k, v in sd.items() if W.is_matrix(k, v)]


@pytest.mark.parametrize('name', ['ln_affine', 'all'])
def test_layer_norm_affine_profile(name):
    dims = W.model_dims(True)
    sd = W.profile_state_dict(dims, 1, name)
    lo, hi = W.GAMMA_RANGE[name]
    gam = torch.cat([sd[k] for k in _ln_keys(sd, 'weight')])
    beta = torch.cat([sd[k] for k in _ln_keys(sd, 'bias')])
    assert len(_ln_keys(sd, 'weight')) == 2 * (2 * 2 + 2 + 1) + 2 * 2
    assert lo * (1 - 1e-6) <= float(gam.abs().min()) and float(gam.abs().max()) <= hi * (1 + 1e-6)
    assert float(gam.abs().max() / gam.abs().min()) >= 0.8 * hi / lo          # the range is used, not only allowed
    assert 0.05 <= float((gam < 0).float().mean()) <= 0.15
    assert abs(float(beta.std()) - W.BETA_STD[name]) <= 0.1 * W.BETA_STD[name]


@pytest.mark.parametrize('name', ['row_spread', 'all'])
def test_row_spread_profile(name):
    dims = W.model_dims(True)
    sd = W.profile_state_dict(dims, 1, name)
    worst = math.inf
    for k in _matrices(sd):
        w = sd[k]
        rows = w.norm(dim=1)
        assert int((rows == 0).sum()) >= 2 and int((w.abs().sum(0) == 0).sum()) >= 2, k
        if w.shape[0] >= 64:
            worst = min(worst, float(rows.max() / rows[rows > 0].min()))
    # 2^14 between the extreme exponents of row_spread; heavy_tail's outliers move a row norm by less than 4
    assert worst >= (2.0 ** 12 if name == 'row_spread' else 2.0 ** 6), worst


def test_heavy_tail_profile():
    dims = W.model_dims(True)
    plain = W.plain_state_dict(dims, 1)
    sd = W.profile_state_dict(dims, 1, 'heavy_tail')
    logs = torch.cat([torch.log(sd[k] / plain[k])[plain[k] != 0] for k in _matrices(sd)])          # a negative factor gives nan
    assert abs(float(logs.median())) <= 0.01 and abs(float(logs.std()) - 0.8) <= 0.05
    # exp(0.8 randn) alone passes e^4 once in 3e6 entries; of the four entries times 50, 45 % do
    assert int((logs > 4.0).sum()) >= len(_matrices(sd))


@pytest.mark.parametrize('name', ['big_bias', 'all'])
def test_big_bias_profile(name):
    dims = W.model_dims(True)
    sd = W.profile_state_dict(dims, 1, name)
    gate = torch.cat([v for k, v in sd.items() if k.endswith('bias') and W.is_gate(k)])
    other = torch.cat([v for k, v in sd.items() if k.endswith('bias') and not W.is_gate(k) and not W.is_ln(k)])
    assert 2.0 <= float(gate.abs().min()) and float(gate.abs().max()) <= 11.0 and 0.4 <= float((gate > 0).float().mean()) <= 0.6
    assert abs(float(other.std()) - 3.0) <= 0.3


@pytest.mark.parametrize('tri', [False, True], ids=['plain', 'triatt'])
def test_saturated_gates_reach_both_overflow_directions(tri, monkeypatch):
    """The kernels' sigmoid is 1 / (1 + exp2(-x log2 e)): exp2 leaves f32 upwards for x < -128 ln 2 (inf, sigmoid 0) and flushes
    to 0 for x > 128 ln 2 (sigmoid 1).  Every argument torch.sigmoid sees in the oracle's run is a gate pre-activation; batch
    entry 0 has no padding, so all of its pairs count."""
    dims = W.model_dims(tri)
    f, rm, rots, trans, ts = W.case_inputs(dims)
    assert bool(rm[0].all())
    sd = W.profile_state_dict(dims, W.WEIGHT_SEED[tri], 'saturated_gates')
    seen = []
    sigmoid = torch.sigmoid

    def recording(x):
        seen.append((int((x[0] < -W.LOG2_E_128).sum()), int((x[0] > W.LOG2_E_128).sum()), float(x[0].abs().max())))
        return sigmoid(x)
    monkeypatch.setattr(torch, 'sigmoid', recording)
    W.reference_taps(sd, dims, f, rots, trans, ts, False)
    monkeypatch.undo()
    n_gate = dims['n_pair_transform_layer'] * 2 * 3
    assert len(seen) >= n_gate + (dims['n_pair_transform_layer'] * 2 * 2 if tri else 0)       # the attention gates come in row chunks
    lo, hi, top = sum(s[0] for s in seen), sum(s[1] for s in seen), max(s[2] for s in seen)
    print('gate pre-activations beyond +-%.1f: %d below, %d above, largest %.0f' % (W.LOG2_E_128, lo, hi, top))
    assert lo > 0 and hi > 0


def test_peaked_coords_and_tiny_profiles():
    dims = W.model_dims(True)
    plain = W.plain_state_dict(dims, 1)
    peaked = W.profile_state_dict(dims, 1, 'peaked_attention')
    scaled = sorted(k for k in plain if not torch.equal(plain[k], peaked[k]))
    assert len(scaled) == 2 * 2 * 3 + 2 * 2 and all(torch.equal(peaked[k], plain[k] * W.PEAK_GAIN) for k in scaled)
    assert all(torch.equal(v, plain[k]) for k, v in W.profile_state_dict(dims, 1, 'coords_x40').items())
    t = torch.ones(2, 3, 3)
    assert torch.equal(W.profile_inputs('coords_x40', t), 40 * t) and W.profile_inputs('all', t) is t
    for e in (40, 70):
        tiny = W.profile_state_dict(dims, 1, 'tiny_matrices_%d' % e)
        scaled = sorted(k for k in plain if not torch.equal(plain[k], tiny[k]))
        assert len(scaled) == 2 * 4 + 2 and all(k.startswith('pair_transform_net.net.0.') for k in scaled)
        assert all(torch.equal(tiny[k], plain[k] * 2.0 ** -e) for k in scaled)


@pytest.mark.parametrize('tri', [False, True], ids=['plain', 'triatt'])
def test_beta_dominant_activations_sit_near_their_bound(tri):
    """linear_a_p of the first triangle multiplication on the float64 taps: the largest projection is above 0.7 of the
    Cauchy-Schwarz bound over the LayerNorm-folded rows (sqrt(c_p) |W diag gamma|_2 + |b + W beta|, what the library's load-time
    scale is derived from) and above 2.5 times the same bound over the unfolded rows; under ln_affine it stays below 0.4 of the
    folded bound, which is why that profile alone cannot tell the two bounds apart."""
    from oracle import genie_oracle as O
    pfx = 'pair_transform_net.net.0.tri_mul_out.'
    ratio = {}
    for name in ('beta_dominant', 'ln_affine'):
        dims, sd, rm, r32, r64 = case(name, tri)
        sd = {k: v.double() for k, v in sd.items()}
        a = float(O._lin(sd, pfx + 'linear_a_p', O._ln(sd, pfx + 'layer_norm_in', r64['p_init'])).abs().max())
        w, b, g, beta = (sd[pfx + k] for k in ('linear_a_p.weight', 'linear_a_p.bias', 'layer_norm_in.weight', 'layer_norm_in.bias'))
        folded = float(((w * g).norm(dim=1) * math.sqrt(w.shape[1]) + (b + w @ beta).abs()).max())
        unfolded = float((w.norm(dim=1) * math.sqrt(w.shape[1]) + b.abs()).max())
        ratio[name] = (a / folded, a / unfolded)
    print(ratio)
    assert 0.7 <= ratio['beta_dominant'][0] <= 1.0 and ratio['beta_dominant'][1] >= 2.5
    assert ratio['ln_affine'][0] <= 0.4
