"""Both arithmetics on weights away from the generator's one point in value space (tests/_weight_profiles.py): trained-like
LayerNorm affines, row norms spread over 2^14, heavy tails, biases of order 1 to 6, saturated gates and logits, far coordinates,
matrices of 2^-40 and 2^-70, and exact power-of-two reparametrisations.  GPU only; test_value_range_host.py decides with the
oracle alone which profiles are admissible.

Reference: the float64 oracle on the same float32 weights and inputs.  Bounds: per tap max(1e-4, 3 e32) * max(1,
|ref|_inf), e32 the float32 oracle's own error against the float64 oracle on exactly these inputs (the factor 3 allows for another
summation order); z and states on valid residues, p_init and p on all elements, p_tri_att0 on valid pairs; p exactly 0 at padded
pairs; no non-finite value.  The max norm lets a flushed small row hide behind a large one, so p and states are also measured per
channel: max over c of |d[..., c]|_inf / max(|ref[..., c]|_inf, 1e-3 |ref|_inf) within max(1e-4, 3 * the float32 oracle's same
measure)."""
import pytest
import torch

import _parity as P
import _triatt as TA
import _weight_profiles as W

pytestmark = pytest.mark.gpu

SMALL, MID, LARGE = tuple(W.LENGTHS), (130, 66), (256, 129)        # one row tile and contraction <1>; NP = 160: <2>; NP = 256: _big
PROFILE_CASES = [(n, t, SMALL) for n in W.PROFILES for t in (False, True)] + [('all', t, L) for L in (MID, LARGE) for t in (False, True)]
# (E, E of the hx structure track, triangular attention, lengths): see test_power_of_two_reparametrisation
REPARAM_CASES = [(E, 6, t, SMALL) for t in (False, True) for E in (6, 10)] + [(8, 6, t, L) for L in (MID, LARGE) for t in (False, True)]
STRUCTURE_TAPS = ('z', 'states', 'channel_states')
_SLOT = {}


def _ids(cases):
    return ['%s-%s-%dx%d' % (c[0], 'triatt' if c[1] else 'plain', c[2][0], c[2][1]) for c in cases]


@pytest.fixture(autouse=True)
def _time_limit():
    with P.hard_time_limit(600):
        yield


def _drop():
    for c in _SLOT.values():
        for eng in c['engines'].values():
            eng.close()
    _SLOT.clear()


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    _drop()


def case(name, tri, lengths):
    """One case at a time (the two arithmetics of a case follow each other): inputs, weights, the float64 reference, the float32
    oracle's error against it, and the engines loaded for it, closed when the next case comes."""
    key = (name, tri, lengths)
    if key not in _SLOT:
        _drop()
        dims = W.model_dims(tri)
        f, rm, rots, trans, ts = W.case_inputs(dims, lengths)
        sd = W.plain_state_dict(dims, W.WEIGHT_SEED[tri]) if name == 'plain' else W.profile_state_dict(dims, W.WEIGHT_SEED[tri], name)
        trans = W.profile_inputs(name, trans)
        ref = W.reference_taps(sd, dims, f, rots, trans, ts, True)
        r32 = W.reference_taps(sd, dims, f, rots, trans, ts, False)
        _SLOT[key] = dict(dims=dims, features=f, rm=rm, rots=rots, trans=trans, ts=ts, sd=sd, ref=ref, e32=W.tap_errors(r32, ref, rm),
                          chan32={t: W.channel_measure(t, r32[t], ref[t], rm) for t in ('p', 'states')}, engines={})
    return _SLOT[key]


def run(c, tag, sd, math):
    """the engine of (case, tag), created on first use, switched to `math`, on the case's inputs"""
    from genie2_amd.engine import GenieEngine
    if tag not in c['engines']:
        c['engines'][tag] = GenieEngine(c['dims'], sd, 'cuda:0')
        c['engines'][tag].bind_features(c['features'])
    eng = c['engines'][tag]
    eng.set_math(math)
    return eng.denoise(c['trans'], c['rots'], c['ts'], None, taps=('states', 'p_init', 'p') + (('p_tri_att0',) if W.has_tri(c['dims']) else ()))


def check(tag, c, out):
    """[(what, error, bound)] of one run against the case's reference, printed with e32; the entries that miss their bound"""
    tol = W.bounds(c['e32'])
    res = P.compare_taps(out, c['ref'], c['rm'], tol)
    if 'p_tri_att0' in out:
        err, scale = TA.tap_error(out['p_tri_att0'], c['ref']['p_tri_att0'], c['rm'])
        res.append(('p_tri_att0', err, tol['p_tri_att0'] * scale))
        res.append(('p_tri_att0_finite', float((~torch.isfinite(out['p_tri_att0'])).sum()), 0.0))
    for tap in ('p', 'states'):
        res.append(('channel_' + tap, W.channel_measure(tap, out[tap], c['ref'][tap], c['rm']), max(P.BAR, 3.0 * c['chan32'][tap])))
    e32 = dict(c['e32'], **{'channel_' + t: v for t, v in c['chan32'].items()})
    scale = {t: b / tol[t] for t, _, b in res if t in tol}
    print(tag, ' '.join('%s=%.2e/%.1e(e32 %.1e)' % (t, e / scale.get(t, 1.0), b / scale.get(t, 1.0), e32[t]) if t in e32 else '%s=%g' % (t, e)
                        for t, e, b in res), flush=True)
    return P.failures(tag, res)


@pytest.mark.parametrize('math', P.MATH_MODES)
@pytest.mark.parametrize('name,tri,lengths', PROFILE_CASES, ids=_ids(PROFILE_CASES))
def test_profile_against_float64_oracle(name, tri, lengths, math):
    """small_dims without and with triangular attention (32, 4), ragged [40, 33] with a six-residue motif on entry 0; the `all`
    profile also at [130, 66] and [256, 129] (several row tiles, the other two contraction kernels, several attention slabs).
    tiny_matrices_70: the product sa sb of the triangle multiplication's operand scales overflows f32, and its reciprocal must
    come out as 0, not NaN.  beta_dominant is the profile on which a load-time activation bound taken from the unfolded weights
    overflows f16 ("Value range").  Measured on MI355X: both arithmetics are within 1.6 e32 of the float64 oracle on
    every profile and tap (DESIGN 4.1 has the table); the slowest case, all with triangular attention at [256, 129], takes 12 s,
    of which the two oracles take 11."""
    c = case(name, tri, lengths)
    assert not check('%s %s %s %s:' % (name, 'triatt' if tri else 'plain', list(lengths), math), c, run(c, 'w', c['sd'], math))


@pytest.mark.parametrize('E,E_hx,tri,lengths', REPARAM_CASES, ids=['%d-%s-%dx%d' % (c[0], 'triatt' if c[2] else 'plain', c[3][0], c[3][1]) for c in REPARAM_CASES])
def test_power_of_two_reparametrisation(E, E_hx, tri, lengths):
    """W.reparametrise leaves every float product and sum of the network unchanged up to exact powers of two, so only the scales
    of the split-f16 path see it.

    f32 mode, E = 6 and 10 at [40, 33], E = 8 at [130, 66] and [256, 129]: outputs bit-equal on the original and the
    reparametrised weights (measured: they are), and within the bounds.

    hx mode, same E: everything finite and the pair stack (p_init, p, p_tri_att0, p per channel: one factor per row OR per column
    of a matrix, a span of 2^2E) within the bounds; measured at E = 10: p 5.9e-6, per channel 1.3e-5.  The structure transition's
    linear_2 carries the factors of BOTH ReLU stages, 2^-k_r on column r and 2^k'_r on row r, a span of 2^4E inside one matrix
    under one scale (max |W s| in [2^13, 2^14)): an entry 2^-d below the maximum keeps min(22, 38 - d) significand bits in its two
    f16 halves (f16's smallest subnormal is 2^-24), and it meets the largest activations of its row chunk, so its term is as
    large as any other.  d = 4E gives 14 bits at E = 6, 10 at E = 7, 6 at E = 8, none from E = 10.  Measured, states per channel
    (bound 1e-4): 1.9e-5 .. 2.5e-5 at E = 6 (the float32 oracle: 1.0e-5 .. 2.1e-5), 1.8e-4 .. 3.4e-4 at E = 7, 2.1e-3 .. 3.1e-3 at E = 8,
    5e-2 at E = 9, 0.2 .. 0.3 at E = 10; states in the max norm: 5.6e-6 .. 1.1e-5, (inside at 7), 7e-4 .. 1.4e-3, 6e-2, 8e-2.  That is
    the arithmetic's envelope, not a defect of a scale (f32 mode is exact throughout): z, states and states per channel are held to
    the bounds at E_hx = 6, the largest exponent inside them with a factor of two to spare, and printed at E."""
    c = case('plain', tri, lengths)
    tag = 'reparametrised %s %s' % ('triatt' if tri else 'plain', list(lengths))
    bad = []
    for math in P.MATH_MODES:
        a = run(c, 'w', c['sd'], math)
        bad += check('%s %s original:' % (tag, math), c, a)
        for e in sorted({E, E_hx}):
            b = run(c, 'E%d' % e, W.reparametrise(c['sd'], c['dims'], e, 5), math)
            miss = check('%s E=%d %s:' % (tag, e, math), c, b)
            apart = W.tap_errors(b, a, c['rm'])
            print('%s E=%d %s: apart from the run on the original weights by' % (tag, e, math), ' '.join('%s=%.2e' % kv for kv in apart.items()), flush=True)
            if math == 'f32':
                bad += miss + [(tag, e, tap + '_bits', 1.0, 0.0) for tap in a if not torch.equal(a[tap], b[tap])]
            else:
                bad += [m for m in miss if e <= E_hx or m[1] not in STRUCTURE_TAPS]
                bad += [(tag, e, tap + '_finite', 1.0, 0.0) for tap in b if not bool(torch.isfinite(b[tap]).all())]
    assert not bad, bad
