"""Conditioned batches across the tile boundaries of k_pair_static<true> / k_pair_init<false> against the float64 oracle.  GPU only.

The rest of the suite sweeps lengths and dispatch paths with fixed_structure_mask all clear (k_pair_init<true>, pstatic never
read) and conditions on motifs only at N <= 50, where both kernels see one j tile with t0 = 0.  Here: _conditioned.scaffold_like
(three entries; motif residues, a chain break, shifted residue indices and interface residues placed across the 64-wide tile
edges, in entry 0 and in an entry with b > 0) at N = 5, 63, 64, 65, 128, 129, 130 in both arithmetics, pair distances beyond the
last template bin, a structure-mask bit that only sets the batch's flag, the promise that both forms of the step-invariant term
are bit-identical where there is no motif, rebinding across the flag, and bind_features' refusals.

Bounds: 2e-5 for s, the project's bar 1e-4 * max(1, |ref|_inf) for z, states (valid residues), p_init and p (all elements),
padded pairs of p exactly zero, everything finite.  test_conditioned_host.py holds the float32 oracle inside a quarter of the
bar on these inputs and shows that no conditioning ingredient can be ignored within it."""
import pytest
import torch

import _conditioned as CD
from _parity import MATH_MODES, conditioned_inputs, failures, hard_time_limit, worst
from oracle import genie_oracle as O

pytestmark = pytest.mark.gpu

_REF = {}
_WORST = {}


@pytest.fixture(autouse=True)
def _time_limit():
    with hard_time_limit(600):
        yield


@pytest.fixture(scope='module')
def model():
    dims = O.small_dims()
    return dims, O.synthetic_state_dict(dims, seed=3)


@pytest.fixture(scope='module')
def engine(model):
    """one engine for the file; position table of 512 rows (entry 0 reads rows past N)"""
    from genie2_amd.engine import GenieEngine
    eng = GenieEngine(model[0], model[1], 'cuda:0', n_pos=CD.N_POS)
    yield eng
    eng.close()


def references(model, key, f, rots, trans, ts):
    """the float64 oracle's s, z, states, p_init, p and the float32 oracle's s, once per case"""
    if key not in _REF:
        dims, sd = model
        ref = CD.reference(sd, dims, f, rots, trans, ts, double=True)
        with torch.no_grad():
            ref['s_f32'] = O.single_feature_net(sd, dims, ts, O.prepare_features(f), trans.shape[1])
        _REF[key] = ref
    return _REF[key]


def run(engine, math, f, trans, rots, ts):
    engine.set_math(math)
    try:
        engine.bind_features(f)
        return engine.denoise(trans, rots, ts, None, taps=('s', 'states', 'p_init', 'p'))
    finally:
        engine.set_math('hx')


def check(tag, math, out, ref, mask):
    """collect every miss of the bounds; print and record the error / bound of every tap"""
    res = CD.compare(out, ref, mask)
    # the engine's encoding tables follow the reference's float32 expression: s against the float32 oracle too, same bound
    res.append(('s_f32', float((out['s'].double() - ref['s_f32'].to(out['s'].device).double()).abs().max()), CD.S_TOL))
    r = CD.ratios(res)
    for tap, v in r.items():
        _WORST[(math, tap)] = max(_WORST.get((math, tap), 0.0), v)
    print('%s %s: error / bound %s, worst %s' % (tag, math, {k: round(v, 4) for k, v in r.items()}, worst(res)))
    print('worst error / bound so far [%s]: %s' % (math, {t: round(v, 4) for (m, t), v in _WORST.items() if m == math}))
    return failures(tag, res)


# ------------------------------------------------------------------ 1, 2: taps against the float64 oracle
@pytest.mark.parametrize('N,math', [(n, m) for n in CD.LENGTHS for m in MATH_MODES])
def test_conditioned_batch_matches_float64_oracle(model, engine, N, math):
    """scaffold_like(N) with 3 * randn coordinates and random timesteps, frames from the oracle"""
    f, mask, trans, ts, rots = CD.case(N, 'randn')
    ref = references(model, (N, 'randn'), f, rots, trans, ts)
    bad = check('N=%d randn' % N, math, run(engine, math, f, trans, rots, ts), ref, mask)
    assert not bad, bad


@pytest.mark.parametrize('N,math', [(n, m) for n in (130, 65) for m in MATH_MODES])
def test_distances_beyond_the_last_bin(model, engine, N, math):
    """the same features on a centred random walk with 3.8 A steps (pair distances several times the last template bin's 20 A,
    where the soft bins saturate on the last bin), timesteps [1, 7, 40]"""
    f, mask, trans, ts, rots = CD.case(N, 'walk')
    far = float(torch.cdist(trans[0], trans[0]).max())
    dims = model[0]
    assert far > 1.5 * (dims['template_dist_min'] + (dims['template_dist_n_bin'] - 1) * dims['template_dist_step']), far
    ref = references(model, (N, 'walk'), f, rots, trans, ts)
    bad = check('N=%d walk (to %.0f A)' % (N, far), math, run(engine, math, f, trans, rots, ts), ref, mask)
    assert not bad, bad


# ------------------------------------------------------------------ 3: the flag set from the padding alone
def _padding_bit_case():
    f0 = O.empty_features([65, 40])
    f1 = O.empty_features([65, 40])
    f1['fixed_structure_mask'][1, 50, 50] = True
    dims = O.small_dims()
    fr = O.prepare_features(f0)
    trans, ts = conditioned_inputs(f0, dims['n_timestep'], 4700)
    rots = O.compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask'])
    return f0, f1, fr['residue_mask'], trans, ts, rots


@pytest.mark.parametrize('math', MATH_MODES)
def test_structure_mask_bit_in_the_padding_only(model, engine, math):
    """[65, 40] unconditioned, fixed_structure_mask[1, 50, 50] set: the batch takes the pstatic form and conditions nothing.
    Within the bar of the oracle (which sees the bit too), padded p exactly zero, and entry 0 bit for bit what the same batch
    gives without the bit (the table form)."""
    f0, f1, mask, trans, ts, rots = _padding_bit_case()
    ref = references(model, 'padding_bit', f1, rots, trans, ts)
    out1 = run(engine, math, f1, trans, rots, ts)
    bad = check('padding bit [65, 40]', math, out1, ref, mask)
    out0 = run(engine, math, f0, trans, rots, ts)
    bad += [('entry 0 differs from the unconditioned bind', tap) for tap in ('z', 'p_init', 'p') if not torch.equal(out1[tap][0], out0[tap][0])]
    assert not bad, bad


# ------------------------------------------------------------------ 4: both forms bit for bit where there is no motif
@pytest.mark.parametrize('N,math', [(n, m) for n in (130, 65) for m in MATH_MODES])
def test_unconditioned_entry_equals_its_table_form_run(engine, N, math):
    """entry 2 of the conditioned batch (pstatic form, b = 2) against the same entry bound alone as an unconditioned batch of
    one padded to N (table form): z, p_init and p torch.equal, as pair_kernels.hip promises above k_pair_init"""
    f, mask, trans, ts, rots = CD.case(N, 'randn')
    out = run(engine, math, f, trans, rots, ts)
    assert bool(f['fixed_structure_mask'][:2].any()) and not bool(f['fixed_structure_mask'][2].any())
    alone = O.empty_features([CD.entry_lengths(N)[2]], n_pad=N)
    for k in ('residue_mask', 'residue_index', 'chain_index', 'aatype', 'atom_positions', 'fixed_sequence_mask', 'interface_mask'):
        assert torch.equal(alone[k][0], f[k][2]), k
    one = run(engine, math, alone, trans[2:3], rots[2:3], ts[2:3])
    bad = [tap for tap in ('z', 'p_init', 'p') if not torch.equal(out[tap][2], one[tap][0])]
    assert torch.isfinite(one['z']).all() and not bad, bad


# ------------------------------------------------------------------ 5: rebinding across the flag
@pytest.mark.parametrize('math', MATH_MODES)
def test_rebinding_flips_the_flag_cleanly(model, engine, math):
    from genie2_amd.engine import GenieEngine
    N = 65
    f, mask, trans, ts, rots = CD.case(N, 'randn')
    plain = O.empty_features(CD.entry_lengths(N), n_pad=N)
    taps = ('z', 's', 'states', 'p_init', 'p')
    first = run(engine, math, f, trans, rots, ts)
    engine.set_math(math)
    try:
        again = engine.denoise(trans, rots, ts, None, taps=('s', 'states', 'p_init', 'p'))      # the same binding, a second call
    finally:
        engine.set_math('hx')
    second = run(engine, math, plain, trans, rots, ts)
    third = run(engine, math, f, trans, rots, ts)
    fresh_engine = GenieEngine(model[0], model[1], 'cuda:0', n_pos=CD.N_POS)
    try:
        fresh = run(fresh_engine, math, plain, trans, rots, ts)
        bad = [('second call', t) for t in taps if not torch.equal(first[t], again[t])]
        bad += [('conditioned again', t) for t in taps if not torch.equal(first[t], third[t])]
        bad += [('unconditioned after conditioned', t) for t in taps if not torch.equal(second[t], fresh[t])]
        assert not torch.equal(first['p_init'], second['p_init'])
    finally:
        fresh_engine.close()
    assert not bad, bad


# ------------------------------------------------------------------ 6: refusals
def test_bind_features_refuses_indices_outside_the_tables(engine):
    from genie2_amd.capi import GenieError
    N = 65
    f, mask, trans, ts, rots = CD.case(N, 'randn')
    before = run(engine, 'hx', f, trans, rots, ts)
    for key, value in (('residue_index', engine.n_pos), ('chain_index', engine.n_chain), ('residue_index', -1), ('chain_index', -1)):
        g = dict(f)
        g[key] = f[key].clone()
        g[key][1, 3] = value
        with pytest.raises(GenieError, match='residue_index / chain_index'):
            engine.bind_features(g)
        g[key][1, 3] = engine.n_pos - 1 if key == 'residue_index' else engine.n_chain - 1       # the last row is accepted
        engine.bind_features(g)
    after = run(engine, 'hx', f, trans, rots, ts)
    assert torch.isfinite(after['z']).all()
    assert all(torch.equal(before[t], after[t]) for t in ('z', 's', 'states', 'p_init', 'p'))
