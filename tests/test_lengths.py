"""Every length and every kernel dispatch path of the sampling library against the oracle.  GPU only.

The launchers pick kernels from NP = ceil(N / 32) * 32, from N itself and from the model dims:

  k_trimul_contract_hx<1>                      NP < 128
  k_trimul_contract_hx<2>                      NP = 128 .. 192 (one or two tiles of 128, NP = 192: one full + one half) and NP > 256
  k_trimul_contract_hx_big                     192 < NP <= 256 (NP = 224: N = 193 .. 224)
  k_ipa_attn_q (four queries), k_ipa_prep_frag base IPA dims, N <= 664 (48 * NP8 + 8848 floats of LDS against 160 KiB)
  k_ipa_attn_t (one query), k_ipa_prep         base IPA dims, N >= 665; no two-stream split of the structure layers
  k_p_sample_frenet past 64 KiB of LDS         N > 682

so the sampler's length sweep (--min_length 50 --max_length 256 --length_step 1) makes every residue of N modulo 4, 8, 32, 64 and
128 a user input.  Here: every N in 2 .. 288 (small_dims), the base model on either side of every switch, long structures up to
the documented limit N = 1706 against the float64 oracle, the documented limits themselves, and two live handles in one process.

Bounds: the project's bar 1e-4 * max(1, |ref|_inf) (SURVEY.md 8c / BASELINE.md 4) for z, states (valid residues), p_init and p
(all elements); 2e-6 for Frenet frames; padded pairs of p exactly zero; everything finite.  Beyond N = 256 the float32 oracle's
own rounding is no longer negligible against that bar, so the long cases use the float64 oracle and, at each N,
max(1e-4, 3 * e32(N)) * max(1, |ref|_inf) with e32(N) the float32 oracle's error against the float64 oracle on the same inputs
(factor 3: the kernels sum in another order, and hx carries about the same significand as f32; not a device measurement).
"""
import pytest
import torch

from _parity import (BAR, FRAME_TOL, MATH_MODES, TAPS, compare_taps, conditioned_inputs, failures, hard_time_limit, oracle_taps,
                     ragged, worst)
from oracle import genie_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """each test of this file under a limit of its own: the oracle's CPU time dominates (a few minutes for the sweep)"""
    with hard_time_limit(2400):
        yield


def mdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def frame_result(got, ref, tol=FRAME_TOL):
    return ('frenet', mdiff(got, ref), tol)


def last_entry_alone(engine, features, trans, rots, ts, out):
    """[('batch1_bits', 0 | 1, 0)]: the last batch entry equals its own batch-1 run bit for bit (z and p), as test_config3.py"""
    B, N = features['residue_mask'].shape
    L = int(features['residue_mask'][B - 1].sum())
    z, p = out['z'][B - 1].clone(), out['p'][B - 1].clone()
    engine.bind_features(O.empty_features([L], n_pad=N))
    o1 = engine.denoise(trans[B - 1:], rots[B - 1:], ts[B - 1:], None, taps=('p',))
    same = torch.equal(o1['z'][0], z) and torch.equal(o1['p'][0], p)
    return [('batch1_bits', 0.0 if same else 1.0, 0.0)]


# ------------------------------------------------------------------ every length
SWEEP_LENGTHS = list(range(288, 1, -1))            # descending: the workspace is allocated once
_SWEEP = {}


def _run_sweep():
    """Both arithmetics at every length in one pass (the oracle once per N; keeping 287 references of p for a second pass would
    take 16 GB): {math: dict(cases, failures, worst)}."""
    if _SWEEP:
        return _SWEEP
    from genie2_amd.engine import GenieEngine
    dims = O.small_dims()
    sd = O.synthetic_state_dict(dims, seed=3)
    eng = GenieEngine(dims, sd, 'cuda:0', n_pos=512)          # position table rows past max_n_res = 256 (the encoding's divisor stays)
    acc = {m: dict(cases=0, failures=[], worst=(None, None, 0.0), worst_frames=(None, None, 0.0)) for m in MATH_MODES}
    try:
        for N in SWEEP_LENGTHS:
            f = O.empty_features(ragged(N))
            fr = O.prepare_features(f)
            trans, ts = conditioned_inputs(f, dims['n_timestep'], 1000 + N)
            eng.bind_features(f)
            rots = eng.frenet(trans)
            fres = frame_result(rots, O.compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask']))
            ref = oracle_taps(sd, dims, f, rots, trans, ts)
            for math in MATH_MODES:
                eng.set_math(math)
                out = eng.denoise(trans, rots, ts, None, taps=('states', 'p_init', 'p'))
                res = [fres] + compare_taps(out, ref, fr['residue_mask'])
                del out
                a = acc[math]
                a['cases'] += 1
                a['failures'] += failures(N, res)
                for key, frames in (('worst', False), ('worst_frames', True)):
                    tap, ratio = worst(res, frames)
                    if ratio > a[key][2]:
                        a[key] = (N, tap, ratio)
            if N % 32 == 0:
                print('sweep: down to N = %d, worst (N, tap, error / bound) so far: %s' % (N, {m: acc[m]['worst'] for m in MATH_MODES}), flush=True)
    finally:
        eng.close()
    _SWEEP.update(acc)
    return _SWEEP


@pytest.mark.parametrize('math', MATH_MODES)
def test_every_length_matches_oracle(math):
    """small_dims (the base model's widths and kernels, 2 + 2 layers), a ragged batch [N, N // 2 + 1] at EVERY N from 288 down to
    2, seeded coordinates and per-entry timesteps, frames from the engine: engine.frenet, z, states, p_init, p against the float32
    oracle under the bar, padded pairs of p exactly zero, all finite.  No length is skipped: every failure is collected and the
    list must be empty, so one run names every bad length.  (The float32 oracle is within 1.2e-5 of its float64 self at every one
    of these lengths: an eighth of the bar.)"""
    r = _run_sweep()
    assert sum(r[m]['cases'] for m in MATH_MODES) == 574 and r[math]['cases'] == len(SWEEP_LENGTHS) == 287
    print('sweep[%s]: %d lengths, worst (N, tap, error / bound) = (%s, %s, %.3f), frames (%s, %s, %.3f)'
          % ((math, r[math]['cases']) + r[math]['worst'] + r[math]['worst_frames']))
    assert not r[math]['failures'], r[math]['failures'][:40]


# ------------------------------------------------------------------ the base model on either side of every switch
BOUNDARY_LENGTHS = [96, 97, 127, 128, 129, 160, 161, 191, 192, 193, 200, 223, 224, 225, 255, 257, 288, 289]
# batch 2 ragged everywhere; 5 entries at 200 and 289, and 6 at 200: the two-stream split of the structure layers needs
# B * N >= 1024 rows, which 5 x 200 misses
BOUNDARY_CASES = [(N, 2) for N in BOUNDARY_LENGTHS] + [(200, 5), (200, 6), (289, 5)]
assert len(BOUNDARY_CASES) == 21
_BOUNDARY_REF = {}


def _batch_lengths(N, B):
    return (ragged(N) + [N - 7, N, N - 1, N - 3])[:B] if B > 2 else ragged(N)


@pytest.fixture(scope='module')
def base_engine_512(base_weights):
    """the base model with a position table of 512 rows: the session engine's ends at max_n_res = 256"""
    from genie2_amd.engine import GenieEngine
    eng = GenieEngine(dict(O.BASE_DIMS), base_weights, 'cuda:0', n_pos=512)
    yield eng
    eng.close()


@pytest.mark.parametrize('N,B,math', [(n, b, m) for n, b in BOUNDARY_CASES for m in MATH_MODES])
def test_base_model_at_dispatch_boundaries(base_engine, base_engine_512, base_weights, N, B, math):
    """Five pair blocks and eight structure layers (k_ipa_bias_hx with 96 rows, the fused chains between blocks) at the lengths
    around every switch of the contraction and attention launchers.  Same taps and bounds as the sweep, plus: the last batch
    entry equals its own batch-1 run bit for bit."""
    dims = dict(O.BASE_DIMS)
    base_engine = base_engine if N <= 256 else base_engine_512
    f = O.empty_features(_batch_lengths(N, B))
    fr = O.prepare_features(f)
    trans, ts = conditioned_inputs(f, dims['n_timestep'], 7000 + 10 * N + B)
    base_engine.set_math(math)
    try:
        base_engine.bind_features(f)
        rots = base_engine.frenet(trans)
        res = [frame_result(rots, O.compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask']))]
        if (N, B) not in _BOUNDARY_REF:            # one reference at a time: both arithmetics of a case follow each other
            _BOUNDARY_REF.clear()
            _BOUNDARY_REF[(N, B)] = oracle_taps(base_weights, dims, f, rots, trans, ts)
        out = base_engine.denoise(trans, rots, ts, None, taps=('states', 'p_init', 'p'))
        res += compare_taps(out, _BOUNDARY_REF[(N, B)], fr['residue_mask'])
        res += last_entry_alone(base_engine, f, trans.cuda(), rots, ts, out)
    finally:
        base_engine.set_math('hx')
    print('boundary N=%d B=%d %s: worst (tap, error / bound) = (%s, %.3f), frames (%s, %.3f)' % ((N, B, math) + worst(res) + worst(res, True)))
    assert not failures((N, B), res), failures((N, B), res)


# ------------------------------------------------------------------ long structures against the float64 oracle
# e32: error of the float32 oracle against the float64 oracle on exactly these inputs, relative to max(1, |ref|_inf), per tap
# (z, states, p_init, p); recorded from a CPU run of this file's own inputs (oracle frames instead of the engine's, which moves
# nothing at this precision).  (N, batch) -> e32
LONG_E32 = {
    (320, 1): (2.4e-06, 7.7e-06, 6.1e-06, 7.5e-06),
    (512, 1): (4.5e-06, 1.4e-05, 1.1e-05, 1.5e-05),
    (512, 2): (3.3e-06, 1.1e-05, 1.2e-05, 1.2e-05),
    (664, 1): (5.0e-06, 1.3e-05, 1.0e-05, 1.5e-05),
    (665, 1): (3.6e-06, 1.3e-05, 1.3e-05, 1.3e-05),
    (672, 1): (3.6e-06, 9.9e-06, 1.4e-05, 1.5e-05),
    (673, 1): (4.0e-06, 1.0e-05, 1.3e-05, 1.2e-05),
    (680, 1): (4.0e-06, 1.1e-05, 1.4e-05, 1.6e-05),
    (680, 2): (6.4e-06, 1.7e-05, 1.4e-05, 2.6e-05),
    (1024, 1): (7.4e-06, 2.2e-05, 2.1e-05, 2.6e-05),
}
LONG_CASES = [(320, 1), (512, 1), (512, 2), (664, 1), (665, 1), (672, 1), (673, 1), (680, 1), (680, 2), (1024, 1)]
assert len(LONG_CASES) == 10
_LONG = {}


def long_dims(**over):
    return O.small_dims(max_n_res=2048, **over)            # the position table must cover the length


def long_inputs(N, B, dims):
    f = O.empty_features(ragged(N) if B == 2 else [N])
    trans, ts = conditioned_inputs(f, dims['n_timestep'], 5000 + 10 * N + B)
    return f, trans, ts


def long_bounds(e32):
    return {tap: max(BAR, 3.0 * e) for tap, e in zip(TAPS, e32)}


@pytest.fixture(scope='module')
def long_engine():
    from genie2_amd.engine import GenieEngine
    dims = long_dims()
    sd = O.synthetic_state_dict(dims, seed=3)
    eng = GenieEngine(dims, sd, 'cuda:0')
    eng._test_weights = sd
    yield eng
    eng.close()


@pytest.mark.parametrize('N,B,math', [(n, b, m) for n, b in LONG_CASES for m in MATH_MODES])
def test_long_structures_match_float64_oracle(long_engine, N, B, math):
    """N = 664 is the last length on the four-query attention kernel and 665 the first on the one-query kernel (and 672 / 673
    the next multiple of 8 and the length the documentation used to name); 1024 runs the contraction over eight tiles and the
    Frenet kernel past 64 KiB of LDS.  z, states, p_init, p, the Frenet frames and one reverse step against the float64 oracle
    (float32 weights and inputs cast up) under max(1e-4, 3 * e32(N)) * max(1, |ref|_inf).  Measured errors: DESIGN.md."""
    eng, dims, sd = long_engine, long_engine.dims, long_engine._test_weights
    f, trans, ts = long_inputs(N, B, dims)
    fr = O.prepare_features(f)
    eng.set_math(math)
    try:
        eng.bind_features(f)
        rots = eng.frenet(trans)
        if (N, B) not in _LONG:
            _LONG.clear()
            r64 = O.compute_frenet_frames(trans.double(), fr['chain_index'], fr['residue_mask'])
            r32 = O.compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask'])
            _LONG[(N, B)] = dict(rots=r64, rots_e32=mdiff(r32, r64), ref=oracle_taps(sd, dims, f, rots, trans, ts, double=True))
        c = _LONG[(N, B)]
        res = [frame_result(rots, c['rots'], max(FRAME_TOL, 3.0 * c['rots_e32']))]
        out = eng.denoise(trans, rots, ts, None, taps=('states', 'p_init', 'p'))
        res += compare_taps(out, c['ref'], fr['residue_mask'], long_bounds(LONG_E32[(N, B)]))
        # one reverse step from these coordinates with the engine's own z (test_p_sample_matches_oracle's bounds, the frames' own
        # float32 error allowed for as above)
        g = torch.Generator().manual_seed(N)
        eps = torch.randn(B, N, 3, generator=g)
        z = out['z'].cpu()
        del out
        sched = O.setup_schedule(dims['n_timestep'])
        nx, nr = O.p_sample_step(sched, 40, 0.6, trans.double(), z.double(), eps.double(), fr)
        _, nr32 = O.p_sample_step(sched, 40, 0.6, trans, z, eps, fr)
        xg = trans.clone().cuda()
        rg = eng.p_sample(40, 0.6, xg, z.cuda(), eps.cuda())
        res.append(('p_sample_x', mdiff(xg, nx), 2e-6 * max(1.0, float(nx.abs().max()))))
        res.append(('p_sample_frames', mdiff(rg, nr), max(5e-6, 3.0 * mdiff(nr32, nr))))
    finally:
        eng.set_math('hx')
    print('long N=%d B=%d %s: ' % (N, B, math) + ', '.join('%s %.2e / %.2e' % r for r in res if r[2] > 0))
    assert not failures((N, B), res), failures((N, B), res)


# ------------------------------------------------------------------ the documented limits
LIMIT_CASES = [   # (N, batch) accepted, (N, batch) refused, what the refusal says
    ((1706, 1), (1707, 1), 'Frenet'),                      # 96 B of LDS per residue against 160 KiB
    ((256, 63), (256, 64), 'split the batch'),             # a [B,NP,NP,128] f32 tensor stays below 2 GiB
    ((512, 15), (512, 16), 'split the batch'),
    ((1024, 3), (1024, 4), 'split the batch'),
]


@pytest.fixture(scope='module')
def thin_engine():
    """one layer of each kind: the limits and the longest structure do not depend on the depth"""
    from genie2_amd.engine import GenieEngine
    dims = long_dims(n_pair_transform_layer=1, n_structure_layer=1)
    sd = O.synthetic_state_dict(dims, seed=3)
    eng = GenieEngine(dims, sd, 'cuda:0')
    eng._test_weights = sd
    yield eng
    eng.close()


@pytest.mark.parametrize('ok,bad,word', LIMIT_CASES, ids=['N%d_B%d' % c[0] for c in LIMIT_CASES])
def test_documented_limits_accept_one_side_refuse_the_other(thin_engine, ok, bad, word):
    from genie2_amd.capi import GenieError
    with pytest.raises(GenieError, match=word):
        thin_engine.bind_features(O.empty_features([bad[0]] * bad[1]))
    thin_engine.bind_features(O.empty_features([ok[0]] * ok[1]))
    torch.cuda.synchronize()
    assert (thin_engine.N, thin_engine.B) == ok
    # the handle stays usable: a small batch gives what a fresh bind gives
    f = O.empty_features([16])
    trans, ts = conditioned_inputs(f, 100, 3)
    thin_engine.bind_features(f)
    rots = thin_engine.frenet(trans)
    ref = oracle_taps(thin_engine._test_weights, thin_engine.dims, f, rots, trans, ts)
    out = thin_engine.denoise(trans, rots, ts, None, taps=('states', 'p_init', 'p'))
    assert not failures(ok, compare_taps(out, ref, f['residue_mask']))


# e32 at N = 1706 with one layer of each kind: float32 oracle against float64 oracle, measured on the CPU (z, states, p_init, p)
E32_1706 = (1.4e-05, 4.1e-05, 3.9e-05, 4.8e-05)


@pytest.mark.parametrize('math', MATH_MODES)
def test_longest_structure_n1706(thin_engine, math):
    """N = 1706, the longest structure the library accepts, batch 1, one layer of each kind: z, states, p_init, p and the frames
    against the FLOAT32 oracle (its float64 form needs about 20 GB of host memory at this length) under
    max(1e-4, 3 * e32) * max(1, |ref|_inf), e32 measured once on the CPU for exactly these inputs (E32_1706)."""
    N = 1706
    eng, dims, sd = thin_engine, thin_engine.dims, thin_engine._test_weights
    f, trans, ts = long_inputs(N, 1, dims)
    fr = O.prepare_features(f)
    eng.set_math(math)
    try:
        eng.bind_features(f)
        rots = eng.frenet(trans)
        res = [frame_result(rots, O.compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask']))]
        if N not in _LONG:
            _LONG.clear()
            _LONG[N] = oracle_taps(sd, dims, f, rots, trans, ts)
        out = eng.denoise(trans, rots, ts, None, taps=('states', 'p_init', 'p'))
        res += compare_taps(out, _LONG[N], fr['residue_mask'], long_bounds(E32_1706))
    finally:
        eng.set_math('hx')
    print('N=1706 %s: ' % math + ', '.join('%s %.2e / %.2e' % r for r in res if r[2] > 0))
    assert not failures(N, res), failures(N, res)


# ------------------------------------------------------------------ two live handles
def _denoise_inputs(eng, lengths, seed):
    f = O.empty_features(lengths)
    trans, ts = conditioned_inputs(f, eng.dims['n_timestep'], seed)
    eng.bind_features(f)
    rots = eng.frenet(trans)
    return trans.cuda(), rots, ts.cuda()


@pytest.mark.parametrize('math', MATH_MODES)
def test_two_live_handles_do_not_share_launch_limits(base_engine, long_engine, math):
    """The dynamic-LDS ceiling of a kernel is process state, not handle state.  A handle bound at N = 256 (75 KiB for the hx
    attention kernel) must still launch after another handle bound N = 50, and the other way round; the same for the one-query
    kernel and the Frenet kernel past 64 KiB at N = 700 beside a handle at N = 64, and for the handle-free
    compute_frenet_frames at N = 1000 after a handle bound N = 50.  Without re-binding, and bit for bit."""
    from genie2_amd.engine import GenieEngine, compute_frenet_frames
    dims = O.small_dims()
    small = GenieEngine(dims, O.synthetic_state_dict(dims, seed=3), 'cuda:0', math=math)
    base_engine.set_math(math)
    long_engine.set_math(math)
    try:
        # A binds 256 and runs; B binds 50 and runs; A runs again as it is
        a_in = _denoise_inputs(base_engine, [256, 129], 11)
        za = base_engine.denoise(*a_in)['z'].clone()
        assert torch.isfinite(za).all()
        b_in = _denoise_inputs(small, [50, 26], 12)
        zb = small.denoise(*b_in)['z'].clone()
        assert torch.equal(base_engine.denoise(*a_in)['z'], za)
        # the other way round: B (small) bound first, A at 256 afterwards, then B again as it is
        b_in = _denoise_inputs(small, [50, 26], 12)
        a_in = _denoise_inputs(base_engine, [256, 129], 11)
        assert torch.equal(base_engine.denoise(*a_in)['z'], za)
        assert torch.equal(small.denoise(*b_in)['z'], zb)
        # one-query attention and a Frenet launch of 67 KiB at N = 700, beside a handle at N = 64
        l_in = _denoise_inputs(long_engine, [700], 13)
        zl = long_engine.denoise(*l_in)['z'].clone()
        rl = long_engine.frenet(l_in[0]).clone()
        assert torch.isfinite(zl).all()
        s_in = _denoise_inputs(small, [64, 33], 14)
        zs = small.denoise(*s_in)['z'].clone()
        assert torch.equal(long_engine.denoise(*l_in)['z'], zl) and torch.equal(long_engine.frenet(l_in[0]), rl)
        assert torch.equal(small.denoise(*s_in)['z'], zs)
        # the handle-free Frenet frames at N = 1000 (96 KB of LDS) after a handle bound N = 50, and the long handle after it
        _denoise_inputs(small, [50, 26], 12)
        f = O.empty_features([1000])
        x, _ = conditioned_inputs(f, 100, 15)
        ref = O.compute_frenet_frames(x, f['chain_index'], f['residue_mask'])
        assert mdiff(compute_frenet_frames(x.cuda(), f['chain_index'], f['residue_mask']), ref) < FRAME_TOL
        assert torch.equal(long_engine.frenet(l_in[0]), rl) and torch.equal(long_engine.denoise(*l_in)['z'], zl)
    finally:
        small.close()
        base_engine.set_math('hx')
        long_engine.set_math('hx')
