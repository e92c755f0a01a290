"""genie_train_forward_backward and genie_denoise_vjp on every row of the GEMM / LayerNorm dispatch table (tests/_train_paths.py:
five batches of 4 418 .. 16 928 pair rows on the two-plus-two-layer small model; test_train_paths_host.py states which kernels each
reaches) against torch autograd over the oracle in float64.

One engine for the module, the cases in descending P (one workspace allocation), every test under a hard time limit."""
import pytest
import torch

import _train_paths as T
from _parity import hard_time_limit
from test_training import check_grads, flat, split

pytestmark = pytest.mark.gpu

NAMES = list(T.CASES)
LIMIT = 300             # seconds; a test takes a few
# Whole-vector bound of test_gradients_on_every_path: relative L2 error against float64 <= L2_FACTOR x max(e32_L2, 1e-6), e32_L2 being
# the float32 oracle's own error (computed in the test).  Twice the largest ratio measured on the MI355X, rounded up: DESIGN.md 7,
# "Training paths by pair rows".
L2_FACTOR = 3
RATES = dict(tri_dropout=0.25, ipa_dropout=0.1, transition_dropout=0.1)


@pytest.fixture(scope='module')
def eng():
    from genie2_amd.engine import GenieEngine
    with hard_time_limit(LIMIT):
        e = GenieEngine(T.dims(), T.weights(), 'cuda:0')
    yield e
    e.close()


@pytest.fixture(scope='module')
def w():
    return flat(T.weights(), T.dims()).cuda()


def _step(eng, w, name, **kw):
    c = T.build(name)
    eng.bind_features(c['features'])
    kw.setdefault('train_mode', False)
    kw.setdefault('fast_math', 0)
    out = eng.train_forward_backward(w, c['trans'], c['rots'], c['ts'], c['z'], c['weight'], **kw)
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.mark.parametrize('name', NAMES)
def test_gradients_on_every_path(eng, w, name):
    """Eval-mode step, f32-grade arithmetic.  z on valid residues and both losses under the bounds of
    test_gradients_match_oracle_autograd_small_dims; every gradient tensor against the FLOAT64 oracle at the project's 5e-3; and the
    whole gradient vector's relative L2 error against float64 within L2_FACTOR of the float32 oracle's own (floored at 1e-6) -- a
    bound a path that is subtly wrong (a lost K range, a misplaced block, a stale mask bit) cannot meet, while per tensor 5e-3 of
    the largest entry might let it through.  Measured ratios per case: DESIGN.md 7, "Training paths by pair rows"."""
    c = T.build(name)
    o32, o64 = T.oracle_grads(name, torch.float32), T.oracle_grads(name, torch.float64)
    e32 = T.rel_l2(o32['grads'], o64['grads'])
    with hard_time_limit(LIMIT):
        out = _step(eng, w, name)
        z, grads = out['z'].cpu(), split(out['grads'].cpu(), T.dims())
    zo = o64['z']
    dz = float(((z.double() - zo) * c['mask']).abs().max())
    got = T.rel_l2(grads, o64['grads'])
    worst = T.worst_tensor(grads, o64['grads'])
    print('%s: |dz| %.2e  loss %.2e / %.2e  worst tensor %.2e (%s)  L2 %.2e  e32_L2 %.2e  ratio %.2f' % (
        name, dz, _rel(out['weighted_loss'], o64['weighted_loss']), _rel(out['unweighted_loss'], o64['unweighted_loss']), worst[0], worst[1],
        got, e32, got / max(e32, 1e-6)))
    assert dz <= 2e-4 * max(1.0, float(zo.abs().max()))
    assert _rel(out['weighted_loss'], o64['weighted_loss']) <= 1e-4 and _rel(out['unweighted_loss'], o64['unweighted_loss']) <= 1e-4
    check_grads(grads, o64['grads'])
    assert got <= L2_FACTOR * max(e32, 1e-6), (got, e32)


@pytest.mark.parametrize('name', NAMES)
def test_vjp_on_every_path(eng, w, name):
    """genie_denoise_vjp: the backward pass with no weight-gradient buffer (the sink targets, k_pair_features_bwd, every dX GEMM)
    at these shapes.  dtrans on valid residues against float64 autograd at 5e-3 of the reference's largest magnitude, z against
    the sampling path's own forward at 2e-4.  A second call gives the same bits: nothing on this path is summed with float atomics
    (the guidance samplers amplify a rounding-level difference of dtrans by 1e4 over twelve steps, so their runs agree only if it does)."""
    c = T.build(name)
    ref = T.vjp_ref(name, torch.float64)
    with hard_time_limit(LIMIT):
        eng.bind_features(c['features'])
        z, dt = eng.denoise_vjp(w, c['x'], c['x_rots'], c['ts'], c['v'])
        z_s = eng.denoise(c['x'], c['x_rots'], c['ts'])['z']
        z2, dt2 = eng.denoise_vjp(w, c['x'], c['x_rots'], c['ts'], c['v'])
        again = bool(torch.equal(z, z2)) and bool(torch.equal(dt, dt2))
        z, dt, z_s = z.cpu(), dt.cpu(), z_s.cpu()
    m = c['mask']
    scale = float((ref['dtrans'] * m).abs().max())
    d = float(((dt.double() - ref['dtrans']) * m).abs().max())
    zscale = max(1.0, float(ref['z'].abs().max()))
    dzs = float(((z_s - z) * m).abs().max())
    dzo = float(((z.double() - ref['z']) * m).abs().max())
    print('%s: dtrans %.2e of %.2e (%.2e)  z vs sampling path %.2e  z vs float64 %.2e' % (name, d, scale, d / scale, dzs, dzo))
    assert torch.isfinite(dt).all()
    assert again, 'two calls of genie_denoise_vjp on the same inputs differ'
    assert d <= 5e-3 * scale
    assert dzs <= 2e-4 * zscale and dzo <= 2e-4 * zscale


@pytest.mark.parametrize('name', NAMES)
def test_repeat_and_rebind_agree(eng, w, name):
    """The case, then another case bound and run on the same handle, then the first again: the two gradient vectors of the first
    agree to relative L2 1e-5 (what equal weights give when only the float-atomic order differs) and the losses to 1e-6.  An
    accumulator left un-zeroed, a stale ReLU mask or fold table, or a race would show here; the test claims no more than that."""
    other = NAMES[(NAMES.index(name) + 1) % len(NAMES)]
    with hard_time_limit(LIMIT):
        a = _step(eng, w, name)
        _step(eng, w, other)
        b = _step(eng, w, name)
        ga, gb = a['grads'].double(), b['grads'].double()
        rel = float((ga - gb).norm() / ga.norm())
    print('%s (between: %s): gradients %.2e  loss %.2e' % (name, other, rel, _rel(b['weighted_loss'], a['weighted_loss'])))
    assert torch.isfinite(ga).all() and rel <= 1e-5
    assert _rel(b['weighted_loss'], a['weighted_loss']) <= 1e-6 and _rel(b['unweighted_loss'], a['unweighted_loss']) <= 1e-6


def test_train_mode_dropout_on_tiled_paths(eng, w):
    """Train mode at [56, 40]: the row-shared triangle dropout index and the fused gate / LayerNorm layout kernels together with the
    64- and 128-tile GEMMs, the ReLU mask bits and the block table.  Loss and every gradient against autograd over the oracle
    under the SAME masks (oracle.train_dropout_masks)."""
    name, seed = 'n56_40', 1234
    ref = T.oracle_grads(name, torch.float64, (seed, RATES['tri_dropout'], RATES['ipa_dropout'], RATES['transition_dropout']))
    plain = T.oracle_grads(name, torch.float64)
    assert _rel(ref['weighted_loss'], plain['weighted_loss']) > 1e-3          # the masks are live in the reference
    with hard_time_limit(LIMIT):
        out = _step(eng, w, name, train_mode=True, seed=seed, **RATES)
        grads = split(out['grads'].cpu(), T.dims())
    print('%s train mode: loss %.2e  worst tensor %s' % (name, _rel(out['weighted_loss'], ref['weighted_loss']), T.worst_tensor(grads, ref['grads'])))
    assert _rel(out['weighted_loss'], ref['weighted_loss']) <= 1e-4
    check_grads(grads, ref['grads'])


@pytest.mark.parametrize('name', ['n56_40', 'n47_31'])
def test_reduced_precision_modes_on_mixed_paths(eng, w, name):
    """fast_math 2 and 1 (two bf16 pieces, plain bf16: the TERMS = 2 and TERMS = 1 instantiations of all three GEMM kernels) against
    mode 0 on the device, under the bounds of test_bf16_operand_mode_points_the_same_way."""
    with hard_time_limit(LIMIT):
        ref = _step(eng, w, name)
        gr, lr_ = ref['grads'].double(), float(ref['weighted_loss'])
        for mode, cos_min, rel_max, loss_tol in ((2, 0.99999, 5e-3, 1e-4), (1, 0.995, 0.1, 2e-2)):
            o = _step(eng, w, name, fast_math=mode)
            gm = o['grads'].double()
            cos = float((gm * gr).sum() / (gm.norm() * gr.norm()))
            rel = float((gm - gr).norm() / gr.norm())
            print(name, 'fast_math', mode, 'cosine', cos, 'relative', rel, 'loss', float(o['weighted_loss']), lr_)
            assert cos >= cos_min and rel <= rel_max, (mode, cos, rel)
            assert abs(float(o['weighted_loss']) - lr_) <= loss_tol * lr_
