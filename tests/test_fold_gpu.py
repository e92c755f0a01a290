"""The fold potential on the GPU (genie_fold_potential, csrc/fold_kernels.hip; FoldPotential in genie2_amd/smc.py) against the float64
oracle of tests/_fold.py, against PairwiseTM, in TwistedSampler against the float32 PyTorch restatement as its twisting function,
summed with the shape potential, and through both command lines.

Bounds (the project's bars for a fused potential, as in test_binder_gpu.py): logp, `tm_of`, `tm_nearest`, `tm_lowest_wanted` and
`e_fold` within 1e-5 max(1, |value|); every particle's gradient within 1e-5 of its largest float64 entry; each widened, per case, to
4 x the error the float32 restatement makes on the same input where that is larger; `nearest` exact where the two best TM-scores
differ by more than the bar, `n_fold_violations` exact where no n_r is within 1e-4 N of an active bound.  A particle is left out of
the logp and gradient comparison only if one of its pairs with an active hinge is ill-posed by the oracle's rule (tests/_fold.py:
another seed within 1e-4 in TM whose fit gives another gradient, or a Horn gap below 1e-4), and at most 5 % of a case's particles may
be: with these inputs none is.

Worst error / bound over the parity cases, measured on an MI355X: 0.224 for tm_of ((8, 40, 300), its bar widened x7.0; 0.013 is the
worst of the others), 0.061 for logp and 0.060 for e_fold ((3, 5, 3)), 0.229 for the gradient ((2, 129, 9), bar widened x5.4); the
gradient's bar was widened in every case, x1.6 to x42 (N = 1706), by the restatement's own error, and against the unwidened 1e-5
the kernel is inside in seven cases and at 1.1, 1.2 and 4.2 x in three; every count was equal; no particle was left out.  The sampler
comparison ends 2.5e-4 of the coordinate RMS apart (bar 1e-3).  DESIGN.md 7.9 has the table per case."""
import math
import os

import numpy as np
import pytest
import torch

import _fold as Fd
import _similarity as S
from _motif import MOTIF, _abar, _tiny_model
from _parity import hard_time_limit
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

STEP = 500
TEMPLATE = os.path.join(GOLDEN, 'dataset_100_0.pdb')
_cache = {}


@pytest.fixture(autouse=True)
def _limit():
    with hard_time_limit(300):
        yield


def _inputs(case):
    if case not in _cache:
        _cache[case] = Fd.inputs(case)
    return _cache[case]


def _potential(ref, bounds, n_res, abar=None, **kw):
    from genie2_amd.smc import FoldPotential
    return FoldPotential(n_res, _abar() if abar is None else abar, ref, bounds, device='cuda', **kw)


def _reference(x, ref, bounds, var, n_iter=16, upper=True):
    """The oracle and the float32 restatement of an input, computed once."""
    key = ('ref', x.data_ptr(), ref.data_ptr(), repr(torch.as_tensor(bounds).tolist()), var, n_iter, upper)
    if key not in _cache:
        _cache[key] = (x, ref, Fd.reference(x, ref, bounds, var, n_iter, upper), Fd.restatement32(x, ref, bounds, var, n_iter, upper))
    return _cache[key][2:]


def _run(pot, x, step=STEP):
    x = x.cuda().requires_grad_(True)
    lp = pot(x, step)
    g, = torch.autograd.grad(lp.sum(), x)
    return lp.detach(), g


def _widen(err, bound):
    """The factor a bar is widened by: 4 x the float32 restatement's error / bound where that is above 1."""
    return max(1.0, 4.0 * float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max())) if err.numel() else 1.0


def _ratio(d, b):
    return float(torch.where(b > 0, d / b.clamp(min=1e-300), torch.where(d > 0, math.inf, 0.0).double()).max()) if d.numel() else 0.0


def _value(what, name, got, r, r32):
    """A float output against the oracle under the 1e-5 max(1, |value|) bar, widened by the restatement's own error."""
    got, r32 = got.double().cpu().reshape(-1), r32.double().cpu().reshape(-1)
    r = r.reshape(-1)
    bound = 1e-5 * r.abs().clamp(min=1.0)
    wide = _widen((r32 - r).abs(), bound)
    print('%s: %s error / bound %.3f (bar widened x%.2f)' % (what, name, _ratio((got - r).abs(), bound * wide), wide))
    assert bool(torch.isfinite(got).all()) and bool(((got - r).abs() <= bound * wide).all()), (what, name, got, r)
    return bound * wide


def _parity(what, x, ref, bounds, n_iter=16, upper=True, pot=None, cap=0.05):
    """Everything the entry returns for x against the oracle; returns (pot, oracle, logp, grad)."""
    bounds = torch.as_tensor(bounds, dtype=torch.float64)
    B, N = x.shape[0], x.shape[1]
    pot = _potential(ref, bounds, N, n_iter=n_iter) if pot is None else pot
    r64, r32 = _reference(x, ref, bounds, float(pot.variance(STEP)), n_iter, upper)
    lp, g = _run(pot, x)
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), what
    keep = ~Fd.left_out(r64)
    print('%s: %d of %d particles left out' % (what, int((~keep).sum()), B))
    assert int((~keep).sum()) <= cap * B, (what, keep)
    tm = pot.tm_of(x.cuda())
    assert tuple(tm.shape) == tuple(r64['tm'].shape) and tm.dtype == torch.float32 and tm.device.type == 'cuda'
    tm_bar = _value(what, 'tm_of', tm, r64['tm'], r32['tm']).reshape(r64['tm'].shape)
    if bool(keep.any()):
        _value(what, 'logp', lp[keep.cuda()], r64['logp'][keep], r32['logp'][keep])
        g_b = 1e-5 * r64['grad'].abs().amax(dim=(1, 2))[keep]
        wide = _widen((r32['grad'].double() - r64['grad']).abs().amax(dim=(1, 2))[keep], g_b)
        d_g = (g.double().cpu() - r64['grad']).abs().amax(dim=(1, 2))[keep]
        print('%s: gradient error / bound %.3f (bar widened x%.2f)' % (what, _ratio(d_g, g_b * wide), wide))
        assert bool((d_g <= g_b * wide).all()), (what, d_g, g_b)
    got = pot.describe(x.cuda())
    assert tuple(got) == Fd.REPORT
    for k in Fd.REPORT:
        assert tuple(got[k].shape) == (B,) and got[k].device.type == 'cuda' and got[k].dtype == (torch.int64 if k in Fd.COUNTS else torch.float32), k
    _value(what, 'tm_nearest', got['tm_nearest'], r64['tm_nearest'], r32['tm_nearest'])
    _value(what, 'tm_lowest_wanted', got['tm_lowest_wanted'], r64['tm_lowest_wanted'], r32['tm_lowest_wanted'])
    if bool(keep.any()):
        _value(what, 'e_fold', got['e_fold'][keep.cuda()], r64['e_fold'][keep], r32['e_fold'][keep])
    # nearest: exact where the two best scores differ by more than the bar (one reference: always)
    top = torch.sort(r64['tm'], dim=1, descending=True).values
    sure = (top[:, 0] - top[:, 1] > 2 * tm_bar.amax(dim=1)) if r64['tm'].shape[1] > 1 else torch.ones(B, dtype=torch.bool)
    assert torch.equal(got['nearest'].cpu()[sure], r64['nearest'][sure]), (what, got['nearest'], r64['nearest'])
    # violations: exact where no n_r is within 1e-4 N of a bound that can be active
    lo, hi = N * bounds[:, 0], N * bounds[:, 1]
    finite = torch.isfinite(hi) & torch.tensor(upper)
    near = (((r64['n'] - lo).abs() < 1e-4 * N) & (lo > 0)) | (((r64['n'] - torch.where(finite, hi, torch.zeros_like(hi))).abs() < 1e-4 * N) & finite)
    sure = ~near.any(dim=1)
    assert torch.equal(got['n_fold_violations'].cpu()[sure], r64['n_fold_violations'][sure]), (what, got['n_fold_violations'], r64['n_fold_violations'])
    return pot, r64, lp, g


@pytest.mark.parametrize('case', Fd.CASES, ids=Fd.case_id)
def test_potential_and_report_match_the_float64_oracle(case):
    x, ref, bounds = _inputs(case)
    _, r64, lp, _ = _parity(Fd.case_id(case), x, ref, bounds)
    Fd.check_inputs(r64, case)
    assert bool((r64['logp'] <= 0).all()) and float(r64['logp'].min()) < 0 and int(r64['n_fold_violations'].sum()) > 0


def test_tm_of_is_pairwise_tm_with_the_design_moving():
    """tm_of(x)[b, r] against PairwiseTM on the stack [x_b, y_r]: of two designs of equal length the one at the lower index moves.
    PairwiseTM keeps the largest score of an ascent and this entry the last; the two are equal to rounding (7.8's bar)."""
    from genie2_amd.similarity import PairwiseTM
    x, ref, bounds = _inputs((3, 65, 5))
    tm = _potential(ref, bounds, 65).tm_of(x.cuda())
    entry, worst = PairwiseTM('cuda'), 0.0
    for b in range(3):
        both = entry(torch.cat([x[b:b + 1], ref]).cuda())['tm'][0, 1:]
        d = (tm[b] - both).abs().double()
        bar = 1e-5 * both.abs().double().clamp(min=1.0)
        worst = max(worst, float((d / bar).max()))
        assert bool((d <= bar).all()), (b, tm[b], both)
    print('tm_of against PairwiseTM: difference / bar %.3f' % worst)


def test_deterministic_and_never_synchronises():
    x, ref, bounds = _inputs((2, 129, 9))
    pot = _potential(ref, bounds, 129)
    xc = x.cuda()
    a, b = _run(pot, xc, 400), _run(pot, xc, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ra, rb = pot.describe(xc), pot.describe(xc)
    assert all(torch.equal(ra[k], rb[k]) for k in ra)
    ta = pot.tm_of(xc)
    assert torch.equal(ta, pot.tm_of(xc))
    xg = xc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(xg, 400)
        g, = torch.autograd.grad(lp.mean(), xg)
        rep = pot.describe(xc)
        tm = pot.tm_of(xc)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.allclose(g, a[1] / 2, rtol=1e-6, atol=0)      # (the backward scales by grad_output = 1/2)
    assert all(torch.equal(rep[k], ra[k]) for k in ra) and torch.equal(tm, ta)
    with pytest.raises(ValueError):
        pot(xc[:, :128], 400)                                                             # a wrong N
    with pytest.raises(ValueError):
        pot(x, 400)                                                                       # a CPU tensor
    with pytest.raises(ValueError):
        pot.tm_of(x)
    with pytest.raises(ValueError):
        pot.describe(xc[:, :64])


def _with_weights(pot, weights):
    """`pot` with the weight column of its device table replaced (the constructor refuses a table of zeros: the entry does not)."""
    table = pot.bounds.clone()
    table[:, 2] = torch.tensor(weights, dtype=torch.float32, device=table.device)
    pot.bounds = table
    return pot


def test_weights_scale_their_reference_and_zero_weights_switch_off():
    x, ref, bounds = _inputs((3, 65, 5))
    xc = x.cuda()
    base = _potential(ref, bounds, 65)
    tm = base.tm_of(xc)
    r64 = Fd.reference(x, ref, bounds, 1.0)
    act = (r64['below'] > 0) | (r64['above'] > 0)
    r0 =int(act.any(dim=0).nonzero()[0])                                # a reference with an active hinge on some particle
    one_hot = lambda r, w: [w if k == r else 0.0 for k in range(5)]      # noqa: E731
    alone = {r: _with_weights(_potential(ref, bounds, 65), one_hot(r, 1.0)).describe(xc)['e_fold'] for r in range(5)}
    assert float(alone[r0].max()) > 0
    scaled = _with_weights(_potential(ref, bounds, 65), one_hot(r0, 2.5))
    assert torch.allclose(scaled.describe(xc)['e_fold'], 2.5 * alone[r0], rtol=1e-6, atol=0)
    lp1, g1 = _run(_with_weights(_potential(ref, bounds, 65), one_hot(r0, 1.0)), x)
    lp2, g2 = _run(scaled, x)
    assert torch.allclose(lp2, 2.5 * lp1, rtol=1e-6, atol=0) and torch.allclose(g2, 2.5 * g1, rtol=1e-5, atol=1e-6 * float(g1.abs().max()))
    # ... and leave the others' bitwise unchanged: scores, and every other reference's energy on its own
    mixed = _with_weights(_potential(ref, bounds, 65), [2.5 if k == r0 else 1.0 for k in range(5)])
    assert torch.equal(mixed.tm_of(xc), tm)
    for r in range(5):
        if r != r0:
            again = _with_weights(_potential(ref, bounds, 65), [2.5 if k == r0 else 1.0 if k == r else 0.0 for k in range(5)]).describe(xc)['e_fold']
            assert torch.allclose(again, 2.5 * alone[r0] + alone[r], rtol=1e-6, atol=0)
            assert torch.equal(_with_weights(_potential(ref, bounds, 65), one_hot(r, 1.0)).describe(xc)['e_fold'], alone[r])
    total = sum(2.5 * alone[r] if r == r0 else alone[r] for r in range(5))
    assert torch.allclose(mixed.describe(xc)['e_fold'], total, rtol=1e-5, atol=0)
    # the oracle with these weights
    weighted = bounds.clone()
    weighted[r0, 2] = 2.5
    _parity('weight 2.5 on reference %d' % r0, x, ref, weighted)
    # all weights 0: logp 0 and a gradient of exactly 0
    lp, g = _run(_with_weights(_potential(ref, bounds, 65), [0.0] * 5), x)
    assert bool((lp == 0).all()) and bool((g == 0).all())


def test_upper_bound_infinite_is_no_upper_hinge():
    x, ref, bounds = _inputs((3, 64, 4))
    open_ = bounds.clone()
    open_[:, 1] = math.inf                                                # (the template's lower hinge stays; the avoided folds are idle)
    _, r64, lp, g = _parity('hi = inf', x, ref, open_, upper=False)       # the oracle without an upper hinge
    assert bool((r64['above'] == 0).all()) and float(r64['below'].max()) > 0
    with_upper = Fd.reference(x, ref, bounds, float(_potential(ref, bounds, 64).variance(STEP)))
    assert float(with_upper['above'].max()) > 0 and float((with_upper['logp'] - r64['logp']).abs().max()) > 0      # it was active before


def test_degenerate_inputs_stay_finite():
    """A particle collapsed to one point (its fit has no rotation: the oracle's gap rule leaves its gradient out, its scores and
    log p stay in) and a reference 1e4 A away (each chain is centred on its own centroid before anything is multiplied)."""
    x, ref, bounds = _inputs((3, 63, 5))
    x = x.clone()
    x[2] = x[2, 5]
    pot = _potential(ref, bounds, 63)
    r64, r32 = _reference(x, ref, bounds, float(pot.variance(STEP)))
    lp, g = _run(pot, x)
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all())
    rep = pot.describe(x.cuda())
    assert all(bool(torch.isfinite(v.double()).all()) for v in rep.values())
    _value('collapsed particle', 'tm_of', pot.tm_of(x.cuda()), r64['tm'], r32['tm'])
    _value('collapsed particle', 'logp', lp, r64['logp'], r32['logp'])
    _value('collapsed particle', 'e_fold', rep['e_fold'], r64['e_fold'], r32['e_fold'])
    assert bool(Fd.left_out(r64)[2]) and float(r64['gap'][2].max()) < 1e-4          # the rule sees it
    keep = ~Fd.left_out(r64)
    g_b = 1e-5 * r64['grad'].abs().amax(dim=(1, 2))
    wide = _widen((r32['grad'].double() - r64['grad']).abs().amax(dim=(1, 2))[keep], g_b[keep])
    assert bool(((g.double().cpu() - r64['grad']).abs().amax(dim=(1, 2))[keep] <= (g_b * wide)[keep]).all())
    x = _inputs((3, 63, 5))[0]
    far = ref + torch.tensor([1e4, 0.0, 0.0])
    _, r_far, lp_far, g_far = _parity('references 1e4 A away', x, far, bounds)
    near = Fd.reference(x, ref, bounds, float(pot.variance(STEP)))
    assert torch.allclose(r_far['tm'], near['tm'], atol=1e-4)                          # a translation changes nothing but float32 rounding


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N_S = 12, 40


def _sampler_noise(B=4):
    """Noise [T, B, N_S, 3] whose particles share all but a thousandth of every draw's variance: the four designs of a run then come
    out as one fold (TM 0.7 to 0.85 to each other), so that a template and avoided backbones made from them are near every particle.
    Near pairs are the well-posed ones: with four unrelated designs the template is far from three of them, their
    seeds tie, and the two float32 paths drift 1e-2 to 3e-2 of the RMS apart at these weights."""
    g = torch.Generator().manual_seed(4)
    common, own = torch.randn(T, 1, N_S, 3, generator=g), torch.randn(T, B, N_S, 3, generator=g)
    return math.sqrt(0.999) * common + math.sqrt(0.001) * own


@pytest.fixture(scope='module')
def ctx(base_weights, tmp_path_factory):
    from genie2_amd import pack
    from genie2_amd.smc import TwistedSampler
    model = _tiny_model(base_weights, T)
    abar = pack.schedule_tensors(T)['alphas_cumprod'].cuda()
    sampler = TwistedSampler(model)

    def run(twist, noise, outdir, **extra):
        out = sampler._sample(dict({'length': N_S, 'scale': 0.6, 'outdir': str(outdir), 'prefix': 'x', 'offset': 0, 'noise': noise,
                                    'last_unguided_steps': 0, 'guidance_alpha': 0.05, 'twisting_function': twist}, **extra))
        attrs = {k: getattr(sampler, k, None) for k in ('last_fit', 'last_shape', 'last_secstruct', 'last_pairs', 'last_positions')}
        return np.stack([r['atom_positions'] for r in out]), out, attrs

    # what the model makes of this noise without guidance ("the previous run"): one template to stay near (a moved copy of its first
    # design, 1 A of noise, wanted at TM 0.8) and three backbones to avoid (moved copies of the others, 0.7 A of noise, TM at most 0.5)
    free, _, _ = run(lambda x0, step: (x0 * 0).sum(dim=(1, 2)), _sampler_noise(), tmp_path_factory.mktemp('fold_free'), num_samples=4, ess_threshold=0.0)
    free = torch.from_numpy(free).float()
    ref = torch.stack([S.moved(free[0], 41, 1.0)] + [S.moved(free[k], 41 + k, 0.7) for k in (1, 2, 3)])
    bounds = torch.tensor([[0.8, math.inf, 1.0]] + [[0.0, 0.5, 1.0]] * 3, dtype=torch.float64)
    return dict(run=run, abar=abar, free=free, ref=ref, bounds=bounds, fused=_potential(ref, bounds, N_S, abar),
                torch=Fd.twisting_function(ref.cuda(), bounds, abar))


def test_sampler_follows_the_torch_path_without_resampling(ctx, tmp_path):
    B = 4
    noise = _sampler_noise(B)
    a, _, attrs_a = ctx['run'](ctx['torch'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    b, _, attrs_b = ctx['run'](ctx['fused'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    rms, d = float(np.sqrt((a ** 2).mean())), float(np.abs(a - b).max())
    start, end = Fd.reference(ctx['free'], ctx['ref'], ctx['bounds'], 1.0), Fd.reference(torch.from_numpy(b).float(), ctx['ref'], ctx['bounds'], 1.0)
    print('TM to the references: unguided %s, guided %s' % (start['tm'].numpy().round(3).tolist(), end['tm'].numpy().round(3).tolist()))
    print('guidance moved the designs by %.3e of their RMS; ill-posed at the end: %s' % (float(np.abs(b - ctx['free'].numpy()).max()) / rms, Fd.left_out(end).tolist()))
    print('no resampling: max |d| = %.3e, coordinate RMS = %.2f, ratio %.3e' % (d, rms, d / rms))
    assert float((start['below'] > 0).sum()) > 0 and float((start['above'] > 0).sum()) > 0      # both hinges pull on what the model makes
    assert float(np.abs(b - ctx['free'].numpy()).max()) > 1e-2 * rms                             # ... and the guidance is felt
    assert np.isfinite(b).all() and d <= 1e-3 * rms
    assert attrs_a['last_shape'] is None                                 # a plain callable
    report = attrs_b['last_shape']
    assert tuple(report) == Fd.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    again = ctx['fused'].describe(torch.from_numpy(b).float().cuda())
    assert all(torch.equal(report[k], again[k].cpu()) for k in report)
    assert attrs_b['last_fit'] is None and attrs_b['last_secstruct'] is None and attrs_b['last_pairs'] is None


def test_sum_of_shape_and_fold_is_bitwise_the_sum(ctx):
    import _shape as Sh
    from genie2_amd.smc import ShapePotential, SumPotential
    shape = ShapePotential(N_S, ctx['abar'], rog_max=6.0, clash_distance=4.0, device='cuda')
    both = SumPotential(shape, ctx['fused'])
    x = Fd.designs(6, N_S, 9).cuda()
    assert torch.equal(both(x, 5), shape(x, 5) + ctx['fused'](x, 5))      # bitwise the sum of its members
    xg = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(both(xg, 5).sum(), xg)
    parts = [torch.autograd.grad(m(xg, 5).sum(), xg)[0] for m in (shape, ctx['fused'])]
    assert torch.equal(g, parts[0] + parts[1]) and float(parts[1].abs().max()) > 0
    report = both.describe(x)
    assert tuple(report) == Sh.REPORT + Fd.REPORT                         # member order
    for m in (shape, ctx['fused']):
        assert all(torch.equal(report[k], v) for k, v in m.describe(x).items())


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('fold_cli') / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return root


def _cli_args(checkpoint_root, out, extra):
    return ['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out, '--min_length', '100',
            '--max_length', '100', '--batch_size', '2', '--num_samples', '2', '--num_steps', '4', '--last_unguided_steps', '0',
            '--guidance_alpha', '0.05'] + extra


def _check_fold_files(out, names, refs, seen=None):
    """Every outdir/fold file: its `ref` lines name `refs` [(name, lo, hi)] in order and agree with the float64 oracle on the written
    PDB -- the file rounds to three decimals (5e-4) and the PDB rounds coordinates to 1e-3 A, which moves a TM-score by at most
    5e-4 sqrt(3) |d tm / d x|_1 <= 5e-4 sqrt(3) 2 / d0 (each g_n has slope at most 0.65 / d0 < 2 / d0 in d_n, averaged over N), plus the
    float32 bar -- and, where the sampler's own tensors were caught (`seen`), with tm_of / describe on last_positions."""
    from genie2_amd.similarity import load_designs, tm_d0
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == sorted(n + '.pdb' for n in names)
    assert sorted(os.listdir(os.path.join(out, 'fold'))) == sorted(n + '.txt' for n in names)
    for i, name in enumerate(names):
        lines = [ln.split() for ln in open(os.path.join(out, 'fold', name + '.txt'))]
        R = len(refs)
        assert [f[0] for f in lines[:R]] == ['ref'] * R and [f[1] for f in lines[:R]] == [r[0] for r in refs]
        assert [(float(f[3]), float(f[4])) for f in lines[:R]] == [(r[1], r[2]) for r in refs]
        assert [f[0] for f in lines[R:]] == list(Fd.REPORT) and all(len(f) == 2 for f in lines[R:])
        assert all(('.' in f[1]) == (f[0] not in Fd.COUNTS) for f in lines[R:])
        got = {f[0]: float(f[1]) for f in lines[R:]}
        x = load_designs([os.path.join(out, 'pdbs', name + '.pdb')])[0]
        y = torch.stack([r[3] for r in refs])
        r64 = Fd.reference(x, y, torch.tensor([[r[1], r[2], 1.0] for r in refs]), 1.0)
        tol = 5e-4 + 5e-4 * math.sqrt(3) * 2 / tm_d0(x.shape[1]) + 1e-5
        for k in range(R):
            assert abs(float(lines[k][2]) - float(r64['tm'][0, k])) <= tol, (name, k, lines[k], r64['tm'])
        assert abs(got['tm_nearest'] - float(r64['tm_nearest'])) <= tol and abs(got['tm_lowest_wanted'] - float(r64['tm_lowest_wanted'])) <= tol
        top = torch.sort(r64['tm'][0], descending=True).values
        if R == 1 or float(top[0] - top[1]) > 2 * tol:
            assert got['nearest'] == int(r64['nearest'])
        # e_fold = sum of squared hinges on n_r = N tm_r: a TM-score off by t moves it by at most 2 hinge N t (+ N^2 t^2)
        N, hinge = x.shape[1], (r64['below'] + r64['above'])[0]
        t = tol - 5e-4
        tol_e = 5e-4 + float((2 * hinge * N * t + (N * t) ** 2).sum()) + 1e-5 * max(1.0, float(r64['e_fold']))
        assert abs(got['e_fold'] - float(r64['e_fold'])) <= tol_e, (name, got, r64['e_fold'], tol_e)
        if float(torch.minimum((r64['n'][0] - N * r64['tm'].new_tensor([r[1] for r in refs])).abs(),
                               (r64['n'][0] - N * r64['tm'].new_tensor([min(r[2], 1e9) for r in refs])).abs()).min()) > N * t:
            assert got['n_fold_violations'] == int(r64['n_fold_violations'])
        if seen is not None:
            pos, report, pot = seen
            tm = pot.tm_of(pos.cuda()).cpu()
            again = pot.describe(pos.cuda())
            assert all(abs(float(lines[k][2]) - float(tm[i, k])) <= 5e-4 + 1e-6 for k in range(R))
            for f in lines[R:]:
                assert torch.equal(report[f[0]][i], again[f[0]][i].cpu())
                assert abs(float(f[1]) - float(report[f[0]][i])) <= 5e-4 + 1e-5 * max(1.0, abs(float(report[f[0]][i]))), (name, f)


def test_both_clis_with_a_template_and_then_an_avoid_dir(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_motif import MotifRunner
    from genie2_amd.sample_unconditional_motif import build_parser as motif_parser
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    from genie2_amd.similarity import load_designs
    from genie2_amd.smc import FoldPotential, TwistedSampler
    template = ('dataset_100_0', 0.6, math.inf, load_designs([TEMPLATE])[0][0])
    first = str(tmp_path / 'first')
    args = build_parser().parse_args(_cli_args(checkpoint_root, first, ['--template_pdb', TEMPLATE, '--write_fold']))
    seen = []
    finish = TwistedSampler._finish

    def spy(self, st, trans, feats, start):                              # the sampler's own last_positions and report, as the CLI had them
        res = finish(self, st, trans, feats, start)
        seen.append((self.last_positions.clone(), {k: v.clone() for k, v in self.last_shape.items()}, st.twist))
        return res

    TwistedSampler._finish = spy
    try:
        torch.manual_seed(0)
        ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    finally:
        TwistedSampler._finish = finish
    assert len(seen) == 1 and isinstance(seen[0][2], FoldPotential) and tuple(seen[0][1]) == Fd.REPORT
    _check_fold_files(first, ['100_0', '100_1'], [template], seen[0])
    assert not any(os.path.exists(os.path.join(first, d)) for d in ('shape', 'binder', 'symmetry'))

    # the motif CLI, away from what the first run wrote and towards the template
    second = str(tmp_path / 'second')
    args = motif_parser().parse_args(_cli_args(checkpoint_root, second, ['--motif_file', MOTIF, '--template_pdb', TEMPLATE, '--avoid_dir', first,
                                                                          '--avoid_tm_max', '0.4', '--write_fold']))
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    avoided = [(n, 0.0, 0.4, load_designs([os.path.join(first, 'pdbs', n + '.pdb')])[0][0]) for n in ('100_0', '100_1')]
    _check_fold_files(second, ['100_0', '100_1'], [template] + avoided)


def test_run_without_fold_flags_writes_no_fold_files(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(_cli_args(checkpoint_root, out, ['--rog_max', '12']))
    torch.manual_seed(0)
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    assert len(os.listdir(os.path.join(out, 'pdbs'))) == 2 and not os.path.exists(os.path.join(out, 'fold'))
