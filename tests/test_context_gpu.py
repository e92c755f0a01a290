"""The context potential on the GPU (genie_context_potential, csrc/context_kernels.hip; ContextPotential in genie2_amd/smc.py) against
the float64 oracle of tests/_context.py, in its motif mode against its fixed mode, in TwistedSampler against the float32 PyTorch
restatement as its twisting function, summed with the motif potential, and through the motif command line.

Bounds (tests/_motif.py:60-72, the project's bars for a fused potential, used as in test_binder_gpu.py): logp within 1e-5
max(1, |logp|); every particle's gradient within 1e-5 of its largest float64 entry; every energy, `context_contacts`, distance,
`anchor_rmsd` and entry of the pose inside the logp bar, 1e-5 max(1, |value|); each widened, per case, to 4 x the error the float32
restatement makes on the same input where that is larger (the kernel is held to float32 arithmetic; the factor covers another
summation order); counts exactly.  Inputs are those of tests/_context.py, chosen by the oracle alone: on each the float64 side asserts
that no pair is within 1e-4 A of a threshold, that every enabled term has positive energy on some particle, that every particle's fit
has a relative eigenvalue gap of at least 0.1, and that on some particle an anchor carries at least 1e-2 of the largest gradient
entry, so a kernel without the part through the rotation fails outright.

Worst error / unwidened bound over the parity cases, measured on an MI355X: 0.18 for logp and 0.16 for the gradient (both at
(3, 63, 7, 65)), 0.04 for `context_contacts`, 0.17 for `context_min_distance`, 0.08 for `anchor_rmsd`, 0.09 / 0.18 for the clash and
contact energies, 0.03 for the rotation and 0.24 for the translation of the pose ((2, 129, 21, 257)); 0.05 for the gradient at
C = 5500.  The restatement widened some bars (by up to 4.2, the gradient at C = 5500; 13.8 for the upper-hinge configuration, whose
energy is a small difference of large counts), none of which the kernel needed; every count was equal (DESIGN.md 7.15 has the table
per case)."""
import math
import os

import numpy as np
import pytest
import torch

import _context as Cx
from _motif import MOTIF, _abar, _pot, _tiny_model, segments_6e6r, walk
from _parity import hard_time_limit

pytestmark = pytest.mark.gpu

STEP = 500
_cache = {}


@pytest.fixture(autouse=True)
def _limit():
    with hard_time_limit(300):
        yield


def _inputs(case):
    """(x, idx, t, y, cfg) of a parity case, made once."""
    if case not in _cache:
        _cache[case] = Cx.inputs(case)
    return _cache[case]


def _reference(x, idx, t, y, cfg, var, grad=True):
    """The oracle and the float32 restatement of an input, computed once."""
    key = ('ref', x.data_ptr(), idx.data_ptr(), t.data_ptr(), y.data_ptr(), repr(sorted(cfg.items())), var, grad)
    if key not in _cache:
        _cache[key] = (x, idx, t, y, Cx.reference(x, idx, t, y, cfg, var, grad), Cx.restatement32(x, idx, t, y, cfg, var, grad))
    return _cache[key][4:]


def _run(pot, x, step=STEP):
    x = x.cuda().requires_grad_(True)
    lp = pot(x, step)
    g, = torch.autograd.grad(lp.sum(), x)
    return lp.detach(), g


def _widen(err, bound):
    """The factor a bar is widened by: 4 x the float32 restatement's error / bound where that is above 1."""
    return max(1.0, 4.0 * float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max()))


def _ratio(d, b):
    return float(torch.where(b > 0, d / b.clamp(min=1e-300), torch.where(d > 0, math.inf, 0.0).double()).max())


def _check(what, lp, g, ref, r32, gradient=True):
    lp, g = lp.double().cpu(), g.double().cpu()
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), what
    lp_b = 1e-5 * ref['logp'].abs().clamp(min=1.0)
    wide = _widen((r32['logp'].double().cpu() - ref['logp']).abs(), lp_b)
    d_lp = (lp - ref['logp']).abs()
    print('%s: logp error / bound %.3f (bar widened x%.2f)' % (what, _ratio(d_lp, lp_b * wide), wide))
    assert bool((d_lp <= lp_b * wide).all()), (what, lp, ref['logp'])
    if gradient:
        g_b = 1e-5 * ref['grad'].abs().amax(dim=(1, 2))
        wide = _widen((r32['grad'].double().cpu() - ref['grad']).abs().amax(dim=(1, 2)), g_b)
        d_g = (g - ref['grad']).abs().amax(dim=(1, 2))
        print('%s: gradient error / bound %.3f (bar widened x%.2f)' % (what, _ratio(d_g, g_b * wide), wide))
        assert bool((d_g <= g_b * wide).all()), (what, d_g, g_b)


def _check_value(what, k, v, r, r32):
    """A float field against the oracle's inside the logp bar, widened by the restatement's own error."""
    v, r = v.double().cpu(), r.double()
    bound = 1e-5 * r.abs().clamp(min=1.0)
    wide = _widen((r32.double().cpu() - r).abs().reshape(-1), bound.reshape(-1))
    print('%s: %s error / bound %.3f (bar widened x%.2f)' % (what, k, _ratio((v - r).abs().reshape(-1), bound.reshape(-1) * wide), wide))
    assert tuple(v.shape) == tuple(r.shape) and bool(torch.isfinite(v).all()) and bool(((v - r).abs() <= bound * wide).all()), (what, k, v, r)


def _check_report(what, pot, x, ref, r32):
    got = pot.describe(x.cuda())
    assert tuple(got) == Cx.REPORT
    for k in Cx.REPORT:
        assert tuple(got[k].shape) == tuple(ref[k].shape) and got[k].device.type == 'cuda', k
        if k in Cx.COUNTS:
            assert got[k].dtype == torch.int64 and torch.equal(got[k].cpu(), ref[k]), (what, k, got[k], ref[k])
            continue
        assert got[k].dtype == torch.float32
        _check_value(what, k, got[k], ref[k], r32[k])
    R, trans = pot.pose_of(x.cuda())
    assert R.dtype == torch.float32 and R.device.type == 'cuda' and tuple(R.shape) == (x.shape[0], 3, 3) and tuple(trans.shape) == (x.shape[0], 3)
    _check_value(what, 'pose R', R, ref['R'], r32['R'])
    _check_value(what, 'pose t', trans, ref['trans'], r32['trans'])
    placed = pot.placed_context(x.cuda())
    assert tuple(placed.shape) == tuple(ref['placed'].shape)
    # R y + t from a pose inside its bars: 1e-5 (|y|_1 + max(1, |t|)) per coordinate, widened as the pose's bars are
    wide = max(_widen((r32[k].double().cpu() - ref[k]).abs().reshape(-1), (1e-5 * ref[k].abs().clamp(min=1.0)).reshape(-1)) for k in ('R', 'trans'))
    bound = 1e-5 * wide * (pot.context.double().cpu().abs().sum(dim=1)[None, :, None] + ref['trans'].abs().clamp(min=1.0)[:, None, :])
    assert bool(((placed.double().cpu() - ref['placed']).abs() <= bound).all()), what


def _parity(what, x, idx, t, y, cfg, gradient=True, report=True):
    pot = Cx.potential(cfg, x.shape[1], idx, t, y, _abar())
    ref, r32 = _reference(x, idx, t, y, cfg, float(pot.variance(STEP)), gradient)
    lp, g = _run(pot, x)
    _check(what, lp, g, ref, r32, gradient)
    if report:
        _check_report(what, pot, x, ref, r32)
    return pot, ref, lp, g


@pytest.mark.parametrize('case', Cx.CASES, ids=Cx.case_id)
def test_potential_report_and_pose_match_the_float64_oracle(case):
    x, idx, t, y, cfg = _inputs(case)
    _, ref, _, g = _parity(Cx.case_id(case), x, idx, t, y, cfg)
    assert bool((ref['logp'] < 0).all()) and float(torch.gather(g.abs().amax(dim=2), 1, idx.cuda()).max()) > 0


def test_context_whose_staging_needs_more_than_64_kib_of_lds():
    """C = 5500: 12 C = 66 000 bytes of staging, above the 65 536 a kernel gets without asking (the entry raises the kernel's limit).
    One particle, the same bars, and two calls bitwise equal."""
    x, idx, t, y, cfg = _inputs(Cx.LDS_CASE)
    pot, ref, lp, g = _parity(Cx.case_id(Cx.LDS_CASE), x, idx, t, y, cfg)
    assert all(float(ref[k]) > 0 for k in ('e_context_clash', 'e_context_contact'))
    again = _run(pot, x)
    assert torch.equal(lp, again[0]) and torch.equal(g, again[1])


@pytest.mark.parametrize('term', ['clash', 'contacts'])
def test_each_term_alone(term):
    x, idx, t, y, cfg = _inputs(Cx.CASES[4])
    one = Cx.only(cfg, term)
    Cx.check_inputs(x, idx, t, y, one)
    _, ref, _, g = _parity('%s alone' % term, x, idx, t, y, one)
    other = 'e_context_contact' if term == 'clash' else 'e_context_clash'
    assert bool((ref[other] == 0).all()) and float(g.abs().max()) > 0


def test_contacts_max_infinite_and_the_weights():
    x, idx, t, y, cfg = _inputs(Cx.CASES[3])
    low = dict(cfg, contacts_min=0.0, contacts_max=0.5 * cfg['contacts_min'] / 1.5)      # half particle 0's own count: an upper hinge
    _, ref, _, _ = _parity('an upper hinge', x, idx, t, y, low)
    assert float(ref['e_context_contact'][0]) > 0
    _parity('contacts_max = inf', x, idx, t, y, dict(cfg, contacts_max=math.inf))
    _, ref, _, _ = _parity('contacts in 0..inf', x, idx, t, y, dict(cfg, contacts_min=0.0, contacts_max=math.inf))
    assert bool((ref['e_context_contact'] == 0).all())
    # the weights multiply as stated
    pot, ref, _, _ = _parity('weights 2.5, 0.125', x, idx, t, y, dict(cfg, clash_weight=2.5, contacts_weight=0.125))
    base = Cx.potential(cfg, x.shape[1], idx, t, y, _abar()).describe(x.cuda())
    got = pot.describe(x.cuda())
    for k, w in (('e_context_clash', 2.5), ('e_context_contact', 0.125)):
        assert torch.allclose(got[k], w * base[k], rtol=1e-6, atol=0), k
    assert all(torch.equal(got[k], base[k]) for k in Cx.REPORT if not k.startswith('e_'))
    # a weight of 0 switches a term off, energy and force: both off is logp 0 and a gradient of exactly 0, anchors included
    off = Cx.potential(dict(cfg, clash_weight=0.0, contacts_weight=0.0), x.shape[1], idx, t, y, _abar())
    lp, g = _run(off, x)
    assert bool((lp == 0).all()) and bool((g == 0).all())


def test_deterministic_and_never_synchronises():
    x, idx, t, y, cfg = _inputs(Cx.CASES[5])
    pot = Cx.potential(cfg, x.shape[1], idx, t, y, _abar())
    xc = x.cuda()
    a, b = _run(pot, xc, 400), _run(pot, xc, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ra, rb = pot.describe(xc), pot.describe(xc)
    assert all(torch.equal(ra[k], rb[k]) for k in ra)
    pa = pot.pose_of(xc)
    assert all(torch.equal(u, v) for u, v in zip(pa, pot.pose_of(xc)))
    xg = xc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(xg, 400)
        g, = torch.autograd.grad(lp.mean(), xg)
        rep = pot.describe(xc)
        pose = pot.pose_of(xc)
        placed = pot.placed_context(xc)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.allclose(g, a[1] / 2, rtol=1e-6, atol=0)      # (the backward scales by grad_output = 1/2)
    assert all(torch.equal(rep[k], ra[k]) for k in ra) and all(torch.equal(u, v) for u, v in zip(pose, pa))
    assert torch.equal(placed, torch.einsum('bij,cj->bci', pa[0], pot.context) + pa[1][:, None])
    with pytest.raises(ValueError):
        pot(xc[:, :128], 400)
    with pytest.raises(ValueError):
        pot(x, 400)                                                                       # (a CPU tensor)
    rows = Cx.potential(cfg, x.shape[1], idx[:1].expand(3, -1), t, y, _abar())            # three rows, two particles
    with pytest.raises(ValueError):
        rows(xc, 400)


def test_invariance_and_balance_of_the_gradient():
    """A rigid motion of x moves the context with it: logp stays inside the logp bar.  The gradient has no net force and no net
    torque: each entry errs by at most the gradient bar, the sums are over N entries, and a cross product multiplies by at most
    2 max|x|."""
    x, idx, t, y, cfg = _inputs(Cx.CASES[4])
    pot, ref, lp, g = _parity('invariance', x, idx, t, y, cfg, report=False)
    r32 = _reference(x, idx, t, y, cfg, float(pot.variance(STEP)))[1]
    Q = Cx.random_rotation(17)
    assert float(torch.linalg.det(Q)) == pytest.approx(1.0, abs=1e-12)
    moved = (x.double() @ Q.T + torch.tensor([13.0, -8.0, 21.0], dtype=torch.float64)).float()
    lp_m, _ = _run(pot, moved)
    lp_b = 1e-5 * ref['logp'].abs().clamp(min=1.0)
    wide = _widen((r32['logp'].double().cpu() - ref['logp']).abs(), lp_b)
    d = (lp_m.double().cpu() - ref['logp']).abs()                        # (the oracle is invariant to 1e-12: tests/test_context_host.py)
    print('moved: logp error / bound %.3f (bar widened x%.2f)' % (_ratio(d, lp_b * wide), wide))
    assert bool((d <= lp_b * wide).all())
    g, N = g.double().cpu(), x.shape[1]
    g_b = 1e-5 * ref['grad'].abs().amax(dim=(1, 2)) * _widen((r32['grad'].double().cpu() - ref['grad']).abs().amax(dim=(1, 2)),
                                                             1e-5 * ref['grad'].abs().amax(dim=(1, 2)))
    force, torque = g.sum(dim=1).abs().amax(dim=1), torch.cross(x.double(), g, dim=2).sum(dim=1).abs().amax(dim=1)
    print('net force / bound %.3f, net torque / bound %.3f' % (_ratio(force, N * g_b), _ratio(torque, 2 * N * float(x.abs().max()) * g_b)))
    assert bool((force <= N * g_b).all()) and bool((torque <= 2 * N * float(x.abs().max()) * g_b).all())


def test_degenerate_inputs_stay_finite():
    """All design residues at one point (the correlation is 0 and the fit has no unique rotation: the oracle has no value here), a
    design residue on a placed context atom (to float32 rounding: the pair's direction is rounding noise in either precision, so logp
    is the oracle's and the gradient finite), and a context 1e4 A from the motif, where every s underflows towards 0 and the hinge
    contacts_min is fully active.  Documented behaviour; nothing here is meant to fault."""
    x, idx, t, y, cfg = _inputs(Cx.CASES[2])
    pot = Cx.potential(cfg, x.shape[1], idx, t, y, _abar())
    point = x.clone()
    point[:] = x[0, 5]
    lp, g = _run(pot, point)
    rep = pot.describe(point.cuda())
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()) and all(bool(torch.isfinite(v.double()).all()) for v in rep.values())
    assert all(bool(torch.isfinite(v).all()) for v in pot.pose_of(point.cuda()))
    # a residue on a placed atom
    ref0 = Cx.reference(x, idx, t, y, cfg, 1.0, grad=False)
    on = x.clone()
    free = [n for n in range(x.shape[1]) if n not in idx[0].tolist()]
    on[0, free[7]] = ref0['placed'][0, 20].float()
    on[1, free[0]] = ref0['placed'][1, 64].float()
    assert Cx.margins(on, idx, t, y, cfg) >= 1e-4
    _, ref, lp, g = _parity('a residue on a placed atom', on, idx, t, y, cfg, gradient=False, report=False)
    assert float(ref['context_min_distance'][0]) < 1e-5 and float(pot.describe(on.cuda())['context_min_distance'][0]) < 1e-4
    assert bool(torch.isfinite(g).all())
    # the context far away
    far = y + torch.tensor([1e4, 0.0, 0.0])
    cfg_far = dict(cfg, contacts_min=50.0, contacts_max=100.0)
    pot, ref, lp, g = _parity('a context 1e4 A away', x, idx, t, far, cfg_far, gradient=False, report=False)
    want = -(50.0 ** 2) / (2 * float(pot.variance(STEP)))
    assert float(ref['context_contacts'].max()) < 1e-12 and torch.allclose(lp.double().cpu(), torch.full((3,), want, dtype=torch.float64), rtol=1e-6)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) < 1e-6
    rep = pot.describe(x.cuda())
    assert all(bool(torch.isfinite(v.double()).all()) for v in rep.values()) and bool((rep['n_context_contacts'] == 0).all())


# ---- motif mode ------------------------------------------------------------------------------------------------------------------

N_M = 60


def _motif_context(segs):
    """A context for the 6E6R motif: a walk of 40 atoms 12 A along x from the motif's centroid, in the motif file's frame."""
    return Cx.walk(40, 77) + torch.cat(segs).mean(dim=0) + torch.tensor([12.0, 0.0, 0.0])


def _anchor_rows(fit, seg_len, which):
    return torch.cat([fit['starts'][:, s:s + 1] + torch.arange(seg_len[s], device=fit['starts'].device)[None] for s in which], dim=1)


@pytest.mark.parametrize('align', ['translation', 'rigid'])
def test_motif_mode_equals_the_fixed_mode_on_the_located_placement(align):
    from genie2_amd.smc import ContextPotential
    segs, abar = segments_6e6r(), _abar()
    motif = _pot(segs, N_M, abar, align=align)
    y, t = _motif_context(segs), torch.cat(segs)
    kw = dict(clash_distance=6.0, contacts=(30.0, 60.0), device='cuda')
    x = walk(3, N_M, 21).cuda()
    fit = motif.locate(x)
    rows = _anchor_rows(fit, motif.seg_len, [0, 1])
    assert len(set(fit['best'].tolist())) > 1                            # the anchors differ between particles
    moving = ContextPotential(N_M, abar, t, y, motif=motif, **kw)
    fixed = ContextPotential(N_M, abar, t, y, anchor_index=rows.cpu(), **kw)
    a, b = _run(moving, x), _run(fixed, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[1].abs().max()) > 0
    ra, rb = moving.describe(x), fixed.describe(x)
    assert all(torch.equal(ra[k], rb[k]) for k in Cx.REPORT)
    assert all(torch.equal(u, v) for u, v in zip(moving.pose_of(x), fixed.pose_of(x)))
    d = (ra['anchor_rmsd'].double() - fit['rmsd'].double()).abs().cpu()
    bound = 1e-5 * fit['rmsd'].double().abs().clamp(min=1.0).cpu()
    print('anchor_rmsd against locate: error / bound %.3f' % _ratio(d, bound))
    assert bool((d <= bound).all()), (ra['anchor_rmsd'], fit['rmsd'])
    # and the fixed mode is the oracle's function of those rows
    cfg = Cx.config(clash_distance=6.0, clash_weight=1.0, contacts_min=30.0, contacts_max=60.0, contacts_weight=1.0)
    ref = Cx.reference(x.cpu(), rows.cpu(), t, y, cfg, float(moving.variance(STEP)))
    r32 = Cx.restatement32(x.cpu(), rows.cpu(), t, y, cfg, float(moving.variance(STEP)))
    _check('motif mode (%s)' % align, a[0], a[1], ref, r32)
    # no host read on the way: the placement search, the gather of the anchors and the entry
    xg = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = moving(xg, STEP)
        g, = torch.autograd.grad(lp.sum(), xg)
        rep = moving.describe(x)
        pose = moving.pose_of(x)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.equal(g, a[1]) and all(torch.equal(rep[k], ra[k]) for k in ra)
    assert all(torch.equal(u, v) for u, v in zip(pose, fixed.pose_of(x)))


def test_motif_groups_tie_the_context_to_one_group():
    from genie2_amd.smc import ContextPotential
    segs, abar = segments_6e6r(), _abar()
    motif = _pot(segs, N_M, abar, align='rigid', groups=['A', 'B'])
    y = _motif_context(segs)
    kw = dict(clash_distance=6.0, contacts=(30.0, 60.0), device='cuda')
    x = walk(3, N_M, 21).cuda()
    fit = motif.locate(x)
    for g, label in enumerate(fit['groups']):
        moving = ContextPotential(N_M, abar, segs[g], y, motif=motif, segments=[g], **kw)
        fixed = ContextPotential(N_M, abar, segs[g], y, anchor_index=_anchor_rows(fit, motif.seg_len, [g]).cpu(), **kw)
        a, b = _run(moving, x), _run(fixed, x)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), label
        d = (moving.describe(x)['anchor_rmsd'].double() - fit['group_rmsd'][:, g].double()).abs().cpu()
        assert bool((d <= 1e-5 * fit['group_rmsd'][:, g].double().abs().clamp(min=1.0).cpu()).all()), label
    for segments, anchors in ((None, torch.cat(segs)), ([0, 1], torch.cat(segs)), ([1], segs[0]), ([2], segs[0]), ([], segs[0])):
        with pytest.raises(ValueError):
            ContextPotential(N_M, abar, anchors, y, motif=motif, segments=segments, **kw)
    with pytest.raises(ValueError):
        ContextPotential(N_M + 1, abar, segs[0], y, motif=motif, segments=[0], **kw)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N_S = 12, 40


def _sampler_context():
    """Nine anchors in three runs of a 40-residue design, the motif a walk's residues at those places, and a 30-atom context 12 A from
    the motif's centroid along x."""
    idx = torch.tensor(Cx.anchor_runs(N_S, 9))
    t = Cx.walk(N_S, 31)[idx]
    y = Cx.walk(30, 7030) + t.mean(dim=0) + torch.tensor([12.0, 0.0, 0.0])
    return idx, t, y, Cx.config(clash_distance=4.0, clash_weight=1.0, contacts_min=40.0, contacts_max=80.0, contacts_weight=1.0)


@pytest.fixture(scope='module')
def ctx(base_weights):
    from genie2_amd import pack
    from genie2_amd.smc import TwistedSampler
    model = _tiny_model(base_weights, T)
    abar = pack.schedule_tensors(T)['alphas_cumprod'].cuda()
    sampler = TwistedSampler(model)

    def run(twist, noise, outdir, **extra):
        out = sampler._sample(dict({'length': N_S, 'scale': 0.6, 'outdir': str(outdir), 'prefix': 'x', 'offset': 0, 'noise': noise,
                                    'last_unguided_steps': 0, 'guidance_alpha': 0.05, 'twisting_function': twist}, **extra))
        attrs = {k: getattr(sampler, k, None) for k in ('last_fit', 'last_shape', 'last_positions')}
        return np.stack([r['atom_positions'] for r in out]), out, attrs

    idx, t, y, cfg = _sampler_context()
    return dict(run=run, abar=abar, fused=Cx.potential(cfg, N_S, idx, t, y, abar), torch=Cx.twisting_function(idx, t.cuda(), y.cuda(), cfg, abar))


def test_sampler_follows_the_torch_path_without_resampling(ctx, tmp_path):
    B = 4
    noise = torch.randn(T, B, N_S, 3, generator=torch.Generator().manual_seed(4))
    a, _, attrs_a = ctx['run'](ctx['torch'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    b, _, attrs_b = ctx['run'](ctx['fused'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    rms, d = float(np.sqrt((a ** 2).mean())), float(np.abs(a - b).max())
    print('no resampling: max |d| = %.3e, coordinate RMS = %.2f, ratio %.3e' % (d, rms, d / rms))
    assert np.isfinite(b).all() and d <= 1e-3 * rms
    assert attrs_a['last_shape'] is None                                 # a plain callable
    report = attrs_b['last_shape']
    assert tuple(report) == Cx.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    again = ctx['fused'].describe(torch.from_numpy(b).float().cuda())
    assert all(torch.equal(report[k], again[k].cpu()) for k in report)
    assert attrs_b['last_fit'] is None


def test_sum_of_motif_and_context_is_the_sum_of_its_members():
    from genie2_amd.smc import ContextPotential, SumPotential
    segs, abar = segments_6e6r(), _abar()
    motif = _pot(segs, N_M, abar, align='rigid')
    context = ContextPotential(N_M, abar, torch.cat(segs), _motif_context(segs), motif=motif, clash_distance=6.0, contacts=(30.0, 60.0), device='cuda')
    both = SumPotential(motif, context)
    x = walk(4, N_M, 9).cuda()
    assert torch.equal(both(x, 5), motif(x, 5) + context(x, 5))          # bitwise the sum of its members
    xg = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(both(xg, 5).sum(), xg)
    parts = [torch.autograd.grad(m(xg, 5).sum(), xg)[0] for m in (motif, context)]
    assert torch.equal(g, parts[0] + parts[1])
    assert tuple(both.describe(x)) == Cx.REPORT and both.has_fit and torch.equal(both.locate(x)['best'], motif.locate(x)['best'])
    from genie2_amd.smc import ShapePotential
    import _shape as Sh
    three = SumPotential(motif, ShapePotential(N_M, abar, rog_max=9.0, device='cuda'), context)
    assert tuple(three.describe(x)) == Sh.REPORT + Cx.REPORT             # member order


# ---- the command line ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('context_cli') / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return root


def _context_file(tmp_path):
    """A context of two chains (20 and 10 residues) in the motif file's frame, 12 A along x from the motif's centroid."""
    segs = segments_6e6r()
    y = (Cx.walk(30, 7030) + torch.cat(segs).mean(dim=0) + torch.tensor([12.0, 0.0, 0.0])).double()
    path = str(tmp_path / 'context.pdb')
    Cx.write_context_pdb(path, y, [20, 10])
    return path


def _check_context_files(out, names, context_pdb, which=(0, 1)):
    """Every outdir/context file against the float64 oracle on the complex its PDB holds.  The complex file rounds coordinates to
    1e-3 A (at most 5e-4 per coordinate) and is centred as a whole, which the refit follows; the report rounds to three decimals
    (5e-4).  The written context must be where refitting the motif file's anchors onto the located placement of the written design
    puts it: a coordinate c of the placed context may differ by its own rounding 5e-4, by 5e-4 |dc/dx|_1 for the rounding of the
    design it is refitted on, and by the float32 bar of a pose, 1e-5 (|y|_1 + max(1, |c|)).  A report field f may differ from the
    oracle's on the written design by 5e-4 + 5e-4 |df/dx|_1 plus the float32 bar 1e-5 max(1, |f|).  Counts are compared where no pair
    of the written complex is within 2e-3 A of a threshold."""
    from genie2_amd.features import parse_pdb
    from genie2_amd.smc import load_target
    for d, ext in (('pdbs', '.pdb'), ('context', '.txt'), ('context_complex', '.pdb'), ('motif_locations', '.txt')):
        assert sorted(os.listdir(os.path.join(out, d))) == sorted(n + ext for n in names), d
    segs = segments_6e6r()
    t = torch.cat([segs[s] for s in which]).double()
    y = load_target(context_pdb)[0]
    cfg = Cx.config(clash_distance=6.0, clash_weight=1.0, contacts_min=30.0, contacts_max=60.0, contacts_weight=1.0)
    for name in names:
        path = os.path.join(out, 'context_complex', name + '.pdb')
        pdb = [ln for ln in open(path) if ln.startswith('ATOM')]
        assert [ln[21] for ln in pdb] == ['A'] * 20 + ['B'] * 10 + ['C'] * N_M           # the context's chains, then the design
        _, chains = parse_pdb(path)
        placed = torch.tensor(np.concatenate(chains[:2]), dtype=torch.float64)
        x = torch.tensor(chains[2], dtype=torch.float64)[None].requires_grad_(True)
        assert float((torch.cdist(placed, placed) - torch.cdist(y, y)).abs().max()) <= 2 * 5e-4 * math.sqrt(3) + 1e-5 * float(y.abs().sum(dim=1).max())
        lines = [ln.split() for ln in open(os.path.join(out, 'motif_locations', name + '.txt')) if not ln.startswith('#')]
        idx = torch.tensor([[i for s in which for i in range(int(lines[s][0]), int(lines[s][1]) + 1)]])
        r = Cx.terms(x, idx, t, y, cfg)
        for c in range(len(y)):
            for k in range(3):
                slope = float(torch.autograd.grad(r['placed'][0, c, k], x, retain_graph=True)[0].abs().sum())
                value = float(r['placed'][0, c, k].detach())
                tol = 5e-4 + 5e-4 * slope + 1e-5 * (float(y[c].abs().sum()) + max(1.0, abs(value)))
                assert abs(float(placed[c, k]) - value) <= tol, (name, c, k, float(placed[c, k]), value, tol)
        lines = [ln.split() for ln in open(os.path.join(out, 'context', name + '.txt'))]
        assert [f[0] for f in lines] == list(Cx.REPORT) and all(len(f) == 2 for f in lines)
        assert all(('.' in f[1]) == (f[0] not in Cx.COUNTS) for f in lines)
        got = {f[0]: float(f[1]) for f in lines}
        for k in Cx.REPORT:
            if k in Cx.COUNTS:
                continue
            gx, = torch.autograd.grad(r[k][0], x, retain_graph=True, allow_unused=True)
            slope = float(gx.abs().sum()) if gx is not None else 0.0
            ref = float(r[k][0].detach())
            tol = 5e-4 + 5e-4 * slope + 1e-5 * max(1.0, abs(ref))
            assert abs(got[k] - ref) <= tol, (name, k, got[k], ref, tol)
        if Cx.margins(x.detach(), idx, t, y, cfg) >= 2e-3:
            assert all(got[k] == int(r[k][0]) for k in Cx.COUNTS), (name, got)


CLI = ['--name', 'base', '--epoch', '7', '--scale', '0.6', '--motif_file', MOTIF, '--min_length', str(N_M), '--max_length', str(N_M), '--batch_size', '2',
       '--num_samples', '2', '--num_steps', '4', '--last_unguided_steps', '0']
CONTEXT_FLAGS = ['--context_clash_distance', '6', '--context_contacts_min', '30', '--context_contacts_max', '60', '--write_context',
                 '--write_context_complex', '--write_motif_locations']


@pytest.mark.parametrize('extra, which', [([], (0, 1)), (['--align', 'rigid', '--motif_groups', 'file', '--context_group', 'B'], (1,))],
                         ids=['joint', 'group-B'])
def test_motif_cli_with_a_context_end_to_end(tmp_path, checkpoint_root, extra, which):
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    from genie2_amd.smc import ContextPotential, MotifPotential, SumPotential, TwistedSampler
    out, context_pdb = str(tmp_path / 'out'), _context_file(tmp_path)
    args = build_parser().parse_args(CLI + ['--rootdir', checkpoint_root, '--outdir', out, '--context_pdb', context_pdb] + CONTEXT_FLAGS + extra)
    seen = []
    finish = TwistedSampler._finish

    def spy(self, st, trans, feats, start):                              # the potential the CLI guided with
        seen.append(st.twist)
        return finish(self, st, trans, feats, start)

    TwistedSampler._finish = spy
    try:
        np.random.seed(0)
        torch.manual_seed(0)
        MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    finally:
        TwistedSampler._finish = finish
    assert len(seen) == 1 and isinstance(seen[0], SumPotential)
    motif, context = seen[0].potentials
    assert isinstance(motif, MotifPotential) and isinstance(context, ContextPotential) and context.motif is motif
    assert context.segments == list(which) and context.A == sum(motif.seg_len[s] for s in which) and context.C == 30
    _check_context_files(out, ['%d_0' % N_M, '%d_1' % N_M], context_pdb, which)


def test_run_without_context_flags_writes_no_context_files(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    from genie2_amd.smc import MotifPotential, TwistedSampler
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(CLI + ['--rootdir', checkpoint_root, '--outdir', out])
    seen = []
    finish = TwistedSampler._finish

    def spy(self, st, trans, feats, start):
        seen.append(st.twist)
        return finish(self, st, trans, feats, start)

    TwistedSampler._finish = spy
    try:
        np.random.seed(0)
        torch.manual_seed(0)
        MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    finally:
        TwistedSampler._finish = finish
    assert len(seen) == 1 and isinstance(seen[0], MotifPotential)        # the motif potential alone, as before
    assert len(os.listdir(os.path.join(out, 'pdbs'))) == 2
    assert not any(os.path.exists(os.path.join(out, d)) for d in ('context', 'context_complex'))
