"""The aligned fold potential on the GPU (genie_fold_align_potential, csrc/fold_align_kernels.hip; AlignedFoldPotential in
genie2_amd/smc.py): a certificate of everything it returns against the float64 oracle of tests/_fold_align.py, its search against
similarity.TMAlign and, with a stride, against the oracle's, its score against FoldPotential's, its exactness, in TwistedSampler, summed
with the shape potential, and through the shape command line.

The certificate leaves no pair out for alignment reasons: the oracle takes the kernel's own `map`, `rot0` and `trans0` and runs the
polish, the energy, the report and the gradient from them.  Bars (DESIGN.md 7.9's): scalars within 1e-5 max(1, |value|); a particle's
gradient within 1e-5 of its largest float64 entry; each widened, per case, to 4 x the error the float32 restatement makes on the same
input where that is larger; counts, `nearest`, `n_aligned` and `map` exact.  A particle is left out only if the oracle finds a Horn
gap of the polish below 1e-4 on a pair with an active hinge; with these seeds none is, which is asserted.  DESIGN.md 7.11 has the
measured error / bound per case."""
import math
import os

import numpy as np
import pytest
import torch

import _fold as Fd
import _fold_align as Fa
import _similarity as S
import _tmalign as Ta
from _motif import _abar, _tiny_model
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
        _cache[case] = Fa.inputs(case)
    return _cache[case]


def _potential(refs, bounds, n_res, abar=None, **kw):
    from genie2_amd.smc import AlignedFoldPotential
    return AlignedFoldPotential(n_res, _abar() if abar is None else abar, refs, bounds, device='cuda', **kw)


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
    r = r.double().reshape(-1)
    bound = 1e-5 * r.abs().clamp(min=1.0)
    wide = _widen((r32 - r).abs(), bound)
    print('%s: %s error / bound %.3f (bar widened x%.2f)' % (what, name, _ratio((got - r).abs(), bound * wide), wide))
    assert bool(torch.isfinite(got).all()) and bool(((got - r).abs() <= bound * wide).all()), (what, name, got, r)
    return bound * wide


def _check_maps(what, amap, n_aligned, lengths):
    """Every map is strictly increasing over its non-negative entries, in range, -1 where unaligned; n_aligned is its count."""
    amap, n_aligned = amap.cpu().long(), n_aligned.cpu().long()
    assert int(amap.min()) >= -1 and torch.equal((amap >= 0).sum(dim=2), n_aligned), what
    for r, L in enumerate(lengths):
        assert int(amap[:, r].max()) < L, (what, r)
        for b in range(amap.shape[0]):
            hit = amap[b, r][amap[b, r] >= 0]
            assert bool((hit[1:] > hit[:-1]).all()), (what, b, r)


def _certificate(what, x, refs, bounds, pot=None, upper=True, **kw):
    """Everything the entry returns for x against the oracle started from the entry's own alignment; returns (pot, oracle, logp, grad,
    alignment)."""
    bounds = torch.as_tensor(bounds, dtype=torch.float64)
    B, N, R = x.shape[0], x.shape[1], len(refs)
    pot = _potential(refs, bounds, N, **kw) if pot is None else pot
    var, xc = float(pot.variance(STEP)), x.cuda()
    al = pot.alignment_of(xc)
    assert tuple(al) == ('tm', 'n_aligned', 'map', 'rot', 'trans', 'rot0', 'trans0')
    assert tuple(al['map'].shape) == (B, R, N) and al['map'].dtype == al['n_aligned'].dtype == torch.int32 and tuple(al['rot0'].shape) == (B, R, 3, 3)
    _check_maps(what, al['map'], al['n_aligned'], [len(y) for y in refs])
    held = (al['map'].cpu(), al['rot0'].cpu().double(), al['trans0'].cpu().double())
    r64 = Fa.evaluate(x, refs, bounds, var, *held, norm=pot.norm, n_iter=pot.n_iter, upper=upper)
    r32 = Fa.evaluate(x, refs, bounds, var, *held, norm=pot.norm, n_iter=pot.n_iter, dtype=torch.float32, upper=upper)
    out = Fa.left_out(r64)
    print('%s: %d of %d particles left out' % (what, int(out.sum()), B))
    assert not bool(out.any()), (what, out, r64['gap'])                 # change seeds, never thresholds
    lp, g = _run(pot, x)
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), what
    tm = pot.tm_of(xc)
    assert tuple(tm.shape) == (B, R) and tm.dtype == torch.float32 and tm.device.type == 'cuda' and torch.equal(tm, al['tm'])
    tm_bar = _value(what, 'tm_of', tm, r64['tm'], r32['tm']).reshape(B, R)
    _value(what, 'logp', lp, r64['logp'], r32['logp'])
    g_b = 1e-5 * r64['grad'].abs().amax(dim=(1, 2))
    wide = _widen((r32['grad'].double() - r64['grad']).abs().amax(dim=(1, 2)), g_b)
    d_g = (g.double().cpu() - r64['grad']).abs().amax(dim=(1, 2))
    print('%s: gradient error / bound %.3f (bar widened x%.2f)' % (what, _ratio(d_g, g_b * wide), wide))
    assert bool((d_g <= g_b * wide).all()), (what, d_g, g_b)
    active = (r64['k'] != 0)[:, :, None] & (held[0] >= 0)                 # an unaligned residue, an idle reference: exactly 0
    assert bool((g.cpu()[~active.any(dim=1)] == 0).all()), what
    _value(what, 'rot', al['rot'], r64['rot'], r32['rot'])
    _value(what, 'trans', al['trans'], r64['trans'], r32['trans'])
    assert float((torch.linalg.det(al['rot'].double().cpu()) - 1).abs().max()) <= 1e-5, what
    got = pot.describe(xc)
    assert tuple(got) == Fa.REPORT
    for k in Fa.REPORT:
        assert tuple(got[k].shape) == (B,) and got[k].device.type == 'cuda' and got[k].dtype == (torch.int64 if k in Fa.COUNTS else torch.float32), k
    _value(what, 'tm_nearest', got['tm_nearest'], r64['tm_nearest'], r32['tm_nearest'])
    _value(what, 'tm_lowest_wanted', got['tm_lowest_wanted'], r64['tm_lowest_wanted'], r32['tm_lowest_wanted'])
    _value(what, 'e_fold', got['e_fold'], r64['e_fold'], r32['e_fold'])
    # nearest: exact where the two best scores differ by more than the bar (one reference: always)
    top = torch.sort(r64['tm'], dim=1, descending=True).values
    sure = (top[:, 0] - top[:, 1] > 2 * tm_bar.amax(dim=1)) if R > 1 else torch.ones(B, dtype=torch.bool)
    assert torch.equal(got['nearest'].cpu()[sure], r64['nearest'][sure]), (what, got['nearest'], r64['nearest'])
    # violations: exact where no n_r is within 1e-4 Lnorm of a bound that can be active
    lo, hi = r64['lnorm'] * bounds[:, 0], r64['lnorm'] * bounds[:, 1]
    finite = torch.isfinite(hi) & torch.tensor(upper)
    n = r64['n'].double()
    near = (((n - lo).abs() < 1e-4 * r64['lnorm']) & (lo > 0)) | (((n - torch.where(finite, hi, torch.zeros_like(hi))).abs() < 1e-4 * r64['lnorm']) & finite)
    sure = ~near.any(dim=1)
    assert torch.equal(got['n_fold_violations'].cpu()[sure], r64['n_fold_violations'][sure]), (what, got['n_fold_violations'], r64['n_fold_violations'])
    return pot, r64, lp, g, al


@pytest.mark.parametrize('case', Fa.CASES, ids=Fa.case_id)
def test_certificate_against_the_float64_oracle(case):
    x, refs, bounds = _inputs(case)
    _, r64, _, _, _ = _certificate(Fa.case_id(case), x, refs, bounds)
    Fa.check_inputs(r64, len(refs))
    assert bool((r64['logp'] <= 0).all()) and float(r64['logp'].min()) < 0 and int(r64['n_fold_violations'].sum()) > 0


# ---- the search ----------------------------------------------------------------------------------------------------------------------

def _family_potential(N, **kw):
    xq, lq, xr, lr = Ta.family(N)
    assert all(v == N for v in lq)
    refs = [xr[k, :lr[k]] for k in range(len(lr))]
    return xq, lq, xr, lr, refs, _potential(refs, [Fd.AVOID] * len(refs), N, **kw)


def _search_is_tmaligns(N, norm):
    from genie2_amd.similarity import TMAlign
    key = ('family', N, norm)
    if key not in _cache:
        _cache[key] = Ta.all_pairs(*Ta.family(N), norm=norm)
    ref = _cache[key]
    xq, lq, xr, lr, refs, pot = _family_potential(N, norm=norm)
    al = pot.alignment_of(xq.cuda())
    want = TMAlign('cuda')(xq, lq, xr, lr, norm=norm, return_alignment=True)
    ok = Ta.well_posed(ref)
    print('N = %d, norm %s: %d of %d pairs ill-posed by the float64 oracle' % (N, norm, int((~ok).sum()), ok.numel()))
    assert int((~ok).sum()) <= 0.15 * ok.numel()
    assert torch.equal(al['map'].cpu()[ok], want['map'].cpu()[ok]) and torch.equal(al['n_aligned'].cpu()[ok], want['n_aligned'].cpu()[ok])
    assert torch.equal(al['map'].cpu()[ok].long(), ref['map'][ok]), (N, norm)
    bar = 1e-5 * want['tm'].abs().clamp(min=1.0)
    short = (want['tm'] - al['tm']) / bar
    print('N = %d, norm %s: tm_of below TMAlign by at most %.3f bars' % (N, norm, float(short.max())))
    assert bool((al['tm'] >= want['tm'] - bar).all()), (N, norm, short.max())
    _check_maps('family %d' % N, al['map'], al['n_aligned'], lr)


@pytest.mark.parametrize('N', Ta.TINY_N + Ta.INDEL_N)
def test_search_is_the_gapped_alignment(N):
    _search_is_tmaligns(N, 'query')


@pytest.mark.parametrize('norm', Ta.NORMS[1:])
def test_search_is_the_gapped_alignment_under_every_norm(norm):
    _search_is_tmaligns(48, norm)


def test_stride_visits_every_third_offset_and_always_the_last():
    xq, lq, xr, lr, refs, pot = _family_potential(48, offset_stride=3)
    ref = Fa.search_all(xq, refs, stride=3)
    ok = Ta.well_posed(ref)
    print('N = 48, stride 3: %d of %d pairs ill-posed by the float64 oracle' % (int((~ok).sum()), ok.numel()))
    assert int((~ok).sum()) <= 0.15 * ok.numel()
    al = pot.alignment_of(xq.cuda())
    assert torch.equal(al['map'].cpu()[ok].long(), ref['map'][ok]) and torch.equal(al['n_aligned'].cpu()[ok].long(), ref['n_aligned'][ok])
    # the 128 x 1024 pair: the true offset 500 is not a multiple of 3
    q, long = Ta.limit_pairs()[1]
    one = Fa.search(q, long, stride=3)
    assert min(one['gap'], one['margin'], one['path_margin'], one['stage_lead']) >= Ta.ILL
    al = _potential([long], [Fd.AVOID], 128, offset_stride=3).alignment_of(q[None].cuda())
    assert al['map'][0, 0].cpu().tolist() == one['map'] and int(al['n_aligned']) == one['n_aligned'] and float(al['tm']) > 0.9
    # a reference whose only good offset is the last one, under strides that do not divide it
    long = Ta.walk(1, 61, 8800)[0]
    tail = S.moved(long[-24:], 8801)
    for stride in (5, 64):
        al = _potential([long], [Fd.AVOID], 24, offset_stride=stride).alignment_of(tail[None].cuda())
        assert float(al['tm']) >= 0.999 and al['map'][0, 0].cpu().tolist() == list(range(37, 61)), stride


def test_without_rounds_the_polish_only_ascends_from_the_gapless_score():
    """References of the particles' own length, n_rounds = 0: the search is 7.9's seeded ascent at offset 0 and the polish starts from its
    winning seed, so tm_of is at least FoldPotential's."""
    from genie2_amd.smc import FoldPotential
    x, ref, bounds = Fd.inputs((3, 65, 5))
    gapless = FoldPotential(65, _abar(), ref, bounds, device='cuda').tm_of(x.cuda())
    tm = _potential(list(ref), bounds, 65, n_rounds=0).tm_of(x.cuda())
    print('n_rounds = 0 against FoldPotential: lowest difference %.3e' % float((tm - gapless).min()))
    assert bool((tm >= gapless - 1e-5).all()), (tm, gapless)


# ---- exactness and hygiene -----------------------------------------------------------------------------------------------------------

CASE = (3, 65, (63, 64, 65, 80))


def _everything(pot, xc, step=400):
    lp, g = _run(pot, xc, step)
    rep, al = pot.describe(xc), pot.alignment_of(xc)
    return [lp, g] + [rep[k] for k in Fa.REPORT] + [al[k] for k in ('tm', 'n_aligned', 'map', 'rot', 'trans', 'rot0', 'trans0')]


def test_deterministic_and_never_synchronises():
    x, refs, bounds = _inputs(CASE)
    pot, xc = _potential(refs, bounds, 65), x.cuda()
    a, b = _everything(pot, xc), _everything(pot, xc)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    xg = xc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(xg, 400)
        g, = torch.autograd.grad(lp.mean(), xg)
        rep, tm, al = pot.describe(xc), pot.tm_of(xc), pot.alignment_of(xc)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.allclose(g, a[1] / 3, rtol=1e-6, atol=0)      # (the backward scales by grad_output = 1/3)
    assert all(torch.equal(rep[k], v) for k, v in zip(Fa.REPORT, a[2:7])) and torch.equal(tm, a[7]) and torch.equal(al['map'], a[9])
    with pytest.raises(ValueError):
        pot(xc[:, :64], 400)                                                              # a wrong N
    with pytest.raises(ValueError):
        pot(x, 400)                                                                       # a CPU tensor
    with pytest.raises(ValueError):
        pot.tm_of(x)
    with pytest.raises(ValueError):
        pot.alignment_of(xc[:, :64])
    assert all(torch.equal(u, v) for u, v in zip(_everything(pot, xc), a))                # the refusals left the next call working


def test_padding_rows_never_reach_a_result():
    x, refs, bounds = _inputs(CASE)
    pot, xc = _potential(refs, bounds, 65), x.cuda()
    want = _everything(pot, xc)
    g = torch.Generator().manual_seed(5)
    padded = 1e3 * torch.randn(4, 96, 3, generator=g)
    padded[1, 70], padded[2, 90, 1], padded[0, 64, 0] = math.nan, math.inf, -math.inf
    for r, y in enumerate(refs):
        padded[r, :len(y)] = y
    again = _potential(padded, bounds, 65, lengths=[len(y) for y in refs])
    assert again.Nr == 80                                                                 # trimmed to the longest chain
    again.references = padded.cuda().contiguous()                                         # ... and here with the noise behind every chain
    again.Nr = 96
    assert all(torch.equal(u, v) for u, v in zip(_everything(again, xc), want))


def _with_weights(pot, weights):
    """`pot` with the weight column of its device table replaced (the constructor refuses a table of zeros: the entry does not)."""
    table = pot.bounds.clone()
    table[:, 2] = torch.tensor(weights, dtype=torch.float32, device=table.device)
    pot.bounds = table
    return pot


def test_weights_scale_their_reference_and_zero_weights_switch_off():
    x, refs, bounds = _inputs(CASE)
    xc, R = x.cuda(), len(refs)
    base = _potential(refs, bounds, 65)
    al = base.alignment_of(xc)
    rep = base.describe(xc)
    one_hot = lambda r, w: [w if k == r else 0.0 for k in range(R)]      # noqa: E731
    alone = {r: _with_weights(_potential(refs, bounds, 65), one_hot(r, 1.0)).describe(xc)['e_fold'] for r in range(R)}
    r0 = next(r for r in range(R) if float(alone[r].max()) > 0)         # a reference with an active hinge on some particle
    lp1, g1 = _run(_with_weights(_potential(refs, bounds, 65), one_hot(r0, 1.0)), x)
    scaled = _with_weights(_potential(refs, bounds, 65), one_hot(r0, 2.5))
    lp2, g2 = _run(scaled, x)
    assert float(g1.abs().max()) > 0 and torch.allclose(scaled.describe(xc)['e_fold'], 2.5 * alone[r0], rtol=1e-6, atol=0)
    assert torch.allclose(lp2, 2.5 * lp1, rtol=1e-6, atol=0) and torch.allclose(g2, 2.5 * g1, rtol=1e-5, atol=1e-6 * float(g1.abs().max()))
    # ... and leave every TM-score and map bitwise unchanged, and the others' energy
    mixed = _with_weights(_potential(refs, bounds, 65), [2.5 if k == r0 else 1.0 for k in range(R)])
    again = mixed.alignment_of(xc)
    assert all(torch.equal(again[k], al[k]) for k in al) and torch.equal(mixed.tm_of(xc), al['tm'])
    total = sum(2.5 * alone[r] if r == r0 else alone[r] for r in range(R))
    assert torch.allclose(mixed.describe(xc)['e_fold'], total, rtol=1e-5, atol=0) and torch.equal(mixed.describe(xc)['tm_nearest'], rep['tm_nearest'])
    weighted = bounds.clone()
    weighted[r0, 2] = 2.5
    _certificate('weight 2.5 on reference %d' % r0, x, refs, weighted)
    # all weights 0: logp 0 and a gradient of exactly 0
    lp, g = _run(_with_weights(_potential(refs, bounds, 65), [0.0] * R), x)
    assert bool((lp == 0).all()) and bool((g == 0).all())
    # both hinges inactive everywhere: the same
    lp, g = _run(_potential(refs, [(0.0, 1.0)] * R, 65), x)
    assert bool((lp == 0).all()) and bool((g == 0).all())
    # hi = inf is no upper hinge
    open_ = bounds.clone()
    open_[:, 1] = math.inf
    _, r64, _, _, _ = _certificate('hi = inf', x, refs, open_, upper=False)
    assert bool((r64['above'] == 0).all()) and float(r64['below'].max()) > 0


def test_single_pair_gives_the_bits_of_the_full_call_and_a_collapsed_particle_stays_finite():
    x, refs, bounds = _inputs(CASE)
    xc = x.cuda()
    full = _potential(refs, bounds, 65).alignment_of(xc)
    for b, r in ((0, 0), (2, 3), (1, 1)):
        one = _potential(refs[r:r + 1], bounds[r:r + 1], 65).alignment_of(xc[b:b + 1])
        assert all(torch.equal(one[k][0, 0], full[k][b, r]) for k in full), (b, r)
    flat = x.clone()
    flat[2] = flat[2, 5]
    pot = _potential(refs, bounds, 65)
    lp, g = _run(pot, flat)
    rep, al = pot.describe(flat.cuda()), pot.alignment_of(flat.cuda())
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all())
    assert all(bool(torch.isfinite(v.double()).all()) for v in rep.values()) and all(bool(torch.isfinite(v.double()).all()) for v in al.values())
    _check_maps('collapsed particle', al['map'], al['n_aligned'], [len(y) for y in refs])
    assert torch.equal(al['tm'][:2], full['tm'][:2])                                      # the other particles do not feel it


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N_S = 12, 40


def _sampler_noise(B=4):
    """tests/test_fold_gpu.py's noise [T, B, N_S, 3]: the particles share all but a thousandth of every draw's variance, so the four
    designs of a run come out as one fold and a template made from one of them is near every particle."""
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

    # what the model makes of this noise without guidance: a 48-residue indel relative of its first design is the template, wanted at
    # TM 0.8 under norm `query`; a 36-residue relative of its second design is to be avoided
    free, _, _ = run(lambda x0, step: (x0 * 0).sum(dim=(1, 2)), _sampler_noise(), tmp_path_factory.mktemp('fold_align_free'), num_samples=4,
                     ess_threshold=0.0)
    free = torch.from_numpy(free).float()
    refs = [Fa.relative(free[0], 48, 41, 1.0), Fa.relative(free[1], 36, 42, 0.7)]
    assert [len(y) for y in refs] == [48, 36]
    bounds = torch.tensor([[0.8, math.inf, 1.0], [0.0, 0.5, 1.0]], dtype=torch.float64)
    return dict(run=run, abar=abar, free=free, refs=refs, bounds=bounds, fused=_potential(refs, bounds, N_S, abar))


def test_sampler_moves_towards_a_template_of_another_length(ctx, tmp_path):
    B = 4
    b, _, attrs = ctx['run'](ctx['fused'], _sampler_noise(B), tmp_path, num_samples=B, ess_threshold=0.0)
    assert np.isfinite(b).all()
    before = ctx['fused'].tm_of(ctx['free'].cuda())[:, 0]
    after = ctx['fused'].tm_of(torch.from_numpy(b).float().cuda())[:, 0]
    print('TM to the 48-residue template: unguided %s (mean %.4f), guided %s (mean %.4f)'
          % (before.cpu().numpy().round(3).tolist(), float(before.mean()), after.cpu().numpy().round(3).tolist(), float(after.mean())))
    assert float(after.mean()) > float(before.mean())
    report = attrs['last_shape']
    assert tuple(report) == Fa.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    again = ctx['fused'].describe(attrs['last_positions'].cuda())
    assert all(torch.equal(report[k], again[k].cpu()) for k in report)
    assert attrs['last_fit'] is None and attrs['last_secstruct'] is None and attrs['last_pairs'] is None


def test_sum_of_shape_and_aligned_fold_is_bitwise_the_sum(ctx):
    import _shape as Sh
    from genie2_amd.smc import ShapePotential, SumPotential
    shape = ShapePotential(N_S, ctx['abar'], rog_max=6.0, clash_distance=4.0, device='cuda')
    both = SumPotential(shape, ctx['fused'])
    x = Fa.particles(6, N_S, 9).cuda()
    assert torch.equal(both(x, 5), shape(x, 5) + ctx['fused'](x, 5))      # bitwise the sum of its members
    xg = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(both(xg, 5).sum(), xg)
    parts = [torch.autograd.grad(m(xg, 5).sum(), xg)[0] for m in (shape, ctx['fused'])]
    assert torch.equal(g, parts[0] + parts[1]) and float(parts[1].abs().max()) > 0
    report = both.describe(x)
    assert tuple(report) == Sh.REPORT + Fa.REPORT                         # member order
    for m in (shape, ctx['fused']):
        assert all(torch.equal(report[k], v) for k, v in m.describe(x).items())


# ---- the command line ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('fold_align_cli') / 'results')
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


def test_shape_cli_with_a_template_of_another_length(tmp_path, checkpoint_root, capsys):
    from genie2_amd import features as F
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    from genie2_amd.similarity import load_designs
    from genie2_amd.smc import AlignedFoldPotential, TwistedSampler
    whole = load_designs([TEMPLATE])[0][0]
    short = torch.cat([whole[:30], whole[40:]])                           # 90 residues: ten deleted
    f = F.create_empty_np_features([len(short)])
    f['atom_positions'] = short.double().numpy()
    template = str(tmp_path / 'template_90.pdb')
    F.save_np_features_to_pdb(f, template)
    out = str(tmp_path / 'gapped')
    args = build_parser().parse_args(_cli_args(checkpoint_root, out, ['--template_pdb', template, '--fold_align', 'gapped', '--write_fold']))
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
    assert len(seen) == 1 and isinstance(seen[0][2], AlignedFoldPotential) and tuple(seen[0][1]) == Fa.REPORT
    pos, report, pot = seen[0]
    assert pot.lengths == [90] and pot.n_res == 100 and pot.norm == 'query'
    al, again = pot.alignment_of(pos.cuda()), pot.describe(pos.cuda())
    assert torch.equal(pot.tm_of(pos.cuda()), al['tm'])
    names = ['100_0', '100_1']
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == [n + '.pdb' for n in names]
    assert sorted(os.listdir(os.path.join(out, 'fold'))) == [n + '.txt' for n in names]
    for i, name in enumerate(names):
        lines = [ln.split() for ln in open(os.path.join(out, 'fold', name + '.txt'))]
        assert len(lines[0]) == 7 and lines[0][:2] == ['ref', 'template_90'] and (float(lines[0][3]), float(lines[0][4])) == (0.6, math.inf)
        assert abs(float(lines[0][2]) - float(al['tm'][i, 0])) <= 5e-4 + 1e-5            # three decimals, and the float32 bar
        assert int(lines[0][5]) == 90 and int(lines[0][6]) == int(al['n_aligned'][i, 0]) and 3 <= int(lines[0][6]) <= 90
        assert [f[0] for f in lines[1:]] == list(Fa.REPORT) and all(len(f) == 2 for f in lines[1:])
        for f in lines[1:]:
            assert torch.equal(report[f[0]][i], again[f[0]][i].cpu())
            assert abs(float(f[1]) - float(report[f[0]][i])) <= 5e-4 + 1e-5 * max(1.0, abs(float(report[f[0]][i]))), (name, f)
    capsys.readouterr()
    # the same run under the identity alignment: a template of another length skips the length, as before
    out = str(tmp_path / 'gapless')
    args = build_parser().parse_args(_cli_args(checkpoint_root, out, ['--template_pdb', template, '--fold_align', 'gapless', '--write_fold']))
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    assert 'skipping lengths without a fold reference of their own length: 100\n' in capsys.readouterr().out
    assert not os.path.exists(os.path.join(out, 'fold'))
