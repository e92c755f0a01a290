"""The sheet potential on the GPU (genie_sheet_potential, csrc/sheet_kernels.hip; SheetPotential, SumPotential in genie2_amd/smc.py)
against the float64 oracle of tests/_sheet.py, in TwistedSampler against the float32 PyTorch restatement as its twisting function,
composed with the motif, the shape and the secondary-structure potential in particle systems, and through both command lines.

Bounds (tests/_motif.py:60-72, the project's bars for a fused potential, used as in test_shape_gpu.py and test_secstruct_gpu.py): logp
within 1e-5 max(1, |logp|); every particle's gradient within 1e-5 of its largest reference entry; each widened, per case, to 4 x the
error the float32 restatement makes on the same input where that is larger (the kernel is held to float32 arithmetic; the factor
covers another summation order).  Report fields: counts and every partner exactly, the rest within the logp bar.

Worst error / bound over the parity cases, measured on an MI355X: 0.028 for logp, 0.191 for the gradient, no bar widened; at N = 4301
(test_chain_whose_staging...) 0.005 / 0.023 of bars the restatement widens x5.5 / x4.9."""
import math
import os

import numpy as np
import pytest
import torch

import _sheet as S
from _motif import MOTIF, _abar, _tiny_model, segments_6e6r, walk

pytestmark = pytest.mark.gpu

STEP = 500
# (B, N, chain seed): no rung (N = 5); the first antiparallel rung (6); three of them (7); the first parallel rungs (9); both sides of a
# 64-residue tile and of the four waves' split of the partners; a long chain, one particle.  Seeds: every case keeps its z-scores 1e-4
# from the class boxes, its soft counts 1e-4 from the content bounds and the scores of one residue's formed rungs 1e-4 apart, and from
# N = 24 on the oracle finds formed rungs of both classes and unpaired residues (test_report...); seed 1 at N = 1512 has a z-score
# 4.8e-5 from a box.
CASES = [(3, 5, 1), (3, 6, 1), (3, 7, 1), (3, 9, 1), (3, 63, 1), (3, 64, 1), (3, 65, 1), (3, 129, 1), (3, 256, 1), (3, 257, 1),
         (3, 300, 1), (1, 1512, 5)]
_cache = {}


def _case(B, N, seed, term=None, **kw):
    """(x, cfg) of a parity case; term: leave only that term on; kw: chain_config's table / separation."""
    if (B, N, seed) not in _cache:
        _cache[(B, N, seed)] = S.sheet_chain(B, N, seed)
    x, key = _cache[(B, N, seed)], (B, N, seed, repr(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = S.chain_config(x, **kw)
    return x, (_cache[key] if term is None else S.only(_cache[key], term))


def _reference(x, cfg, var):
    """The oracle and the float32 restatement of an input, computed once."""
    key = ('ref', x.data_ptr(), tuple(x.shape), repr(sorted(cfg.items())), var)
    if key not in _cache:
        _cache[key] = (x, S.reference(x, cfg, var), S.restatement32(x.cpu(), cfg, var))      # (x kept: its data_ptr stays its own)
    return _cache[key][1:]


def _run(pot, x, step=STEP):
    x = x.cuda().requires_grad_(True)
    lp = pot(x, step)
    g, = torch.autograd.grad(lp.sum(), x)
    return lp.detach(), g


def _bounds(ref, r32):
    """The bars of one case: (logp bound [B], gradient bound [B]), widened by the float32 restatement's error."""
    lp_b = 1e-5 * ref['logp'].abs().clamp(min=1.0)
    g_b = 1e-5 * ref['grad'].abs().amax(dim=(1, 2))
    e_lp = (r32['logp'].double() - ref['logp']).abs()
    e_g = (r32['grad'].double() - ref['grad']).abs().amax(dim=(1, 2))
    widen_lp = max(1.0, 4.0 * float((e_lp / lp_b).max()))
    widen_g = max(1.0, 4.0 * float(torch.where(g_b > 0, e_g / g_b.clamp(min=1e-300), torch.zeros_like(e_g)).max()))
    return lp_b * widen_lp, g_b * widen_g, widen_lp, widen_g


def _check(what, lp, g, x, cfg, var, refs=None):
    ref, r32 = _reference(x, cfg, var) if refs is None else refs
    lp, g = lp.double().cpu(), g.double().cpu()
    lp_b, g_b, widen_lp, widen_g = _bounds(ref, r32)
    d_lp, d_g = (lp - ref['logp']).abs(), (g - ref['grad']).abs().amax(dim=(1, 2))
    ratio = lambda d, b: float(torch.where(b > 0, d / b.clamp(min=1e-300), torch.where(d > 0, math.inf, 0.0).double()).max())      # noqa: E731
    print('%s: logp error / bound %.3f (bound widened x%.2f), gradient error / bound %.3f (x%.2f)'
          % (what, ratio(d_lp, lp_b), widen_lp, ratio(d_g, g_b), widen_g))
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), what
    assert bool((d_lp <= lp_b).all()), (what, lp, ref['logp'])
    assert bool((d_g <= g_b).all()), (what, d_g, g_b)
    return ref


@pytest.mark.parametrize('B,N,seed', CASES)
def test_potential_matches_the_float64_oracle(B, N, seed):
    x, cfg = _case(B, N, seed)
    pot = S.potential(cfg, N, _abar())
    ref = _check('B=%d N=%d' % (B, N), *_run(pot, x), x, cfg, float(pot.variance(STEP)))
    if N >= 24:                                                          # all three terms act, one class under its minimum, one over its maximum
        assert all(bool((ref[k] > 0).all()) for k in ('e_antiparallel', 'e_parallel', 'e_ladder'))
        assert bool((ref['n'][:, 0] < N * cfg['antiparallel'][0]).all()) and bool((ref['n'][:, 1] > N * cfg['parallel'][1]).all())
        listed = S.rungs(cfg['ladder'])
        assert min(r[0] for r in listed) == 1 and max(r[1] for r in listed) == N - 2      # the ladder reaches both ends of the chain


def test_chain_whose_staging_needs_more_than_64_kib_of_lds():
    """N = 4301: 12 N + 14 336 bytes of dynamic LDS are 65 948, above the 65 536 a kernel gets without asking (from N = 4267 on the
    entry raises the kernel's limit).  The float64 oracle is the same torch code run on the device: on the CPU it takes several seconds
    at this length.  logp and the gradient only: the margins of the counts are not looked at."""
    N = 4301
    x = S.sheet_chain(1, N, 1)
    xc = x.cuda()
    cfg = S.chain_config(xc)
    pot = S.potential(cfg, N, _abar())
    var = float(pot.variance(STEP))
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}      # noqa: E731
    refs = cpu(S.reference(xc, cfg, var, device='cuda')), cpu(S.restatement32(xc, cfg, var))
    ref = _check('B=1 N=%d' % N, *_run(pot, x), x, cfg, var, refs)
    assert all(bool((ref[k] > 0).all()) for k in ('e_antiparallel', 'e_parallel', 'e_ladder')) and int(ref['n_antiparallel']) > 500
    a, b = _run(pot, x), _run(pot, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('term', ['antiparallel', 'parallel', 'ladder'])
def test_each_term_alone(term):
    x, cfg = _case(3, 65, 1, term)
    pot = S.potential(cfg, 65, _abar())
    ref = _check('N=65 %s alone' % term, *_run(pot, x), x, cfg, float(pot.variance(STEP)))
    assert bool((ref['logp'] < 0).all())
    # the same term switched on through the constructor alone
    from genie2_amd.smc import SheetPotential
    kw = {'antiparallel': dict(antiparallel=cfg['antiparallel'], antiparallel_weight=cfg['antiparallel_weight']),
          'parallel': dict(parallel=cfg['parallel'], parallel_weight=cfg['parallel_weight']),
          'ladder': dict(ladder=cfg['ladder'], ladder_weight=cfg['ladder_weight'])}[term]
    alone = SheetPotential(65, _abar(), device='cuda', **kw)
    a, b = _run(pot, x), _run(alone, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('kw', [dict(table=(5.3, 0.8, 4.6, 0.35)), dict(separation=(4, 3)), dict(separation=(7, 9))],
                         ids=['table', 'separation-4-3', 'separation-7-9'])
def test_custom_table_and_separations(kw):
    """Other targets and tolerances, and other separations: a parallel class that counts a helix's (i, i+3) pairs, and classes that
    skip tight hairpins."""
    x, cfg = _case(3, 65, 1, **kw)
    pot = S.potential(cfg, 65, _abar())
    ref = _check('N=65 %s' % (kw,), *_run(pot, x), x, cfg, float(pot.variance(STEP)))
    base = S.reference(x, _case(3, 65, 1)[1], float(pot.variance(STEP)))
    assert not torch.allclose(ref['n'], base['n'], rtol=1e-2)            # (the table / the separations are the ones in use)
    assert min(S.margins(x, cfg)) >= 1e-4, 'a count of this case could flip in float32: change the table'
    xc = x.cuda()
    got = pot.describe(xc)
    assert torch.equal(pot.pairs(xc).cpu(), ref['pairs']) and all(torch.equal(got[k].cpu(), ref[k]) for k in S.COUNTS)


@pytest.mark.parametrize('B,N,seed', CASES)
def test_report_and_pairs_match_the_oracle(B, N, seed):
    x, cfg = _case(B, N, seed)
    box, hinge, tie = S.margins(x, cfg)
    print('B=%d N=%d: smallest margin of a z-score to a class box %.3e, of a soft count to a content bound %.3e, between the scores of '
          'two formed rungs of one residue %.3e' % (B, N, box, hinge, tie))
    assert box >= 1e-4 and hinge >= 1e-4 and tie >= 1e-4, 'a count or a partner of this case could flip in float32: take another seed'
    pot = S.potential(cfg, N, _abar())
    got, pairs = pot.describe(x.cuda()), pot.pairs(x.cuda())
    ref, r32 = _reference(x, cfg, 1.0)
    assert pairs.dtype == torch.int32 and tuple(pairs.shape) == (B, N, 2) and pairs.device.type == 'cuda'
    assert torch.equal(pairs.cpu(), ref['pairs'])
    if N >= 24:                                                          # formed rungs of both classes, and unpaired residues
        assert int(ref['n_antiparallel'].sum()) > 0 and int(ref['n_parallel'].sum()) > 0 and bool((ref['n_paired'] < N).all())
        assert bool((ref['pairs'][:, :, 0] >= 0).any()) and bool((ref['pairs'][:, :, 1] >= 0).any()) and bool((ref['pairs'] < 0).all(dim=2).any())
    else:
        assert N >= 6 or bool((ref['pairs'] == -1).all())
    assert tuple(got) == S.REPORT
    for k in S.REPORT:
        assert tuple(got[k].shape) == (B,) and got[k].device.type == 'cuda', k
        if k in S.COUNTS:
            assert got[k].dtype == torch.int64 and torch.equal(got[k].cpu(), ref[k]), (k, got[k], ref[k])
            continue
        g, r = got[k].double().cpu(), ref[k]
        bound = 1e-5 * r.abs().clamp(min=1.0)
        bound = bound * max(1.0, 4.0 * float(((r32[k].double() - r).abs() / bound).max()))
        assert bool(((g - r).abs() <= bound).all()), (k, g, r)
    assert torch.equal(got['n_paired'].cpu(), (pairs >= 0).any(dim=2).sum(dim=1).cpu())
    if cfg['ladder'] is not None:
        assert bool((ref['n_ladder_missed'] > 0).all())                  # the ladder does not follow the chain


def test_edges():
    from genie2_amd.smc import SheetPotential
    abar = _abar()
    inf = math.inf
    # a straight 3.8 A chain with only upper bounds: no pair is near a rung, logp 0 and a gradient of exactly 0
    N = 70
    line = torch.zeros(2, N, 3)
    line[0, :, 0] = 3.8 * torch.arange(N)
    line[1, :, 1] = 3.8 * torch.arange(N) - 20.0
    cfg = S.config(antiparallel=(0.0, 0.2), antiparallel_weight=1.0, parallel=(0.0, 0.1), parallel_weight=2.0)
    pot = S.potential(cfg, N, abar)
    lp, g = _run(pot, line)
    _check('a straight line', lp, g, line, cfg, float(pot.variance(STEP)))
    assert bool((lp == 0).all()) and bool((g == 0).all())
    rep = pot.describe(line.cuda())
    assert rep['n_paired'].tolist() == [0, 0] and bool((pot.pairs(line.cuda()) == -1).all()) and float(rep['antiparallel_content'].max()) < 0.01

    # two coincident residues inside a rung (a d0 of exactly 0, in an eligible and in a listed rung): finite, the oracle's values
    x = S.sheet_chain(2, 24, 1)
    x[0, 9] = x[0, 3]
    x[1, 22] = x[1, 1]
    cfg = S.chain_config(S.sheet_chain(2, 24, 1))
    assert (1, 22, 0, 0.7) in S.rungs(cfg['ladder'])
    pot = S.potential(cfg, 24, abar)
    ref = _check('coincident residues', *_run(pot, x), x, cfg, float(pot.variance(STEP)))
    assert min(S.margins(x, cfg)) >= 1e-4
    assert torch.equal(pot.pairs(x.cuda()).cpu(), ref['pairs'])
    # every residue in one point: no direction anywhere, the gradient is exactly 0
    x = torch.ones(1, 9, 3) * 2.5
    cfg = S.config(antiparallel=(0.5, inf), antiparallel_weight=1.0, parallel=(0.0, 0.01), parallel_weight=1.0, ladder=[(1, 7, 1, 'A'), (2, 7, 1, 'P')],
                   ladder_weight=1.0)
    pot = S.potential(cfg, 9, abar)
    lp, g = _run(pot, x)
    ref = _check('one point', lp, g, x, cfg, float(pot.variance(STEP)))
    assert bool((ref['grad'] == 0).all()) and bool((g == 0).all()) and float(ref['logp']) < 0

    # N = 3 and N = 5: no eligible rung, n_c = 0, a gradient of exactly 0, every pair -1; a positive minimum gives the oracle's logp
    for n in (3, 5):
        x = S.sheet_chain(2, n, 1)
        cfg = S.config(antiparallel=(0.2, inf), antiparallel_weight=1.5, parallel=(0.1, 0.3), parallel_weight=1.0)
        pot = S.potential(cfg, n, abar)
        lp, g = _run(pot, x)
        ref = _check('N=%d' % n, lp, g, x, cfg, float(pot.variance(STEP)))
        assert bool((g == 0).all()) and bool((ref['logp'] < 0).all()) and bool((pot.pairs(x.cuda()) == -1).all())
        rep = pot.describe(x.cuda())
        assert all(bool((rep[k] == 0).all()) for k in ('antiparallel_content', 'parallel_content', 'n_antiparallel', 'n_parallel', 'n_paired'))
        expect = torch.tensor([1.5 * (0.2 * n) ** 2, 1.0 * (0.1 * n) ** 2], dtype=torch.float64)
        assert torch.allclose(torch.stack([rep['e_antiparallel'], rep['e_parallel']], dim=1).double().cpu(), expect.expand(2, 2), rtol=1e-6)

    # a weight of 0 is the oracle with that term off, and bitwise the potential built without the term
    x, cfg = _case(3, 65, 1)
    full = dict(antiparallel=cfg['antiparallel'], antiparallel_weight=cfg['antiparallel_weight'], parallel=cfg['parallel'],
                parallel_weight=cfg['parallel_weight'], ladder=cfg['ladder'], ladder_weight=cfg['ladder_weight'])
    for off, without, field in ((dict(antiparallel_weight=0.0), ('antiparallel', 'antiparallel_weight'), 'e_antiparallel'),
                                (dict(parallel_weight=0.0), ('parallel', 'parallel_weight'), 'e_parallel'),
                                (dict(ladder_weight=0.0), ('ladder', 'ladder_weight'), 'e_ladder')):
        c = dict(cfg, **off)
        pot = S.potential(c, 65, abar)
        a = _run(pot, x)
        _check('N=65 with %s' % off, *a, x, c, float(pot.variance(STEP)))
        b = _run(SheetPotential(65, abar, device='cuda', **{k: v for k, v in full.items() if k not in without}), x)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        rep = pot.describe(x.cuda())
        assert bool((rep[field] == 0).all()) and all(bool((rep[k] > 0).all()) for k in ('e_antiparallel', 'e_parallel', 'e_ladder') if k != field)
    # (the ladder is still reported against at weight 0)
    assert torch.equal(rep['n_ladder_missed'].cpu(), S.reference(x, dict(cfg, ladder_weight=0.0), 1.0)['n_ladder_missed'])

    # the ideal two-stranded sheets: six formed rungs each, in their own column, with the partners across the sheet
    anti, par = S.ideal_sheet(2).float()[None].cuda(), S.ideal_sheet(2, parallel=True).float()[None].cuda()
    pot = SheetPotential(16, abar, antiparallel=(0.3, inf), device='cuda')
    a, b = pot.describe(anti), pot.describe(par)
    assert int(a['n_antiparallel']) == 6 and int(a['n_parallel']) == 0 and int(a['n_paired']) == 12 and float(a['e_antiparallel']) == 0
    assert int(b['n_antiparallel']) == 0 and int(b['n_parallel']) == 6 and int(b['n_paired']) == 12 and float(b['e_antiparallel']) > 0
    pa, pp = pot.pairs(anti)[0].cpu(), pot.pairs(par)[0].cpu()
    assert pa[:, 0].tolist() == [-1] + [15 - k for k in range(1, 7)] + [-1, -1] + [15 - k for k in range(9, 15)] + [-1]
    assert pa[:, 1].tolist() == [-1] * 16 and pp[:, 0].tolist() == [-1] * 16
    assert pp[:, 1].tolist() == [-1] + list(range(9, 15)) + [-1, -1] + list(range(1, 7)) + [-1]
    assert float(pot(anti, STEP)) == 0 and float(pot(par, STEP)) < 0
    # a listed ladder the sheet fulfils is not missed; the same ladder on the parallel sheet is
    pot = SheetPotential(16, abar, ladder=[(1, 14, 6, 'A')], device='cuda')
    assert int(pot.describe(anti)['n_ladder_missed']) == 0 and int(pot.describe(par)['n_ladder_missed']) == 6


def test_deterministic_and_never_synchronises():
    x, cfg = _case(3, 300, 1)
    pot = S.potential(cfg, 300, _abar())
    xc = x.cuda()
    a, b = _run(pot, xc, 400), _run(pot, xc, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ra, rb = pot.describe(xc), pot.describe(xc)
    sa, sb = pot.pairs(xc), pot.pairs(xc)
    assert all(torch.equal(ra[k], rb[k]) for k in ra) and torch.equal(sa, sb)
    xg = xc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(xg, 400)
        g, = torch.autograd.grad(lp.mean(), xg)
        rep = pot.describe(xc)
        sc = pot.pairs(xc)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.allclose(g, a[1] / 3, rtol=1e-6, atol=0)      # (the backward scales by grad_output = 1/3)
    assert all(torch.equal(rep[k], ra[k]) for k in ra) and torch.equal(sc, sa)
    with pytest.raises(ValueError):
        pot(xc[:, :299], 400)
    with pytest.raises(ValueError):
        pot(x, 400)                                                                       # (a CPU tensor)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N_S = 12, 40
SAMPLER_LADDER = [(3, 30, 4, 'A'), (8, 20, 3, 'P', 0.5)]
SAMPLER_CFG = S.config(antiparallel=(0.2, math.inf), antiparallel_weight=1.0, parallel=(0.0, 0.0), parallel_weight=1.0,
                       ladder=SAMPLER_LADDER, ladder_weight=0.02)
RESAMPLING_SEED = 5


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
        attrs = {k: getattr(sampler, k, None) for k in ('last_fit', 'last_shape', 'last_secstruct', 'last_pairs', 'last_choice')}
        return np.stack([r['atom_positions'] for r in out]), sampler.resampled_at, sampler.ess_trace, attrs

    return dict(run=run, abar=abar, fused=S.potential(SAMPLER_CFG, N_S, abar), torch=S.twisting_function(SAMPLER_CFG, abar))


def _noise(B, seed):
    return torch.randn(T, B, N_S, 3, generator=torch.Generator().manual_seed(seed))


def test_sampler_follows_the_torch_path_without_resampling(ctx, tmp_path):
    B, noise = 4, _noise(4, 4)
    a, ra, _, attrs_a = ctx['run'](ctx['torch'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    b, rb, _, attrs_b = ctx['run'](ctx['fused'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    rms, d = float(np.sqrt((a ** 2).mean())), float(np.abs(a - b).max())
    print('no resampling: max |d| = %.3e, coordinate RMS = %.2f, ratio %.3e' % (d, rms, d / rms))
    assert np.isfinite(b).all() and ra == rb == [] and d <= 1e-3 * rms
    assert attrs_a['last_shape'] is None and attrs_a['last_pairs'] is None and attrs_a['last_fit'] is None      # a plain callable
    assert attrs_b['last_fit'] is None and attrs_b['last_secstruct'] is None
    again = ctx['fused'].pairs(torch.from_numpy(b).float().cuda())
    assert attrs_b['last_pairs'].device.type == 'cpu' and torch.equal(attrs_b['last_pairs'], again.cpu())


def test_sampler_resamples_where_the_torch_path_does(ctx, tmp_path):
    B, noise, u = 4, _noise(4, RESAMPLING_SEED), [0.37] * T
    a, ra, ess_a, _ = ctx['run'](ctx['torch'], noise, tmp_path, num_samples=B, ess_threshold=0.5, resample_u=u)
    gap = min(abs(e - 0.5 * B) / (0.5 * B) for e in ess_a)
    print('noise seed %d: the ESS of the torch run stays %.3e of the threshold away from it' % (RESAMPLING_SEED, gap))
    assert gap >= 1e-3, 'the ESS of the torch run comes within %.1e of the threshold: take another noise seed' % gap
    b, rb, ess_b, attrs = ctx['run'](ctx['fused'], noise, tmp_path, num_samples=B, ess_threshold=0.5, resample_u=u)
    print('resampled at', ra, rb, 'ESS', ess_a, ess_b)
    assert ra == rb and len(ra) > 0 and np.isfinite(b).all()
    report, pairs = attrs['last_shape'], attrs['last_pairs']
    assert tuple(report) == S.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    xb = torch.from_numpy(b).float().cuda()
    again = ctx['fused'].describe(xb)
    assert all(torch.equal(report[k], again[k].cpu()) for k in report)
    assert pairs.dtype == torch.int32 and tuple(pairs.shape) == (B, N_S, 2) and torch.equal(pairs, ctx['fused'].pairs(xb).cpu())


def test_particle_systems_with_the_sum_of_four_potentials(ctx, tmp_path):
    import _secstruct as Ss
    import _shape as Sh
    from genie2_amd.smc import MotifPotential, SecStructPotential, ShapePotential, SumPotential
    S_, K = 2, 3
    motif = MotifPotential(segments_6e6r(), N_S, ctx['abar'], rng=np.random.RandomState(0), device='cuda')
    shape = ShapePotential(N_S, ctx['abar'], rog_max=6.0, clash_distance=4.0, device='cuda')
    secstruct = SecStructPotential(N_S, ctx['abar'], extended=(0.3, 1.0), device='cuda')
    members = (motif, shape, secstruct, ctx['fused'])
    all4 = SumPotential(*members)
    x = walk(S_ * K, N_S, 9).cuda()
    assert torch.equal(all4(x, 5), ((motif(x, 5) + shape(x, 5)) + secstruct(x, 5)) + ctx['fused'](x, 5))
    xg = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(all4(xg, 5).sum(), xg)
    parts = [torch.autograd.grad(m(xg, 5).sum(), xg)[0] for m in members]
    assert torch.allclose(g, ((parts[0] + parts[1]) + parts[2]) + parts[3], rtol=1e-6, atol=1e-6 * float(g.abs().max()))
    noise = torch.randn(T, S_ * K, N_S, 3, generator=torch.Generator().manual_seed(11))
    best, _, ess, attrs = ctx['run'](all4, noise, tmp_path, num_samples=S_, num_particles=K, ess_threshold=0.5,
                                     resample_u=[[0.05, 0.21]] * T, return_particles='best')
    assert tuple(best.shape) == (S_, N_S, 3) and np.isfinite(best).all() and tuple(ess.shape) == (T - 1, S_)
    fit, report, assign, pairs = attrs['last_fit'], attrs['last_shape'], attrs['last_secstruct'], attrs['last_pairs']
    assert fit is not None and tuple(fit['rmsd'].shape) == (S_,)
    assert tuple(report) == Sh.REPORT + Ss.REPORT + S.REPORT and all(tuple(v.shape) == (S_,) for v in report.values())      # member order
    xb = torch.from_numpy(best).float().cuda()
    for m in (shape, secstruct, ctx['fused']):
        assert all(torch.equal(report[k], v.cpu()) for k, v in m.describe(xb).items())
    assert tuple(assign.shape) == (S_, N_S) and torch.equal(assign, secstruct.assign(xb).cpu())
    assert pairs.dtype == torch.int32 and tuple(pairs.shape) == (S_, N_S, 2) and torch.equal(pairs, ctx['fused'].pairs(xb).cpu())
    assert torch.equal(fit['rmsd'], motif.locate(xb)['rmsd'].cpu())


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('sheet_cli') / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return root


def _check_sheet_files(out, names, cfg):
    """Every outdir/sheet file against the float64 oracle on the coordinates its PDB holds: `i j A|P` lines, each rung once, then the
    nine fields.  The PDB rounds coordinates to 1e-3 A (at most 5e-4 per coordinate, so 2 sqrt(3) 5e-4 = 1.8e-3 A per distance and
    3.5e-3 per z-score at the smaller sigma of 0.5 A) and the report its values to three decimals: a float may differ from the
    oracle's on the written coordinates by 5e-4 + 1.5 * 5e-4 |d value / d x|_1 plus the float32 bar 1e-5 max(1, |value|); the rungs
    and the counts may differ by the number of rungs with a z-score within 4e-3 of the box (none, for most seeds), n_paired by twice
    that."""
    from genie2_amd.features import parse_pdb
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == sorted(n + '.pdb' for n in names)
    assert sorted(os.listdir(os.path.join(out, 'sheet'))) == sorted(n + '.txt' for n in names)
    for name in names:
        y = torch.tensor(parse_pdb(os.path.join(out, 'pdbs', name + '.pdb'))[1][0], dtype=torch.float64)[None].requires_grad_(True)
        assert tuple(y.shape) == (1, N_S, 3)
        lines = [ln.split() for ln in open(os.path.join(out, 'sheet', name + '.txt'))]
        rungs, fields = lines[:-len(S.REPORT)], lines[-len(S.REPORT):]
        assert [f[0] for f in fields] == list(S.REPORT) and all(len(f) == 2 for f in fields)
        got = {f[0]: f[1] for f in fields}
        assert all('.' not in got[k] for k in S.COUNTS) and all('.' in got[k] for k in S.REPORT if k not in S.COUNTS)
        assert all(len(r) == 3 and r[2] in 'AP' and int(r[0]) < int(r[1]) for r in rungs) and len({tuple(r) for r in rungs}) == len(rungs)
        t = S.terms(y, cfg)
        z = S.zscores(y.detach(), cfg)
        near = ((z.abs() - 1).abs() < 4e-3).any(dim=-1) & S.eligible(N_S, cfg)[None]
        slack = int(near.sum())
        # every residue names its best partner per class: the rungs a file can list are those either end names
        named = {(min(n, m), max(n, m), 'AP'[c]) for n, row in enumerate(t['pairs'][0].tolist()) for c, m in enumerate(row) if m >= 0}
        assert len(named ^ {(int(r[0]), int(r[1]), r[2]) for r in rungs}) <= slack, (name, rungs, named)
        for k in S.REPORT:
            ref = t[k][0]
            if k in S.COUNTS:
                assert abs(int(got[k]) - int(ref)) <= (2 * slack if k == 'n_paired' else slack), (name, k, got[k], int(ref))
                continue
            grad, = torch.autograd.grad(ref, y, retain_graph=True, allow_unused=True)
            l1 = 0.0 if grad is None else float(grad.abs().sum())
            tol = 5e-4 + 1.5 * 5e-4 * l1 + 1e-5 * max(1.0, abs(float(ref.detach())))
            assert abs(float(got[k]) - float(ref.detach())) <= tol, (name, k, got[k], float(ref.detach()), tol)


def test_shape_cli_with_sheet_terms_end_to_end(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    out = str(tmp_path / 'out')
    lad = tmp_path / 'ladder.txt'
    lad.write_text('# a hairpin over residues 3..6 and 27..30\n3 30 4 A\n8 20 3 P 0.5\n')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--min_length', '40', '--max_length', '40', '--batch_size', '2', '--num_samples', '2',
                                      '--num_steps', '4', '--last_unguided_steps', '0', '--guidance_alpha', '0.05',
                                      '--antiparallel_min', '0.2', '--parallel_max', '0', '--ladder_file', str(lad), '--ladder_weight', '0.02',
                                      '--write_sheet'])
    torch.manual_seed(0)
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_sheet_files(out, ['40_0', '40_1'], SAMPLER_CFG)
    assert not os.path.exists(os.path.join(out, 'shape')) and not os.path.exists(os.path.join(out, 'secstruct'))


def test_motif_cli_with_every_kind_of_term_end_to_end(tmp_path, checkpoint_root):
    import _secstruct as Ss
    import _shape as Sh
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    out = str(tmp_path / 'out')
    lad = tmp_path / 'ladder.txt'
    lad.write_text('3 38 4 A\n')                                                              # the centre 38 needs 40 residues
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--motif_file', MOTIF, '--min_length', '39', '--max_length', '40', '--batch_size', '2',
                                      '--num_samples', '2', '--num_steps', '4', '--last_unguided_steps', '0', '--ladder_file', str(lad),
                                      '--ladder_weight', '0.02', '--parallel_max', '0.01', '--rog_max', '6', '--extended_min', '0.3',
                                      '--write_shape_report', '--write_secstruct', '--write_sheet', '--write_motif_locations'])
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    names = ['40_0', '40_1']                                                                  # (length 39 cannot hold the ladder: skipped)
    _check_sheet_files(out, names, S.config(parallel=(0.0, 0.01), parallel_weight=1.0, ladder=[(3, 38, 4, 'A')], ladder_weight=0.02))
    for folder, report in (('shape', Sh.REPORT), ('secstruct', Ss.REPORT)):
        assert sorted(os.listdir(os.path.join(out, folder))) == sorted(n + '.txt' for n in names)
        for name in names:
            lines = [ln.split() for ln in open(os.path.join(out, folder, name + '.txt'))][folder == 'secstruct':]
            assert [ln[0] for ln in lines] == list(report) and all(len(ln) == 2 for ln in lines)      # exactly their own keys
    assert sorted(os.listdir(os.path.join(out, 'motif_locations'))) == sorted(n + '.txt' for n in names)
