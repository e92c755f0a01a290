"""The shape potential on the GPU (genie_shape_potential, csrc/shape_kernels.hip; ShapePotential, SumPotential in genie2_amd/smc.py)
against the float64 oracle of tests/_shape.py, in TwistedSampler against the float32 PyTorch restatement as its twisting function,
composed with the motif potential in particle systems, and through both command lines.

Bounds (tests/_motif.py:60-72, the project's bars for a fused potential): logp within 1e-5 max(1, |logp|); every particle's gradient
within 1e-5 of its largest reference entry; each widened, per case, to 4 x the error the float32 restatement makes on the same input
where that is larger (the kernel is held to float32 arithmetic; the factor covers another summation order).  Report fields: counts
exactly, the rest within the logp bar.

Worst error / bound over the parity cases, measured on an MI355X: 0.023 for logp, 0.049 for the gradient, no bar widened."""
import math
import os

import numpy as np
import pytest
import torch

import _shape as S
from _motif import MOTIF, _abar, _ca_coordinates, _tiny_model, segments_6e6r, walk

pytestmark = pytest.mark.gpu

STEP = 500
# (B, N, walk seed): below, at and above the 64-residue tile, several tiles, a quarter of N that is no multiple of the chunk, and the
# longest N genie_create accepts.  Seeds: every case keeps 1e-4 A between its distances and their thresholds (test_report...).
CASES = [(3, 2, 1), (3, 3, 1), (3, 63, 1), (3, 64, 2), (3, 65, 1), (3, 129, 2), (3, 256, 1), (3, 300, 2), (1, 1512, 1)]
_cache = {}


def _case(B, N, seed, term=None):
    """(x, cfg) of a parity case; term: leave only that term on."""
    if (B, N, seed) not in _cache:
        x = walk(B, N, seed)
        _cache[(B, N, seed)] = (x, S.walk_config(x, 40, seed))
    x, cfg = _cache[(B, N, seed)]
    return x, (cfg if term is None else S.only(cfg, term))


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


def _check(what, lp, g, x, cfg, var):
    ref, r32 = S.reference(x, cfg, var), S.restatement32(x.cpu(), cfg, var)
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
    assert len(cfg['restraints']) == min(40, N * (N - 1) // 2)
    pot = S.potential(cfg, N, _abar())
    ref = _check('B=%d N=%d' % (B, N), *_run(pot, x), x, cfg, float(pot.variance(STEP)))
    if N > 3:
        assert float(ref['e_rog'][0]) > 0 and float(ref['e_clash'][0]) > 0 and float(ref['e_restraint'][0]) > 0      # all three terms act


@pytest.mark.parametrize('term', ['rog', 'clash', 'restraints'])
def test_each_term_alone(term):
    x, cfg = _case(3, 65, 1, term)
    pot = S.potential(cfg, 65, _abar())
    _check('N=65 %s alone' % term, *_run(pot, x), x, cfg, float(pot.variance(STEP)))
    # the same term switched on through the constructor alone
    from genie2_amd.smc import ShapePotential
    kw = {'rog': dict(rog_max=cfg['rog_max']), 'clash': dict(clash_distance=cfg['clash_distance']),
          'restraints': dict(restraints=cfg['restraints'])}[term]
    alone = ShapePotential(65, _abar(), device='cuda', **kw)
    a, b = _run(pot, x), _run(alone, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('B,N,seed', CASES)
def test_report_matches_the_oracle(B, N, seed):
    x, cfg = _case(B, N, seed)
    margin = S.margins(x, cfg)
    print('B=%d N=%d: smallest margin of a distance or rog to its threshold %.3e A' % (B, N, margin))
    assert margin >= 1e-4, 'a count of this case could flip in float32: take another walk seed'
    pot = S.potential(cfg, N, _abar())
    got = pot.describe(x.cuda())
    ref, r32 = S.reference(x, cfg, 1.0), S.restatement32(x, cfg, 1.0)
    assert set(got) == set(S.REPORT)
    for k in S.REPORT:
        assert tuple(got[k].shape) == (B,) and got[k].device.type == 'cuda', k
        if k in S.COUNTS:
            assert got[k].dtype == torch.int64 and torch.equal(got[k].cpu(), ref[k]), (k, got[k], ref[k])
            continue
        g, r = got[k].double().cpu(), ref[k]
        fin = torch.isfinite(r)
        assert torch.equal(g[~fin], r[~fin]), (k, g, r)
        bound = 1e-5 * r[fin].abs().clamp(min=1.0)
        bound = bound * max(1.0, 4.0 * float(((r32[k].double()[fin] - r[fin]).abs() / bound).max()) if bool(fin.any()) else 1.0)
        assert bool(((g[fin] - r[fin]).abs() <= bound).all()), (k, g, r)


def test_edges():
    abar = _abar()
    # a straight 3.8 A chain, nothing violated: logp and the gradient are exactly 0
    N = 70
    line = torch.zeros(2, N, 3)
    line[0, :, 0] = 3.8 * torch.arange(N)
    line[1, :, 1] = 3.8 * torch.arange(N) - 20.0
    cfg = S.config(rog_max=100.0, rog_weight=1.0, clash_distance=4.0, clash_weight=1.0, restraints=[(0, 10, 30.0, 40.0, 1.0), (69, 5, 0.0, math.inf, 2.0)])
    pot = S.potential(cfg, N, abar)
    lp, g = _run(pot, line)
    assert bool((lp == 0).all()) and bool((g == 0).all())
    rep = pot.describe(line.cuda())
    assert rep['n_clash'].tolist() == [0, 0] and rep['n_violated'].tolist() == [0, 0] and bool((rep['max_violation'] == 0).all())
    assert torch.allclose(rep['min_distance'].cpu(), torch.tensor([7.6, 7.6]), rtol=1e-5)       # (float32 spacing of a 250 A coordinate)

    # two coincident residues, clashing and restrained: finite, and the oracle's value
    x = walk(2, 20, 5)
    x[:, 7] = x[:, 3]
    cfg = S.config(rog_max=3.0, rog_weight=1.0, clash_distance=4.0, clash_weight=1.0, restraints=[(3, 7, 1.0, 2.0, 1.0), (0, 19, 0.0, 5.0, 1.0)])
    pot = S.potential(cfg, 20, abar)
    ref = _check('coincident residues', *_run(pot, x), x, cfg, float(pot.variance(STEP)))
    assert bool((ref['min_distance'] == 0).all()) and bool((pot.describe(x.cuda())['min_distance'] == 0).all())
    # every residue in one point: rog is exactly 0 too
    x = torch.ones(1, 5, 3) * 2.5
    pot = S.potential(S.config(rog_max=0.0, rog_weight=1.0, clash_distance=4.0, clash_weight=1.0), 5, abar)
    ref = _check('one point', *_run(pot, x), x, S.config(rog_max=0.0, rog_weight=1.0, clash_distance=4.0, clash_weight=1.0), float(pot.variance(STEP)))
    assert bool((ref['grad'] == 0).all()) and bool((pot.describe(x.cuda())['rog'] == 0).all())

    # N = 2 with clash_separation 2: no eligible pair
    x = walk(3, 2, 1)
    pot = S.potential(S.config(rog_max=1.0, rog_weight=1.0, clash_distance=4.0, clash_weight=1.0), 2, abar)
    rep = pot.describe(x.cuda())
    assert bool(torch.isinf(rep['min_distance']).all()) and bool((rep['min_distance'] > 0).all()) and rep['n_clash'].tolist() == [0, 0, 0]

    # a weight of 0, or no restraints, is the oracle with that term off; the report's minimum and count stay
    x, cfg = _case(3, 65, 1)
    for off in (dict(rog_weight=0.0), dict(clash_weight=0.0), dict(restraints=[])):
        c = dict(cfg, **off)
        pot = S.potential(c, 65, abar)
        ref = _check('N=65 with %s' % off, *_run(pot, x), x, c, float(pot.variance(STEP)))
        rep = pot.describe(x.cuda())
        assert torch.equal(rep['n_clash'].cpu(), ref['n_clash']) and int(ref['n_clash'].min()) > 0
        assert bool((rep[{'rog_weight': 'e_rog', 'clash_weight': 'e_clash', 'restraints': 'e_restraint'}[next(iter(off))]] == 0).all())


def test_deterministic_and_never_synchronises():
    x, cfg = _case(3, 300, 2)
    pot = S.potential(cfg, 300, _abar())
    xc = x.cuda()
    a, b = _run(pot, xc, 400), _run(pot, xc, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ra, rb = pot.describe(xc), pot.describe(xc)
    assert all(torch.equal(ra[k], rb[k]) for k in ra)
    xg = xc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(xg, 400)
        g, = torch.autograd.grad(lp.mean(), xg)
        rep = pot.describe(xc)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.allclose(g, a[1] / 3, rtol=1e-6, atol=0)      # (the backward scales by grad_output = 1/3)
    assert all(torch.equal(rep[k], ra[k]) for k in ra)
    with pytest.raises(ValueError):
        pot(xc[:, :299], 400)
    with pytest.raises(ValueError):
        pot(x, 400)                                                                       # (a CPU tensor)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N_S = 12, 40
SAMPLER_CFG = S.config(rog_max=6.0, rog_weight=1.0, clash_distance=4.0, clash_separation=2, clash_weight=1.0,
                       restraints=[(0, 39, 0.0, 12.0, 1.0), (25, 5, 4.0, 8.0, 2.0), (10, 30, 15.0, math.inf, 1.0)])


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
        attrs = {k: getattr(sampler, k, None) for k in ('last_fit', 'last_shape', 'last_choice')}
        return np.stack([r['atom_positions'] for r in out]), sampler.resampled_at, sampler.ess_trace, attrs

    return dict(run=run, abar=abar, fused=S.potential(SAMPLER_CFG, N_S, abar), torch=S.twisting_function(SAMPLER_CFG, abar))


def _noise(B, seed):
    return torch.randn(T, B, N_S, 3, generator=torch.Generator().manual_seed(seed))


def test_sampler_follows_the_torch_path_without_resampling(ctx, tmp_path):
    B, noise = 4, _noise(4, 4)
    a, ra, _, attrs_a = ctx['run'](ctx['torch'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    b, rb, _, attrs_b = ctx['run'](ctx['fused'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    rms, d = float(np.sqrt((a ** 2).mean())), float(np.abs(a - b).max())
    print('no resampling: max |d| = %.3e, coordinate RMS = %.2f' % (d, rms))
    assert np.isfinite(b).all() and ra == rb == [] and d <= 1e-3 * rms
    assert attrs_a['last_shape'] is None and attrs_a['last_fit'] is None and attrs_b['last_fit'] is None      # a plain callable has no describe


def test_sampler_resamples_where_the_torch_path_does(ctx, tmp_path):
    B, noise, u = 4, _noise(4, 4), [0.37] * T
    a, ra, ess_a, _ = ctx['run'](ctx['torch'], noise, tmp_path, num_samples=B, ess_threshold=0.5, resample_u=u)
    gap = min(abs(e - 0.5 * B) / (0.5 * B) for e in ess_a)
    assert gap >= 1e-3, 'the ESS of the torch run comes within %.1e of the threshold: take another noise seed' % gap
    b, rb, ess_b, attrs = ctx['run'](ctx['fused'], noise, tmp_path, num_samples=B, ess_threshold=0.5, resample_u=u)
    print('resampled at', ra, rb, 'ESS', ess_a, ess_b)
    assert ra == rb and len(ra) > 0 and np.isfinite(b).all()
    shape = attrs['last_shape']
    assert set(shape) == set(S.REPORT) and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in shape.values())
    again = ctx['fused'].describe(torch.from_numpy(b).float().cuda())
    assert all(torch.equal(shape[k], again[k].cpu()) for k in shape)


def test_particle_systems_with_the_sum_of_both_potentials(ctx, tmp_path):
    from genie2_amd.smc import MotifPotential, SumPotential
    S_, K = 2, 3
    motif = MotifPotential(segments_6e6r(), N_S, ctx['abar'], rng=np.random.RandomState(0), device='cuda')
    both = SumPotential(motif, ctx['fused'])
    x = walk(S_ * K, N_S, 9).cuda()
    assert torch.equal(both(x, 5), motif(x, 5) + ctx['fused'](x, 5))
    xg = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(both(xg, 5).sum(), xg)
    g_m, g_s = torch.autograd.grad(motif(xg, 5).sum(), xg)[0], torch.autograd.grad(ctx['fused'](xg, 5).sum(), xg)[0]
    assert torch.allclose(g, g_m + g_s, rtol=1e-6, atol=0)
    noise = torch.randn(T, S_ * K, N_S, 3, generator=torch.Generator().manual_seed(11))
    best, _, ess, attrs = ctx['run'](both, noise, tmp_path, num_samples=S_, num_particles=K, ess_threshold=0.5,
                                     resample_u=[[0.05, 0.21]] * T, return_particles='best')
    assert tuple(best.shape) == (S_, N_S, 3) and np.isfinite(best).all() and tuple(ess.shape) == (T - 1, S_)
    fit, shape = attrs['last_fit'], attrs['last_shape']
    assert tuple(fit['rmsd'].shape) == (S_,) and tuple(fit['starts'].shape)[0] == S_
    assert set(shape) == set(S.REPORT) and all(tuple(v.shape) == (S_,) for v in shape.values())
    xb = torch.from_numpy(best).float().cuda()
    assert all(torch.equal(shape[k], v.cpu()) for k, v in ctx['fused'].describe(xb).items())
    assert torch.equal(fit['rmsd'], motif.locate(xb)['rmsd'].cpu()) and torch.equal(fit['best'], motif.locate(xb)['best'].cpu())


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('shape_cli') / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return root


def _check_reports(out, cfg, names):
    """Every outdir/shape file against the float64 oracle on the coordinates its PDB holds.  The PDB rounds coordinates to 1e-3 A
    (an error of at most 5e-4 per coordinate) and the report its values to three decimals (5e-4), so a value may differ from the
    oracle's on the written coordinates by 5e-4 + 5e-4 * |d value / d x|_1 (first order; taken with a factor 1.5 for the rest) plus
    the float32 bar 1e-5 max(1, |value|).  rog, min_distance and max_violation move by at most 2 sqrt(3) * 5e-4 whichever pair is the
    extreme one.  A count may differ by the number of distances within 2e-3 A of their threshold (none, for most seeds)."""
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == sorted(n + '.pdb' for n in names)
    assert sorted(os.listdir(os.path.join(out, 'shape'))) == sorted(n + '.txt' for n in names)
    for name in names:
        y = torch.tensor(_ca_coordinates(os.path.join(out, 'pdbs', name + '.pdb')), dtype=torch.float64)[None].requires_grad_(True)
        assert tuple(y.shape) == (1, N_S, 3)
        lines = [ln.split() for ln in open(os.path.join(out, 'shape', name + '.txt'))]
        assert [ln[0] for ln in lines] == list(S.REPORT) and all(len(ln) == 2 for ln in lines)
        got = {ln[0]: float(ln[1]) for ln in lines}
        t = S.terms(y, cfg)
        i, j = torch.triu_indices(N_S, N_S, offset=cfg['clash_separation'])
        d = (y[0, i] - y[0, j]).norm(dim=-1).detach()
        slack = {'n_clash': int(((d - cfg['clash_distance']).abs() < 2e-3).sum()), 'n_violated': 0}
        for a, b, lo, hi, _ in cfg['restraints']:
            dr = float((y[0, a] - y[0, b]).detach().norm())
            slack['n_violated'] += int(abs(dr - lo) < 2e-3 or abs(dr - hi) < 2e-3)
        for k in S.REPORT:
            ref = float(t[k][0].detach())
            if k in S.COUNTS:
                assert abs(got[k] - ref) <= slack[k], (name, k, got[k], ref)
            elif k in ('rog', 'min_distance', 'max_violation'):
                assert abs(got[k] - ref) <= 5e-4 + 2 * math.sqrt(3) * 5e-4 + 1e-5 * max(1.0, abs(ref)), (name, k, got[k], ref)
            else:
                l1 = float(torch.autograd.grad(t[k][0], y, retain_graph=True)[0].abs().sum()) if t[k].requires_grad else 0.0
                assert abs(got[k] - ref) <= 5e-4 + 1.5 * 5e-4 * l1 + 1e-5 * max(1.0, abs(ref)), (name, k, got[k], ref, l1)


def test_shape_cli_end_to_end(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    rfile = tmp_path / 'restraints.txt'
    rfile.write_text('# i j lo hi [weight]\n0 39 0 12\n25 5 4 8 2\n10 30 15 inf\n')
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--min_length', '40', '--max_length', '40', '--batch_size', '2', '--num_samples', '2',
                                      '--num_steps', '4', '--last_unguided_steps', '0', '--guidance_alpha', '0.05', '--rog_max', '6',
                                      '--clash_distance', '4', '--restraint_file', str(rfile), '--write_shape_report'])
    torch.manual_seed(0)
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_reports(out, SAMPLER_CFG, ['40_0', '40_1'])


def test_motif_cli_with_shape_terms_end_to_end(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--motif_file', MOTIF, '--min_length', '40', '--max_length', '40', '--batch_size', '2',
                                      '--num_samples', '2', '--num_steps', '4', '--last_unguided_steps', '0', '--rog_max', '6',
                                      '--clash_distance', '4', '--write_shape_report', '--write_motif_locations'])
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_reports(out, S.config(rog_max=6.0, rog_weight=1.0, clash_distance=4.0, clash_weight=1.0), ['40_0', '40_1'])
    assert sorted(os.listdir(os.path.join(out, 'motif_locations'))) == ['40_0.txt', '40_1.txt']
