"""The secondary-structure potential on the GPU (genie_secstruct_potential, csrc/secstruct_kernels.hip; SecStructPotential, SumPotential
in genie2_amd/smc.py) against the float64 oracle of tests/_secstruct.py, in TwistedSampler against the float32 PyTorch restatement as
its twisting function, composed with the motif and the shape potential in particle systems, and through both command lines.

Bounds (tests/_motif.py:60-72, the project's bars for a fused potential, used as in test_shape_gpu.py): logp within
1e-5 max(1, |logp|); every particle's gradient within 1e-5 of its largest reference entry; each widened, per case, to 4 x the error the
float32 restatement makes on the same input where that is larger (the kernel is held to float32 arithmetic; the factor covers another
summation order).  Report fields: counts and the assignment exactly, the rest within the logp bar.

Worst error / bound over the parity cases, measured on an MI355X: 0.090 for logp, 0.129 for the gradient, no bar widened."""
import math
import os

import numpy as np
import pytest
import torch

import _secstruct as S
from _motif import MOTIF, _abar, _tiny_model, segments_6e6r, walk

pytestmark = pytest.mark.gpu

STEP = 500
# (B, N, chain seed): one window; the first residue that sits in five windows (N = 9); the wave boundary; W and N across the
# 256-thread stride; the longest N genie_create accepts.  Seeds: every case keeps its z-scores 1e-4 from the class boxes and its soft
# counts 1e-4 from the content bounds, and from N = 24 on the oracle's assignment holds H, E and C (test_report...).
CASES = [(3, 5, 1), (3, 6, 1), (3, 8, 1), (3, 9, 1), (3, 63, 1), (3, 64, 1), (3, 65, 1), (3, 129, 1), (3, 256, 1), (3, 257, 1),
         (3, 300, 1), (1, 1512, 1)]
_cache = {}


def _case(B, N, seed, term=None):
    """(x, cfg) of a parity case; term: leave only that term on."""
    if (B, N, seed) not in _cache:
        x = S.mixed_chain(B, N, seed)
        _cache[(B, N, seed)] = (x, S.chain_config(x))
    x, cfg = _cache[(B, N, seed)]
    return x, (cfg if term is None else S.only(cfg, term))


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


def _check(what, lp, g, x, cfg, var):
    ref, r32 = _reference(x, cfg, var)
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
        assert bool((ref['e_helix'] > 0).all()) and bool((ref['e_extended'] > 0).all()) and bool((ref['e_target'] > 0).all())
        W = N - 4
        assert bool((ref['n'][:, 0] < W * cfg['helix'][0]).all()) and bool((ref['n'][:, 1] > W * cfg['extended'][1]).all())


@pytest.mark.parametrize('term', ['helix', 'extended', 'target'])
def test_each_term_alone(term):
    x, cfg = _case(3, 65, 1, term)
    pot = S.potential(cfg, 65, _abar())
    ref = _check('N=65 %s alone' % term, *_run(pot, x), x, cfg, float(pot.variance(STEP)))
    assert bool((ref['logp'] < 0).all())
    # the same term switched on through the constructor alone
    from genie2_amd.smc import SecStructPotential
    kw = {'helix': dict(helix=cfg['helix'], helix_weight=cfg['helix_weight']),
          'extended': dict(extended=cfg['extended'], extended_weight=cfg['extended_weight']),
          'target': dict(target=cfg['target'], target_weight=cfg['target_weight'])}[term]
    alone = SecStructPotential(65, _abar(), device='cuda', **kw)
    a, b = _run(pot, x), _run(alone, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_custom_table():
    """Other targets and tolerances: a 3-10-like helix class and a tighter extended class."""
    x, cfg = _case(3, 65, 1)
    table = (5.2, 5.9, 7.9, 0.6, 0.4, 0.7, 0.9, 0.3, 6.5, 9.7, 12.9, -0.2, 0.3, 0.45, 0.55, 0.2)
    cfg = S.chain_config(x, table=table)
    pot = S.potential(cfg, 65, _abar())
    ref = _check('N=65 custom table', *_run(pot, x), x, cfg, float(pot.variance(STEP)))
    base = S.reference(x, _case(3, 65, 1)[1], float(pot.variance(STEP)))
    assert not torch.allclose(ref['n'], base['n'], rtol=1e-2)             # (the table is the one in use)
    margin = S.margins(x, cfg)
    assert min(margin) >= 1e-4, 'a z-score of this case is too close to a class box: change the table'
    assert torch.equal(pot.assign(x.cuda()).cpu(), ref['assign'])


@pytest.mark.parametrize('B,N,seed', CASES)
def test_report_and_assignment_match_the_oracle(B, N, seed):
    x, cfg = _case(B, N, seed)
    box, hinge = S.margins(x, cfg)
    print('B=%d N=%d: smallest margin of a z-score to a class box %.3e, of a soft count to a content bound %.3e' % (B, N, box, hinge))
    assert box >= 1e-4 and hinge >= 1e-4, 'a count of this case could flip in float32: take another seed'
    pot = S.potential(cfg, N, _abar())
    got, assign = pot.describe(x.cuda()), pot.assign(x.cuda())
    ref, r32 = _reference(x, cfg, 1.0)
    assert assign.dtype == torch.int8 and tuple(assign.shape) == (B, N) and assign.device.type == 'cuda'
    assert torch.equal(assign.cpu(), ref['assign'])
    if N >= 24:
        assert all(sorted(set(row.tolist())) == [0, 1, 2] for row in ref['assign'])          # H, E and C all occur
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
    assert torch.equal(got['n_helix'].cpu(), (assign == 1).sum(dim=1).cpu()) and torch.equal(got['n_extended'].cpu(), (assign == 2).sum(dim=1).cpu())


def test_edges():
    abar = _abar()
    # a straight 3.8 A chain: chi is exactly 0, everything is finite and the oracle's
    N = 70
    line = torch.zeros(2, N, 3)
    line[0, :, 0] = 3.8 * torch.arange(N)
    line[1, :, 1] = 3.8 * torch.arange(N) - 20.0
    cfg = S.config(helix=(0.3, 1.0), helix_weight=1.0, extended=(0.0, 0.1), extended_weight=1.0, target=S.blueprint(N), target_weight=0.5)
    assert bool((S.features(line)[..., 3] == 0).all())
    pot = S.potential(cfg, N, abar)
    _check('a straight line', *_run(pot, line), line, cfg, float(pot.variance(STEP)))
    rep = pot.describe(line.cuda())
    assert rep['n_helix'].tolist() == [0, 0] and rep['n_extended'].tolist() == [0, 0] and bool((pot.assign(line.cuda()) == 0).all())

    # coincident residues inside a window (a distance of 0) and a bond of length 0 (chi = 0, no chi force): finite, the oracle's value
    x = S.mixed_chain(2, 24, 1)
    x[0, 7] = x[0, 5]
    x[1, 11] = x[1, 10]
    cfg = S.chain_config(S.mixed_chain(2, 24, 1))
    pot = S.potential(cfg, 24, abar)
    _check('coincident residues', *_run(pot, x), x, cfg, float(pot.variance(STEP)))
    assert torch.equal(pot.assign(x.cuda()).cpu(), S.reference(x, cfg, 1.0)['assign'])
    # every residue in one point: no direction anywhere, the gradient is exactly 0
    x = torch.ones(1, 9, 3) * 2.5
    cfg = S.config(helix=(0.5, 1.0), helix_weight=1.0, extended=(0.0, 0.01), extended_weight=1.0, target='HHHHHEEEE', target_weight=1.0)
    pot = S.potential(cfg, 9, abar)
    lp, g = _run(pot, x)
    ref = _check('one point', lp, g, x, cfg, float(pot.variance(STEP)))
    assert bool((ref['grad'] == 0).all()) and bool((g == 0).all()) and float(ref['logp']) < 0

    # a weight of 0 is the oracle with that term off, and bitwise the potential built without the term
    from genie2_amd.smc import SecStructPotential
    x, cfg = _case(3, 65, 1)
    full = dict(helix=cfg['helix'], helix_weight=cfg['helix_weight'], extended=cfg['extended'], extended_weight=cfg['extended_weight'],
                target=cfg['target'], target_weight=cfg['target_weight'])
    for off, without, field in ((dict(helix_weight=0.0), ('helix', 'helix_weight'), 'e_helix'),
                                (dict(extended_weight=0.0), ('extended', 'extended_weight'), 'e_extended'),
                                (dict(target_weight=0.0), ('target', 'target_weight'), 'e_target')):
        c = dict(cfg, **off)
        pot = S.potential(c, 65, abar)
        a = _run(pot, x)
        _check('N=65 with %s' % off, *a, x, c, float(pot.variance(STEP)))
        b = _run(SecStructPotential(65, abar, device='cuda', **{k: v for k, v in full.items() if k not in without}), x)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        rep = pot.describe(x.cuda())
        assert bool((rep[field] == 0).all()) and all(bool((rep[k] > 0).all()) for k in ('e_helix', 'e_extended', 'e_target') if k != field)
    # (the blueprint is still reported against at weight 0)
    assert torch.equal(rep['n_target_missed'].cpu(), S.reference(x, dict(cfg, target_weight=0.0), 1.0)['n_target_missed'])

    # a mirrored helix has the helix's distances and is no helix
    helix, mirror = S.ideal_helix(30).float()[None], S.ideal_helix(30, -1.0).float()[None]
    pot = SecStructPotential(30, abar, helix=(0.5, 1.0), device='cuda')
    a, b = pot.describe(helix.cuda()), pot.describe(mirror.cuda())
    assert float(a['helix_content']) > 0.8 and int(a['n_helix']) == 30 and float(a['e_helix']) == 0
    assert float(b['helix_content']) < 1 / 6 and int(b['n_helix']) == 0 and float(b['e_helix']) > 0
    assert bool((pot.assign(helix.cuda()) == 1).all()) and bool((pot.assign(mirror.cuda()) == 0).all())
    assert float(pot(helix.cuda(), STEP)) == 0 and float(pot(mirror.cuda(), STEP)) < 0


def test_deterministic_and_never_synchronises():
    x, cfg = _case(3, 300, 1)
    pot = S.potential(cfg, 300, _abar())
    xc = x.cuda()
    a, b = _run(pot, xc, 400), _run(pot, xc, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ra, rb = pot.describe(xc), pot.describe(xc)
    sa, sb = pot.assign(xc), pot.assign(xc)
    assert all(torch.equal(ra[k], rb[k]) for k in ra) and torch.equal(sa, sb)
    xg = xc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(xg, 400)
        g, = torch.autograd.grad(lp.mean(), xg)
        rep = pot.describe(xc)
        sc = pot.assign(xc)
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
SAMPLER_CFG = S.config(helix=(0.5, 1.0), helix_weight=1.0, extended=(0.0, 0.05), extended_weight=1.0, target=S.blueprint(N_S),
                       target_weight=0.2)


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
        attrs = {k: getattr(sampler, k, None) for k in ('last_fit', 'last_shape', 'last_secstruct', 'last_choice')}
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
    assert attrs_a['last_shape'] is None and attrs_a['last_secstruct'] is None and attrs_a['last_fit'] is None      # a plain callable
    assert attrs_b['last_fit'] is None
    again = ctx['fused'].assign(torch.from_numpy(b).float().cuda())
    assert attrs_b['last_secstruct'].device.type == 'cpu' and torch.equal(attrs_b['last_secstruct'], again.cpu())


def test_sampler_resamples_where_the_torch_path_does(ctx, tmp_path):
    # (noise seed 5: with seed 4 two copies of one resampled ancestor tie at step 6 and the ESS is 1.99988, on the threshold)
    B, noise, u = 4, _noise(4, 5), [0.37] * T
    a, ra, ess_a, _ = ctx['run'](ctx['torch'], noise, tmp_path, num_samples=B, ess_threshold=0.5, resample_u=u)
    gap = min(abs(e - 0.5 * B) / (0.5 * B) for e in ess_a)
    assert gap >= 1e-3, 'the ESS of the torch run comes within %.1e of the threshold: take another noise seed' % gap
    b, rb, ess_b, attrs = ctx['run'](ctx['fused'], noise, tmp_path, num_samples=B, ess_threshold=0.5, resample_u=u)
    print('resampled at', ra, rb, 'ESS', ess_a, ess_b)
    assert ra == rb and len(ra) > 0 and np.isfinite(b).all()
    report, assign = attrs['last_shape'], attrs['last_secstruct']
    assert tuple(report) == S.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    xb = torch.from_numpy(b).float().cuda()
    again = ctx['fused'].describe(xb)
    assert all(torch.equal(report[k], again[k].cpu()) for k in report)
    assert assign.dtype == torch.int8 and tuple(assign.shape) == (B, N_S) and torch.equal(assign, ctx['fused'].assign(xb).cpu())


def test_particle_systems_with_the_sum_of_three_potentials(ctx, tmp_path):
    import _shape as Sh
    from genie2_amd.smc import MotifPotential, ShapePotential, SumPotential
    S_, K = 2, 3
    motif = MotifPotential(segments_6e6r(), N_S, ctx['abar'], rng=np.random.RandomState(0), device='cuda')
    shape = ShapePotential(N_S, ctx['abar'], rog_max=6.0, clash_distance=4.0, device='cuda')
    all3 = SumPotential(motif, shape, ctx['fused'])
    x = walk(S_ * K, N_S, 9).cuda()
    assert torch.equal(all3(x, 5), (motif(x, 5) + shape(x, 5)) + ctx['fused'](x, 5))
    xg = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(all3(xg, 5).sum(), xg)
    parts = [torch.autograd.grad(m(xg, 5).sum(), xg)[0] for m in (motif, shape, ctx['fused'])]
    assert torch.allclose(g, (parts[0] + parts[1]) + parts[2], rtol=1e-6, atol=1e-6 * float(g.abs().max()))
    noise = torch.randn(T, S_ * K, N_S, 3, generator=torch.Generator().manual_seed(11))
    best, _, ess, attrs = ctx['run'](all3, noise, tmp_path, num_samples=S_, num_particles=K, ess_threshold=0.5,
                                     resample_u=[[0.05, 0.21]] * T, return_particles='best')
    assert tuple(best.shape) == (S_, N_S, 3) and np.isfinite(best).all() and tuple(ess.shape) == (T - 1, S_)
    fit, report, assign = attrs['last_fit'], attrs['last_shape'], attrs['last_secstruct']
    assert fit is not None and tuple(fit['rmsd'].shape) == (S_,)
    assert tuple(report) == Sh.REPORT + S.REPORT and all(tuple(v.shape) == (S_,) for v in report.values())      # member order
    xb = torch.from_numpy(best).float().cuda()
    assert all(torch.equal(report[k], v.cpu()) for k, v in shape.describe(xb).items())
    assert all(torch.equal(report[k], v.cpu()) for k, v in ctx['fused'].describe(xb).items())
    assert tuple(assign.shape) == (S_, N_S) and torch.equal(assign, ctx['fused'].assign(xb).cpu())
    assert torch.equal(fit['rmsd'], motif.locate(xb)['rmsd'].cpu())


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('secstruct_cli') / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return root


def _check_secstruct_files(out, names, target=None):
    """Every outdir/secstruct file: an assignment line over HEC of the structure's length, then the eight report fields, the counts
    consistent with the assignment line (and with the blueprint, when there is one)."""
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == sorted(n + '.pdb' for n in names)
    assert sorted(os.listdir(os.path.join(out, 'secstruct'))) == sorted(n + '.txt' for n in names)
    for name in names:
        lines = open(os.path.join(out, 'secstruct', name + '.txt')).read().splitlines()
        ss, fields = lines[0], [ln.split() for ln in lines[1:]]
        assert len(ss) == N_S and set(ss) <= set('HEC'), (name, ss)
        assert [f[0] for f in fields] == list(S.REPORT) and all(len(f) == 2 for f in fields)
        got = {f[0]: f[1] for f in fields}
        assert all('.' not in got[k] for k in S.COUNTS) and all('.' in got[k] for k in S.REPORT if k not in S.COUNTS)
        assert int(got['n_helix']) == ss.count('H') and int(got['n_extended']) == ss.count('E')
        missed = 0 if target is None else sum(1 for t, s in zip(target, ss) if t in 'HE' and t != s)
        assert int(got['n_target_missed']) == missed
        assert 0.0 <= float(got['helix_content']) <= 1.0 and 0.0 <= float(got['extended_content']) <= 1.0
        assert all(float(got[k]) >= 0 for k in ('e_helix', 'e_extended', 'e_target'))
        if target is None:
            assert float(got['e_target']) == 0


def test_shape_cli_with_a_helix_minimum_end_to_end(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--min_length', '40', '--max_length', '40', '--batch_size', '2', '--num_samples', '2',
                                      '--num_steps', '4', '--last_unguided_steps', '0', '--guidance_alpha', '0.05', '--helix_min', '0.5',
                                      '--write_secstruct'])
    torch.manual_seed(0)
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_secstruct_files(out, ['40_0', '40_1'])
    assert not os.path.exists(os.path.join(out, 'shape'))


def test_motif_cli_with_a_blueprint_and_shape_terms_end_to_end(tmp_path, checkpoint_root):
    import _shape as Sh
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    out = str(tmp_path / 'out')
    bp = tmp_path / 'blueprint.txt'
    bp.write_text('# 40 residues\n' + 'H' * 12 + '\nCC--\n' + 'E' * 8 + '\n' + '-' * 16 + '\n')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--motif_file', MOTIF, '--min_length', '39', '--max_length', '40', '--batch_size', '2',
                                      '--num_samples', '2', '--num_steps', '4', '--last_unguided_steps', '0', '--ss_target', str(bp),
                                      '--rog_max', '6', '--write_shape_report', '--write_secstruct', '--write_motif_locations'])
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    names = ['40_0', '40_1']                                                                  # (length 39 is not the blueprint's: skipped)
    _check_secstruct_files(out, names, 'H' * 12 + '----' + 'E' * 8 + '-' * 16)
    assert sorted(os.listdir(os.path.join(out, 'shape'))) == sorted(n + '.txt' for n in names)
    for name in names:
        lines = [ln.split() for ln in open(os.path.join(out, 'shape', name + '.txt'))]
        assert [ln[0] for ln in lines] == list(Sh.REPORT) and all(len(ln) == 2 for ln in lines)      # exactly the eight old keys
    assert sorted(os.listdir(os.path.join(out, 'motif_locations'))) == sorted(n + '.txt' for n in names)
