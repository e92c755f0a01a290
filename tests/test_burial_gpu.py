"""The burial potential on the GPU (genie_burial_potential, csrc/burial_kernels.hip; BurialPotential in genie2_amd/smc.py) against the
float64 oracle of tests/_burial.py, in TwistedSampler against the float32 PyTorch restatement as its twisting function, summed with
the shape potential in particle systems, and through both command lines.

Bounds (tests/_motif.py:60-72, the project's bars for a fused potential, used as in test_shape_gpu.py): logp within 1e-5
max(1, |logp|); every particle's gradient within 1e-5 of its largest float64 entry; every report value and every c_n of burial_of
inside the logp bar, 1e-5 max(1, |value|); each widened, per case, to 4 x the error the float32 restatement makes on the same input
where that is larger (the kernel is held to float32 arithmetic; the factor covers another summation order); the count exactly.
Inputs are those of tests/_burial.py, chosen by the oracle alone: on each the float64 side asserts that no targeted c_n is within
1e-4 of one of its bounds.

Worst error / bound over the ten parity cases, measured on an MI355X: 0.022 for logp ((3, 300)), 0.098 for the gradient ((3, 63)),
0.191 for burial_of ((1, 1512)), 0.009 / 0.010 / 0.022 for burial_mean, burial_min and burial_max, 0.013 for max_burial_violation,
0.026 / 0.105 for the target and the mean energy; no bar was widened there and every count was equal.  Over all tests: 0.298 for
logp (one target at n = 64, its bar x 4.0 by the restatement's own error on that single hinge), 0.296 for the gradient (the
straight chain, unwidened) (DESIGN.md 7.13 has the table per case)."""
import math
import os

import numpy as np
import pytest
import torch

import _burial as Bu
from _motif import MOTIF, _abar, _ca_coordinates, _tiny_model, walk
from _parity import hard_time_limit

pytestmark = pytest.mark.gpu

STEP = 500
_cache = {}


@pytest.fixture(autouse=True)
def _limit():
    with hard_time_limit(300):
        yield


def _inputs(case, **kw):
    """(x, cfg) of a parity case, made once."""
    key = (case, repr(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = Bu.inputs(case, **kw)
    return _cache[key]


def _reference(x, cfg, var):
    """The oracle and the float32 restatement of an input, computed once and left unchanged."""
    key = ('ref', x.data_ptr(), repr(sorted(cfg.items())), var)
    if key not in _cache:
        _cache[key] = (x, Bu.reference(x, cfg, var), Bu.restatement32(x, cfg, var))      # (x kept: its data_ptr stays its own)
    return _cache[key][1:]


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


def _check(what, lp, g, ref, r32):
    lp, g = lp.double().cpu(), g.double().cpu()
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), what
    lp_b = 1e-5 * ref['logp'].abs().clamp(min=1.0)
    wide = _widen((r32['logp'].double().cpu() - ref['logp']).abs(), lp_b)
    d_lp = (lp - ref['logp']).abs()
    print('%s: logp error / bound %.3f (bar widened x%.2f)' % (what, _ratio(d_lp, lp_b * wide), wide))
    assert bool((d_lp <= lp_b * wide).all()), (what, lp, ref['logp'])
    g_b = 1e-5 * ref['grad'].abs().amax(dim=(1, 2))
    wide = _widen((r32['grad'].double().cpu() - ref['grad']).abs().amax(dim=(1, 2)), g_b)
    d_g = (g - ref['grad']).abs().amax(dim=(1, 2))
    print('%s: gradient error / bound %.3f (bar widened x%.2f)' % (what, _ratio(d_g, g_b * wide), wide))
    assert bool((d_g <= g_b * wide).all()), (what, d_g, g_b)


def _check_report(what, pot, x, cfg, ref, r32):
    m = Bu.margins(x, cfg)
    assert m >= 1e-4, '%s: a targeted residue is %.1e from a bound: take another seed' % (what, m)
    got = pot.describe(x.cuda())
    assert tuple(got) == Bu.REPORT
    got['burial'] = pot.burial_of(x.cuda())
    assert tuple(got['burial'].shape) == tuple(x.shape[:2])
    for k in Bu.REPORT + ('burial',):
        assert tuple(got[k].shape) == tuple(ref[k].shape) and got[k].device.type == 'cuda', k
        if k in Bu.COUNTS:
            assert got[k].dtype == torch.int64 and torch.equal(got[k].cpu(), ref[k]), (what, k, got[k], ref[k])
            continue
        v, r = got[k].double().cpu().reshape(-1), ref[k].reshape(-1)
        assert got[k].dtype == torch.float32
        bound = 1e-5 * r.abs().clamp(min=1.0)
        wide = _widen((r32[k].double().cpu().reshape(-1) - r).abs(), bound)
        print('%s: %s error / bound %.3f (bar widened x%.2f)' % (what, k, _ratio((v - r).abs(), bound * wide), wide))
        assert bool(torch.isfinite(v).all()) and bool(((v - r).abs() <= bound * wide).all()), (what, k, v, r)


def _parity(what, x, cfg, report=True):
    pot = Bu.potential(cfg, x.shape[1], _abar())
    ref, r32 = _reference(x, cfg, float(pot.variance(STEP)))
    lp, g = _run(pot, x)
    _check(what, lp, g, ref, r32)
    if report:
        _check_report(what, pot, x, cfg, ref, r32)
    return pot, ref, lp, g


@pytest.mark.parametrize('case', Bu.CASES, ids=Bu.case_id)
def test_potential_and_report_match_the_float64_oracle(case):
    """No interior residue (N = 1, 2), one (N = 3), fewer residues than `separation` allows pairs (N <= 3), below / at / above the
    64-residue tile, several tiles, and the longest length the model accepts."""
    x, cfg = _inputs(case)
    _, ref, _, _ = _parity(Bu.case_id(case), x, cfg)
    assert bool((ref['logp'] < 0).all())
    if case[1] >= 65:
        assert float(ref['e_burial_target'][0]) > 0 and float(ref['e_burial_mean'][0]) > 0      # both terms act on the particle that set them


@pytest.mark.parametrize('term', ['target', 'mean'])
def test_each_term_alone(term):
    x, cfg = _inputs(Bu.CASES[6])
    _, ref, _, g = _parity('%s alone' % term, x, Bu.only(cfg, term))
    other = 'e_burial_mean' if term == 'target' else 'e_burial_target'
    assert bool((ref[other] == 0).all()) and float(ref['e_burial_' + term][0]) > 0 and float(g.abs().max()) > 0


@pytest.mark.parametrize('n', [63, 64])
def test_one_target_whose_stencil_straddles_a_tile_edge(n):
    """N = 130: residues 63 and 64 sit on either side of the first tile's edge, so the targeted residue's k v reaches a residue of
    the other tile."""
    x = walk(2, 130, 130 + n)
    c = Bu.counts(x.double(), Bu.config())[:, n]
    cfg = Bu.config(targets=[(n, round(float(c.max()) + 2.0, 3), math.inf, 1.5)])
    _, ref, _, g = _parity('one target at %d' % n, x, cfg)
    assert ref['n_burial_violated'].tolist() == [1, 1]
    assert all(float(g[:, i].abs().max()) > 0 for i in (n - 1, n, n + 1, 0, 129))
    assert float(g[:, n - 2].abs().max()) == 0 and float(g[:, n + 2].abs().max()) == 0      # inside the separation window, outside the stencil


def test_edges():
    abar = _abar()
    # nothing violated: logp and the gradient are exactly 0
    x, cfg = _inputs(Bu.CASES[6])
    idle = Bu.config(targets=[(i, 0.0, math.inf if i % 2 else 1e4, w) for i, _, _, w in cfg['targets']], mean_min=0.0, mean_max=1e4, mean_weight=1.0)
    lp, g = _run(Bu.potential(idle, 65, abar), x)
    assert bool((lp == 0).all()) and bool((g == 0).all())

    # the straight chain (to float32's rounding of the coordinates: b_n ~ 1e-6 A against eps = 0.1 A): finite, and the oracle's
    line = torch.zeros(2, 65, 3)
    line[:, :, 0] = 3.8 * torch.arange(65, dtype=torch.float32)
    line[1] = line[1] @ torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(3)))[0].T
    cfg_line = Bu.config(targets=[(4, 2.0, math.inf, 1.0), (30, 0.0, 0.5, 2.0), (64, 0.0, 0.25, 1.0)], mean_min=3.0, mean_weight=1.0)
    pot, ref, _, g = _parity('the straight chain', line, cfg_line)
    assert float(g.abs().max()) > 0 and float(ref['burial'].max()) < 0.5 and float(ref['e_burial_mean'].min()) > 0

    # two coincident residues, and all residues of a particle in one point (c_n = half the eligible residues, gradient exactly 0)
    x = _inputs(Bu.CASES[6])[0].clone()
    x[0, 7] = x[0, 20]
    x[1, 40] = x[1, 41]
    x[2] = x[2, 5]
    cfg_c = Bu.walk_config(x, 11)
    pot, ref, lp, g = _parity('coincident residues', x, cfg_c)
    assert bool((g[2] == 0).all()) and float(ref['burial'][2, 0]) == 0.5 * 62 and float(ref['burial'][2, 30]) == 0.5 * 60
    assert torch.equal(pot.burial_of(x.cuda())[2].cpu(), ref['burial'][2].float())

    # N = 2 with lo > 0: no pair at separation 3, c = 0, the energy is the constant w lo^2 and the gradient exactly 0
    x2 = walk(3, 2, 2)
    pot = Bu.potential(Bu.config(targets=[(1, 1.5, math.inf, 2.0)]), 2, abar)
    lp, g = _run(pot, x2)
    want = torch.full((3,), -2.0 * 1.5 ** 2 / (2 * float(pot.variance(STEP))), dtype=torch.float64)
    assert torch.allclose(lp.double().cpu(), want, rtol=1e-6, atol=0) and bool((g == 0).all())
    rep = pot.describe(x2.cuda())
    assert rep['n_burial_violated'].tolist() == [1, 1, 1] and bool((rep['max_burial_violation'] == 1.5).all()) and bool((rep['burial_max'] == 0).all())

    # a weight of 0, or no table, is the oracle with that term off
    x, cfg = _inputs(Bu.CASES[6])
    zero = dict(cfg, targets=[(i, lo, hi, 0.0) for i, lo, hi, _ in cfg['targets']])
    for what, c in (('every target weight 0', zero), ('no table', Bu.only(cfg, 'mean')), ('mean_weight 0', Bu.only(cfg, 'target'))):
        pot, ref, _, _ = _parity(what, x, c, report=False)
        rep = pot.describe(x.cuda())
        off = 'e_burial_mean' if what == 'mean_weight 0' else 'e_burial_target'
        assert bool((rep[off] == 0).all()) and bool((ref[off] == 0).all())
        if what != 'mean_weight 0':
            assert rep['n_burial_violated'].tolist() == [0, 0, 0] and bool((rep['max_burial_violation'] == 0).all())
    assert Bu.potential(Bu.only(cfg, 'mean'), 65, abar).table == (None, None, None)


def test_deterministic_and_never_synchronises():
    x, cfg = _inputs(Bu.CASES[8])
    pot = Bu.potential(cfg, 300, _abar())
    xc = x.cuda()
    a, b = _run(pot, xc, 400), _run(pot, xc, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ra, rb = pot.describe(xc), pot.describe(xc)
    assert all(torch.equal(ra[k], rb[k]) for k in ra)
    ca = pot.burial_of(xc)
    assert torch.equal(ca, pot.burial_of(xc))
    xg = xc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(xg, 400)
        g, = torch.autograd.grad(lp.mean(), xg)
        rep = pot.describe(xc)
        c = pot.burial_of(xc)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.allclose(g, a[1] / 3, rtol=1e-6, atol=0)      # (the backward scales by grad_output = 1/3)
    assert all(torch.equal(rep[k], ra[k]) for k in ra) and torch.equal(c, ca)
    with pytest.raises(ValueError):
        pot(xc[:, :299], 400)
    with pytest.raises(ValueError):
        pot(x, 400)                                                                       # (a CPU tensor)
    with pytest.raises(ValueError):
        pot.burial_of(x)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N_S = 12, 40
SAMPLER_CFG = Bu.config(targets=[(10, 8.0, math.inf, 1.0), (11, 8.0, math.inf, 1.0), (25, 9.0, math.inf, 2.0)] + [(i, 0.0, 2.0, 1.0) for i in range(5, 10)],
                        mean_min=6.0, mean_max=10.0, mean_weight=1.0)


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
        attrs = {k: getattr(sampler, k, None) for k in ('last_fit', 'last_shape', 'last_choice', 'last_positions')}
        return np.stack([r['atom_positions'] for r in out]), sampler.resampled_at, sampler.ess_trace, attrs

    return dict(run=run, abar=abar, fused=Bu.potential(SAMPLER_CFG, N_S, abar), torch=Bu.twisting_function(SAMPLER_CFG, abar))


def _noise(B, seed):
    return torch.randn(T, B, N_S, 3, generator=torch.Generator().manual_seed(seed))


def test_sampler_follows_the_torch_path_without_resampling(ctx, tmp_path):
    B, noise = 4, _noise(4, 4)
    a, ra, _, attrs_a = ctx['run'](ctx['torch'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    b, rb, _, attrs_b = ctx['run'](ctx['fused'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    rms, d = float(np.sqrt((a ** 2).mean())), float(np.abs(a - b).max())
    print('no resampling: max |d| = %.3e, coordinate RMS = %.2f, ratio %.3e' % (d, rms, d / rms))
    assert np.isfinite(b).all() and ra == rb == [] and d <= 1e-3 * rms
    assert attrs_a['last_shape'] is None and attrs_b['last_fit'] is None                 # a plain callable has no describe
    report = attrs_b['last_shape']
    print('report of the guided samples', {k: v.tolist() for k, v in report.items()})
    assert tuple(report) == Bu.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    again = ctx['fused'].describe(torch.from_numpy(b).float().cuda())
    assert all(torch.equal(report[k], again[k].cpu()) for k in report)


def test_sampler_resamples_where_the_torch_path_does(ctx, tmp_path):
    B, noise, u = 4, _noise(4, 4), [0.37] * T
    a, ra, ess_a, _ = ctx['run'](ctx['torch'], noise, tmp_path, num_samples=B, ess_threshold=0.5, resample_u=u)
    gap = min(abs(e - 0.5 * B) / (0.5 * B) for e in ess_a)
    assert gap >= 1e-3, 'the ESS of the torch run comes within %.1e of the threshold: take another noise seed' % gap
    b, rb, ess_b, attrs = ctx['run'](ctx['fused'], noise, tmp_path, num_samples=B, ess_threshold=0.5, resample_u=u)
    print('resampled at', ra, rb, 'ESS', ess_a, ess_b)
    assert ra == rb and len(ra) > 0 and np.isfinite(b).all()
    report = attrs['last_shape']
    assert tuple(report) == Bu.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    again = ctx['fused'].describe(torch.from_numpy(b).float().cuda())
    assert all(torch.equal(report[k], again[k].cpu()) for k in report)


def test_particle_systems_with_the_sum_of_shape_and_burial(ctx, tmp_path):
    import _shape as Sh
    from genie2_amd.smc import ShapePotential, SumPotential
    S_, K = 2, 3
    shape = ShapePotential(N_S, ctx['abar'], rog_max=6.0, clash_distance=4.0, device='cuda')
    both = SumPotential(shape, ctx['fused'])
    x = walk(S_ * K, N_S, 9).cuda()
    assert torch.equal(both(x, 5), shape(x, 5) + ctx['fused'](x, 5))      # bitwise the sum of its members
    xg = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(both(xg, 5).sum(), xg)
    parts = [torch.autograd.grad(m(xg, 5).sum(), xg)[0] for m in (shape, ctx['fused'])]
    assert torch.equal(g, parts[0] + parts[1]) and float(parts[1].abs().max()) > 0
    noise = torch.randn(T, S_ * K, N_S, 3, generator=torch.Generator().manual_seed(11))
    best, _, ess, attrs = ctx['run'](both, noise, tmp_path, num_samples=S_, num_particles=K, ess_threshold=0.5, resample_u=[[0.05, 0.21]] * T,
                                     return_particles='best')
    assert tuple(best.shape) == (S_, N_S, 3) and np.isfinite(best).all() and tuple(ess.shape) == (T - 1, S_)
    report = attrs['last_shape']
    assert tuple(report) == Sh.REPORT + Bu.REPORT and all(tuple(v.shape) == (S_,) for v in report.values())      # member order, S rows
    xb = torch.from_numpy(best).float().cuda()
    for m in (shape, ctx['fused']):
        assert all(torch.equal(report[k], v.cpu()) for k, v in m.describe(xb).items())
    assert tuple(attrs['last_positions'].shape) == (S_, N_S, 3)


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('burial_cli') / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return root


BURIAL_FLAGS = ['--expose', '5-9', '--expose_max', '2', '--burial_mean_min', '6', '--write_burial']
CLI_CFG = Bu.config(targets=[(i, 0.0, 2.0, 1.0) for i in range(5, 10)], mean_min=6.0, mean_weight=1.0)


def _check_burial_files(out, names):
    """Every outdir/burial file against the float64 oracle on the coordinates its PDB holds.  The PDB rounds coordinates to 1e-3 A (an
    error of at most 5e-4 per coordinate) and the report its values to three decimals (5e-4), so a value may differ from the oracle's
    on the written coordinates by 5e-4 + 5e-4 |d value / d x|_1 (first order; taken with a factor 1.5 for the rest) plus the float32
    bar 1e-5 max(1, |value|): test_shape_gpu._check_reports' bar.  The count may differ by the number of targeted c_n within that bar
    of a bound."""
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == sorted(n + '.pdb' for n in names)
    assert sorted(os.listdir(os.path.join(out, 'burial'))) == sorted(n + '.txt' for n in names)
    ranges = {i: ('%g' % lo, '%g' % hi) for i, lo, hi, _ in CLI_CFG['targets']}

    def bar(value, y):
        l1 = float(torch.autograd.grad(value, y, retain_graph=True)[0].abs().sum()) if value.requires_grad else 0.0
        return 5e-4 + 1.5 * 5e-4 * l1 + 1e-5 * max(1.0, abs(float(value.detach())))

    for name in names:
        y = torch.tensor(_ca_coordinates(os.path.join(out, 'pdbs', name + '.pdb')), dtype=torch.float64)[None].requires_grad_(True)
        assert tuple(y.shape) == (1, N_S, 3)
        lines = [ln.split() for ln in open(os.path.join(out, 'burial', name + '.txt'))]
        rows, fields = lines[:N_S], lines[N_S:]
        assert [f[0] for f in fields] == list(Bu.REPORT) and all(len(f) == 2 for f in fields)
        assert all(('.' in f[1]) == (f[0] not in Bu.COUNTS) for f in fields)
        t = Bu.terms(y, CLI_CFG)
        slack = 0
        for n, row in enumerate(rows):
            assert row[:2] == ['residue', str(n)] and len(row) == 5 and tuple(row[3:]) == ranges.get(n, ('-', '-')), (name, row)
            c = t['burial'][0, n]
            tol = bar(c, y)
            assert abs(float(row[2]) - float(c.detach())) <= tol, (name, n, row, float(c.detach()), tol)
            if n in ranges:
                slack += int(abs(float(c.detach()) - 2.0) <= tol)
        got = {f[0]: float(f[1]) for f in fields}
        for k in Bu.REPORT:
            ref = float(t[k][0].detach())
            if k in Bu.COUNTS:
                assert abs(got[k] - ref) <= slack, (name, k, got[k], ref, slack)
            else:
                tol = bar(t[k][0], y)
                assert abs(got[k] - ref) <= tol, (name, k, got[k], ref, tol)
        print(name, got)


def test_shape_cli_with_a_burial_term_end_to_end(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--min_length', '40', '--max_length', '40', '--batch_size', '2', '--num_samples', '2',
                                      '--num_steps', '4', '--last_unguided_steps', '0', '--guidance_alpha', '0.05'] + BURIAL_FLAGS)
    torch.manual_seed(0)
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_burial_files(out, ['40_0', '40_1'])
    assert not any(os.path.exists(os.path.join(out, d)) for d in ('shape', 'secstruct', 'sheet', 'symmetry', 'binder', 'fold'))


def test_motif_cli_with_a_burial_term_end_to_end(tmp_path, checkpoint_root):
    import _shape as Sh
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--motif_file', MOTIF, '--min_length', '40', '--max_length', '40', '--batch_size', '2',
                                      '--num_samples', '2', '--num_steps', '4', '--last_unguided_steps', '0', '--rog_max', '8',
                                      '--write_shape_report'] + BURIAL_FLAGS)
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_burial_files(out, ['40_0', '40_1'])
    for name in ('40_0', '40_1'):
        lines = [ln.split() for ln in open(os.path.join(out, 'shape', name + '.txt'))]
        assert [ln[0] for ln in lines] == list(Sh.REPORT)                # exactly its own keys
