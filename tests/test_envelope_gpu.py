"""The envelope potential on the GPU (genie_envelope_potential, csrc/envelope_kernels.hip; EnvelopePotential in genie2_amd/smc.py)
against the float64 oracle of tests/_envelope.py, in TwistedSampler against the float32 PyTorch restatement as its twisting function,
summed with the shape potential in particle systems, and through both command lines.

Bounds (tests/_motif.py:60-72, the project's bars for a fused potential, used as in test_burial_gpu.py): logp within 1e-5
max(1, |logp|); every particle's gradient within 1e-5 of its largest float64 entry; every report value, every a_n of distance_of and
every c_m of gap_of inside the logp bar, 1e-5 max(1, |value|); each widened, per case, to 4 x the error the float32 restatement makes
on the same input where that is larger (the kernel is held to float32 arithmetic; the factor covers another summation order); the
counts exactly.  Inputs are those of tests/_envelope.py, chosen by the oracle alone: on each the float64 side asserts that no a_n is
within 1e-4 of inside_distance and no c_m within 1e-4 of cover_distance.

Every test prints its error / bound.  Measured on an MI355X over the twenty parity cases: where no bar was widened the worst are 0.085
for logp, 0.382 for the gradient ((3, 64, 257)), 0.229 for distance_of and 0.371 for gap_of; seven gradient bars and one gap_of bar
were widened, all but one by less than 1.75; the gradient of (1, 1025, 257) has its bar x 32 (the restatement is 8.0 unwidened bars
off on that input, the kernel 8.0: float32's q at 100 A and more); every count was equal (DESIGN.md 7.14 has the table per case)."""
import math
import os

import numpy as np
import pytest
import torch

import _envelope as En
from _motif import MOTIF, _abar, _tiny_model, walk
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
        _cache[key] = En.inputs(case, **kw)
    return _cache[key]


def _reference(x, cfg, var):
    """The oracle and the float32 restatement of an input, computed once and left unchanged."""
    key = ('ref', x.data_ptr(), En.cfg_key(cfg), var)
    if key not in _cache:
        _cache[key] = (x, En.reference(x, cfg, var), En.restatement32(x, cfg, var))      # (x kept: its data_ptr stays its own)
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
    m = En.margins(x, cfg)
    assert m >= 1e-4, '%s: a soft distance is %.1e from its bound: take another seed' % (what, m)
    got = pot.describe(x.cuda())
    assert tuple(got) == En.REPORT
    got['distance'], got['gap'] = pot.distance_of(x.cuda()), pot.gap_of(x.cuda())
    assert tuple(got['distance'].shape) == tuple(x.shape[:2]) and tuple(got['gap'].shape) == (x.shape[0], len(cfg['points']))
    for k in En.REPORT + ('distance', 'gap'):
        assert tuple(got[k].shape) == tuple(ref[k].shape) and got[k].device.type == 'cuda', k
        if k in En.COUNTS:
            assert got[k].dtype == torch.int64 and torch.equal(got[k].cpu(), ref[k]), (what, k, got[k], ref[k])
            continue
        v, r = got[k].double().cpu().reshape(-1), ref[k].reshape(-1)
        assert got[k].dtype == torch.float32
        bound = 1e-5 * r.abs().clamp(min=1.0)
        wide = _widen((r32[k].double().cpu().reshape(-1) - r).abs(), bound)
        print('%s: %s error / bound %.3f (bar widened x%.2f)' % (what, k, _ratio((v - r).abs(), bound * wide), wide))
        assert bool(torch.isfinite(v).all()) and bool(((v - r).abs() <= bound * wide).all()), (what, k, v, r)


def _parity(what, x, cfg, report=True):
    pot = En.potential(cfg, x.shape[1], _abar())
    assert torch.equal(pot.points.cpu().double(), cfg['points'])                        # the envelope as placed is the oracle's
    ref, r32 = _reference(x, cfg, float(pot.variance(STEP)))
    lp, g = _run(pot, x)
    _check(what, lp, g, ref, r32)
    if report:
        _check_report(what, pot, x, cfg, ref, r32)
    return pot, ref, lp, g


@pytest.mark.parametrize('case', En.CASES, ids=En.case_id)
def test_potential_and_report_match_the_float64_oracle(case):
    """The five specified cases (below / at / above the 64-row tile on either side, several tiles, the longest length the model accepts
    against 4169 points), one residue against one point, fewer rows than a wave's quarter of a chunk (N = 2, M = 3), N and M at
    GENIE_ENVELOPE_CHUNK - 1, at it and one above, random point weights, and batches on either side of GENIE_ENVELOPE_FILL work-groups,
    from which a launch runs 4 waves per work-group instead of 16 (once for the soft minima, once for the gather, once over two chunks)."""
    x, cfg = _inputs(case)
    _, ref, _, _ = _parity(En.case_id(case), x, cfg)
    if case[1] >= 2:
        assert bool((ref['logp'] < 0).all()) and float(ref['e_envelope_inside'].max()) > 0 and float(ref['e_envelope_cover'].max()) > 0
    assert (cfg['weights'] is not None) == case[6]


def test_a_particle_300_angstrom_away_stays_finite_and_at_parity():
    """Where a design is at high noise: every exp(-q / tau) underflows (q / tau > 2e4) unless the running minimum is subtracted."""
    x, cfg = _inputs(En.CASES[1])
    far = (x + torch.tensor([300.0, 0.0, 0.0])).contiguous()
    _, ref, lp, g = _parity('300 A away', far, cfg)
    assert ref['n_outside'].tolist() == [65] * 3 and float(ref['max_outside'].min()) > 250 and float(g.abs().max()) > 0


def test_edges():
    abar = _abar()
    x, cfg = _inputs(En.CASES[1])
    # a particle lying entirely on envelope points: E_inside = 0 and that term's gradient exactly 0; the cover term still acts
    on = cfg['points'][None, 40:105].float().repeat(2, 1, 1).contiguous()
    inside_only = dict(cfg, cover_weight=0.0)
    pot, ref, lp, g = _parity('on the points, inside term alone', on, inside_only)
    assert bool((lp == 0).all()) and bool((g == 0).all()) and bool((pot.describe(on.cuda())['e_envelope_inside'] == 0).all())
    pot, ref, lp, g = _parity('on the points, both terms', on, cfg)
    rep = pot.describe(on.cuda())
    assert bool((rep['e_envelope_inside'] == 0).all()) and rep['n_outside'].tolist() == [0, 0] and float(rep['e_envelope_cover'].min()) > 0
    assert float(g.abs().max()) > 0 and bool((pot.distance_of(on.cuda()) == float(np.sqrt(np.float32(En.EPS) * np.float32(En.EPS)))).all())

    # residues coinciding with points (q = 0) among others that do not
    mixed = x.clone()
    mixed[0, 7], mixed[1, 64], mixed[2, 0] = cfg['points'][17].float(), cfg['points'][252].float(), cfg['points'][0].float()
    _parity('coincident residues', mixed, cfg)

    # either weight 0: that term's report energy is 0, the other term's is the bits of the run with both on
    both = En.potential(cfg, 65, abar).describe(x.cuda())
    for off, on_key, c in (('e_envelope_cover', 'e_envelope_inside', dict(cfg, cover_weight=0.0)),
                           ('e_envelope_inside', 'e_envelope_cover', dict(cfg, inside_weight=0.0))):
        pot, ref, lp, g = _parity('%s off' % off, x, c)
        rep = pot.describe(x.cuda())
        assert bool((rep[off] == 0).all()) and bool((ref[off] == 0).all()) and torch.equal(rep[on_key], both[on_key]) and float(rep[on_key].min()) > 0
        assert all(torch.equal(rep[k], both[k]) for k in ('n_outside', 'max_outside', 'n_uncovered', 'max_uncovered'))
        lp_want = -rep[on_key] / (2 * pot.variance(STEP))
        assert torch.allclose(lp, lp_want, rtol=1e-6, atol=0) and float(g.abs().max()) > 0

    # the frame of the points kept: the oracle on the points as they are
    shifted = En.config(cfg['raw'] + torch.tensor([4.0, -3.0, 2.0], dtype=torch.float64), center=False)
    pot, _, _, _ = _parity('frame kept', x, shifted)
    assert float(pot.points.mean(dim=0).abs().max()) > 1.9


def test_deterministic_and_never_synchronises():
    x, cfg = _inputs(En.CASES[3])
    pot = En.potential(cfg, 300, _abar())
    xc = x.cuda()
    a, b = _run(pot, xc, 400), _run(pot, xc, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ra, rb = pot.describe(xc), pot.describe(xc)
    assert all(torch.equal(ra[k], rb[k]) for k in ra)
    da, ga = pot.distance_of(xc), pot.gap_of(xc)
    assert torch.equal(da, pot.distance_of(xc)) and torch.equal(ga, pot.gap_of(xc))
    xg = xc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(xg, 400)
        g, = torch.autograd.grad(lp.mean(), xg)
        rep = pot.describe(xc)
        d = pot.distance_of(xc)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.allclose(g, a[1] / 2, rtol=1e-6, atol=0)      # (the backward scales by grad_output = 1/2)
    assert all(torch.equal(rep[k], ra[k]) for k in ra) and torch.equal(d, da)
    xg = xc.clone().requires_grad_(True)
    scale = torch.tensor([2.0, -0.5], device='cuda')
    g2, = torch.autograd.grad((pot(xg, 400) * scale).sum(), xg)
    assert torch.equal(g2, scale[:, None, None] * a[1])
    with pytest.raises(ValueError):
        pot(xc[:, :299], 400)
    with pytest.raises(ValueError):
        pot(x, 400)                                                                       # (a CPU tensor)
    with pytest.raises(ValueError):
        pot.gap_of(x)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N_S = 12, 24
SAMPLER_CFG = En.case_config((0, 0, 0, 'ellipsoid:12,6,6', 3.0, 61, False))


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

    return dict(run=run, abar=abar, fused=En.potential(SAMPLER_CFG, N_S, abar), torch=En.twisting_function(SAMPLER_CFG, abar))


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
    assert tuple(report) == En.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    again = ctx['fused'].describe(attrs_b['last_positions'].cuda())
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
    assert tuple(report) == En.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())


def test_particle_systems_with_the_sum_of_shape_and_envelope(ctx, tmp_path):
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
    assert tuple(report) == Sh.REPORT + En.REPORT and all(tuple(v.shape) == (S_,) for v in report.values())      # member order, S rows
    xb = attrs['last_positions'].cuda()
    assert tuple(xb.shape) == (S_, N_S, 3)
    for m in (shape, ctx['fused']):
        assert all(torch.equal(report[k], v.cpu()) for k, v in m.describe(xb).items())


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('envelope_cli') / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return root


ENVELOPE_FLAGS = ['--envelope_shape', 'ellipsoid:12,6,6', '--write_envelope']


def _check_envelope_files(out, names, length):
    """outdir/envelope: one report per design -- `residue I A` per residue, covered_fraction, the six report fields, the counts
    consistent with the lines above them -- and envelope.pdb, the 61 lattice points of the solid as placed, read back by
    load_envelope."""
    from genie2_amd.smc import envelope_shape_points, load_envelope
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == sorted(n + '.pdb' for n in names)
    assert sorted(os.listdir(os.path.join(out, 'envelope'))) == sorted([n + '.txt' for n in names] + ['envelope.pdb'])
    pts, w = load_envelope(os.path.join(out, 'envelope', 'envelope.pdb'))
    assert torch.equal(pts, envelope_shape_points('ellipsoid:12,6,6', 3.0)) and bool((w == 1).all()) and len(pts) == 61
    for name in names:
        lines = [ln.split() for ln in open(os.path.join(out, 'envelope', name + '.txt'))]
        assert len(lines) == length + 1 + len(En.REPORT)
        rows, fraction, fields = lines[:length], lines[length], lines[length + 1:]
        assert all(r[:2] == ['residue', str(n)] and len(r) == 3 and float(r[2]) >= 0.1 for n, r in enumerate(rows)), name
        assert fraction[0] == 'covered_fraction' and len(fraction) == 2 and 0.0 <= float(fraction[1]) <= 1.0
        assert [f[0] for f in fields] == list(En.REPORT) and all(len(f) == 2 for f in fields)
        assert all(('.' in f[1]) == (f[0] not in En.COUNTS) for f in fields)
        got = {f[0]: float(f[1]) for f in fields}
        outside = [float(r[2]) - 3.0 for r in rows]
        sure, maybe = sum(1 for v in outside if v > 1e-3), sum(1 for v in outside if abs(v) <= 1e-3)
        assert sure <= got['n_outside'] <= sure + maybe and abs(got['max_outside'] - max(0.0, max(outside))) <= 2e-3
        assert got['e_envelope_inside'] >= 0 and got['e_envelope_cover'] >= 0 and 0 <= got['n_uncovered'] <= 61
        print(name, fraction, got)


def test_shape_cli_with_an_envelope_term_end_to_end(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--min_length', '24', '--max_length', '24', '--batch_size', '2', '--num_samples', '2',
                                      '--num_steps', '4', '--last_unguided_steps', '0', '--guidance_alpha', '0.05'] + ENVELOPE_FLAGS)
    torch.manual_seed(0)
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_envelope_files(out, ['24_0', '24_1'], 24)
    assert not any(os.path.exists(os.path.join(out, d)) for d in ('shape', 'secstruct', 'sheet', 'symmetry', 'binder', 'fold', 'burial'))


def test_motif_cli_with_an_envelope_term_end_to_end(tmp_path, checkpoint_root):
    import _shape as Sh
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--motif_file', MOTIF, '--min_length', '40', '--max_length', '40', '--batch_size', '2',
                                      '--num_samples', '2', '--num_steps', '4', '--last_unguided_steps', '0', '--rog_max', '8',
                                      '--write_shape_report'] + ENVELOPE_FLAGS)
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_envelope_files(out, ['40_0', '40_1'], 40)
    for name in ('40_0', '40_1'):
        lines = [ln.split() for ln in open(os.path.join(out, 'shape', name + '.txt'))]
        assert [ln[0] for ln in lines] == list(Sh.REPORT)                # exactly its own keys
