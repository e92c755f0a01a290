"""The binder potential on the GPU (genie_binder_potential, csrc/binder_kernels.hip; BinderPotential in genie2_amd/smc.py) against the
float64 oracle of tests/_binder.py, in TwistedSampler against the float32 PyTorch restatement as its twisting function, summed with
the shape potential in particle systems, and through both command lines.

Bounds (tests/_motif.py:60-72, the project's bars for a fused potential, used as in test_symmetry_gpu.py): logp within 1e-5
max(1, |logp|); every particle's gradient within 1e-5 of its largest float64 entry; every energy, `contacts`, distance and
hotspot_out value inside the logp bar, 1e-5 max(1, |value|); each widened, per case, to 4 x the error the float32 restatement makes on
the same input where that is larger (the kernel is held to float32 arithmetic; the factor covers another summation order); counts
exactly.  Inputs are those of tests/_binder.py, chosen by the oracle alone: on each the float64 side asserts that no pair is within
1e-4 A of a threshold and that every enabled term has positive energy on some particle.

Worst error / bound over the parity tests, measured on an MI355X: 0.040 for logp ((3, 64, 64)), 0.046 for the gradient (the target
1e4 A away; 0.044 at M = 5500), 0.014 for `contacts`, 0.007 for `target_min_distance`, 0.016 / 0.042 / 0.092 for the clash, contact
and hotspot energies (the last at (3, 5, 3)), 0.037 for hotspot_out; no bar was widened, every count was equal (DESIGN.md 7.7 has
the table per case)."""
import math
import os

import numpy as np
import pytest
import torch

import _binder as Bd
from _motif import MOTIF, _abar, _tiny_model, walk
from _parity import hard_time_limit
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

STEP = 500
TARGET = os.path.join(GOLDEN, 'dataset_100_0.pdb')
_cache = {}


@pytest.fixture(autouse=True)
def _limit():
    with hard_time_limit(300):
        yield


def _inputs(case, H=None):
    """(x, y, cfg) of a parity case, made once."""
    if (case, H) not in _cache:
        _cache[(case, H)] = Bd.inputs(case, H)
    return _cache[(case, H)]


def _reference(x, y, cfg, var, grad=True):
    """The oracle and the float32 restatement of an input, computed once."""
    key = ('ref', x.data_ptr(), y.data_ptr(), repr(sorted(cfg.items())), var, grad)
    if key not in _cache:
        _cache[key] = (x, y, Bd.reference(x, y, cfg, var, grad), Bd.restatement32(x, y, cfg, var, grad))      # (x, y kept: their data_ptr stays theirs)
    return _cache[key][2:]


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


def _check_report(what, pot, x, ref, r32):
    got = pot.describe(x.cuda())
    assert tuple(got) == Bd.REPORT
    for k in Bd.REPORT:
        assert tuple(got[k].shape) == tuple(ref[k].shape) and got[k].device.type == 'cuda', k
        if k in Bd.COUNTS:
            assert got[k].dtype == torch.int64 and torch.equal(got[k].cpu(), ref[k]), (what, k, got[k], ref[k])
            continue
        v, r = got[k].double().cpu(), ref[k]
        assert got[k].dtype == torch.float32
        bound = 1e-5 * r.abs().clamp(min=1.0)
        wide = _widen((r32[k].double().cpu() - r).abs(), bound)
        print('%s: %s error / bound %.3f (bar widened x%.2f)' % (what, k, _ratio((v - r).abs(), bound * wide), wide))
        assert bool(torch.isfinite(v).all()) and bool(((v - r).abs() <= bound * wide).all()), (what, k, v, r)
    c = pot.hotspot_contacts_of(x.cuda())
    assert tuple(c.shape) == tuple(ref['hotspot'].shape) and c.dtype == torch.float32 and c.device.type == 'cuda'
    if c.numel():
        r = ref['hotspot']
        bound = 1e-5 * r.abs().clamp(min=1.0)
        wide = _widen((r32['hotspot'].double().cpu() - r).abs().reshape(-1), bound.reshape(-1))
        d = (c.double().cpu() - r).abs()
        print('%s: hotspot_out error / bound %.3f (bar widened x%.2f)' % (what, _ratio(d.reshape(-1), bound.reshape(-1) * wide), wide))
        assert bool((d <= bound * wide).all()), (what, c, r)


def _parity(what, x, y, cfg, gradient=True):
    pot = Bd.potential(cfg, x.shape[1], y, _abar())
    ref, r32 = _reference(x, y, cfg, float(pot.variance(STEP)), gradient)
    lp, g = _run(pot, x)
    _check(what, lp, g, ref, r32, gradient)
    _check_report(what, pot, x, ref, r32)
    return pot, ref, lp, g


@pytest.mark.parametrize('case', Bd.CASES, ids=Bd.case_id)
def test_potential_and_report_match_the_float64_oracle(case):
    x, y, cfg = _inputs(case)
    _, ref, _, _ = _parity(Bd.case_id(case), x, y, cfg)
    assert bool((ref['logp'] < 0).all())


def test_target_whose_staging_needs_more_than_64_kib_of_lds():
    """M = 5500: 12 M = 66 000 bytes of staging, above the 65 536 a kernel gets without asking (the entry raises the kernel's limit).
    One particle, the same bars, and two calls bitwise equal."""
    x, y, cfg = _inputs(Bd.LDS_CASE)
    pot, ref, lp, g = _parity(Bd.case_id(Bd.LDS_CASE), x, y, cfg)
    assert all(float(ref[k]) > 0 for k in ('e_target_clash', 'e_contact', 'e_hotspot'))
    again = _run(pot, x)
    assert torch.equal(lp, again[0]) and torch.equal(g, again[1])


@pytest.mark.parametrize('term', ['clash', 'contacts', 'hotspots'])
def test_each_term_alone(term):
    x, y, cfg = _inputs(Bd.CASES[4])
    one = Bd.only(cfg, term)
    Bd.check_inputs(x, y, one)
    _, ref, _, g = _parity('%s alone' % term, x, y, one)
    others = [k for k, t in (('e_target_clash', 'clash'), ('e_contact', 'contacts'), ('e_hotspot', 'hotspots')) if t != term]
    assert all(bool((ref[k] == 0).all()) for k in others) and float(g.abs().max()) > 0


@pytest.mark.parametrize('H', [0, 1, 64])
def test_hotspot_counts(H):
    x, y, cfg = _inputs(Bd.CASES[4], H)
    assert len(cfg['hotspots']) == H
    pot, ref, _, _ = _parity('H = %d' % H, x, y, cfg)
    assert pot.H == H and tuple(pot.hotspot_contacts_of(x.cuda()).shape) == (3, H)
    if H == 0:
        assert bool((ref['e_hotspot'] == 0).all()) and bool((pot.describe(x.cuda())['e_hotspot'] == 0).all())


def test_deterministic_and_never_synchronises():
    x, y, cfg = _inputs(Bd.CASES[5])
    pot = Bd.potential(cfg, x.shape[1], y, _abar())
    xc = x.cuda()
    a, b = _run(pot, xc, 400), _run(pot, xc, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ra, rb = pot.describe(xc), pot.describe(xc)
    assert all(torch.equal(ra[k], rb[k]) for k in ra)
    ha = pot.hotspot_contacts_of(xc)
    assert torch.equal(ha, pot.hotspot_contacts_of(xc))
    xg = xc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(xg, 400)
        g, = torch.autograd.grad(lp.mean(), xg)
        rep = pot.describe(xc)
        hot = pot.hotspot_contacts_of(xc)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.allclose(g, a[1] / 2, rtol=1e-6, atol=0)      # (the backward scales by grad_output = 1/2)
    assert all(torch.equal(rep[k], ra[k]) for k in ra) and torch.equal(hot, ha)
    with pytest.raises(ValueError):
        pot(xc[:, :128], 400)
    with pytest.raises(ValueError):
        pot(x, 400)                                                                       # (a CPU tensor)
    with pytest.raises(ValueError):
        pot.hotspot_contacts_of(x)


def test_degenerate_inputs_stay_finite():
    """A design residue exactly on a target atom (a clash pair without a direction), all design residues at one point, and a target
    1e4 A away, where every s underflows towards 0 and the hinges contacts_min and hotspot_contacts are fully active: finite
    outputs and the oracle's logp (the gradient too where the oracle has one: autograd follows the same zero-distance rule)."""
    x, y, cfg = _inputs(Bd.CASES[2])
    x = x.clone()
    x[0, 7] = y[20]
    x[1, 0] = y[64]
    x[2] = x[2, 5]
    assert Bd.margins(x, y, cfg) >= 1e-4
    pot, ref, lp, g = _parity('coincident atoms', x, y, cfg)
    assert float(ref['target_min_distance'][0]) == 0.0 and float(pot.describe(x.cuda())['target_min_distance'][0]) == 0.0
    far = y + torch.tensor([1e4, 0.0, 0.0])
    cfg_far = dict(cfg, contacts_min=50.0, contacts_max=100.0)
    x = _inputs(Bd.CASES[2])[0]
    pot, ref, lp, g = _parity('a target 1e4 A away', x, far, cfg_far)
    H, var = len(cfg['hotspots']), float(pot.variance(STEP))
    want = -(50.0 ** 2 + H * cfg['hotspot_contacts'] ** 2) / (2 * var)
    assert float(ref['contacts'].max()) < 1e-12 and torch.allclose(lp.double().cpu(), torch.full((3,), want, dtype=torch.float64), rtol=1e-6)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) < 1e-6
    rep = pot.describe(x.cuda())
    assert all(bool(torch.isfinite(v.double()).all()) for v in rep.values()) and bool((rep['n_contacts'] == 0).all())


def test_contacts_max_infinite_and_the_weights():
    x, y, cfg = _inputs(Bd.CASES[3])
    # no upper hinge: particle 1 of this input sits above a finite maximum, and not with an infinite one
    low = dict(cfg, contacts_min=0.0, contacts_max=0.5 * cfg['contacts_min'] / 1.5)
    _, ref, _, _ = _parity('an upper hinge', x, y, low)
    assert bool((ref['e_contact'] > 0).all())
    _, ref, _, _ = _parity('contacts_max = inf', x, y, dict(cfg, contacts_max=math.inf))
    open_ = dict(cfg, contacts_min=0.0, contacts_max=math.inf)
    _, ref, _, _ = _parity('contacts in 0..inf', x, y, open_)
    assert bool((ref['e_contact'] == 0).all())
    # the weights multiply as stated
    scaled = dict(cfg, clash_weight=2.5, contacts_weight=0.125, hotspot_weight=3.0)
    pot, ref, _, _ = _parity('weights 2.5, 0.125, 3', x, y, scaled)
    base = Bd.potential(cfg, x.shape[1], y, _abar()).describe(x.cuda())
    got = pot.describe(x.cuda())
    for k, w in (('e_target_clash', 2.5), ('e_contact', 0.125), ('e_hotspot', 3.0)):
        assert torch.allclose(got[k], w * base[k], rtol=1e-6, atol=0), k
    assert all(torch.equal(got[k], base[k]) for k in Bd.REPORT if not k.startswith('e_'))
    # a weight of 0 switches a term off, energy and force: all three off is logp 0 and a gradient of exactly 0
    off = Bd.potential(dict(cfg, clash_weight=0.0, contacts_weight=0.0, hotspot_weight=0.0), x.shape[1], y, _abar())
    lp, g = _run(off, x)
    assert bool((lp == 0).all()) and bool((g == 0).all())


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N_S = 12, 40


def _sampler_target():
    """A 30-residue target 12 A from the origin along x, with three hotspots."""
    y = Bd.target(30, 12.0)
    return y, Bd.config(clash_distance=4.0, clash_weight=1.0, contacts_min=40.0, contacts_max=80.0, contacts_weight=1.0, hotspot_contacts=2.0,
                        hotspot_weight=1.0, hotspots=[3, 11, 20])


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
        attrs = {k: getattr(sampler, k, None) for k in ('last_fit', 'last_shape', 'last_secstruct', 'last_pairs', 'last_choice', 'last_positions')}
        return np.stack([r['atom_positions'] for r in out]), out, attrs

    y, cfg = _sampler_target()
    return dict(run=run, abar=abar, model=model, fused=Bd.potential(cfg, N_S, y, abar), torch=Bd.twisting_function(y.cuda(), cfg, abar))


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
    assert tuple(report) == Bd.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    again = ctx['fused'].describe(torch.from_numpy(b).float().cuda())
    assert all(torch.equal(report[k], again[k].cpu()) for k in report)
    assert attrs_b['last_fit'] is None and attrs_b['last_secstruct'] is None and attrs_b['last_pairs'] is None
    # last_positions: the returned coordinates in the sampler's frame, for a plain callable too
    for got, attrs in ((a, attrs_a), (b, attrs_b)):
        pos = attrs['last_positions']
        assert pos.dtype == torch.float32 and pos.device.type == 'cpu' and tuple(pos.shape) == (B, N_S, 3)
        assert np.array_equal(pos.numpy().astype(got.dtype), got)


def test_particle_systems_with_the_sum_of_shape_and_binder(ctx, tmp_path):
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
    assert torch.equal(g, parts[0] + parts[1])
    noise = torch.randn(T, S_ * K, N_S, 3, generator=torch.Generator().manual_seed(11))
    best, _, attrs = ctx['run'](both, noise, tmp_path, num_samples=S_, num_particles=K, ess_threshold=0.5, resample_u=[[0.05, 0.21]] * T,
                                return_particles='best')
    assert tuple(best.shape) == (S_, N_S, 3) and np.isfinite(best).all()
    report = attrs['last_shape']
    assert tuple(report) == Sh.REPORT + Bd.REPORT and all(tuple(v.shape) == (S_,) for v in report.values())      # member order, S rows
    xb = torch.from_numpy(best).float().cuda()
    for m in (shape, ctx['fused']):
        assert all(torch.equal(report[k], v.cpu()) for k, v in m.describe(xb).items())
    assert tuple(attrs['last_positions'].shape) == (S_, N_S, 3) and np.array_equal(attrs['last_positions'].numpy().astype(best.dtype), best)


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('binder_cli') / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return root


BINDER_FLAGS = ['--target_pdb', TARGET, '--hotspots', 'A10,A11,A12', '--target_standoff', '12', '--target_clash_distance', '4', '--write_binder',
                '--write_complex']


def _check_binder_files(out, names):
    """Every outdir/binder file against the float64 oracle on the complex its PDB holds, and the PDB's chains.  The complex file keeps
    relative placement and rounds coordinates to 1e-3 A (at most 5e-4 per coordinate, so 2 x 5e-4 x sqrt(3) A on a distance between
    two atoms); the report rounds to three decimals (5e-4).  A field f may therefore differ from the oracle's on the written
    coordinates by 5e-4 + 5e-4 |df/dx|_1 over design and target atoms plus the float32 bar 1e-5 max(1, |f|); the smallest distance,
    whose gradient is two unit vectors, by 5e-4 + 2 x 5e-4 x sqrt(3) + the bar.  Counts are compared where no pair of the written
    complex is within 2e-3 A of a threshold."""
    from genie2_amd.features import parse_pdb
    from genie2_amd.smc import load_target
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == sorted(n + '.pdb' for n in names)
    assert sorted(os.listdir(os.path.join(out, 'binder'))) == sorted(n + '.txt' for n in names)
    assert sorted(os.listdir(os.path.join(out, 'complex'))) == sorted(n + '.pdb' for n in names)
    cfg = Bd.config(clash_distance=4.0, clash_weight=1.0, hotspot_contacts=1.0, hotspot_weight=1.0, hotspots=[9, 10, 11])
    for name in names:
        path = os.path.join(out, 'complex', name + '.pdb')
        pdb = [ln for ln in open(path) if ln.startswith('ATOM')]
        assert [ln[21] for ln in pdb] == ['A'] * 100 + ['B'] * N_S
        seqs, chains = parse_pdb(path)
        assert [len(c) for c in chains] == [100, N_S] and seqs[0] == parse_pdb(TARGET)[0][0]
        y = torch.tensor(chains[0], dtype=torch.float64).requires_grad_(True)
        x = torch.tensor(chains[1], dtype=torch.float64)[None].requires_grad_(True)
        # the target is the file's, translated: same internal distances, hotspot centroid 12 A from where the design was born
        file_xyz = load_target(TARGET)[0]
        assert float((torch.cdist(y.detach(), y.detach()) - torch.cdist(file_xyz, file_xyz)).abs().max()) <= 2 * 5e-4 * math.sqrt(3) + 1e-9
        lines = [ln.split() for ln in open(os.path.join(out, 'binder', name + '.txt'))]
        assert [f[:2] for f in lines[:3]] == [['hotspot', 'A10'], ['hotspot', 'A11'], ['hotspot', 'A12']]
        assert [f[0] for f in lines[3:]] == list(Bd.REPORT) and all(len(f) == 2 for f in lines[3:])
        got = {f[0]: float(f[1]) for f in lines[3:]}
        assert all(('.' in f[1]) == (f[0] not in Bd.COUNTS) for f in lines[3:])
        t = Bd.terms(x, y, cfg)
        fields = [(k, t[k][0], got[k]) for k in ('contacts', 'e_target_clash', 'e_contact', 'e_hotspot')]
        fields += [('hotspot %d' % h, t['hotspot'][0, h], float(lines[h][2])) for h in range(3)]
        for k, ref, value in fields:
            gx, gy = torch.autograd.grad(ref, (x, y), retain_graph=True, allow_unused=True)
            slope = sum(float(v.abs().sum()) for v in (gx, gy) if v is not None)
            ref = float(ref.detach())
            tol = 5e-4 + 5e-4 * slope + 1e-5 * max(1.0, abs(ref))
            assert abs(value - ref) <= tol, (name, k, value, ref, tol)
        # the inter-chain distances of the complex reproduce target_min_distance
        dmin = float(t['target_min_distance'][0])
        assert abs(got['target_min_distance'] - dmin) <= 5e-4 + 2 * 5e-4 * math.sqrt(3) + 1e-5 * max(1.0, dmin), (name, got, dmin)
        if Bd.margins(x.detach(), y.detach(), cfg) >= 2e-3:
            assert all(got[k] == int(t[k][0]) for k in Bd.COUNTS), (name, got)


def test_shape_cli_with_a_binder_term_end_to_end(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    from genie2_amd.smc import BinderPotential, TwistedSampler
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--min_length', '40', '--max_length', '40', '--batch_size', '2', '--num_samples', '2',
                                      '--num_steps', '4', '--last_unguided_steps', '0', '--guidance_alpha', '0.05'] + BINDER_FLAGS)
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
    _check_binder_files(out, ['40_0', '40_1'])
    assert not any(os.path.exists(os.path.join(out, d)) for d in ('shape', 'secstruct', 'sheet', 'symmetry'))
    assert len(seen) == 1                                                # (one device: the run was in this process)
    if seen:
        pos, report, pot = seen[-1]
        assert isinstance(pot, BinderPotential) and tuple(report) == Bd.REPORT
        again = pot.describe(pos.cuda())
        hot = pot.hotspot_contacts_of(pos.cuda()).cpu()
        for i, name in enumerate(('40_0', '40_1')):
            lines = [ln.split() for ln in open(os.path.join(out, 'binder', name + '.txt'))]
            assert all(abs(float(lines[h][2]) - float(hot[i, h])) <= 5e-4 + 1e-6 for h in range(3))
            for f in lines[3:]:
                assert torch.equal(report[f[0]][i], again[f[0]][i].cpu())
                assert abs(float(f[1]) - float(report[f[0]][i])) <= 5e-4 + 1e-5 * max(1.0, abs(float(report[f[0]][i]))), (name, f)


def test_motif_cli_with_a_binder_term_end_to_end(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--motif_file', MOTIF, '--min_length', '40', '--max_length', '40', '--batch_size', '2',
                                      '--num_samples', '2', '--num_steps', '4', '--last_unguided_steps', '0', '--rog_max', '8',
                                      '--write_shape_report'] + BINDER_FLAGS)
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_binder_files(out, ['40_0', '40_1'])
    import _shape as Sh
    for name in ('40_0', '40_1'):
        lines = [ln.split() for ln in open(os.path.join(out, 'shape', name + '.txt'))]
        assert [ln[0] for ln in lines] == list(Sh.REPORT)                # exactly its own keys


def test_run_without_binder_flags_writes_no_binder_files(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--min_length', '40', '--max_length', '40', '--batch_size', '2', '--num_samples', '2',
                                      '--num_steps', '4', '--last_unguided_steps', '0', '--rog_max', '8'])
    torch.manual_seed(0)
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    assert len(os.listdir(os.path.join(out, 'pdbs'))) == 2
    assert not any(os.path.exists(os.path.join(out, d)) for d in ('binder', 'complex'))
