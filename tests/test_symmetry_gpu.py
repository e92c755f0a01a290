"""The symmetry potential on the GPU (genie_symmetry_potential, csrc/symmetry_kernels.hip; SymmetryPotential in genie2_amd/smc.py)
against the float64 oracle of tests/_symmetry.py, in TwistedSampler against the float32 PyTorch restatement as its twisting function,
summed with the shape potential in particle systems, with the units as separate chains against the oracle's loop, and through both
command lines.

Bounds (tests/_motif.py:60-72, the project's bars for a fused potential, used as in test_sheet_gpu.py): logp within 1e-5
max(1, |logp|); every particle's gradient within 1e-5 of its largest float64 entry; every report field inside the logp bar, angles
within 1e-3 degrees; each widened, per case, to 4 x the error the float32 restatement makes on the same input where that is larger
(the kernel is held to float32 arithmetic; the factor covers another summation order).  Inputs are 3.8 A random walks of seeds
100 N + {0, 1, 2}, chosen by the oracle alone: on each the float64 side asserts that the two largest eigenvalues of every Horn matrix
differ by at least 1e-2 of the spectral radius and that every angle of a generator that is not a two-fold is above 5 degrees.

Worst error / bound over the parity cases, measured on an MI355X: 0.055 for logp and 0.155 for the gradient (both at N = 9), 0.050 for
an energy or RMSD field, 0.024 for an angle, 0.051 for a rise; only rise bars were widened (x1.1 to x3.1; x12 at N = 5460), and the
kernel's rise is inside the unwidened bar everywhere."""
import math
import os

import numpy as np
import pytest
import torch

import _symmetry as S
from _motif import MOTIF, _abar, _tiny_model, walk
from _parity import hard_time_limit

pytestmark = pytest.mark.gpu

STEP = 500
_cache = {}


@pytest.fixture(autouse=True)
def _limit():
    with hard_time_limit(300):
        yield


def _potential(case, abar=None, **kw):
    from genie2_amd.smc import SymmetryPotential
    B, N, sym, m, linker, offset = case
    return SymmetryPotential(N, _abar() if abar is None else abar, symmetry=sym, unit_length=m, linker=linker, offset=offset, device='cuda', **kw)


def _case(case):
    """(x, generators) of a parity case, made once."""
    if case not in _cache:
        B, N, sym, m, linker, offset = case
        _cache[case] = (S.walks(B, N), S.generators(sym, m, N, linker, offset))
    return _cache[case]


def _reference(x, gens, var, weights=None, grad=True):
    """The oracle and the float32 restatement of an input, computed once; the oracle's own conditions are asserted here."""
    key = ('ref', x.data_ptr(), tuple(x.shape), repr(gens), var, repr(weights), grad)
    if key not in _cache:
        ref = S.reference(x, gens, var, weights, grad=grad)
        if grad:
            assert float(ref['gap'].min()) >= 1e-2, 'a Horn matrix of this input is near-degenerate (gap %.3e): take another seed' % float(ref['gap'].min())
            for g, gen in enumerate(gens):
                assert S.is_swap(gen) or float(ref['angle_%d' % g].min()) > 5.0, 'a generator of this input turns by less than 5 degrees'
        _cache[key] = (x, ref, S.restatement32(x, gens, var, weights))      # (x kept: its data_ptr stays its own)
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


def _check(what, lp, g, ref, r32, gradient=True):
    lp, g = lp.double().cpu(), g.double().cpu()
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), what
    lp_b = 1e-5 * ref['logp'].abs().clamp(min=1.0)
    lp_b = lp_b * _widen((r32['logp'].double() - ref['logp']).abs(), lp_b)
    d_lp = (lp - ref['logp']).abs()
    print('%s: logp error / bound %.3f' % (what, _ratio(d_lp, lp_b)))
    assert bool((d_lp <= lp_b).all()), (what, lp, ref['logp'])
    if gradient:
        g_b = 1e-5 * ref['grad'].abs().amax(dim=(1, 2))
        g_b = g_b * _widen((r32['grad'].double() - ref['grad']).abs().amax(dim=(1, 2)), g_b)
        d_g = (g - ref['grad']).abs().amax(dim=(1, 2))
        print('%s: gradient error / bound %.3f' % (what, _ratio(d_g, g_b)))
        assert bool((d_g <= g_b).all()), (what, d_g, g_b)


def _check_report(what, got, ref, r32):
    assert tuple(got) == S.REPORT
    for k in S.REPORT:
        v, r = got[k].double().cpu(), ref[k]
        assert tuple(got[k].shape) == tuple(r.shape) and got[k].dtype == torch.float32 and got[k].device.type == 'cuda', k
        bound = torch.full_like(r, 1e-3) if k.startswith('angle') else 1e-5 * r.abs().clamp(min=1.0)
        bound = bound * _widen((r32[k].double() - r).abs(), bound)
        print('%s: %s error / bound %.3f' % (what, k, _ratio((v - r).abs(), bound)))
        assert bool(torch.isfinite(v).all()) and bool(((v - r).abs() <= bound).all()), (what, k, v, r)


@pytest.mark.parametrize('case', S.CASES, ids=S.case_id)
def test_potential_and_report_match_the_float64_oracle(case):
    x, gens = _case(case)
    pot = _potential(case)
    var = float(pot.variance(STEP))
    ref, r32 = _reference(x, gens, var)
    lp, g = _run(pot, x)
    _check(S.case_id(case), lp, g, ref, r32)
    assert bool((ref['logp'] < 0).all())
    # residues in no unit are free: a gradient of exactly 0 there, and nowhere else
    B, N, sym, m, linker, offset = case
    used = torch.zeros(N, dtype=torch.bool)
    for src, dst in gens:
        used[src] = True
        used[dst] = True
    assert int((~used).sum()) == N - (2 if sym[0] == 'D' else 1) * int(sym[1:]) * m
    assert bool((g[:, ~used.cuda()] == 0).all()) and bool((g[:, used.cuda()].abs().amax(dim=2) > 0).all())
    _check_report(S.case_id(case), pot.describe(x.cuda()), ref, r32)
    if len(gens) == 1:
        got = pot.describe(x.cuda())
        assert all(bool((got[k] == 0).all()) for k in ('rmsd_1', 'angle_1', 'rise_1'))      # an unused slot reports zeros


def test_chain_whose_staging_needs_more_than_64_kib_of_lds():
    """N = 5460 (C3, m 1820): 12 N + 320 bytes of dynamic LDS are 65 840, above the 65 536 a kernel gets without asking (from
    N = 5435 on the entry raises the kernel's limit).  One particle, the same bars."""
    case = (1, 5460, 'C3', 1820, 0, 0)
    x, gens = _case(case)
    pot = _potential(case)
    ref, r32 = _reference(x, gens, float(pot.variance(STEP)))
    _check(S.case_id(case), *_run(pot, x), ref, r32)
    _check_report(S.case_id(case), pot.describe(x.cuda()), ref, r32)
    a, b = _run(pot, x), _run(pot, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_generator_weights_one_zero_is_the_one_generator_oracle():
    case = (3, 129, 'D2', 31, 1, 2)
    x, gens = _case(case)
    pot = _potential(case, generator_weights=(1, 0))
    var = float(pot.variance(STEP))
    lp, g = _run(pot, x)
    ref, r32 = _reference(x, gens[:1], var)
    _check('D2 with weights (1, 0)', lp, g, ref, r32)
    # the report still describes the generator that is switched off; the weighted energy leaves it out
    full, _ = _reference(x, gens, var)
    got = pot.describe(x.cuda())
    assert torch.allclose(got['e_symmetry'].double().cpu(), ref['e_symmetry'], rtol=1e-5)
    assert torch.allclose(got['rmsd_1'].double().cpu(), full['rmsd_1'], rtol=1e-5) and bool((got['rmsd_1'] > 0).all())
    # an overall weight and generator weights multiply
    pot = _potential(case, weight=0.5, generator_weights=(2.0, 0.25))
    ref, r32 = _reference(x, gens, var, weights=[1.0, 0.125])
    _check('D2 with weight 0.5 and weights (2, 0.25)', *_run(pot, x), ref, r32)


def test_explicit_generators_equal_the_symbol():
    from genie2_amd.smc import SymmetryPotential
    case = (3, 65, 'C3', 21, 0, 1)
    x, gens = _case(case)
    a = _run(_potential(case), x)
    b = _run(SymmetryPotential(65, _abar(), generators=gens, device='cuda'), x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_deterministic_and_never_synchronises():
    case = (3, 256, 'D2', 60, 4, 2)
    x, _ = _case(case)
    pot = _potential(case)
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
        pot(xc[:, :255], 400)
    with pytest.raises(ValueError):
        pot(x, 400)                                                                       # (a CPU tensor)


def test_exact_assemblies_in_float32():
    """An exact C3 built in float64 within 50 A of the origin and rounded to float32: the rounding of a coordinate is at most
    50 * 2^-24 = 3e-6 A, that of the rotation's nine entries 6e-8 each on arms below 50 A another 2e-5 A per residue, about 5e-5 A
    with the centroids': symmetry_rmsd below 1e-3 A with a factor of 20 to spare.  The bound is derived, not measured."""
    x = S.exact_cyclic(3, 20)
    assert float(x.abs().max()) < 50.0
    pot = _potential((1, 60, 'C3', 20, 0, 0))
    got = pot.describe(x.float()[None].cuda())
    print('exact C3: symmetry_rmsd %.3e A, angle %.5f, rise %.3e' % (float(got['symmetry_rmsd']), float(got['angle_0']), float(got['rise_0'])))
    assert float(got['symmetry_rmsd']) < 1e-3 and abs(float(got['angle_0']) - 120.0) < 1e-3 and float(got['rise_0']) < 1e-3
    # a repeat reports its twist and its rise; a dihedral assembly two two-folds at 180 degrees
    x = S.exact_repeat(4, 15, 40.0, 7.0)
    got = _potential((1, 60, 'R4', 15, 0, 0)).describe(x.float()[None].cuda())
    assert float(got['symmetry_rmsd']) < 1e-3 and abs(float(got['angle_0']) - 40.0) < 1e-3 and abs(float(got['rise_0']) - 7.0) < 1e-3
    x = S.exact_dihedral(2, 10)
    got = _potential((1, 40, 'D2', 10, 0, 0)).describe(x.float()[None].cuda())
    assert float(got['symmetry_rmsd']) < 1e-3 and all(abs(float(got[k]) - 180.0) < 1e-3 for k in ('angle_0', 'angle_1'))
    assert float(got['rise_0']) < 1e-3 and float(got['rise_1']) < 1e-3
    # a mirror-image dimer does not fit: the rotation is proper
    unit = S.exact_unit(20, 4)
    mirror = torch.cat([unit, unit * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)])
    got = _potential((1, 40, 'C2', 20, 0, 0)).describe(mirror.float()[None].cuda())
    want = S.describe(mirror[None], S.generators('C2', 20, 40))
    assert float(want['symmetry_rmsd']) > 1.0 and float(got['symmetry_rmsd']) == pytest.approx(float(want['symmetry_rmsd']), rel=1e-5)


def test_degenerate_inputs_stay_finite():
    """A straight chain (collinear: Horn's matrix has a double largest eigenvalue, so the rotation is one of a family and the
    gradient is not compared) and N points in one place: finite outputs and the oracle's logp."""
    case = (2, 40, 'R4', 10, 0, 0)
    gens = S.generators('R4', 10, 40)
    k = torch.arange(40, dtype=torch.float32)
    x = torch.zeros(2, 40, 3)
    x[0, :, 0] = 3.8 * k                                                 # evenly spaced: every unit is a translate of the first
    x[1, :, 1] = 3.0 * k + 0.05 * k * k - 20.0                           # unevenly spaced: the units differ
    pot = _potential(case)
    var = float(pot.variance(STEP))
    ref, r32 = _reference(x, gens, var, grad=False)
    lp, g = _run(pot, x)
    _check('a straight chain', lp, g, ref, r32, gradient=False)
    assert float(ref['logp'][1]) < -1.0 and float(ref['logp'][0]) > -1e-6      # (3.8 k is rounded to float32: not quite translates)
    rep = pot.describe(x.cuda())
    assert all(bool(torch.isfinite(v).all()) for v in rep.values())
    x = torch.full((2, 40, 3), 2.5)
    lp, g = _run(pot, x)
    rep = pot.describe(x.cuda())
    assert bool((lp == 0).all()) and bool((g == 0).all()) and all(bool((v == 0).all()) for v in rep.values())


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N_S = 12, 40
SAMPLER_CASE = (4, N_S, 'C2', 20, 0, 0)


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
        return np.stack([r['atom_positions'] for r in out]), out, attrs

    gens = S.generators('C2', 20, N_S)
    return dict(run=run, abar=abar, model=model, fused=_potential(SAMPLER_CASE, abar), torch=S.twisting_function(gens, abar))


def _noise(B, seed):
    return torch.randn(T, B, N_S, 3, generator=torch.Generator().manual_seed(seed))


def test_sampler_follows_the_torch_path_without_resampling(ctx, tmp_path):
    B, noise = 4, _noise(4, 4)
    a, _, attrs_a = ctx['run'](ctx['torch'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    b, _, attrs_b = ctx['run'](ctx['fused'], noise, tmp_path, num_samples=B, ess_threshold=0.0)
    rms, d = float(np.sqrt((a ** 2).mean())), float(np.abs(a - b).max())
    print('no resampling: max |d| = %.3e, coordinate RMS = %.2f, ratio %.3e' % (d, rms, d / rms))
    assert np.isfinite(b).all() and d <= 1e-3 * rms
    assert attrs_a['last_shape'] is None                                 # a plain callable
    report = attrs_b['last_shape']
    assert tuple(report) == S.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    again = ctx['fused'].describe(torch.from_numpy(b).float().cuda())
    assert all(torch.equal(report[k], again[k].cpu()) for k in report)
    assert attrs_b['last_fit'] is None and attrs_b['last_secstruct'] is None and attrs_b['last_pairs'] is None


def test_particle_systems_with_the_sum_of_shape_and_symmetry(ctx, tmp_path):
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
    assert tuple(report) == Sh.REPORT + S.REPORT and all(tuple(v.shape) == (S_,) for v in report.values())      # member order, S rows
    xb = torch.from_numpy(best).float().cuda()
    for m in (shape, ctx['fused']):
        assert all(torch.equal(report[k], v.cpu()) for k, v in m.describe(xb).items())


def test_units_as_chains_follow_the_oracle_loop(ctx, tmp_path, base_weights):
    """chain_lengths = [20, 20] through UnconditionalSampler against the oracle's sample_loop on two-chain features, on the same noise:
    the bar of test_sampler_api_end_to_end (tests/test_hip_parity.py), 1e-4 of the coordinates' RMS."""
    from oracle import genie_oracle as O
    from genie2_amd.sampler import UnconditionalSampler
    chains = ctx['fused'].chain_lengths()
    assert chains == [20, 20]
    sampler = UnconditionalSampler(ctx['model'])
    noise = _noise(2, 8)
    params = {'length': N_S, 'scale': 0.6, 'num_samples': 2, 'outdir': str(tmp_path), 'prefix': '40', 'offset': 0, 'noise': noise,
              'chain_lengths': chains}
    got = sampler._sample(params)
    assert all(g['chain_index'].tolist() == [0] * 20 + [1] * 20 and g['residue_index'].tolist() == list(range(20)) * 2 for g in got)
    xyz = torch.tensor(np.stack([g['atom_positions'] for g in got]), dtype=torch.float32)
    dims = dict(O.BASE_DIMS, n_timestep=T)
    ref, _, _ = O.sample_loop(base_weights, dims, O.empty_features([N_S, N_S], chains_per_sample=[chains, chains]), noise, 0.6, 'closed')
    d, rms = float((xyz - ref).abs().max()), float(ref.pow(2).mean().sqrt())
    print('two chains: max |d| = %.3e, RMS %.2f, ratio / 1e-4 = %.3f' % (d, rms, d / (1e-4 * rms)))
    assert d <= 1e-4 * rms
    one, _, _ = O.sample_loop(base_weights, dims, O.empty_features([N_S, N_S]), noise, 0.6, 'closed')
    assert float((one - ref).abs().max()) > 1e-2 * rms                   # (the chain break is felt: one chain gives other coordinates)
    sampler.sample(params)
    lines = (tmp_path / 'pdbs' / '40_0.pdb').read_text().splitlines()
    assert [ln[21] for ln in lines] == ['A'] * 20 + ['B'] * 20 and lines[20][22:26].strip() == '1'


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('symmetry_cli') / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return root


def _check_symmetry_files(out, names):
    """Every outdir/symmetry file against the float64 oracle on the coordinates its PDB holds, and the PDB's chains.  The PDB rounds
    coordinates to 1e-3 A (at most 5e-4 per coordinate) and the report its values to three decimals: an energy or an RMSD may differ
    from the oracle's on the written coordinates by 5e-4 + 5e-4 |d value / d x|_1 plus the float32 bar 1e-5 max(1, |value|).  The one
    generator of C2 is a two-fold: its angle is 180 or 0 (two units that are translates of each other) and its rise 0 whatever the
    coordinates, to the float32 rounding of the fit
    (1e-3 degrees, the parity bar; 1e-5 max(1, |c|) A on centroids of a few tens of A, taken as 1e-3) plus the 5e-4 of the file."""
    from genie2_amd.features import parse_pdb
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == sorted(n + '.pdb' for n in names)
    assert sorted(os.listdir(os.path.join(out, 'symmetry'))) == sorted(n + '.txt' for n in names)
    gens = S.generators('C2', 20, N_S)
    for name in names:
        pdb = [ln for ln in open(os.path.join(out, 'pdbs', name + '.pdb')) if ln.startswith('ATOM')]
        assert [ln[21] for ln in pdb] == ['A'] * 20 + ['B'] * 20 and [int(ln[22:26]) for ln in pdb] == list(range(1, 21)) * 2
        chains = parse_pdb(os.path.join(out, 'pdbs', name + '.pdb'))[1]
        y = torch.tensor(np.concatenate(chains), dtype=torch.float64)[None].requires_grad_(True)
        assert tuple(y.shape) == (1, N_S, 3)
        lines = [ln.split() for ln in open(os.path.join(out, 'symmetry', name + '.txt'))]
        assert lines[0] == 'symmetry C2 units 2 unit_length 20 linker 0 offset 0'.split()
        assert [f[0] for f in lines[1:]] == list(S.REPORT) and all(len(f) == 2 and '.' in f[1] for f in lines[1:])
        got = {f[0]: float(f[1]) for f in lines[1:]}
        e = S.energy(y, gens)[0]
        for k, ref in (('e_symmetry', e), ('symmetry_rmsd', (e / 40.0).sqrt()), ('rmsd_0', (e / 40.0).sqrt())):
            grad, = torch.autograd.grad(ref, y, retain_graph=True)
            ref = float(ref.detach())
            tol = 5e-4 + 5e-4 * float(grad.abs().sum()) + 1e-5 * max(1.0, abs(ref))
            assert abs(got[k] - ref) <= tol, (name, k, got[k], ref, tol)
        assert min(abs(got['angle_0']), abs(got['angle_0'] - 180.0)) <= 1.5e-3 and got['rise_0'] <= 1.5e-3, (name, got)
        want = S.describe(y.detach(), gens)
        if float(want['gap']) >= 1e-2:                                   # (which of the two it is, where the fit is not near a tie)
            assert abs(got['angle_0'] - float(want['angle_0'])) <= 1.5e-3, (name, got, float(want['angle_0']))
        assert got['rmsd_1'] == got['angle_1'] == got['rise_1'] == 0.0


def test_shape_cli_with_a_symmetry_term_end_to_end(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--min_length', '39', '--max_length', '40', '--batch_size', '2', '--num_samples', '2',
                                      '--num_steps', '4', '--last_unguided_steps', '0', '--guidance_alpha', '0.05',
                                      '--symmetry', 'C2', '--unit_chains', '--write_symmetry'])
    torch.manual_seed(0)
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_symmetry_files(out, ['40_0', '40_1'])                          # (39 residues do not divide into two units: skipped)
    assert not any(os.path.exists(os.path.join(out, d)) for d in ('shape', 'secstruct', 'sheet'))


def test_motif_cli_with_a_symmetry_term_end_to_end(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out,
                                      '--motif_file', MOTIF, '--min_length', '40', '--max_length', '40', '--batch_size', '2',
                                      '--num_samples', '2', '--num_steps', '4', '--last_unguided_steps', '0', '--rog_max', '8',
                                      '--symmetry', 'C2', '--unit_chains', '--write_symmetry', '--write_shape_report'])
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    _check_symmetry_files(out, ['40_0', '40_1'])
    import _shape as Sh
    for name in ('40_0', '40_1'):
        lines = [ln.split() for ln in open(os.path.join(out, 'shape', name + '.txt'))]
        assert [ln[0] for ln in lines] == list(Sh.REPORT)                # exactly its own keys
