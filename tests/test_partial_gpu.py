"""Partial diffusion on the GPU: every sampler entered at start_step = t0 from a given backbone (genie2_amd/sampler.py, smc.py),
through the existing device entries genie_q_sample, genie_sample_loop(first_step = t0) and genie_sample_loop_steps(state).

Bars, all taken from the tests of the loops from noise:
  tail equivalence   max|dx| <= 1e-4 coordinate RMS (test_consecutive_steps_equal_the_schedule_table_loop);
  few-step iterates  |dx| <= 2e-6 max(1, |x|_inf) per step (test_reverse_step_matches_the_float64_formula);
  start state        1e-6 (1 + |x|): one float32 rounding of each product and of their sum against the float64 value;
  twisted, constant potential against the unconditional sampler  2e-3 RMS (test_twisted_sampler_num_steps)."""
import os

import numpy as np
import pytest
import torch

import _fewstep as R
import _partial as P
from _motif import _ca_coordinates, _pot, _tiny_model, segments_6e6r, walk
from _parity import hard_time_limit
from conftest import GOLDEN
from oracle import genie_oracle as O

pytestmark = pytest.mark.gpu

T20, SCALE, N = 20, 0.6, 40
PROBLEM = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')
NAME = 'motif_problem_6E6R'


def mdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def xyz(items):
    return torch.tensor(np.stack([it['atom_positions'] for it in items]), dtype=torch.float32)


@pytest.fixture(scope='module')
def genie20(base_weights):
    model = _tiny_model(base_weights, T20)
    yield model
    model.model._drop_engine()


@pytest.fixture(scope='module')
def full_loop(genie20):
    """The T-step loop from noise, once: (Z [20,2,N,3], its final coordinates, the record of every iteration)."""
    eng = genie20.model.engine()
    eng.bind_features(O.empty_features([N, N]))
    genie20.model._bound = None
    Z = torch.randn(T20, 2, N, 3, generator=torch.Generator().manual_seed(8))
    final, _, rec = eng.sample_loop(Z, SCALE, record=True)
    return Z, final.cpu().clone(), rec.cpu().clone()


def _base(B, **over):
    return dict({'length': N, 'scale': SCALE, 'num_samples': B, 'outdir': 'unused', 'prefix': 'x', 'offset': 0}, **over)


# --------------------------------------------------------------- 7. tail equivalence: pins the noise indexing
@pytest.mark.parametrize('t0', [1, 7, 19, 20])
def test_tail_of_the_full_loop_is_reproduced_from_its_own_state(genie20, full_loop, t0):
    """The issue's t0 of 1, 7 and 19, and T itself.  Printed on the MI355X: worst |dx| / (1e-4 rms) = 0.002, 0.000, 0.008, 0.000 at t0 = 1, 7,
    19, 20; bitwise equal to the full loop at t0 = 7 and 20 (where x_t0 / c1 * c1 rounds back to x_t0), not at 1 and 19."""
    from genie2_amd.sampler import UnconditionalSampler
    Z, final, rec = full_loop
    sampler = UnconditionalSampler(genie20)
    with hard_time_limit(120):
        got = P.tail_case(None, sampler, T20, t0, Z, rec, SCALE, 2, N)
    rms = float(final.pow(2).mean().sqrt())
    print('tail t0 = %d: worst |dx| / (1e-4 rms) = %.3f, bitwise equal: %s' % (t0, mdiff(got, final) / (1e-4 * rms), torch.equal(got, final)))
    assert mdiff(got, final) <= 1e-4 * rms
    assert sampler.last_start_rmsd.shape == (2,) and bool(torch.isfinite(sampler.last_start_rmsd).all())


def test_sample_loop_checks_the_rows_it_will_read(genie20):
    eng = genie20.model.engine()
    eng.bind_features(O.empty_features([N, N]))
    genie20.model._bound = None
    state = (torch.zeros(2, N, 3, device='cuda'), torch.zeros(2, N, 3, 3, device='cuda'))
    tail = torch.zeros(7, 2, N, 3, device='cuda')
    for kw in (dict(first_step=7, noise_first=12), dict(first_step=9, noise_first=13), dict(first_step=7, noise_first=15),
               dict(first_step=20, noise_first=13), dict(first_step=7, noise_first=-1)):
        with pytest.raises(ValueError, match='noise must hold rows'):
            eng.sample_loop(tail, SCALE, state=state, **kw)
    with pytest.raises(ValueError, match='noise must hold rows'):
        eng.sample_loop(torch.zeros(7, 2, N - 1, 3, device='cuda'), SCALE, first_step=7, state=state, noise_first=13)
    assert float(state[0].abs().max()) == 0.0                        # nothing was launched


# --------------------------------------------------------------- 8. few-step partial against float64
@pytest.mark.parametrize('sampler,eta', [('ancestral', None), ('ddim', 0.0), ('ddim', 0.5)])
def test_few_step_partial_iterates_match_the_float64_formula(genie20, sampler, eta):
    """Printed on the MI355X: worst |dx| / bar over the four iterates 0.071 (ancestral), 0.056 (ddim 0), 0.063 (ddim 0.5)."""
    from genie2_amd import pack
    from genie2_amd.sampler import UnconditionalSampler, prepare_init_structure
    t0, K, B = 13, 4, 2
    steps = pack.partial_steps(T20, t0, K)
    assert steps == [13, 9, 5, 1]
    x_in = walk(B, N, 3)
    noise = torch.randn(K, B, N, 3, generator=torch.Generator().manual_seed(21))
    smp = UnconditionalSampler(genie20)
    params = _base(B, init_structure=x_in, start_step=t0, num_steps=K, noise=noise, sampler=sampler)
    if eta is not None:
        params['eta'] = eta
    with hard_time_limit(120):
        got = xyz(smp._sample(params))
        # the same calls, recorded: the start state, then the loop carrying it in
        eng = genie20.model.engine()
        mask = torch.ones(B, N, dtype=torch.int32)
        start = smp.start_state(eng, prepare_init_structure(x_in, mask), noise[0].cuda(), t0)
        x0 = start[0].clone()
        coef = pack.reverse_coefficients(T20, steps, sampler, eta or 0.0)
        final, _, rec = eng.sample_loop_steps(noise, SCALE, steps, coef, state=start, record=True)
        assert torch.equal(final.cpu(), got)
        rows = R.coefficient_rows(T20, steps, sampler, eta or 0.0)
        worst = 0.0
        for i, step in enumerate(steps):
            x = x0 if i == 0 else rec[i - 1]
            z = eng.denoise(x, eng.frenet(x), torch.full((B,), step, dtype=torch.int32))['z']
            ref = R.reverse_step(rows[i], SCALE, x.cpu(), z.cpu(), None if i == K - 1 else noise[i + 1], mask)
            bar = 2e-6 * max(1.0, float(ref.abs().max()))
            worst = max(worst, mdiff(rec[i], ref) / bar)
    print('few-step partial %s eta %s: worst |dx| / bar over %d iterates = %.3f' % (sampler, eta, K, worst))
    assert worst <= 1.0


# --------------------------------------------------------------- 9. the start state
def test_start_state_is_q_samples(genie20):
    from genie2_amd import pack
    from genie2_amd.sampler import UnconditionalSampler, prepare_init_structure
    f = O.empty_features([40, 33])
    eng = genie20.model.engine()
    eng.bind_features(f)
    genie20.model._bound = None
    mask = f['residue_mask']
    x_in = prepare_init_structure(walk(2, 40, 4) + 25.0, mask)
    z0 = torch.randn(2, 40, 3, generator=torch.Generator().manual_seed(2))
    sched = pack.schedule_tensors(T20)
    smp = UnconditionalSampler(genie20)
    for t0 in (1, 7, 20):
        trans, rots = smp.start_state(eng, x_in, (z0 * mask.unsqueeze(-1)).cuda(), t0)
        c0, c1 = float(sched['sqrt_alphas_cumprod'][t0]), float(sched['sqrt_one_minus_alphas_cumprod'][t0])
        want = (c0 * x_in.double() + c1 * z0.double()) * mask.unsqueeze(-1).double()
        err = ((trans.cpu().double() - want).abs() / (1.0 + want.abs())).max()
        print('start state t0 = %d: worst |dx| / (1e-6 (1 + |x|)) = %.3f' % (t0, float(err) / 1e-6))
        assert float(err) <= 1e-6
        assert float(trans[1, 33:].abs().max()) == 0.0
        assert torch.equal(rots, eng.frenet(trans))


# --------------------------------------------------------------- 10. scaffold: re-scaffold a previous run's designs (the CLI)
@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory, base_weights):
    """results/base: the T = 20 model as the CLIs load it."""
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('results'))
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps %d\n' % T20)
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return ['--name', 'base', '--epoch', '7', '--rootdir', root, '--scale', str(SCALE)]


def _rmsd_line(path):
    text = open(path).read()
    assert text.startswith('# rmsd ') and text.endswith('\n') and text.count('\n') == 1, text
    value = text.split()[2]
    assert len(value.split('.')[1]) == 3
    return float(value)


def test_scaffold_cli_rescaffolds_a_previous_run(tmp_path, checkpoint):
    from genie2_amd import features as F
    from genie2_amd.sample_scaffold import ScaffoldRunner, build_parser
    out1, out2 = str(tmp_path / 'out1'), str(tmp_path / 'out2')
    common = checkpoint + ['--datadir', GOLDEN, '--motif_name', NAME, '--num_samples', '2', '--batch_size', '2']
    np.random.seed(3)
    torch.manual_seed(3)
    with hard_time_limit(240):
        a = build_parser().parse_args(common + ['--outdir', out1, '--num_steps', '4'])
        ScaffoldRunner().run(vars(a), a.num_devices)
        d1 = os.path.join(out1, 'motif=' + NAME)
        first = {x: _ca_coordinates(os.path.join(d1, 'pdbs', x + '.pdb')) for x in (NAME + '_0', NAME + '_1')}
        assert len({len(v) for v in first.values()}) == 2, 'the from-noise batch is meant to be ragged: another seed'
        os.remove(os.path.join(d1, 'motif_pdbs', NAME + '_0.pdb'))            # an orphan: skipped
        a = build_parser().parse_args(common + ['--outdir', out2, '--input_dir', out1, '--start_step', '5', '--write_start_rmsd'])
        state = np.random.get_state()[1].copy()
        ScaffoldRunner().run(vars(a), a.num_devices)
        assert np.array_equal(np.random.get_state()[1], state)                 # the features of a design take no draw
    d2 = os.path.join(out2, 'motif=' + NAME)
    names = [NAME + '_1_0', NAME + '_1_1']
    assert sorted(os.listdir(d2)) == ['motif_pdbs', 'pdbs', 'start_rmsd']
    assert sorted(os.listdir(os.path.join(d2, 'pdbs'))) == [n + '.pdb' for n in names]
    assert sorted(os.listdir(os.path.join(d2, 'motif_pdbs'))) == [n + '.pdb' for n in names]
    assert sorted(os.listdir(os.path.join(d2, 'start_rmsd'))) == [n + '.txt' for n in names]
    want = F.create_np_features_from_design(os.path.join(d1, 'pdbs', NAME + '_1.pdb'), os.path.join(d1, 'motif_pdbs', NAME + '_1.pdb'))
    motif1 = open(os.path.join(d1, 'motif_pdbs', NAME + '_1.pdb')).read()
    for n in names:
        ca = _ca_coordinates(os.path.join(d2, 'pdbs', n + '.pdb'))
        assert ca.shape == first[NAME + '_1'].shape and np.isfinite(ca).all()
        assert open(os.path.join(d2, 'motif_pdbs', n + '.pdb')).read() == motif1       # the same motif rows
        got = F.create_np_features_from_design(os.path.join(d2, 'pdbs', n + '.pdb'), os.path.join(d2, 'motif_pdbs', n + '.pdb'))
        for k in ('fixed_sequence_mask', 'fixed_structure_mask', 'fixed_group', 'aatype'):
            assert np.array_equal(got[k], want[k]), k
        r = _rmsd_line(os.path.join(d2, 'start_rmsd', n + '.txt'))
        print('%s: start RMSD %.3f' % (n, r))
        assert np.isfinite(r) and r >= 0.0
    assert not np.array_equal(_ca_coordinates(os.path.join(d2, 'pdbs', names[0] + '.pdb')),
                              _ca_coordinates(os.path.join(d2, 'pdbs', names[1] + '.pdb')))


def test_scaffold_sampler_takes_a_design(tmp_path, genie20):
    """The sampler itself on a design: the conditioning features of the first run, its coordinates as the start."""
    from genie2_amd import features as F
    from genie2_amd.sampler import ScaffoldSampler
    smp = ScaffoldSampler(genie20)
    p1 = {'filepath': PROBLEM, 'scale': SCALE, 'strength': 0, 'num_samples': 2, 'outdir': str(tmp_path / 'a'), 'prefix': 'd', 'offset': 0,
          'num_steps': 4}
    np.random.seed(3)
    torch.manual_seed(3)
    with hard_time_limit(120):
        smp.on_sample_start(p1)
        run1 = smp._sample(p1)
        smp.on_sample_end(p1, run1)
        assert smp.last_start_rmsd is None
        p2 = dict(p1, outdir=str(tmp_path / 'b'), design_filepath=str(tmp_path / 'a' / 'pdbs' / 'd_1.pdb'),
                  motif_filepath=str(tmp_path / 'a' / 'motif_pdbs' / 'd_1.pdb'), start_step=5, num_steps=None, prefix='d_1')
        run2 = smp._sample(p2)
    assert len(run1[0]['residue_mask']) != len(run1[1]['residue_mask'])
    for r in run2:
        assert np.isfinite(r['atom_positions']).all() and r['atom_positions'].shape == run1[1]['atom_positions'].shape
        for k in ('fixed_sequence_mask', 'fixed_structure_mask', 'fixed_group', 'aatype', 'residue_index'):
            assert np.array_equal(r[k], run1[1][k]), k
    assert smp.last_start_rmsd.shape == (2,) and bool(torch.isfinite(smp.last_start_rmsd).all())
    with pytest.raises(ValueError, match='start_step.*missing'):
        smp._sample(dict(p2, start_step=None))


# --------------------------------------------------------------- 11. twisted: a constant potential is the unconditional partial run
@pytest.mark.parametrize('systems', [False, True])
@pytest.mark.parametrize('num_steps', [None, 4])
def test_twisted_partial_with_a_constant_potential_is_the_unconditional_partial_run(genie20, systems, num_steps):
    """Printed on the MI355X: |dx| / (2e-3 rms) = 0.001 without num_steps and 0.000 with num_steps = 4, for one system and for S = K = 2."""
    from genie2_amd.sampler import UnconditionalSampler
    from genie2_amd.smc import TwistedSampler
    B, t0 = 4, 7
    n = t0 if num_steps is None else num_steps
    x_in = walk(1, N, 6)[0]
    noise = torch.randn(n, B, N, 3, generator=torch.Generator().manual_seed(12))
    base = _base(B, init_structure=x_in, start_step=t0, noise=noise, num_steps=num_steps)
    tw = TwistedSampler(genie20)
    extra = dict(twisting_function=lambda x0, step: (x0 * 0).sum(dim=(1, 2)), last_unguided_steps=0, ess_threshold=0.0)
    if systems:
        extra.update(num_samples=2, num_particles=2)
    with hard_time_limit(240):
        ref = xyz(UnconditionalSampler(genie20)._sample(dict(base)))
        got = xyz(tw._sample(dict(base, **extra)))
    rms = float(ref.pow(2).mean().sqrt())
    print('twisted partial, constant potential (systems %s, num_steps %s): |dx| / (2e-3 rms) = %.3f'
          % (systems, num_steps, mdiff(got, ref) / (2e-3 * rms)))
    assert mdiff(got, ref) <= 2e-3 * rms
    assert len(tw.ess_trace) == n - 1
    if systems:
        assert tuple(tw.ess_trace.shape) == (n - 1, 2) and tw.resampled_at == [[], []]
    else:
        assert tw.resampled_at == []
    assert tw.last_start_rmsd.shape == (B,)


# --------------------------------------------------------------- 12. guided partial
def test_guided_partial_run_reports_a_fit_for_every_sample(genie20):
    from genie2_amd import pack
    from genie2_amd.smc import TwistedSampler
    B, t0 = 4, T20 // 2
    segs = segments_6e6r()
    abar = pack.schedule_tensors(T20)['alphas_cumprod'].cuda()
    pot = _pot(segs, N, abar, tausq=0.5, align='rigid')
    x_in = walk(B, N, 9)
    far = pot.locate(x_in.cuda())['rmsd'].cpu()
    assert float(far.min()) > 1.0, far                     # a start whose motif RMSD is large
    seen = []

    def twist(x0, step):
        seen.append(step)
        return pot(x0, step)

    twist.locate, twist.has_fit = pot.locate, pot.has_fit
    tw = TwistedSampler(genie20)
    torch.manual_seed(1)
    with hard_time_limit(240):
        out = tw._sample(_base(B, init_structure=x_in, start_step=t0, twisting_function=twist, last_unguided_steps=0, guidance_alpha=0.05,
                               ess_threshold=0.5))
    assert seen == list(range(t0, 0, -1))                  # the potential reads the timestep itself
    assert bool(torch.isfinite(xyz(out)).all())
    fit = tw.last_fit
    assert fit['rmsd'].shape == (B,) and bool(torch.isfinite(fit['rmsd']).all()) and fit['starts'].shape == (B, len(segs))
    assert len(tw.ess_trace) == t0 - 1 and all(1 <= s <= t0 for s in tw.resampled_at)
    print('guided partial: motif RMSD of the start %s, of the result %s' % (far.tolist(), fit['rmsd'].tolist()))


# --------------------------------------------------------------- the two unconditional CLIs
def test_unconditional_clis_start_from_a_file(tmp_path, checkpoint):
    from genie2_amd import features as F
    from genie2_amd import sample_unconditional as su
    from genie2_amd import sample_unconditional_motif as sm
    f = F.create_empty_np_features([N])
    f['atom_positions'] = walk(1, N, 13)[0].numpy().astype(float)
    pdb = str(tmp_path / 'in.pdb')
    F.save_np_features_to_pdb(f, pdb)
    partial = ['--input_pdb', pdb, '--start_step', '4', '--write_start_rmsd', '--num_samples', '3', '--batch_size', '2']
    np.random.seed(0)
    torch.manual_seed(0)
    with hard_time_limit(240):
        out = str(tmp_path / 'u')
        a = su.build_parser().parse_args(checkpoint + partial + ['--outdir', out])
        su.UnconditionalRunner().run(vars(a), a.num_devices, a.sequential_order)
        out2 = str(tmp_path / 'm')
        a = sm.build_parser().parse_args(checkpoint + partial + ['--outdir', out2, '--motif_file', PROBLEM, '--align', 'rigid', '--num_particles', '2',
                                                                 '--num_steps', '3', '--last_unguided_steps', '0', '--motif_groups', 'file'])
        sm.MotifRunner().run(vars(a), a.num_devices, a.sequential_order)
    start = _ca_coordinates(pdb)
    for d in (out, out2):
        names = ['%d_%d' % (N, i) for i in range(3)]
        assert sorted(os.listdir(os.path.join(d, 'pdbs'))) == [n + '.pdb' for n in names]
        assert sorted(os.listdir(os.path.join(d, 'start_rmsd'))) == [n + '.txt' for n in names]
        for n in names:
            ca = _ca_coordinates(os.path.join(d, 'pdbs', n + '.pdb'))
            assert ca.shape == (N, 3) and np.isfinite(ca).all()
            r = _rmsd_line(os.path.join(d, 'start_rmsd', n + '.txt'))
            from genie2_amd.sampler import start_rmsd
            want = float(start_rmsd(torch.tensor(ca)[None], torch.tensor(start)[None], torch.ones(1, N))[0])
            print('%s %s: start RMSD %.3f, from the two files %.3f' % (d[-1], n, r, want))
            assert abs(r - want) <= 2e-3                   # (the PDB rounds coordinates to 3 decimals)
