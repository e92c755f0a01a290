"""Partial diffusion, host side: pack.partial_steps, the samplers' parameter checks (a model on the CPU: nothing may reach the
library), the features of an existing scaffold design, the CLIs' flags and pairing, the start-RMSD report, and the tail equivalence
of test_partial_gpu.py through a CPU stand-in for the engine over the oracle (tests/_partial.py)."""
import math
import os

import numpy as np
import pytest
import torch

import _partial as P
from conftest import GOLDEN

PROBLEM = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')
BASE = ['--name', 'b', '--epoch', '1', '--scale', '0.6', '--outdir', 'o']


# --------------------------------------------------------------- 1. the step list
def test_partial_steps():
    from genie2_amd import pack
    for T in (20, 1000):
        for K in (1, 2, 7, T):
            assert pack.partial_steps(T, T, K) == pack.respaced_steps(T, K)
    for T, t0 in ((20, 13), (1000, 300), (1000, 1), (50, 2)):
        for K in sorted({1, min(2, t0), min(4, t0), t0}):
            s = pack.partial_steps(T, t0, K)
            assert len(s) == K and s[0] == t0 and all(a > b for a, b in zip(s, s[1:])) and all(isinstance(v, int) for v in s)
            assert s[-1] == (1 if K > 1 else t0)
        assert pack.partial_steps(T, t0, 1) == [t0]
        assert pack.partial_steps(T, t0, t0) == list(range(t0, 0, -1))
    assert pack.partial_steps(20, 13, 4) == [13, 9, 5, 1]
    for args, word in (((20, 13, 0), '0'), ((20, 13, 14), '14'), ((20, 0, 1), '0'), ((20, 21, 1), '21'), ((20, 13, 2.5), '2.5'),
                       ((20, 6.5, 2), '6.5'), ((20, True, 1), 'True')):
        with pytest.raises(ValueError, match=word.replace('.', r'\.')):
            pack.partial_steps(*args)


# --------------------------------------------------------------- 2. parameter checks, before the device
def _params(**over):
    return dict({'length': 12, 'scale': 0.6, 'num_samples': 2, 'outdir': 'unused', 'prefix': 'x', 'offset': 0}, **over)


def _samplers():
    from genie2_amd.sampler import ScaffoldSampler, UnconditionalSampler
    from genie2_amd.smc import TwistedSampler
    model = P.host_model(10)
    twist = {'twisting_function': lambda x0, step: (x0 * 0).sum(dim=(1, 2))}
    return [(UnconditionalSampler(model), {}), (TwistedSampler(model), twist), (TwistedSampler(model), dict(twist, num_particles=2)),
            (ScaffoldSampler(model), {'filepath': PROBLEM})]


def test_param_validation_never_reaches_the_library():
    from genie2_amd.capi import GenieError
    x = torch.randn(12, 3)
    for sampler, extra in _samplers():
        scaffold = 'filepath' in extra
        B = 4 if 'num_particles' in extra else 2

        def run(**kw):
            np.random.seed(0)
            return sampler._sample(_params(**extra, **kw))

        with pytest.raises(ValueError, match='init_structure.*missing'):
            run(start_step=3)
        with pytest.raises(ValueError, match='start_step.*missing'):
            run(init_structure=x)
        for bad in (0, 11, True, 2.5, float('nan'), float('inf'), '3'):
            with pytest.raises(ValueError, match='start_step must be an integer in 1..10, got'):
                run(init_structure=x, start_step=bad)
        with pytest.raises(ValueError, match=r'init_structure must be \[\d+, 3\] or \[\d+, \d+, 3\], got \(11, 3\)'):
            run(init_structure=torch.randn(11, 3), start_step=3)
        with pytest.raises(ValueError, match=r'got \(3, 12, 3\)'):
            run(init_structure=torch.randn(3, 12, 3), start_step=3)
        if scaffold:
            continue                                  # (its length is drawn per sample: the remaining cases need a fixed N)
        nan = x.clone()
        nan[5, 1] = float('nan')
        with pytest.raises(ValueError, match='non-finite'):
            run(init_structure=nan, start_step=3)
        with pytest.raises(ValueError, match='non-finite'):
            run(init_structure=np.full((12, 3), np.inf), start_step=3)
        with pytest.raises(ValueError, match=r'noise must be \[n, B, N, 3\] = \[3, .*got \(4, %d, 12, 3\)' % B):
            run(init_structure=x, start_step=3, noise=torch.randn(4, B, 12, 3))
        with pytest.raises(ValueError, match=r'noise must be \[n, B, N, 3\] = \[2, .*got \(3, %d, 12, 3\)' % B):
            run(init_structure=x, start_step=3, num_steps=2, noise=torch.randn(3, B, 12, 3))
        with pytest.raises(ValueError, match=r'noise must be \[n, B, N, 3\] = \[3, %d, 12, 3\].*got \(3, %d, 11, 3\)' % (B, B)):
            run(init_structure=x, start_step=3, noise=torch.randn(3, B, 11, 3))
        with pytest.raises(ValueError, match=r'num_steps must be an integer in 1..3 with start_step=3, got 4'):
            run(init_structure=x, start_step=3, num_steps=4)
        # a valid request gets as far as the engine, which does not exist on the CPU: the checks above came before it
        with pytest.raises(GenieError):
            run(init_structure=x, start_step=3, noise=torch.randn(3, B, 12, 3))
    for sampler, extra in _samplers()[1:3]:
        with pytest.raises(ValueError, match="the twisted sampler has the ancestral kernel only, got sampler='ddim'"):
            sampler._sample(_params(**extra, init_structure=x, start_step=3, num_steps=2, sampler='ddim'))
    scaffold = _samplers()[3][0]
    with pytest.raises(ValueError, match='motif_filepath is missing'):
        scaffold._sample(_params(filepath=PROBLEM, design_filepath='d.pdb', start_step=3))
    with pytest.raises(ValueError, match='design_filepath is missing'):
        scaffold._sample(_params(filepath=PROBLEM, motif_filepath='m.pdb', start_step=3))


def test_init_structure_is_centred_on_valid_residues_and_padded_rows_are_zero():
    from genie2_amd.sampler import prepare_init_structure
    mask = np.zeros((2, 40), dtype=int)
    mask[0, :40] = 1
    mask[1, :33] = 1
    x = torch.randn(2, 40, 3, dtype=torch.float64) * 8 + 30
    out = prepare_init_structure(x, mask)
    assert out.dtype == torch.float32 and out.shape == (2, 40, 3)
    assert float(out[1, 33:].abs().max()) == 0.0
    for b, n in ((0, 40), (1, 33)):
        want = x[b, :n] - x[b, :n].mean(dim=0, keepdim=True)
        assert float((out[b, :n].double() - want).abs().max()) <= 1e-5
    shared = prepare_init_structure(x[0].numpy(), mask)       # [N, 3]: every sample, each centred over its own mask
    assert float((shared[1, :33].double().mean(dim=0)).abs().max()) <= 1e-5 and float(shared[1, 33:].abs().max()) == 0.0
    x[1, 36] = float('nan')                                  # non-finite anywhere, a padded row included
    with pytest.raises(ValueError, match='non-finite'):
        prepare_init_structure(x, mask)


def test_sample_loop_refuses_rows_outside_its_noise_before_the_library():
    """GenieEngine.sample_loop's check of the rows genie_sample_loop will read, on an engine object without a library behind it: a
    case that passed the check would fail on the missing handle (AttributeError), not with the ValueError."""
    from genie2_amd.engine import GenieEngine
    eng = object.__new__(GenieEngine)
    eng.device, eng.dims, eng.B, eng.N = torch.device('cpu'), {'n_timestep': 20}, 2, 40
    state = (torch.zeros(2, 40, 3), torch.zeros(2, 40, 3, 3))
    tail = torch.zeros(7, 2, 40, 3)
    # entered at 7 the loop reads rows 14..19 of the 20-row layout: `tail` has to cover them
    for kw in (dict(first_step=7, noise_first=12), dict(first_step=9, noise_first=13), dict(first_step=7, noise_first=15),
               dict(first_step=20, noise_first=13), dict(first_step=7, noise_first=-1), dict(first_step=20)):
        with pytest.raises(ValueError, match='noise must hold rows'):
            eng.sample_loop(tail, 0.6, state=state, **kw)
    with pytest.raises(ValueError, match='noise must hold rows'):
        eng.sample_loop(torch.zeros(7, 2, 39, 3), 0.6, first_step=7, state=state, noise_first=13)
    for kw in (dict(first_step=7, noise_first=13), dict(first_step=8, noise_first=13), dict(first_step=7, noise_first=14),
               dict(first_step=1, noise_first=19), dict(first_step=7, last_step=5, noise_first=14)):
        with pytest.raises(AttributeError):
            eng.sample_loop(tail, 0.6, state=state, **kw)


# --------------------------------------------------------------- 3. the features of an existing design
FEATURE_KEYS = ('aatype', 'num_chains', 'num_residues', 'num_residues_per_chain', 'atom_positions', 'residue_mask',
                'residue_index', 'chain_index', 'fixed_sequence_mask', 'fixed_structure_mask', 'fixed_group', 'interface_mask')


def _write_design(f, tmp_path, tag):
    from genie2_amd import features as F
    from genie2_amd.motif import save_motif_pdb
    design, motif = str(tmp_path / ('design%s.pdb' % tag)), str(tmp_path / ('motif%s.pdb' % tag))
    g = dict(f, atom_positions=np.random.RandomState(7).randn(len(f['residue_mask']), 3) * 10)      # any coordinates
    F.save_np_features_to_pdb(g, design)
    save_motif_pdb(PROBLEM, f['fixed_sequence_mask'], motif)
    return design, motif


@pytest.mark.parametrize('seed', range(4))
def test_features_from_design_round_trip(seed, tmp_path):
    from genie2_amd import features as F
    np.random.seed(seed)
    f = F.create_np_features_from_motif_pdb(PROBLEM)
    design, motif = _write_design(f, tmp_path, '')
    state = np.random.get_state()[1].copy()
    g = F.create_np_features_from_design(design, motif)
    assert np.array_equal(np.random.get_state()[1], state)                     # no random draw
    assert tuple(g) == tuple(f) and set(g) == set(FEATURE_KEYS)
    for k in FEATURE_KEYS:
        assert g[k].dtype == f[k].dtype and g[k].shape == f[k].shape and np.array_equal(g[k], f[k]), k


def test_features_from_design_name_the_first_mismatch(tmp_path):
    from genie2_amd import features as F
    np.random.seed(1)
    f = F.create_np_features_from_motif_pdb(PROBLEM)
    design, motif = _write_design(f, tmp_path, '')
    lines = open(motif).read().splitlines(keepends=True)
    first = int(lines[0][22:26])
    free = next(i + 1 for i, on in enumerate(f['fixed_sequence_mask']) if not on)

    def variant(name, edit, target=motif, source=None):
        out = str(tmp_path / name)
        src = open(target).read().splitlines(keepends=True) if source is None else source
        with open(out, 'w') as fh:
            fh.writelines(edit(src))
        return out

    # one motif residue moved to a scaffold position: all its records, as a re-indexing would move them
    moved = variant('moved.pdb', lambda ls: [ln[:22] + str(free).rjust(4) + ln[26:] if int(ln[22:26]) == first else ln for ln in ls])
    with pytest.raises(ValueError, match='motif positions: residue %d' % min(first, free)):
        F.create_np_features_from_design(design, moved)
    # its C-alpha record alone
    ca_only = variant('ca.pdb', lambda ls: [ln[:22] + str(free).rjust(4) + ln[26:] if int(ln[22:26]) == first and ln[13:15] == 'CA' else ln
                                            for ln in ls])
    with pytest.raises(ValueError):
        F.create_np_features_from_design(design, ca_only)
    n = len(f['residue_mask'])
    beyond = variant('beyond.pdb', lambda ls: [ln[:22] + str(n + 3).rjust(4) + ln[26:] if int(ln[22:26]) == first else ln for ln in ls])
    with pytest.raises(ValueError, match='length: the motif file places residue %d' % (n + 3)):
        F.create_np_features_from_design(design, beyond)
    retyped = variant('retyped.pdb', lambda ls: [ln[:17] + 'TRP' + ln[20:] if int(ln[22:26]) == first else ln for ln in ls])
    with pytest.raises(ValueError, match='residue types: residue %d is ALA in the design and TRP' % first):
        F.create_np_features_from_design(design, retyped)
    regrouped = variant('regrouped.pdb', lambda ls: [ln[:72] + 'B   ' + ln[76:] if int(ln[22:26]) == first else ln for ln in ls])
    with pytest.raises(ValueError, match='motif positions: residue %d is in group A in the design and B' % first):
        F.create_np_features_from_design(design, regrouped)
    short = variant('short.pdb', lambda ls: ls[:-1], target=design)
    if f['fixed_sequence_mask'][-1]:
        with pytest.raises(ValueError, match='length'):
            F.create_np_features_from_design(short, motif)
    else:
        assert int(F.create_np_features_from_design(short, motif)['num_residues']) == n - 1


# --------------------------------------------------------------- 4. CLIs
def test_cli_flags_come_together():
    import genie.sample_scaffold as gs
    import genie.sample_unconditional as gu
    import genie.sample_unconditional_motif as gm
    from genie2_amd import sample_scaffold, sample_unconditional, sample_unconditional_motif
    for mod, flag, extra in ((sample_unconditional, '--input_pdb', []), (gu, '--input_pdb', []),
                             (sample_unconditional_motif, '--input_pdb', ['--motif_file', PROBLEM]), (gm, '--input_pdb', ['--motif_file', PROBLEM]),
                             (sample_scaffold, '--input_dir', []), (gs, '--input_dir', [])):
        base = BASE + extra
        a = mod.build_parser().parse_args(base)
        assert (getattr(a, flag[2:]), a.start_step, a.write_start_rmsd) == (None, None, False)
        a = mod.build_parser().parse_args(base + [flag, 'x', '--start_step', '300', '--write_start_rmsd'])
        assert (getattr(a, flag[2:]), a.start_step, a.write_start_rmsd) == ('x', 300, True)
        for alone in ([flag, 'x'], ['--start_step', '300'], ['--write_start_rmsd'], ['--start_step', '2.5', flag, 'x']):
            with pytest.raises(SystemExit):
                mod.build_parser().parse_args(base + alone)
    a = sample_unconditional_motif.build_parser().parse_args(
        BASE + ['--motif_file', PROBLEM, '--input_pdb', 'x', '--start_step', '5', '--align', 'rigid', '--motif_groups', 'file',
                '--num_particles', '4', '--num_steps', '3'])
    assert (a.align, a.motif_groups, a.num_particles, a.num_steps, a.start_step) == ('rigid', 'file', 4, 3, 5)


def test_unconditional_cli_collapses_to_the_files_length(tmp_path, capsys):
    from genie2_amd import features as F
    from genie2_amd.sample_unconditional import UnconditionalRunner, build_parser, check_start_step_flag
    f = F.create_empty_np_features([37])
    f['atom_positions'] = np.random.RandomState(0).randn(37, 3) * 10
    pdb = str(tmp_path / 'in.pdb')
    F.save_np_features_to_pdb(f, pdb)
    a = vars(build_parser().parse_args(BASE + ['--input_pdb', pdb, '--start_step', '300', '--min_length', '50']))
    assert UnconditionalRunner().create_tasks(a) == [{'length': 37}]
    assert 'are ignored' in capsys.readouterr().out
    c = UnconditionalRunner().create_constants(a)
    assert c['start_step'] == 300 and c['init_structure'].shape == (37, 3) and c['write_start_rmsd'] is False
    assert UnconditionalRunner.partial_params(c).keys() == {'init_structure', 'start_step'}
    plain = UnconditionalRunner().create_constants(vars(build_parser().parse_args(BASE)))
    assert UnconditionalRunner.partial_params(plain) == {} and 'init_structure' not in plain
    # --start_step against the model's n_timestep, from its configuration file alone
    (tmp_path / 'm').mkdir()
    (tmp_path / 'm' / 'configuration').write_text('name m\nnumTimesteps 200\n')
    check_start_step_flag({'rootdir': str(tmp_path), 'name': 'm', 'start_step': 200})
    with pytest.raises(SystemExit, match='start_step must be an integer in 1..200, got 201'):
        check_start_step_flag({'rootdir': str(tmp_path), 'name': 'm', 'start_step': 201})
    with pytest.raises(SystemExit, match='got 0'):
        UnconditionalRunner().create_constants(dict(a, rootdir=str(tmp_path), name='m', start_step=0))


def test_scaffold_cli_pairs_designs_and_skips_orphans(tmp_path, capsys):
    from genie2_amd.sample_scaffold import ScaffoldRunner, build_parser, pair_designs
    run = tmp_path / 'run' / 'motif=6E6R_long'
    for sub, names in (('pdbs', ('6E6R_long_0', '6E6R_long_1', '6E6R_long_7')), ('motif_pdbs', ('6E6R_long_0', '6E6R_long_1'))):
        (run / sub).mkdir(parents=True)
        for n in names:
            (run / sub / (n + '.pdb')).write_text('')
    for root in (tmp_path / 'run', run):                      # the outdir, or one of its motif=<name> folders
        pairs = pair_designs(str(root))
        assert [p[0] for p in pairs] == ['6E6R_long_0', '6E6R_long_1']
        assert all(d == str(run / 'pdbs' / (x + '.pdb')) and m == str(run / 'motif_pdbs' / (x + '.pdb')) for x, d, m in pairs)
        out = capsys.readouterr().out
        assert out.count('skipping') == 1 and '6E6R_long_7.pdb' in out
    a = vars(build_parser().parse_args(BASE + ['--input_dir', str(tmp_path / 'run'), '--start_step', '5', '--write_start_rmsd']))
    tasks = ScaffoldRunner().create_tasks(a)
    assert [(t['motif_name'], t['design']) for t in tasks] == [('6E6R_long', '6E6R_long_0'), ('6E6R_long', '6E6R_long_1')]
    c = ScaffoldRunner().create_constants(a)
    assert c['start_step'] == 5 and c['write_start_rmsd'] is True


# --------------------------------------------------------------- 5. the start-RMSD report
def _walk(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cumsum(torch.randn(n, 3, generator=g, dtype=torch.float64) * 2.2, dim=0)


def test_start_rmsd(tmp_path):
    from genie2_amd.sample_unconditional import write_start_rmsd
    from genie2_amd.sampler import start_rmsd
    x = torch.stack([_walk(40, 1), _walk(40, 2)])
    c, s = math.cos(0.7), math.sin(0.7)
    rz = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(2.1), -math.sin(2.1)], [0.0, math.sin(2.1), math.cos(2.1)]], dtype=torch.float64)
    rot = rz @ rx
    assert abs(float(torch.linalg.det(rot)) - 1.0) < 1e-12
    moved = x @ rot.T + torch.tensor([5.0, -30.0, 12.0], dtype=torch.float64)
    mask = torch.ones(2, 40, dtype=torch.int32)
    r = start_rmsd(moved, x, mask)
    assert r.dtype == torch.float64 and r.shape == (2,) and float(r.max()) <= 1e-9
    mirror = x * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)
    assert float(torch.linalg.matrix_rank(x[0] - x[0].mean(dim=0, keepdim=True))) == 3          # not planar
    assert float(start_rmsd(mirror, x, mask).min()) > 0.1
    assert float(start_rmsd(mirror @ rot.T, x, mask).min()) > 0.1
    # padded rows are ignored, whatever they hold
    mask[1, 33:] = 0
    junk = moved.clone()
    junk[1, 33:] = 1e6
    r2 = start_rmsd(junk, x, mask)
    assert float(r2.max()) <= 1e-9
    # the report's own format
    write_start_rmsd(torch.tensor([0.12345, 2.0], dtype=torch.float64), str(tmp_path / 'start_rmsd'), ['40_0', '40_1'])
    assert (tmp_path / 'start_rmsd' / '40_0.txt').read_text() == '# rmsd 0.123\n'
    assert (tmp_path / 'start_rmsd' / '40_1.txt').read_text() == '# rmsd 2.000\n'
    # against a direct restatement on a noisy copy (float32 inputs as the samplers pass them)
    noisy = (moved + 0.5 * torch.randn(2, 40, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)).float()
    got = start_rmsd(noisy, x.float(), torch.ones(2, 40))
    for b in range(2):
        a, y = noisy[b].double(), x[b].float().double()
        a, y = a - a.mean(0), y - y.mean(0)
        u, sv, vh = torch.linalg.svd(a.T @ y)
        d = torch.sign(torch.linalg.det(u @ vh))
        want = math.sqrt(max(0.0, float((a.pow(2).sum() + y.pow(2).sum() - 2 * (sv[0] + sv[1] + d * sv[2])) / 40)))
        assert abs(float(got[b]) - want) <= 1e-9 * max(1.0, want)


# --------------------------------------------------------------- 6. tail equivalence over the oracle
def test_unconditional_tail_equivalence_over_the_oracle():
    """test_partial_gpu.py's tail test with the engine replaced by the oracle (float32, CPU): the same case, the same bar."""
    from genie2_amd.sampler import UnconditionalSampler
    T, B, N, scale = 20, 2, 40, 0.6
    model, eng = P.oracle_model(T)
    sampler = UnconditionalSampler(model)
    Z = torch.randn(T, B, N, 3, generator=torch.Generator().manual_seed(11))
    from oracle import genie_oracle as O
    eng.bind_features(O.empty_features([N] * B))
    ref, _, rec = eng.sample_loop(Z, scale, record=True)
    ref = ref.clone()
    rms = float(ref.pow(2).mean().sqrt())
    for t0 in (1, 7, 19, 20):
        eng.rows_read = []
        got = P.tail_case(eng, sampler, T, t0, Z, rec, scale, B, N)
        ratio = float((got - ref).abs().max()) / (1e-4 * rms)
        print('oracle tail t0 = %d: |dx| / (1e-4 rms) = %.4f, noise rows read by the loop %s' % (t0, ratio, eng.rows_read))
        assert ratio <= 1.0, t0
        assert eng.rows_read == list(range(1 if t0 < T else 2, t0))            # noise[0] is the forward draw alone
        assert sampler.last_start_rmsd.shape == (B,) and bool(torch.isfinite(sampler.last_start_rmsd).all())
    # the few-step form: the steps of pack.partial_steps, the state carried in
    from genie2_amd import pack
    x_in = torch.cumsum(torch.randn(N, 3, generator=torch.Generator().manual_seed(5)) * 2.2, dim=0)
    noise = torch.randn(4, B, N, 3, generator=torch.Generator().manual_seed(6))
    got = sampler._sample({'length': N, 'scale': scale, 'num_samples': B, 'init_structure': x_in, 'start_step': 13, 'num_steps': 4,
                           'noise': noise, 'sampler': 'ddim', 'eta': 0.5})
    sched = pack.schedule_tensors(T)
    xc = (x_in - x_in.mean(dim=0, keepdim=True)).expand(B, N, 3)
    start = sched['sqrt_alphas_cumprod'][13] * xc + sched['sqrt_one_minus_alphas_cumprod'][13] * noise[0]
    steps = pack.partial_steps(T, 13, 4)
    want = eng.sample_loop_steps(noise, scale, steps, pack.reverse_coefficients(T, steps, 'ddim', 0.5),
                                 state=(start.clone(), eng.frenet(start)))[0]
    assert float((torch.tensor(np.stack([g['atom_positions'] for g in got])) - want).abs().max()) <= 1e-4 * rms
