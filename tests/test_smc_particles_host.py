"""Independent particle systems, host side: the float64 oracle of the GPU tests against smc.py's own functions, the C-ABI symbol and
its refusals, the sampler's parameter checks and the CLI flag.  CPU only."""
import os
import re

import pytest
import torch

import _smc_particles as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTIF = os.path.join(ROOT, 'tests', 'golden', 'motif_problem_6E6R.pdb')


@pytest.mark.parametrize('K,N,sigma,seed,fraction', [(1, 2, 0.2, 0, 0.5), (5, 40, 0.2, 0, 0.5), (5, 40, 0.2, 0, 0.99), (64, 40, 0.2, 1, 0.5),
                                                     (64, 40, 0.2, 1, 0.99), (8, 257, 0.02, 0, 0.99)])
def test_oracle_at_one_system_is_smc_py_in_float64(K, N, sigma, seed, fraction):
    """At S = 1 the oracle is smc.py's functions on the same float64 inputs: the indices exactly, the rest to 1e-12.  (A fraction of
    0.99 makes the even, gently weighted system of the recipe resample as well.)"""
    from genie2_amd import smc
    inp = P.make_inputs(1, K, N, sigma, seed)
    ref = P.oracle(1, K, inp, fraction)
    d = {k: v.double() for k, v in inp.items()}
    var = d['sigma'].reshape(()) ** 2
    log_rev = smc.log_normal_density(d['x_new'], d['mean_un'], var).sum(dim=(1, 2))
    log_tw = smc.log_normal_density(d['x_new'], d['mean_tw'], var).sum(dim=(1, 2))
    log_w_acc = ((log_rev + d['log_prob'] - log_tw) - d['log_proposal']) + d['log_w_acc']
    ess = smc.compute_ess_from_log_w(log_w_acc)
    assert abs(float(ess) - float(ref['ess'][0])) <= 1e-12 * K
    assert bool(ess < fraction * K) == bool(ref['resampled'][0])
    if bool(ref['resampled'][0]):
        _, zeros, idx = smc.systematic_resampling(d['x_new'], torch.softmax(log_w_acc, dim=0), float(d['u'][0]))
        assert torch.equal(idx, ref['index']) and float(zeros.abs().max()) == 0.0 and float(ref['log_w_acc'].abs().max()) == 0.0
        assert torch.equal(ref['log_proposal'], d['log_prob'][idx])
    else:
        acc = smc.normalize_log_weights(log_w_acc, dim=0) + torch.log(torch.tensor(float(K), dtype=torch.float64))
        assert float((acc - ref['log_w_acc']).abs().max()) <= 1e-12
        assert torch.equal(ref['index'], torch.arange(K)) and torch.equal(ref['log_proposal'], d['log_prob'])


def test_cases_exercise_both_branches_with_room_to_spare():
    """The input recipe does what the GPU tests rely on: even systems stay, odd ones resample, and no discrete output is close."""
    for S, K, N, sigma, seed in P.CASES:
        ref = P.oracle(S, K, P.make_inputs(S, K, N, sigma, seed))
        ess_margin, point_margin = P.margins(S, K, ref)
        print((S, K, N), 'ESS / K', (ref['ess'] / K).tolist(), 'margins (of K, of 1 / K)', ess_margin, point_margin)
        assert ref['resampled'].tolist() == [s % 2 == 1 for s in range(S)]
        assert ess_margin >= 0.05 and point_margin >= 1e-3


def test_symbol_is_declared_bound_and_exported():
    from genie2_amd import build, capi
    build.build()
    lib = capi.load_library()
    header = open(os.path.join(ROOT, 'include', 'genie_hip.h')).read()
    assert re.search(r'\bint genie_smc_reweight\s*\(', header) and re.search(r'\bsize_t genie_smc_reweight_work_bytes\s*\(', header)
    for name, n_args in (('genie_smc_reweight', P.N_ARGS), ('genie_smc_reweight_work_bytes', 3)):
        assert name in capi.SYMBOLS and len(capi.SYMBOLS[name][1]) == n_args and getattr(lib, name) is not None
    assert 'smc_step_kernels.hip' in build.SOURCES
    assert lib.genie_smc_reweight_work_bytes(2, 4, 40) >= 8 * 8
    assert lib.genie_smc_reweight_work_bytes(2, 65, 40) == 0 and lib.genie_smc_reweight_work_bytes(0, 4, 40) == 0


def test_entry_refuses_bad_arguments_without_a_device():
    from genie2_amd import build, capi
    build.build()
    lib = capi.load_library()
    S, K, N = 2, 4, 40
    # never dereferenced: every call below fails a check made on the host.  Spaced so that nothing overlaps.
    good = {k: 0x100000 * (i + 1) for i, k in enumerate(('x_new', 'mean_tw', 'mean_un', 'sigma', 'log_prob', 'u', 'log_proposal',
                                                          'log_w_acc', 'x_out', 'index_out', 'ess_out', 'resampled_out'))}
    work, need = 0x4000000, lib.genie_smc_reweight_work_bytes(S, K, N)

    def refused(word, S=S, K=K, N=N, ess_fraction=0.5, work=work, work_bytes=need, **over):
        rc = P.raw_call(lib, S, K, N, dict(good, **over), ess_fraction, work, work_bytes)
        msg = lib.genie_last_error(None)
        assert rc == -1 and b'genie_smc_reweight' in msg and word in msg, (rc, msg, word)

    for k in good:
        refused(b'null', **{k: 0})
    refused(b'null', work=0)
    refused(b'K', K=0)
    refused(b'K', K=65)
    refused(b'S', S=0)
    refused(b'N', N=0)
    refused(b'overlap', x_out=good['x_new'])
    refused(b'overlap', x_out=good['x_new'] + 4 * (S * K * N * 3 - 1))         # the last float of x_new
    refused(b'ess_fraction', ess_fraction=float('nan'))
    refused(b'ess_fraction', ess_fraction=float('inf'))
    refused(b'work_bytes', work_bytes=need - 1)


def test_sampler_refuses_bad_particle_parameters_before_any_work(tmp_path):
    from genie2_amd.smc import TwistedSampler
    tw = TwistedSampler(P.cpu_model(10))
    touched = []
    tw.create_np_features = lambda params: touched.append(1)                    # the first thing _sample does after the checks
    base = {'length': 12, 'scale': 0.6, 'num_samples': 2, 'outdir': str(tmp_path), 'prefix': 'x', 'offset': 0}
    for bad in (0, -1, 65, 2.5, True, '4'):
        with pytest.raises(ValueError, match='num_particles'):
            tw._sample(dict(base, num_particles=bad))
    for bad in ('worst', 'ALL', 1):
        with pytest.raises(ValueError, match='return_particles'):
            tw._sample(dict(base, num_particles=4, return_particles=bad))
    with pytest.raises(ValueError, match='num_particles'):
        tw._sample(dict(base, return_particles='best'))
    with pytest.raises(ValueError, match=r'\(10, 2, 12, 3\)'):                  # noise is [T, S K, N, 3]
        tw._sample(dict(base, num_particles=4, noise=torch.zeros(10, 2, 12, 3)))
    with pytest.raises(ValueError, match='resample_u'):
        tw._sample(dict(base, num_particles=4, resample_u=[[0.1, 0.1, 0.1]]))
    with pytest.raises(ValueError, match="ancestral kernel only.*'ddim'"):      # refused exactly as without particles
        tw._sample(dict(base, num_particles=4, num_steps=5, sampler='ddim'))
    assert touched == []


def test_cli_parses_num_particles():
    import genie.sample_unconditional_motif as gm
    from genie2_amd import sample_unconditional_motif as sm
    base = ['--name', 'b', '--epoch', '1', '--scale', '0.6', '--outdir', 'o', '--motif_file', MOTIF]
    for mod in (sm, gm):
        assert mod.build_parser().parse_args(base).num_particles is None
        assert mod.build_parser().parse_args(base + ['--num_particles', '16']).num_particles == 16
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(base + ['--num_particles', 'many'])
    assert sm.MotifRunner().create_constants(vars(sm.build_parser().parse_args(base)))['num_particles'] is None
    assert sm.MotifRunner().create_constants(vars(sm.build_parser().parse_args(base + ['--num_particles', '3'])))['num_particles'] == 3
    help_text = ' '.join(sm.build_parser().format_help().split())
    assert help_text.count('(not in the reference CLI)') == 7
