"""Few-step sampling, host side: the strided schedule and its coefficients (pack.respaced_steps / reverse_coefficients /
twisted_coefficients), the refusals of the samplers, the CLI flags and the two C-ABI symbols.  CPU only."""
import math
import os
import re
import types

import pytest
import torch

import _fewstep as R
from genie2_amd import pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('K', [2, 5, 10, 50, 100, 250, 999, 1000])
def test_respaced_steps_are_distinct_and_span_the_schedule(K):
    steps = pack.respaced_steps(1000, K)
    assert len(steps) == K and steps[0] == 1000 and steps[-1] == 1
    assert all(isinstance(s, int) for s in steps) and all(a > b for a, b in zip(steps, steps[1:]))
    ref = [int(round(1000 + (1 - 1000) * i / (K - 1))) for i in range(K)]
    assert all(abs(a - b) <= 1 for a, b in zip(steps, ref))            # (rint and round differ at exact halves only)
    if K == 1000:
        assert steps == list(range(1000, 0, -1))


def test_respaced_steps_edges_and_refusals():
    assert pack.respaced_steps(1000, 1) == [1000]
    assert pack.respaced_steps(20, 5) == [20, 15, 10, 6, 1]
    assert pack.respaced_steps(1, 1) == [1]
    for bad in (0, -3, 1001, 2.5):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            pack.respaced_steps(1000, bad)


def test_consecutive_ancestral_coefficients_are_the_schedule_tensors():
    T = 1000
    sched = pack.schedule_tensors(T)
    c = pack.reverse_coefficients(T, list(range(T, 0, -1)))
    assert c.dtype == torch.float64 and tuple(c.shape) == (T, 3)
    idx = torch.arange(T, 0, -1)
    w_z = (1.0 - sched['alphas'].double()) / sched['sqrt_one_minus_alphas_cumprod'].double()
    today = torch.stack([1.0 / sched['sqrt_alphas'].double(), -w_z / sched['sqrt_alphas'].double(), sched['sqrt_betas'].double()], dim=1)[idx]
    rel = ((c - today).abs() / today.abs()).max(dim=0).values
    print('worst relative difference to schedule_tensors (A, Bz, C):', rel.tolist())
    assert float(rel[0]) <= 1e-6 and float(rel[1]) <= 1e-4 and float(rel[2]) <= 1e-6


@pytest.mark.parametrize('sampler,eta', [('ancestral', 0.0), ('ddim', 0.0), ('ddim', 0.5), ('ddim', 1.0)])
def test_coefficients_match_the_float64_restatement(sampler, eta):
    T = 1000
    steps = pack.respaced_steps(T, 10)
    got = pack.reverse_coefficients(T, steps, sampler, eta)
    ref = torch.tensor(R.coefficient_rows(T, steps, sampler, eta), dtype=torch.float64)
    assert tuple(got.shape) == (10, 3)
    assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    if sampler == 'ddim' and eta == 0.0:
        assert float(got[:, 2].abs().max()) == 0.0
    if sampler == 'ddim' and eta == 1.0:            # eta = 1 is the ancestral variance
        anc = pack.reverse_coefficients(T, steps, 'ancestral')
        assert float((got[:, 2] - anc[:, 2] * torch.sqrt((1 - pack.alphas_cumprod64(T)[steps[1:] + [0]]) /
                                                         (1 - pack.alphas_cumprod64(T)[steps]))).abs().max()) <= 1e-12


def test_ddim_eta0_step_with_the_true_noise_lands_on_the_forward_marginal():
    T = 1000
    g = torch.Generator().manual_seed(3)
    abar = torch.tensor(R.abar64(T), dtype=torch.float64)
    for _ in range(20):
        t = int(torch.randint(2, T + 1, (1,), generator=g))
        s = int(torch.randint(1, t, (1,), generator=g))
        x0 = 5.0 * torch.randn(7, 3, generator=g, dtype=torch.float64)
        z = torch.randn(7, 3, generator=g, dtype=torch.float64)
        a, bz, c = pack.reverse_coefficients(T, [t, s], 'ddim', 0.0)[0].tolist()
        xt = math.sqrt(abar[t]) * x0 + math.sqrt(1 - abar[t]) * z
        xs = math.sqrt(abar[s]) * x0 + math.sqrt(1 - abar[s]) * z
        assert c == 0.0 and float((a * xt + bz * z - xs).abs().max()) <= 1e-12, (t, s)


def test_coefficient_refusals():
    with pytest.raises(ValueError, match='1.5'):
        pack.reverse_coefficients(1000, [1000, 1], 'ddim', 1.5)
    with pytest.raises(ValueError, match='-0.1'):
        pack.reverse_coefficients(1000, [1000, 1], 'ddim', -0.1)
    with pytest.raises(ValueError, match='heun'):
        pack.reverse_coefficients(1000, [1000, 1], 'heun')
    for steps in ([1, 1000], [1000, 1000], [1001, 1], [5, 0], []):
        with pytest.raises(ValueError, match='strictly decreasing'):
            pack.reverse_coefficients(1000, steps)


def test_twisted_coefficients_give_the_ancestral_mean():
    """coef1 x0 + coef2 x_t with x0 = (x_t - sqrt(1 - abar_t) z) / sqrt(abar_t) is A x_t + Bz z, and sigma is C."""
    T = 1000
    steps = pack.respaced_steps(T, 10)
    tw, anc = pack.twisted_coefficients(T, steps), pack.reverse_coefficients(T, steps)
    abar = torch.tensor(R.abar64(T), dtype=torch.float64)[steps]
    assert float((tw[:, 0] / torch.sqrt(abar) + tw[:, 1] - anc[:, 0]).abs().max()) <= 1e-12
    assert float((-tw[:, 0] * torch.sqrt(1 - abar) / torch.sqrt(abar) - anc[:, 1]).abs().max()) <= 1e-12
    assert torch.equal(tw[:, 2], anc[:, 2])


def test_new_symbols_are_declared_bound_and_exported():
    from genie2_amd import build, capi
    build.build()
    lib = capi.load_library()
    header = open(os.path.join(ROOT, 'include', 'genie_hip.h')).read()
    for name in ('genie_reverse_step', 'genie_sample_loop_steps'):
        assert re.search(r'\bint %s\s*\(' % name, header), name
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
    assert len(capi.SYMBOLS['genie_reverse_step'][1]) == 9 and len(capi.SYMBOLS['genie_sample_loop_steps'][1]) == 11
    # a NULL handle is refused without touching a device
    assert lib.genie_reverse_step(None, None, 1.0, 0.0, 0.0, None, None, None, None) == -1
    assert lib.genie_sample_loop_steps(None, None, 1, None, None, None, None, 1, None, None, None) == -1


def _cpu_model(T=10):
    """A Genie stand-in on the CPU device (as tests/test_triatt_host.py builds one): anything that reaches the engine fails, so a
    ValueError shows that the parameters were checked first."""
    from genie2_amd.config import Config
    from genie2_amd.model import Denoiser
    cfg = Config()
    cfg.model.update(n_pair_transform_layer=1, n_structure_layer=1)
    cfg.diffusion['n_timestep'] = T
    m = Denoiser(**cfg.model, n_timestep=T, max_n_res=64, max_n_chain=1)
    return types.SimpleNamespace(model=m, config=cfg, device=torch.device('cpu'), setup_schedule=lambda: None)


def test_samplers_refuse_bad_few_step_parameters_before_any_work(tmp_path):
    from genie2_amd.sampler import ScaffoldSampler, UnconditionalSampler
    from genie2_amd.smc import TwistedSampler
    model = _cpu_model(10)
    base = {'length': 12, 'scale': 0.6, 'num_samples': 2, 'outdir': str(tmp_path), 'prefix': 'x', 'offset': 0}
    touched = []
    for cls in (UnconditionalSampler, ScaffoldSampler, TwistedSampler):
        s = cls(model)
        s.create_np_features = lambda params: touched.append(1)          # the first thing _sample does after the checks
        for over, word in ((dict(num_steps=0), '0'), (dict(num_steps=11), '11'), (dict(num_steps=5, sampler='heun'), 'heun'),
                           (dict(num_steps=5, sampler='ancestral', eta=0.3), '0.3'),
                           (dict(num_steps=5, noise=torch.zeros(10, 2, 12, 3)), r'\(10, 2, 12, 3\)')):
            with pytest.raises(ValueError, match=word):
                s._sample(dict(base, **over))
    for cls in (UnconditionalSampler, ScaffoldSampler):
        s = cls(model)
        s.create_np_features = lambda params: touched.append(1)
        for over, word in ((dict(num_steps=5, sampler='ddim', eta=1.5), '1.5'), (dict(num_steps=5, sampler='ddim', eta=-0.25), '-0.25'),
                           (dict(sampler='ddim'), 'num_steps')):
            with pytest.raises(ValueError, match=word):
                s._sample(dict(base, **over))
    tw = TwistedSampler(model)
    tw.create_np_features = lambda params: touched.append(1)
    with pytest.raises(ValueError, match="ancestral kernel only.*'ddim'"):
        tw._sample(dict(base, num_steps=5, sampler='ddim'))
    assert touched == []
    # a good plan: the steps and their rows, nothing else
    steps, coef = UnconditionalSampler(model).few_step_plan(dict(base, num_steps=4, sampler='ddim', eta=0.5))
    assert steps == [10, 7, 4, 1] and torch.equal(coef, pack.reverse_coefficients(10, steps, 'ddim', 0.5))
    assert UnconditionalSampler(model).few_step_plan(dict(base)) is None
    assert UnconditionalSampler(model).few_step_plan(dict(base, sampler='ancestral')) is None


def _help(parser, flag):
    return next(a for a in parser._actions if flag in a.option_strings).help


def test_clis_parse_the_few_step_flags():
    import genie.sample_scaffold as gs
    import genie.sample_unconditional as gu
    import genie.sample_unconditional_motif as gm
    from genie2_amd import sample_scaffold, sample_unconditional, sample_unconditional_motif
    base = ['--name', 'b', '--epoch', '1', '--scale', '0.6', '--outdir', 'o']
    for mod in (sample_unconditional, sample_scaffold, gu, gs):
        a = mod.build_parser().parse_args(base)
        assert (a.num_steps, a.sampler, a.eta) == (None, None, None)
        a = mod.build_parser().parse_args(base + ['--num_steps', '100', '--sampler', 'ddim', '--eta', '0.5'])
        assert (a.num_steps, a.sampler, a.eta) == (100, 'ddim', 0.5)
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(base + ['--sampler', 'heun'])
        for flag in ('--num_steps', '--sampler', '--eta'):
            assert _help(mod.build_parser(), flag).endswith('(not in the reference CLI)'), flag
    c = sample_unconditional.UnconditionalRunner().create_constants(
        vars(sample_unconditional.build_parser().parse_args(base + ['--num_steps', '50', '--sampler', 'ddim', '--eta', '1'])))
    assert (c['num_steps'], c['sampler'], c['eta']) == (50, 'ddim', 1.0)
    c = sample_scaffold.ScaffoldRunner().create_constants(vars(sample_scaffold.build_parser().parse_args(base + ['--num_steps', '50'])))
    assert c['num_steps'] == 50 and 'sampler' not in c and 'eta' not in c
    motif = os.path.join(ROOT, 'tests', 'golden', 'motif_two_segments.pdb')
    for mod in (sample_unconditional_motif, gm):
        p = mod.build_parser()
        assert p.parse_args(base + ['--motif_file', motif]).num_steps is None
        assert p.parse_args(base + ['--motif_file', motif, '--num_steps', '100']).num_steps == 100
        for flag in ('--sampler', '--eta'):
            with pytest.raises(SystemExit):
                p.parse_args(base + ['--motif_file', motif, flag, '0'])
        assert 'default: all' in _help(p, '--num_steps') and 'addition to the reference CLI' in _help(p, '--num_steps')
