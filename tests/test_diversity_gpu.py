"""The diversity potential on the GPU (genie_diversity_potential, csrc/diversity_kernels.hip; DiversityPotential in genie2_amd/smc.py)
against the float64 oracle of tests/_diversity.py, against FoldPotential with the batch for its references, under regrouping, in
TwistedSampler against the float32 PyTorch restatement as its twisting function, summed with the fold potential, and through both
command lines.

Bounds (the project's bars for a fused potential, as in test_fold_gpu.py): logp, `tm_of`, `tm_nearest_design`, `tm_mean_design` and
`e_diversity` within 1e-5 max(1, |value|); every particle's gradient within 1e-5 of its largest float64 entry; each widened, per case,
to 4 x the error the float32 restatement makes on the same input where that is larger; `nearest_design` exact where the two best
TM-scores differ by more than the bar, `n_similar` exact where no n_bj is within 1e-4 N of the bound.  A particle is left out of the
logp and gradient comparison only if one of its pairs with an active hinge is ill-posed by the oracle's rule (tests/_diversity.py:
another seed within 1e-4 in TM whose fit gives the particle another gradient, or a Horn gap below 1e-4), and at most 5 % of a case's
particles may be: with these inputs none is.

logp, the gradient and the report under the case's own grouping are compared on the whole batch; `describe` and `tm_of`, which score
every row as a design of its own, on every row of a batch of up to 16 and on every (B / 16)-th row of a larger one, so that the
float64 oracle stays at a few seconds per case.

Worst error / bound over the parity cases, measured on an MI355X: 0.075 for the grouped scores ((8, 8, 40); 0.046 of a bar widened
x8.9 at (2, 64, 24), the only scalar bar that was widened), 0.020 for tm_of, 0.116 for logp and for e_diversity ((2, 64, 24)), 0.161
for the gradient ((2, 1, 1706), bar widened x4.2); the gradient's bar was widened in every case, x3.2 to x15.6, by the restatement's
own error, and against the unwidened 1e-5 the kernel is inside in eight cases and at 1.2, 1.5 and 1.8 x in three (N = 4, 24, 5); every
count was equal; no particle was left out.  tm_of is bitwise FoldPotential's on the batch.  The sampler comparisons end 2.4e-6 and
1.4e-6 of the coordinate RMS apart (bar 1e-3).  DESIGN.md 7.12 has the table per case."""
import math
import os

import numpy as np
import pytest
import torch

import _diversity as Dv
import _fold as Fd
import _similarity as S
from _motif import MOTIF, _abar, _tiny_model
from _parity import hard_time_limit

pytestmark = pytest.mark.gpu

STEP = 500
_cache = {}


@pytest.fixture(autouse=True)
def _limit():
    with hard_time_limit(300):
        yield


def _inputs(case):
    if case not in _cache:
        _cache[case] = Dv.inputs(case)
    return _cache[case]


def _potential(n_res, K, abar=None, **kw):
    from genie2_amd.smc import DiversityPotential
    return DiversityPotential(n_res, _abar() if abar is None else abar, K, device='cuda', **kw)


def _reference(x, K, var, **kw):
    """The oracle and the float32 restatement of an input, computed once."""
    key = ('ref', x.data_ptr(), tuple(x.shape), K, var, repr(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = (x, Dv.reference(x, K, var, **kw), Dv.restatement32(x, K, var, **kw))
    return _cache[key][1:]


def _run(pot, x, step=STEP):
    x = x.detach().cuda().clone().requires_grad_(True)
    lp = pot(x, step)
    g, = torch.autograd.grad(lp.sum(), x)
    return lp.detach(), g


def _widen(err, bound):
    """The factor a bar is widened by: 4 x the float32 restatement's error / bound where that is above 1."""
    return max(1.0, 4.0 * float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max())) if err.numel() else 1.0


def _ratio(d, b):
    return float(torch.where(b > 0, d / b.clamp(min=1e-300), torch.where(d > 0, math.inf, 0.0).double()).max()) if d.numel() else 0.0


def _value(what, name, got, r, r32):
    """A float output against the oracle under the 1e-5 max(1, |value|) bar, widened by the restatement's own error."""
    got, r32 = got.double().cpu().reshape(-1), r32.double().cpu().reshape(-1)
    r = r.reshape(-1)
    bound = 1e-5 * r.abs().clamp(min=1.0)
    wide = _widen((r32 - r).abs(), bound)
    print('%s: %s error / bound %.3f (bar widened x%.2f)' % (what, name, _ratio((got - r).abs(), bound * wide), wide))
    assert bool(torch.isfinite(got).all()) and bool(((got - r).abs() <= bound * wide).all()), (what, name, got, r)
    return bound * wide


def _report(what, got, r64, r32, tm_bar, N, keep=None):
    """A decoded report against the oracle's: the floats under their bars, the counts exact where the oracle's margins allow."""
    B = r64['tm'].shape[0]
    keep = torch.ones(B, dtype=torch.bool) if keep is None else keep
    assert tuple(got) == Dv.REPORT
    for k in Dv.REPORT:
        assert tuple(got[k].shape) == (B,) and got[k].device.type == 'cuda' and got[k].dtype == (torch.int64 if k in Dv.COUNTS else torch.float32), k
    _value(what, 'tm_nearest_design', got['tm_nearest_design'], r64['tm_nearest_design'], r32['tm_nearest_design'])
    _value(what, 'tm_mean_design', got['tm_mean_design'], r64['tm_mean_design'], r32['tm_mean_design'])
    if bool(keep.any()):
        _value(what, 'e_diversity', got['e_diversity'][keep.cuda()], r64['e_diversity'][keep], r32['e_diversity'][keep])
    # nearest_design: exact where the two best scored TM-scores differ by more than the bar (one partner: always; none: -1)
    scored = torch.where(r64['scored'], r64['tm'], torch.full_like(r64['tm'], -1.0))
    top = torch.sort(scored, dim=1, descending=True).values
    sure = (top[:, 0] - top[:, 1] > 2 * tm_bar.amax()) if B > 1 else torch.ones(B, dtype=torch.bool)
    assert torch.equal(got['nearest_design'].cpu()[sure], r64['nearest_design'][sure]), (what, got['nearest_design'], r64['nearest_design'])
    # n_similar: exact where no scored n_bj is within 1e-4 N of the bound
    near = (((r64['n'] - N * Dv.TM_MAX).abs() < 1e-4 * N) & r64['scored']).any(dim=1)
    assert torch.equal(got['n_similar'].cpu()[~near], r64['n_similar'][~near]), (what, got['n_similar'], r64['n_similar'])


def _decoded(pot, x, K):
    """The entry's report of x under systems of K (describe is the K = 1 form of this)."""
    from genie2_amd import capi
    from genie2_amd.smc import _decode_report
    report, = pot._launch(pot._checked(x, K), pot._one, want='report', K=K)
    return _decode_report(report, capi.DIVERSITY_REPORT, capi.DIVERSITY_COUNTS)


def _parity(what, x, K, pot=None, cap=0.05, **kw):
    """Everything the entry returns for x against the oracle; returns (pot, oracle, logp, grad)."""
    B, N = x.shape[0], x.shape[1]
    pot = _potential(N, K, **kw) if pot is None else pot
    r64, r32 = _reference(x, K, float(pot.variance(STEP)), **kw)
    lp, g = _run(pot, x)
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), what
    keep = ~Dv.left_out(r64)
    print('%s: %d of %d particles left out' % (what, int((~keep).sum()), B))
    assert int((~keep).sum()) <= cap * B, (what, keep)
    if bool(keep.any()):
        _value(what, 'logp', lp[keep.cuda()], r64['logp'][keep], r32['logp'][keep])
        g_b = 1e-5 * r64['grad'].abs().amax(dim=(1, 2))[keep]
        wide = _widen((r32['grad'].double() - r64['grad']).abs().amax(dim=(1, 2))[keep], g_b)
        d_g = (g.double().cpu() - r64['grad']).abs().amax(dim=(1, 2))[keep]
        print('%s: gradient error / bound %.3f (bar widened x%.2f)' % (what, _ratio(d_g, g_b * wide), wide))
        assert bool((d_g <= g_b * wide).all()), (what, d_g, g_b)
        idle = (r64['a'] == 0).all(dim=1)
        assert bool((g.cpu()[idle] == 0).all()) and bool((lp.cpu()[idle] == 0).all())      # no active pair: exactly 0
    # the report and the scores under the case's grouping
    tm = pot._launch(pot._checked(x.cuda()), pot._one, want='tm')[0]
    assert tuple(tm.shape) == (B, B) and tm.dtype == torch.float32 and tm.device.type == 'cuda'
    tm_bar = _value(what, 'tm (grouped)', tm, r64['tm'], r32['tm'])
    assert torch.equal(tm, tm.T) and bool((tm.cpu()[~r64['scored']] == 0).all())
    _report(what + ' (grouped)', _decoded(pot, x.cuda(), K), r64, r32, tm_bar, N, keep)
    # describe and tm_of: every row a design of its own
    rows = x if B <= 16 else x[::B // 16]
    d64, d32 = _reference(rows, 1, 1.0, **kw) if (K > 1 or B > 16) else (r64, r32)
    tm1 = pot.tm_of(rows.cuda())
    assert tuple(tm1.shape) == (len(rows), len(rows)) and tm1.dtype == torch.float32 and tm1.device.type == 'cuda'
    tm1_bar = _value(what, 'tm_of', tm1, d64['tm'], d32['tm'])
    assert torch.equal(tm1, tm1.T) and bool((torch.diagonal(tm1) == 0).all())
    _report(what, pot.describe(rows.cuda()), d64, d32, tm1_bar, N)
    return pot, r64, lp, g


@pytest.mark.parametrize('case', Dv.CASES, ids=Dv.case_id)
def test_potential_and_report_match_the_float64_oracle(case):
    x = _inputs(case)
    _, r64, lp, _ = _parity(Dv.case_id(case), x, case[1])
    Dv.check_inputs(r64, case)
    assert bool((r64['logp'] <= 0).all()) and float(r64['logp'].min()) < 0 and int(r64['n_similar'].sum()) > 0


def test_tm_of_is_the_fold_potential_with_the_batch_for_references():
    """tm_of(x)[i, j], i < j, against FoldPotential(references = x).tm_of(x)[i, j] (particle i moving onto reference j): the ascent is
    the same arithmetic, so the two should be bitwise equal, which is reported; what is asserted is the 1e-5 bar."""
    from genie2_amd.smc import FoldPotential
    for case in ((3, 2, 65), (4, 2, 129)):
        x = _inputs(case)
        B, N = x.shape[0], x.shape[1]
        pot = _potential(N, case[1])
        tm = pot.tm_of(x.cuda())
        fold = FoldPotential(N, _abar(), x, [(0.0, 0.5)] * B, device='cuda').tm_of(x.cuda())
        upper = torch.triu(torch.ones(B, B, dtype=torch.bool), diagonal=1).cuda()
        d = (tm - fold).abs().double()[upper]
        bar = 1e-5 * fold.double()[upper].clamp(min=1.0)
        print('%s: tm_of against FoldPotential, difference / bar %.3f, bitwise equal: %s'
              % (Dv.case_id(case), float((d / bar).max()), bool(torch.equal(tm[upper], fold[upper]))))
        assert bool((d <= bar).all()), (case, tm, fold)
        assert torch.equal(tm, tm.T) and bool((torch.diagonal(tm) == 0).all())
        grouped = pot._launch(x.cuda().contiguous(), pot._one, want='tm')[0]             # systems of K: same-system entries are 0, the rest the same bits
        same = (torch.arange(B)[:, None] // case[1] == torch.arange(B)[None] // case[1]).cuda()
        assert bool((grouped[same] == 0).all()) and torch.equal(grouped[~same], tm[~same]) and torch.equal(grouped, grouped.T)


def test_grouping():
    """With K = 2 a particle's logp and gradient are those of a K = 1 call on the batch without its system-mate, times 1 / 2 (bitwise:
    the pairs keep their order and their moving member, and the factor is a power of two); B = K gives exact zeros without reading
    `work`."""
    x = _inputs((3, 2, 64)).cuda()
    two, one = _potential(64, 2), _potential(64, 1)
    lp, g = _run(two, x)
    assert float(lp.abs().max()) > 0
    for b in range(6):
        rest = [k for k in range(6) if k != (b ^ 1)]
        lp1, g1 = _run(one, x[rest])
        at = rest.index(b)
        assert torch.equal(lp[b], lp1[at] * 0.5) and torch.equal(g[b], g1[at] * 0.5), b
    for K, rows in ((2, x[:2]), (1, x[:1]), (2, x[2:4])):
        pot = _potential(64, K)
        pot._work = torch.full((4096,), float('nan'), dtype=torch.float32, device='cuda').view(torch.uint8)      # what a read of `work` would meet
        lp0, g0 = _run(pot, rows)
        assert bool((lp0 == 0).all()) and bool((g0 == 0).all())
        report = _decoded(pot, rows, K)
        assert report['nearest_design'].tolist() == [-1] * len(rows) and all(bool((report[k] == 0).all()) for k in Dv.REPORT if k != 'nearest_design')
        assert bool((pot._launch(rows.contiguous(), pot._one, want='tm')[0] == 0).all())
    single = one.describe(x[:1])                                          # one design: a report without a partner
    assert single['nearest_design'].tolist() == [-1] and float(single['tm_nearest_design']) == 0.0 and float(one.tm_of(x[:1])) == 0.0


def test_deterministic_and_never_synchronises():
    x = _inputs((4, 2, 129))
    pot = _potential(129, 2)
    xc = x.cuda()
    a, b = _run(pot, xc, 400), _run(pot, xc, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ra, rb = pot.describe(xc), pot.describe(xc)
    assert all(torch.equal(ra[k], rb[k]) for k in ra)
    ta = pot.tm_of(xc)
    assert torch.equal(ta, pot.tm_of(xc))
    xg = xc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(xg, 400)
        g, = torch.autograd.grad(lp.mean(), xg)
        rep = pot.describe(xc)
        tm = pot.tm_of(xc)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.allclose(g, a[1] / 8, rtol=1e-6, atol=0)      # (the backward scales by grad_output = 1/8)
    assert all(torch.equal(rep[k], ra[k]) for k in ra) and torch.equal(tm, ta)
    with pytest.raises(ValueError):
        pot(xc[:, :128], 400)                                                             # a wrong N
    with pytest.raises(ValueError, match='multiple of num_particles'):
        pot(xc[:7], 400)                                                                  # B not divisible by K
    with pytest.raises(ValueError):
        pot(x, 400)                                                                       # a CPU tensor
    with pytest.raises(ValueError):
        pot.tm_of(x)
    with pytest.raises(ValueError):
        pot.describe(xc[:, :64])
    assert tuple(pot.describe(xc[:7])['n_similar'].shape) == (7,)                         # (every row a design: any number of rows)


def test_degenerate_inputs_stay_finite():
    """A particle collapsed to one point (its fits have no rotation: the oracle's gap rule leaves the gradients it touches out, the
    scores and log p stay in) and a batch 1e4 A from the origin (each chain is centred on its own centroid before anything is
    multiplied)."""
    x = _inputs((2, 2, 63)).clone()
    x[3] = x[3, 5]
    pot = _potential(63, 2)
    r64, r32 = _reference(x, 2, float(pot.variance(STEP)))
    lp, g = _run(pot, x)
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all())
    rep = _decoded(pot, x.cuda(), 2)
    assert all(bool(torch.isfinite(v.double()).all()) for v in rep.values())
    tm = pot._launch(x.cuda().contiguous(), pot._one, want='tm')[0]
    _value('collapsed particle', 'tm', tm, r64['tm'], r32['tm'])
    _value('collapsed particle', 'logp', lp, r64['logp'], r32['logp'])
    _value('collapsed particle', 'e_diversity', rep['e_diversity'], r64['e_diversity'], r32['e_diversity'])
    assert float(r64['gap'][3][r64['scored'][3]].max()) < 1e-4             # the rule sees it
    x = _inputs((2, 2, 63))
    far = x + torch.tensor([1e4, 0.0, 0.0])
    _, r_far, _, _ = _parity('a batch 1e4 A away', far, 2)
    near = Dv.reference(x, 2, float(pot.variance(STEP)))
    assert torch.allclose(r_far['tm'], near['tm'], atol=1e-4)              # a translation changes nothing but float32 rounding


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

T, N_S = 12, 40


def _sampler_noise(B):
    """Noise [T, B, N_S, 3] whose particles share all but a thousandth of every draw's variance (test_fold_gpu.py's trick): all
    designs of a run then start out as one fold, which is what this potential is for, and near pairs are the well-posed ones
    (DESIGN.md 7.9)."""
    g = torch.Generator().manual_seed(4)
    common, own = torch.randn(T, 1, N_S, 3, generator=g), torch.randn(T, B, N_S, 3, generator=g)
    return math.sqrt(0.999) * common + math.sqrt(0.001) * own


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
        attrs = {k: getattr(sampler, k, None) for k in ('last_fit', 'last_shape', 'last_secstruct', 'last_pairs', 'last_positions')}
        return np.stack([r['atom_positions'] for r in out]), out, attrs

    return dict(run=run, abar=abar)


@pytest.mark.parametrize('S_,K', [(4, 1), (2, 3)], ids=['4x1', '2x3'])
def test_sampler_follows_the_torch_path_without_resampling(ctx, tmp_path, S_, K):
    B = S_ * K
    noise = _sampler_noise(B)
    kw = dict(num_samples=S_, num_particles=K, ess_threshold=0.0)
    fused = _potential(N_S, K, ctx['abar'])
    free, _, _ = ctx['run'](lambda x0, step: (x0 * 0).sum(dim=(1, 2)), noise, tmp_path, **kw)
    a, _, attrs_a = ctx['run'](Dv.twisting_function(K, ctx['abar']), noise, tmp_path, **kw)
    b, _, attrs_b = ctx['run'](fused, noise, tmp_path, **kw)
    assert a.shape == b.shape == free.shape == (B, N_S, 3)
    rms, d = float(np.sqrt((a ** 2).mean())), float(np.abs(a - b).max())
    start, end = Dv.reference(torch.from_numpy(free).float(), K, 1.0), Dv.reference(torch.from_numpy(b).float(), K, 1.0)
    top = lambda r: float(r['tm'][r['scored']].max())      # noqa: E731
    print('largest cross-system TM: unguided %.3f, guided %.3f' % (top(start), top(end)))
    print('guidance moved the designs by %.3e of their RMS; ill-posed at the end: %s' % (float(np.abs(b - free).max()) / rms, Dv.left_out(end).tolist()))
    print('no resampling: max |d| = %.3e, coordinate RMS = %.2f, ratio %.3e' % (d, rms, d / rms))
    assert int(start['n_similar'].sum()) > 0                                                    # the hinge pulls on what the model makes
    assert float(np.abs(b - free).max()) > 1e-2 * rms                                           # ... and the guidance is felt
    assert np.isfinite(b).all() and d <= 1e-3 * rms
    assert top(end) < top(start)
    assert attrs_a['last_shape'] is None                                 # a plain callable
    report = attrs_b['last_shape']
    assert tuple(report) == Dv.REPORT and all(v.device.type == 'cpu' and tuple(v.shape) == (B,) for v in report.values())
    again = fused.describe(torch.from_numpy(b).float().cuda())
    assert all(torch.equal(report[k], again[k].cpu()) for k in report)
    assert attrs_b['last_fit'] is None and attrs_b['last_secstruct'] is None and attrs_b['last_pairs'] is None


def test_sum_of_fold_and_diversity_is_bitwise_the_sum(ctx):
    from genie2_amd.smc import FoldPotential, SumPotential
    x = _inputs((3, 2, N_S)).cuda()
    fold = FoldPotential(N_S, ctx['abar'], torch.stack([S.moved(x[0].cpu(), 41, 1.0), Fd.walk(N_S, 77)]), [(0.8, math.inf), (0.0, 0.5)], device='cuda')
    div = _potential(N_S, 2, ctx['abar'])
    both = SumPotential(fold, div)
    assert torch.equal(both(x, 5), fold(x, 5) + div(x, 5))               # bitwise the sum of its members
    xg = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(both(xg, 5).sum(), xg)
    parts = [torch.autograd.grad(m(xg, 5).sum(), xg)[0] for m in (fold, div)]
    assert torch.equal(g, parts[0] + parts[1]) and float(parts[0].abs().max()) > 0 and float(parts[1].abs().max()) > 0
    report = both.describe(x)
    assert tuple(report) == Fd.REPORT + Dv.REPORT                         # member order, no key of one hides the other's
    for m in (fold, div):
        assert all(torch.equal(report[k], v) for k, v in m.describe(x).items())


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def checkpoint_root(tmp_path_factory, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    root = str(tmp_path_factory.mktemp('diversity_cli') / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    return root


def _cli_args(checkpoint_root, out, extra):
    return ['--name', 'base', '--epoch', '7', '--rootdir', checkpoint_root, '--scale', '0.6', '--outdir', out, '--min_length', '100',
            '--max_length', '100', '--batch_size', '2', '--num_samples', '2', '--num_steps', '4', '--last_unguided_steps', '0',
            '--guidance_alpha', '0.05'] + extra


DIVERSITY_FLAGS = ['--num_particles', '2', '--diversity_tm_max', '0.5', '--write_diversity']


def _check_diversity_files(out, names, seen):
    """Every outdir/batch_diversity file: its `design` lines name the other designs of the batch in order and agree with the float64
    oracle on the written PDBs -- the file rounds to three decimals (5e-4) and the PDBs round coordinates to 1e-3 A, which moves a
    TM-score by at most 5e-4 sqrt(3) 2 / d0 per rounded chain (test_fold_gpu.py's _check_fold_files has the reasoning), here twice
    because both chains of a pair were written, plus the float32 bar -- and with tm_of / describe on the sampler's own
    last_positions (`seen`)."""
    from genie2_amd.similarity import load_designs, tm_d0
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == sorted(n + '.pdb' for n in names)
    assert sorted(os.listdir(os.path.join(out, 'batch_diversity'))) == sorted(n + '.txt' for n in names)
    x = torch.cat([load_designs([os.path.join(out, 'pdbs', n + '.pdb')])[0] for n in names])
    N, M = x.shape[1], len(names)
    r64 = Dv.reference(x, 1, 1.0)
    tol = 5e-4 + 2 * 5e-4 * math.sqrt(3) * 2 / tm_d0(N) + 1e-5
    pos, report, pot = seen
    assert tuple(pos.shape) == (M, N, 3) and all(tuple(v.shape) == (M,) for v in report.values())
    tm, again = pot.tm_of(pos.cuda()).cpu(), pot.describe(pos.cuda())
    for i, name in enumerate(names):
        lines = [ln.split() for ln in open(os.path.join(out, 'batch_diversity', name + '.txt'))]
        others = [k for k in range(M) if k != i]
        head, tail = lines[:M - 1], lines[M - 1:]
        assert [f[0] for f in head] == ['design'] * (M - 1) and [f[1] for f in head] == [names[k] for k in others] and all(len(f) == 3 for f in head)
        assert [f[0] for f in tail] == list(Dv.REPORT) and all(len(f) == 2 for f in tail)
        assert all(('.' in f[1]) == (f[0] not in Dv.COUNTS) for f in tail)
        got = {f[0]: float(f[1]) for f in tail}
        for f, k in zip(head, others):
            assert abs(float(f[2]) - float(r64['tm'][i, k])) <= tol, (name, f, r64['tm'])
            assert abs(float(f[2]) - float(tm[i, k])) <= 5e-4 + 1e-6, (name, f, tm)
        assert abs(got['tm_nearest_design'] - float(r64['tm_nearest_design'][i])) <= tol and abs(got['tm_mean_design'] - float(r64['tm_mean_design'][i])) <= tol
        top = torch.sort(r64['tm'][i][r64['scored'][i]], descending=True).values
        if len(top) == 1 or float(top[0] - top[1]) > 2 * tol:
            assert got['nearest_design'] == int(r64['nearest_design'][i])
        # e_diversity = sum of squared hinges on n = N tm: a TM-score off by t moves it by at most 2 hinge N t (+ N^2 t^2)
        t, hinge = tol - 5e-4, r64['a'][i]
        tol_e = 5e-4 + float((2 * hinge * N * t + (N * t) ** 2)[r64['scored'][i]].sum()) + 1e-5 * max(1.0, float(r64['e_diversity'][i]))
        assert abs(got['e_diversity'] - float(r64['e_diversity'][i])) <= tol_e, (name, got, r64['e_diversity'], tol_e)
        if float((r64['n'][i] - N * 0.5).abs()[r64['scored'][i]].min()) > N * t:
            assert got['n_similar'] == int(r64['n_similar'][i])
        for f in tail:
            assert torch.equal(report[f[0]][i], again[f[0]][i].cpu())
            assert abs(float(f[1]) - float(report[f[0]][i])) <= 5e-4 + 1e-5 * max(1.0, abs(float(report[f[0]][i]))), (name, f)


def _spied(run):
    """Runs `run()` with TwistedSampler._finish watched: the sampler's own last_positions, report and twisting function per batch."""
    from genie2_amd.smc import TwistedSampler
    seen, finish = [], TwistedSampler._finish

    def spy(self, st, trans, feats, start):
        res = finish(self, st, trans, feats, start)
        seen.append((self.last_positions.clone(), {k: v.clone() for k, v in self.last_shape.items()}, st.twist))
        return res

    TwistedSampler._finish = spy
    try:
        run()
    finally:
        TwistedSampler._finish = finish
    return seen


def test_both_clis_write_the_batch_diversity_files(tmp_path, checkpoint_root):
    from genie2_amd import capi
    from genie2_amd.sample_unconditional_motif import MotifRunner
    from genie2_amd.sample_unconditional_motif import build_parser as motif_parser
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    from genie2_amd.smc import DiversityPotential, MotifPotential, SumPotential
    first = str(tmp_path / 'first')
    args = build_parser().parse_args(_cli_args(checkpoint_root, first, DIVERSITY_FLAGS))
    torch.manual_seed(0)
    seen = _spied(lambda: ShapeRunner().run(vars(args), args.num_devices, args.sequential_order))
    assert len(seen) == 1 and isinstance(seen[0][2], DiversityPotential) and tuple(seen[0][1]) == Dv.REPORT and seen[0][2].K == 2
    _check_diversity_files(first, ['100_0', '100_1'], seen[0])
    assert not any(os.path.exists(os.path.join(first, d)) for d in ('shape', 'fold', 'binder', 'symmetry'))

    # the motif CLI: the term is summed last
    second = str(tmp_path / 'second')
    args = motif_parser().parse_args(_cli_args(checkpoint_root, second, ['--motif_file', MOTIF] + DIVERSITY_FLAGS))
    np.random.seed(0)
    torch.manual_seed(0)
    seen = _spied(lambda: MotifRunner().run(vars(args), args.num_devices, args.sequential_order))
    assert len(seen) == 1 and isinstance(seen[0][2], SumPotential)
    members = seen[0][2].potentials
    assert isinstance(members[0], MotifPotential) and isinstance(members[-1], DiversityPotential) and len(members) == 2
    pos, report, _ = seen[0]
    _check_diversity_files(second, ['100_0', '100_1'], (pos, {k: report[k] for k in capi.DIVERSITY_REPORT}, members[-1]))


def test_run_without_the_flag_writes_no_batch_diversity_files(tmp_path, checkpoint_root):
    from genie2_amd.sample_unconditional_shape import ShapeRunner, build_parser
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(_cli_args(checkpoint_root, out, ['--rog_max', '12', '--num_particles', '2']))
    torch.manual_seed(0)
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    assert len(os.listdir(os.path.join(out, 'pdbs'))) == 2 and not os.path.exists(os.path.join(out, 'batch_diversity'))
    # the term without --write_diversity: guided, but no such directory either
    out = str(tmp_path / 'quiet')
    args = build_parser().parse_args(_cli_args(checkpoint_root, out, ['--num_particles', '2', '--diversity_tm_max', '0.5']))
    torch.manual_seed(0)
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)
    assert len(os.listdir(os.path.join(out, 'pdbs'))) == 2 and not os.path.exists(os.path.join(out, 'batch_diversity'))
