"""The gradient gather of the motif potentials (k_motif<Form, SPILL>, csrc/smc_kernels.hip) where many placements carry weight: every
case of tests/_motif_gather.py (whose regime tests/test_motif_gather_host.py decides on the CPU: listed with K from 1 to 2048, the
list exactly full, one past full, unlisted with every placement active; one to three residue tiles; records in LDS and in `work`)
through all four forms, against the float64 oracles.

Bounds, the project's bar: logp within 1e-5 max(1, |logp|); gradient within 1e-5 of the particle's largest gradient entry; each
widened to 4 x the error of the float32 restatement of the same oracle on the same input where that is above the bar, never beyond
10 x (the rule of tests/test_tmalign_gpu.py: measured against the reference, never against the kernel; `_motif_gather.widen`).
Every test prints error / bound.  The metamorphic checks need no oracle: duplicating or permuting the placement list changes
nothing beyond the bar, the gradient of every particle sums to zero over the residues, and residues that no active placement covers
have exactly zero gradient.  Bitwise: two calls agree, and particle b of a batched call equals its own call (k_motif's work-groups of
particle b read x0[b] and their own records and nothing that depends on B)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _motif_gather as G
from _motif import _abar, _fix_var, _pot, _run
from _parity import hard_time_limit

pytestmark = pytest.mark.gpu

BAR = G.BAR
ALL = [(name, form) for name in G.CASES for form in G.FORMS]
BATCHED = [(name, form) for name, form in ALL if G.CASES[name]['B'] > 1]
_pots, _results = {}, {}


@pytest.fixture(autouse=True)
def _limit():
    with hard_time_limit(120):
        yield


def _potential(form, n_res, starts, var):
    """The form's MotifPotential for n_res residues (built once, with one placement) with its placement list replaced by `starts`,
    validated as the constructor validates its own, and its variance fixed."""
    from genie2_amd.smc import _check_starts
    if 'abar' not in _pots:
        _pots['abar'] = _abar()
    if (form, n_res) not in _pots:
        _pots[form, n_res] = _pot(G.motif(form)[0], n_res, _pots['abar'], P=1, **G.pot_kwargs(form))
    pot = _pots[form, n_res]
    _check_starts(starts, pot.seg_len, pot.n_res)
    pot.starts, pot.P = starts.to(pot.device).contiguous(), len(starts)
    _fix_var(pot, var)
    return pot


def _case(name, form):
    c = G.CASES[name]
    x0, starts = G.inputs(name, form)
    return c, x0, starts, _potential(form, c['n_res'], starts, c['var'])


def _result(name, form):
    """(logp, grad) of the case's first run on the device, kept for the tests that share it."""
    if (name, form) not in _results:
        c, x0, starts, pot = _case(name, form)
        _results[name, form] = _run(pot, x0)
    return _results[name, form]


def _within_bar(a, b, what):
    """(logp, grad) a against b, both from the device, within the plain bar of b."""
    rl = float(((a[0].double() - b[0].double()).abs() / (BAR * b[0].double().abs().clamp(min=1.0))).max())
    rg = max(float((a[1][i].double() - b[1][i].double()).abs().max() / (BAR * b[1][i].double().abs().max())) for i in range(len(b[1])))
    print('%s: difference / bar: logp %.3f, grad %.3f' % (what, rl, rg))
    assert rl <= 1.0 and rg <= 1.0, (what, rl, rg)


@pytest.mark.parametrize('name,form', ALL)
def test_gather_matches_the_float64_oracle(name, form):
    c, x0, starts, pot = _case(name, form)
    spill = G.work_bytes(pot.lib, form, c['B'], pot.P) > 0
    ref, r32 = G.reference(name, form, pot.target.cpu())
    act = G.activity(ref['score'])
    assert act['between'] == [0] * c['B'] and act['count'] == G.expected_counts(name, form)       # (the host file's decision holds here)
    lp, g = _result(name, form)
    err, widen = G.error_ratios(lp, g, ref), G.widen(r32)
    runs = [G.replica(form, c['n_res'], pot.P, n, spill) for n in act['count']]
    print('%s %s %s %s: error / bound: logp %.3f, grad %.3f (bound = %.2f, %.2f bars; float32 restatement %.3f, %.3f bars)'
          % (name, form, runs[0]['kernel'], ['%s K=%d' % ('listed' if r['listed'] else 'unlisted', r['K']) for r in runs],
             err['logp'] / widen['logp'], err['grad'] / widen['grad'], widen['logp'], widen['grad'], r32['logp'], r32['grad']))
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all())
    assert err['logp'] <= widen['logp'] and err['grad'] <= widen['grad'], (name, form, err, widen)


@pytest.mark.parametrize('name,form', ALL)
def test_gradient_sums_to_zero_and_is_zero_where_no_active_placement_reaches(name, form):
    c, x0, starts, pot = _case(name, form)
    ref, _ = G.reference(name, form, pot.target.cpu())
    lp, g = _result(name, form)
    g = g.double().cpu()
    lens = G.motif(form)[1]
    on = (ref['score'].max(dim=1, keepdim=True).values - ref['score']) < G.ON
    for b in range(c['B']):
        total, bound = float(g[b].sum(dim=0).abs().max()), BAR * float(g[b].abs().max()) * c['n_res'] ** 0.5
        covered = torch.zeros(c['n_res'], dtype=torch.bool)
        for s, n in enumerate(lens):
            for i in range(n):
                covered[(starts[on[b], s].long() + i).unique()] = True
        print('%s %s particle %d: |sum_n grad| / bound %.3f; %d residues uncovered' % (name, form, b, total / bound, int((~covered).sum())))
        assert total <= bound, (name, form, b, total, bound)
        assert bool((g[b, ~covered] == 0).all()) and bool((g[b, covered] != 0).any()), (name, form, b)


@pytest.mark.parametrize('name,form', ALL)
def test_two_calls_give_the_same_bits(name, form):
    c, x0, starts, pot = _case(name, form)
    first = _result(name, form)
    again = _run(pot, x0)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), (name, form)


@pytest.mark.parametrize('name,form', BATCHED)
def test_a_particle_of_a_batch_equals_its_own_call_bit_for_bit(name, form):
    """k_motif's work-groups of particle b stage x0[b], read record base b and write logp[b], grad[b]: nothing depends on B (SPILL is
    decided by P alone)."""
    c, x0, starts, pot = _case(name, form)
    lp, g = _result(name, form)
    for b in range(c['B']):
        one = _run(pot, x0[b:b + 1])
        assert torch.equal(one[0][0], lp[b]) and torch.equal(one[1][0], g[b]), (name, form, b)


@pytest.mark.parametrize('form', G.FORMS)
@pytest.mark.parametrize('chain', [(1500, 3000), (1024, 2048, 3072)])
def test_duplicating_every_placement_changes_nothing(chain, form):
    """P -> 2P (-> 3P) with every placement active at N = 129: the list grows past its cap and, for Translate, the records move from
    LDS to `work`, while logp (the mean over placements) and the gradient stay."""
    c = G.CASES['n129-all-P4100']
    x0 = c['x0']()
    base = G.thinned(G.every_start(129, G.motif(form)[1]), chain[0], seed=3)
    act = G.activity(G.oracle(form, x0, base, G.centred_target(form), c['var'], want_grad=False)['score'])
    assert act['count'] == [chain[0]] * 3 and act['between'] == [0] * 3
    out = []
    for P in chain:
        starts = base.repeat(P // chain[0], 1)
        pot = _potential(form, 129, starts, c['var'])
        out.append(_run(pot, x0))
        print('P = %d: %s' % (P, G.replica(form, 129, P, P, G.work_bytes(pot.lib, form, 3, P) > 0)))
    for P, o in zip(chain[1:], out[1:]):
        _within_bar(o, out[0], '%s P = %d against P = %d' % (form, P, chain[0]))
    # interleaved instead of appended copies: every placement next to its twin
    twins = base.repeat_interleave(2, dim=0)
    _within_bar(_run(_potential(form, 129, twins, c['var']), x0), out[0], '%s twins' % form)


@pytest.mark.parametrize('form', G.FORMS)
@pytest.mark.parametrize('name', ['n129-all-P2049', 'n129-some-P4100', 'n129-cnt2048-P2349', 'n129-cnt2049-P2050', 'n65-K5-P2500'])
def test_permuting_the_placement_list_changes_nothing(name, form):
    c, x0, starts, pot = _case(name, form)
    first = _result(name, form)
    for seed in (1, 2):
        perm = torch.from_numpy(np.random.RandomState(seed).permutation(len(starts)))
        _within_bar(_run(_potential(form, c['n_res'], starts[perm].contiguous(), c['var']), x0), first, '%s %s permuted' % (name, form))
    _within_bar(_run(_potential(form, c['n_res'], starts.flip(0).contiguous(), c['var']), x0), first, '%s %s reversed' % (name, form))


def _entry(pot, form, x, var, want_potential=True, want_fit=True):
    """The rigid or grouped C entry itself with every output, or with one half NULL: (logp, grad, best, rmsd[, group_rmsd])."""
    B = x.shape[0]
    grouped = form.startswith('grouped')
    need = G.work_bytes(pot.lib, form, B, pot.P)
    work = torch.empty(max(need, 16), dtype=torch.uint8, device='cuda')
    v = torch.tensor([var], dtype=torch.float32, device='cuda')
    logp, grad = torch.full((B,), 7.0, device='cuda'), torch.full_like(x, 7.0)
    best, rmsd = torch.full((B,), -7, dtype=torch.int32, device='cuda'), torch.full((B,), 7.0, device='cuda')
    p = lambda t, on=True: C.c_void_p(t.data_ptr()) if on else None      # noqa: E731
    head = (C.c_void_p(torch.cuda.current_stream().cuda_stream), B, pot.n_res, p(x), pot.P, pot.S, pot.M)
    outs = (p(logp, want_potential), p(grad, want_potential), p(best, want_fit), p(rmsd, want_fit))
    if grouped:
        grmsd = torch.full((B, pot.G), 7.0, device='cuda')
        rc = pot.lib.genie_motif_potential_grouped(*head, pot.G, p(pot.seg_len_t), p(pot.seg_group_t), p(pot.starts), p(pot.target), p(v),
                                                   int(form == 'grouped_rigid'), *outs, p(grmsd, want_fit), p(work, need > 0), work.numel())
    else:
        grmsd = None
        rc = pot.lib.genie_motif_potential_rigid(*head, p(pot.seg_len_t), p(pot.starts), p(pot.target), p(v), *outs, p(work, need > 0),
                                                 work.numel())
    torch.cuda.synchronize()
    assert rc == 0
    return logp, grad, best, rmsd, grmsd


@pytest.mark.parametrize('form', ['rigid', 'grouped_rigid'])
@pytest.mark.parametrize('P', [300, 2500])
@pytest.mark.parametrize('K', [2, 5, 7])
def test_locate_returns_the_lowest_of_equal_best_placements(K, P, form):
    """locate() on a list that holds the best placement K times: the lowest index of the ties, its rmsd (and group_rmsd) the
    oracle's.  P = 2500 reads the records from `work`."""
    name = 'n65-K%d-P%d' % (K, P)
    c, x0, starts, pot = _case(name, form)
    assert (G.work_bytes(pot.lib, form, 1, P) > 0) == (P == 2500)
    ref = G.oracle(form, x0, starts, pot.target.cpu(), 1.0, want_grad=False)
    top = int(ref['score'][0].argmax())
    ties = (starts == starts[top]).all(dim=1).nonzero().flatten().tolist()
    assert len(ties) == K and float((ref['score'][0, ties] - ref['score'][0, top]).abs().max()) <= 1e-12 * abs(float(ref['score'][0, top]))
    others = torch.ones(P, dtype=torch.bool)
    others[ties] = False
    gap = float((ref['score'][0, top] - ref['score'][0, others].max()) / ref['score'][0, top].abs())
    assert gap > 1e-4                                                   # the argmax is the oracle's to decide
    fit = pot.locate(x0.cuda())
    rmsd = float(ref['rmsd'][0])
    print('%s %s: ties %s, best %d, rmsd %.6f (oracle %.6f), gap to the next %.2e' % (name, form, ties, int(fit['best'][0]), float(fit['rmsd'][0]),
                                                                                    rmsd, gap))
    assert int(fit['best'][0]) == min(ties)
    assert abs(float(fit['rmsd'][0]) - rmsd) <= 1e-5 * rmsd + 1e-4
    assert fit['starts'][0].tolist() == starts[top].tolist()
    if form == 'grouped_rigid':
        gr, want = fit['group_rmsd'][0].double().cpu(), ref['group_rmsd'][0]
        assert bool(((gr - want).abs() <= 1e-5 * want + 1e-4).all()), (gr, want)


@pytest.mark.parametrize('form', ['rigid', 'grouped_rigid'])
@pytest.mark.parametrize('name', ['n65-K5-P2500', 'n129-cnt2049-P2349', 'n129-some-P2048'])
def test_fit_only_call_and_potential_call_agree(name, form):
    """The entries take logp and grad together or not at all, so the fit-only call (grid of one tile, no gather) has no logp of its
    own to compare: instead the call with every output gives the fit-only call's best / rmsd / group_rmsd and the potential call's
    logp / grad, each bit for bit, at the variance locate() uses."""
    c, x0, starts, pot = _case(name, form)
    x = x0.cuda().contiguous()
    logp, grad, best, rmsd, grmsd = _entry(pot, form, x, 1.0)
    lp1, g1, b1, r1, gr1 = _entry(pot, form, x, 1.0, want_fit=False)
    lp2, g2, b2, r2, gr2 = _entry(pot, form, x, 1.0, want_potential=False)
    assert torch.equal(lp1, logp) and torch.equal(g1, grad) and bool((b1 == -7).all()) and bool((r1 == 7.0).all())
    assert torch.equal(b2, best) and torch.equal(r2, rmsd) and bool((lp2 == 7.0).all()) and bool((g2 == 7.0).all())
    if grmsd is not None:
        assert torch.equal(gr2, grmsd) and bool((gr1 == 7.0).all())
    fit = pot.locate(x)
    assert torch.equal(fit['best'], best.long()) and torch.equal(fit['rmsd'], rmsd)
    _fix_var(pot, 1.0)
    lp, g = _run(pot, x0)
    assert torch.equal(lp, logp) and torch.equal(g, grad)
    ref = G.oracle(form, x0, starts, pot.target.cpu(), 1.0)
    r32 = G.oracle(form, x0, starts, pot.target.cpu(), 1.0, dtype=torch.float32)
    err, widen = G.error_ratios(logp, grad, ref), G.widen(G.error_ratios(r32['logp'], r32['grad'], ref))
    print('%s %s at var = 1: error / bound: logp %.3f, grad %.3f (bound = %.2f, %.2f bars)'
          % (name, form, err['logp'] / widen['logp'], err['grad'] / widen['grad'], widen['logp'], widen['grad']))
    assert err['logp'] <= widen['logp'] and err['grad'] <= widen['grad'], (name, form, err, widen)


@pytest.mark.parametrize('form', G.FORMS)
@pytest.mark.parametrize('name', ['n80-all-var100', 'n129-all-P4100', 'n129-mixed-P4100'])
def test_outputs_are_finite_at_both_ends_of_the_variance_range(name, form):
    """The lists of the unlisted cases at var = 1e4 (every placement active) and var = 1e-4 (one-hot), against the oracle's logp."""
    c, x0, starts, _ = _case(name, form)
    for var in (1e-4, 1e4):
        pot = _potential(form, c['n_res'], starts, var)
        lp, g = _run(pot, x0)
        ref = G.oracle(form, x0, starts, pot.target.cpu(), float(np.float32(var)), want_grad=False)
        rl = float(((lp.double().cpu() - ref['logp']).abs() / (BAR * ref['logp'].abs().clamp(min=1.0))).max())
        print('%s %s var = %g: logp error / bar %.3f, active %s' % (name, form, var, rl, G.activity(ref['score'])['count']))
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()) and rl <= 1.0
