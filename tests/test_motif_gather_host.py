"""The cases of tests/_motif_gather.py, decided on the CPU from the float64 oracle alone: which instantiation of k_motif<Form, SPILL>
(csrc/smc_kernels.hip) each one runs, whether its gather is listed, with which K over how many residue tiles, and that no case's
regime hangs on where float32 expf underflows (every placement's max - score is below 50 or above 200).  The table is printed; the
assertions say that, across the cases, every form reaches every branch of the gather that tests/test_motif_gather_gpu.py is there to
run.  SPILL comes from the library's host-side *_work_bytes functions, which need no device."""
import pytest
import torch

import _motif_gather as G

_ROWS = {}


def _lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


def _row(name, form):
    """One line of the table: the case's activity by the oracle and the replica's account of every particle."""
    if (name, form) not in _ROWS:
        c = G.CASES[name]
        x0, starts = G.inputs(name, form)
        score = G.oracle(form, x0, starts, G.centred_target(form), c['var'], want_grad=False)['score']
        act = G.activity(score)
        spill = G.work_bytes(_lib(), form, c['B'], len(starts)) > 0
        _ROWS[name, form] = dict(P=len(starts), act=act, spill=spill,
                                 runs=[G.replica(form, c['n_res'], len(starts), n, spill) for n in act['count']])
    return _ROWS[name, form]


def test_every_case_is_decided_by_the_oracle_with_a_margin():
    print()
    print('%-20s %-14s %-30s %5s %-22s %-18s %5s  %s' % ('case', 'form', 'kernel', 'P', 'active', 'gather (K)', 'tiles', 'margins: on <=, off >='))
    for name, c in G.CASES.items():
        for form in G.FORMS:
            r = _row(name, form)
            gather = ', '.join('%s %d' % ('listed' if run['listed'] else 'unlisted', run['K']) for run in r['runs'])
            print('%-20s %-14s %-30s %5d %-22s %-18s %5d  %.1f, %.0f' % (name, form, r['runs'][0]['kernel'], r['P'], r['act']['count'], gather,
                                                                      r['runs'][0]['tiles'], max(r['act']['on_max']), min(r['act']['off_min'])))
            assert r['act']['between'] == [0] * c['B'], (name, form, r['act'])
            assert r['act']['count'] == G.expected_counts(name, form), (name, form, r['act']['count'])
            torch.testing.assert_close(G.inputs(name, form)[0], c['x0'](), rtol=0, atol=0)          # (the inputs are reproducible)


def test_every_form_reaches_every_branch_of_the_gather():
    for form in G.FORMS:
        runs = [(name, G.CASES[name], _row(name, form), run) for name in G.CASES for run in _row(name, form)['runs']]
        P_of = lambda r: r['P']                                      # noqa: E731
        listed_many = [n for n, c, r, run in runs if run['listed'] and run['K'] >= 2 * G.CHUNK and run['K'] < P_of(r)]
        at_cap = [n for n, c, r, run in runs if run['listed'] and run['K'] == run['cap']]
        at_cap_subset = [n for n, c, r, run in runs if run['listed'] and run['K'] == run['cap'] < P_of(r)]
        past_cap = [n for n, c, r, run in runs if not run['listed'] and r['act']['count'][0] == run['cap'] + 1]
        unlisted_all = [n for n, c, r, run in runs if not run['listed'] and min(r['act']['count']) == P_of(r)]
        print(form, 'listed-many', sorted(set(listed_many)), 'cnt == cap', sorted(set(at_cap)), 'cnt == cap + 1', sorted(set(past_cap)),
              'unlisted, all active', sorted(set(unlisted_all)))
        assert listed_many and at_cap and at_cap_subset and past_cap and unlisted_all, form
        # many terms over more than one residue tile, over a last tile with one live lane, and with the records in `work`
        many = [(c, r, run) for n, c, r, run in runs if run['K'] >= 2 * G.CHUNK]
        assert any(run['tiles'] == 3 and run['live_in_last_tile'] == 1 for c, r, run in many), form
        assert any(run['spill'] for c, r, run in many) and any(not run['spill'] for c, r, run in many), form
        assert any(run['spill'] and not run['listed'] for c, r, run in many) and any(run['spill'] and run['listed'] for c, r, run in many), form
        # small K: every count from 1 to 7 that leaves a wave empty or the quarters uneven, records in LDS and in `work`
        for spill in (False, True):
            ks = {run['K'] for n, c, r, run in runs if run['listed'] and run['spill'] == spill}
            assert {1, 2, 3, 5, 7} <= ks, (form, spill, ks)
        # one launch whose work-groups disagree about `listed`
        assert any(len({run['listed'] for run in _row(n, form)['runs']}) == 2 and _row(n, form)['spill'] for n in G.CASES), form


def test_translate_is_reached_at_its_record_cap_with_many_placements_active():
    """P = 2048 keeps the records of the Translate form in LDS, P = 2049 spills them; both with every placement and with 137 active."""
    for P, spill in ((2048, False), (2049, True)):
        for kind, K in (('all', P), ('some', 137)):
            r = _row('n129-%s-P%d' % (kind, P), 'translate')
            assert r['P'] == P and r['spill'] == spill, (P, r)
            assert all(run['K'] == K and run['listed'] == (kind == 'some' or P == 2048) for run in r['runs']), (P, kind, r['runs'])
            assert r['runs'][0]['kernel'] == 'k_motif<Translate, %s>' % ('true' if spill else 'false')


def test_the_translate_oracle_here_is_the_potential_tests_reference_bit_for_bit():
    from test_motif_potential import _reference
    x0, starts = G.inputs('n63-all-P257', 'translate')
    tgt = G.centred_target('translate')
    lp, g = _reference(x0, starts, G.motif('translate')[1], tgt, 0.37)
    mine = G.oracle('translate', x0, starts, tgt, 0.37)
    assert torch.equal(lp, mine['logp']) and torch.equal(g, mine['grad'])


@pytest.mark.parametrize('form', G.FORMS)
def test_float32_restatement_stays_within_ten_bars_or_is_not_used(form):
    """The parity bar may widen to 4 x the error of the float32 restatement of the oracle, never beyond 10 x.  Every case's restatement
    stays below 10 bars but those of duplicated placements at var = 1e-4: there float32 rounds logsumexp (about -1.8e6 + log K) to a
    multiple of 0.125, which rescales every weight alike by up to 6 %; the kernel keeps the max and the sum apart, so these cases
    are held to the plain bar instead."""
    for name in G.CASES:
        r = G.restatement_ratios(name, form, G.centred_target(form))
        print('%-20s %-14s float32 restatement / bar: logp %.3f, grad %.3f, widen %s' % (name, form, r['logp'], r['grad'], G.widen(r)))
        assert (max(r['logp'], r['grad']) <= 10.0) != name.startswith('n65-K') or name.startswith('n65-K1-'), (name, form, r)
        assert 1.0 <= min(G.widen(r).values()) and max(G.widen(r).values()) <= 10.0


def test_replica_of_the_quarters_and_the_ties():
    r = G.replica('translate', 65, 300, 7, False)
    assert r['quarters'] == [(0, 1), (1, 3), (3, 5), (5, 7)] and r['listed'] and r['tiles'] == 2 and r['live_in_last_tile'] == 1
    assert G.replica('rigid', 64, 255, 255, False)['quarters'] == [(0, 63), (63, 127), (127, 191), (191, 255)]
    assert G.replica('rigid', 129, 2049, 2049, True)['K'] == 2049 and not G.replica('rigid', 129, 2049, 2049, True)['listed']
    assert G.replica('rigid', 129, 2050, 2048, True)['listed'] and G.replica('rigid', 129, 2048, 2048, True)['cap'] == 2048
    assert G.replica('rigid', 129, 300, 300, False)['cap'] == 300
    x0, _ = G.inputs('n65-K5-P300', 'rigid')
    st, ties = G.with_ties('rigid', x0, G.thinned(G.every_start(65, [6, 7]), 300), 5, 350)
    assert torch.equal(st, G.inputs('n65-K5-P300', 'rigid')[1]) and len(ties) == 5 and len({tuple(st[i].tolist()) for i in ties}) == 1
    from genie2_amd.smc import _check_starts
    for form in G.FORMS:
        for name, c in G.CASES.items():
            _check_starts(G.inputs(name, form)[1], G.motif(form)[1], c['n_res'])
