"""CPU part of the training-path coverage (tests/_train_paths.py): the case list reaches every row of the GEMM / LayerNorm
dispatch table, and the float32 autograd reference the GPU tests are read against is itself well inside its bound."""
import pytest
import torch

import _train_paths as T


def test_case_list_covers_the_dispatch_table():
    """gemm_kernel_choice / gemm_splits replayed over CASES plus the two shapes test_training.py already runs: each row of the
    table must be reached by one of them; a missing row fails by name."""
    rows = [T.dispatch_row(c['lengths']) for c in T.CASES.values()] + [T.dispatch_row(l) for l in T.SUITE_SHAPES]
    new = rows[:len(T.CASES)]
    for r in rows:
        print(r)
    have = set()
    for r in rows:
        for k in r['fwd'].values():
            have.add(('forward Linear', k))
        have.add(('contraction', r['contraction']))
        for w in r['wgrad'].values():
            if w['empty'] > 0:
                have.add(('weight gradient with an empty K range', w['kernel']))
            if w['branch'] == 'long_k':
                have.add('first branch of gemm_splits')
            have.add(('row sums', w['row_sums']))
            if w['cblk']:
                have.add(('cblk weight gradient', w['cblk']))
        have.add(('cblk forward', r['cblk_fwd']))
        if r['P'] >= 4096:
            have.add(('ReLU sign-bit mask at P >= 4096', r['mask']))
        if r['ln128'] and r['P_mod8']:
            have.add('LN128 with P % 8 != 0')
        if r['ln128'] and r['P_mod32']:
            have.add('LN128 with P % 32 != 0')
        have.add(('LN128', r['ln128']))
    want = [(kind, k) for kind in ('forward Linear', 'contraction', 'weight gradient with an empty K range') for k in (T.GENERIC, T.TILE64, T.TILE128)]
    want += ['first branch of gemm_splits', ('ReLU sign-bit mask at P >= 4096', True), ('ReLU sign-bit mask at P >= 4096', False),
             ('cblk forward', 'table'), ('cblk forward', 'fallback'), ('cblk weight gradient', 'table'), ('cblk weight gradient', 'fallback'),
             ('row sums', 'gemm'), ('row sums', 'k_colsum'), 'LN128 with P % 8 != 0', 'LN128 with P % 32 != 0', ('LN128', True), ('LN128', False)]
    missing = [w for w in want if w not in have]
    assert not missing, missing
    # the mixes the issue lists: tiled kernels of both sizes inside ONE step, and an empty range on each kernel among the new cases
    assert any(set(r['fwd'].values()) == {T.TILE64, T.TILE128} for r in new)
    assert {w['kernel'] for r in new for w in r['wgrad'].values() if w['empty'] > 0} == {T.GENERIC, T.TILE64, T.TILE128}
    assert [r['P'] for r in new] == sorted((r['P'] for r in new), reverse=True)          # descending: one workspace allocation


def test_replica_matches_recorded_launches():
    """the split factors and empty ranges of the weight gradients at the five cases, as replayed when the cases were chosen:
    (kernel, nsplit, empty K ranges) of the five-Linear stack, transition and z gradients"""
    want = {'n47_31': [(T.GENERIC, 32, 4)] * 3, 'n40_33_21': [(T.TILE64, 32, 2)] * 3,
            'n56_40': [(T.TILE128, 40, 0), (T.TILE128, 48, 8), (T.TILE64, 48, 8)],
            'n64_33': [(T.TILE128, 40, 3), (T.TILE128, 48, 5), (T.TILE64, 64, 0)],
            'n92_60': [(T.TILE128, 96, 7), (T.TILE128, 128, 22), (T.TILE64, 128, 22)]}
    for name, w in want.items():
        r = T.dispatch_row(T.CASES[name]['lengths'])['wgrad']
        got = [(r[k]['kernel'], r[k]['nsplit'], r[k]['empty']) for k in ('stack5', 'transition1', 'z')]
        assert got == w, (name, got)
    # the shapes test_train_gemm.py adds are these launches
    for (M, N, K), ns, kern, empty in [((640, 128, 16928), 96, T.TILE128, 7), ((128, 128, 16928), 128, T.TILE64, 22), ((512, 128, 6272), 48, T.TILE128, 8)]:
        assert T.gemm_splits(M, N, K) == ns and T.gemm_kernel_choice(M, N, K, nsplit=ns) == kern and T.empty_k_ranges(K, ns) == empty


@pytest.mark.parametrize('name', list(T.CASES))
def test_float32_oracle_is_inside_its_own_bound(name):
    """Each tensor of the float32 oracle's gradients within 1e-3 of that tensor's largest magnitude (check_grads' floor) of the
    float64 oracle's on the same float32 values: a fifth of the 5e-3 the kernels are held to, so that the bar means something at
    these shapes.  (What is left is rows at a ReLU threshold.)  A seed that misses is replaced by the oracle's verdict alone."""
    g32, g64 = T.oracle_grads(name, torch.float32)['grads'], T.oracle_grads(name, torch.float64)['grads']
    worst = T.worst_tensor(g32, g64)
    print(name, 'P', T.dispatch_row(T.CASES[name]['lengths'])['P'], 'worst tensor', worst, 'e32_L2 %.3g' % T.rel_l2(g32, g64))
    assert worst[0] <= 1e-3, worst
