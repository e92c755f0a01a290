"""Group-wise motif guidance: genie_motif_potential_grouped (csrc/smc_kernels.hip), MotifPotential(groups=...) and its locate in
genie2_amd/smc.py, TwistedSampler.last_fit and the CLI's --motif_groups, against the float64 oracle of tests/_motif_groups.py (every
group centred and fitted on its own, Kabsch by SVD, torch autograd).

Bounds, those the translation and rigid kernels are held to (tests/test_motif_rigid.py): logp within 1e-5 max(1, |logp|); gradient
within 1e-5 of the particle's largest gradient entry; rmsd and group_rmsd within 1e-5 relative + 1e-4 A; `best` equal to the oracle's,
asserted only where the oracle's two best scores differ by more than 1e-4 relative for every particle (they do for every case below:
the smallest gap is 2.4e-3, found on the CPU in float64).  The planted fit alone compares its gradient to
1e-5 (max|g_b| + max|t_c| / var): there the gradient is the difference of two terms of size |t_c| / var."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from _motif import (MOTIF, _abar, _ca_coordinates, _check, _fix_var, _lds_cap, _pot, _run, _tiny_model, _var500, all_starts, segments_6e6r,
                    top_two_gap, walk)
from _motif_groups import canonical, group_fit_rmsd, grouped_logp_only, grouped_oracle, planted, random_rotation, segments_343
from _motif_rigid import rigid_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE = {}


def _oracle(key, x0, starts, lens, seg_group, target, var, **kw):
    """One float64 reference per (case, var), shared by the tests that need it."""
    k = (key, float(var), tuple(sorted(kw.items())))
    if k not in _ORACLE:
        _ORACLE[k] = grouped_oracle(x0, starts, lens, seg_group, target, var, **kw)
    return _ORACLE[k]


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rigid', [True, False])
def test_grouped_oracle_gradient_matches_central_differences(rigid):
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    starts = all_starts(20, lens)
    assert starts.shape == (36, 2)
    x0, tgt, var = walk(2, 20, 3), torch.cat(segs), 0.5
    ref = grouped_oracle(x0, starts, lens, [0, 1], tgt, var, rigid=rigid)
    gmax = float(ref['grad'].abs().max())
    x, h = x0.double(), 1e-5
    fd = torch.zeros_like(x)
    for i in range(x.numel()):
        e = torch.zeros(x.numel(), dtype=torch.float64)
        e[i] = h
        e = e.reshape(x.shape)
        fd.view(-1)[i] = (grouped_logp_only(x + e, starts, lens, [0, 1], tgt, var, rigid)
                          - grouped_logp_only(x - e, starts, lens, [0, 1], tgt, var, rigid)) / (2 * h)
    d = float((ref['grad'] - fd).abs().max())
    print('grouped oracle gradient against central differences: %.2e of the largest entry' % (d / gmax))
    assert d <= 1e-6 * gmax
    # one group is the single-motif oracle
    one = grouped_oracle(x0, starts, lens, [0, 0], tgt, var, rigid=True)
    old = rigid_oracle(x0, starts, lens, tgt, var)
    assert torch.allclose(one['logp'], old['logp'], rtol=1e-12, atol=0) and torch.allclose(one['grad'], old['grad'], rtol=0, atol=1e-12 * gmax)


def test_per_group_fit_finds_the_planted_motifs_and_the_welded_fit_does_not():
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    starts, tgt = all_starts(60, lens), torch.cat(segs)
    x0 = planted(segs)
    ref = grouped_oracle(x0, starts, lens, [0, 1], tgt, 1.0, want_grad=False)
    assert starts[ref['best'][0]].tolist() == [5, 30] and float(ref['group_rmsd'][0].max()) < 1e-5
    old = rigid_oracle(x0, starts, lens, tgt, 1.0, want_grad=False)
    print('welded fit: placement %s at %.2f A' % (starts[old['best'][0]].tolist(), float(old['rmsd'][0])))
    assert starts[old['best'][0]].tolist() != [5, 30] and float(old['rmsd'][0]) > 1.0


def test_grouped_entry_rejects_impossible_shapes_and_sizes_its_work():
    """The C entry validates its shape before it touches the device (so this runs without one), and says how much work it needs."""
    from genie2_amd import build, capi
    build.build()
    lib = capi.load_library()
    header = open(os.path.join(ROOT, 'include', 'genie_hip.h')).read()
    gmax = int(re.search(r'#define\s+GENIE_MOTIF_MAX_GROUPS\s+(\d+)', header).group(1))
    assert gmax == capi.MOTIF_MAX_GROUPS >= 8
    wb = lib.genie_motif_potential_grouped_work_bytes
    assert wb(8, 1000, 2, 1) == 0 and wb(8, 1000, 2, 0) == 0
    assert wb(2, 20000, 2, 1) >= 2 * 20000 * (2 * 32 + 4) and wb(2, 20000, 2, 0) >= 2 * 20000 * (2 * 16 + 4)
    for align in (0, 1):
        for G in (1, 2, gmax):
            seq = [wb(3, P, G, align) for P in (1, 100, 378, 379, 1445, 1446, 3000, 5000, 20000)]
            assert seq == sorted(seq) and seq[0] == 0 and seq[-1] > 0, (align, G, seq)
        for P in (379, 1446, 5000):
            seq = [wb(3, P, G, align) for G in range(1, gmax + 1)]
            assert seq == sorted(seq), (align, P, seq)
    need = wb(2, 20000, 2, 1)
    d = C.c_void_p(64)                                           # never dereferenced: every call below fails its shape check

    def call(B=2, N=60, P=10, S=2, M=13, G=2, align=1, x0=d, seg_group=d, logp=d, grad=d, best=d, rmsd=d, grmsd=d, work=None,
             work_bytes=0):
        return lib.genie_motif_potential_grouped(None, B, N, x0, P, S, M, G, d, seg_group, d, d, d, align, logp, grad, best, rmsd, grmsd,
                                                 work, work_bytes)

    assert call(G=0) == -1 and call(G=3) == -1 and call(G=gmax + 1, S=gmax + 1, M=40) == -1          # G < 1, G > S, G > max
    assert call(align=2) == -1 and call(align=-1) == -1
    assert call(M=5) == -1 and call(M=5, align=0, P=20000) == -1           # rigid needs M >= 3 G; translation gets as far as `work`
    assert call(P=0) == -1 and call(S=0) == -1 and call(B=0) == -1 and call(N=0) == -1 and call(M=0) == -1
    assert call(M=61) == -1 and call(S=14) == -1
    assert call(P=20000) == -1                                   # large P needs work
    assert call(P=20000, work=d, work_bytes=need - 1) == -1
    assert call(grad=d, logp=None) == -1 and call(logp=d, grad=None) == -1
    assert call(logp=None, grad=None, best=None, rmsd=None, grmsd=None) == -1
    assert call(x0=None) == -1 and call(seg_group=None) == -1


def test_motif_groups_are_read_from_the_problem_file_and_canonicalised():
    from genie2_amd.sample_unconditional_motif import load_motif_groups, load_motif_segments
    from genie2_amd.smc import canonical_groups
    assert load_motif_groups(MOTIF) == ['A', 'B'] and len(load_motif_segments(MOTIF)) == 2
    assert canonical_groups(['B', 'A', 'B'], 3) == (['B', 'A'], [0, 1, 0])
    assert canonical_groups([(1, 'x'), (1, 'x')], 2) == ([(1, 'x')], [0, 0])
    assert canonical(['B', 'A', 'B']) == (['B', 'A'], [0, 1, 0])
    with pytest.raises(ValueError, match='one label per segment'):
        canonical_groups(['A'], 2)
    import genie.sample_unconditional_motif as cli
    assert cli.build_parser().parse_args(['--name', 'b', '--epoch', '1', '--scale', '0.6', '--outdir', 'o', '--motif_file', MOTIF,
                                          '--motif_groups', 'file']).motif_groups == 'file'


def test_motif_cli_parser_has_the_groups_flag():
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    base = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o', '--motif_file', MOTIF]
    a = build_parser().parse_args(base)
    assert a.motif_groups == 'joint'
    c = MotifRunner().create_constants(vars(a))
    assert c['motif_groups'] == 'joint' and c['groups'] is None
    a = build_parser().parse_args(base + ['--motif_groups', 'file'])
    c = MotifRunner().create_constants(vars(a))
    assert a.motif_groups == 'file' and c['motif_groups'] == 'file' and c['groups'] == ['A', 'B']
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ['--motif_groups', 'welded'])


def test_motif_potential_validates_its_groups_on_the_host():
    """Every refusal is made before the device is looked at (so this runs without one)."""
    from genie2_amd import build, capi
    from genie2_amd.smc import MotifPotential
    build.build()
    segs = segments_6e6r()
    abar = torch.linspace(0.99, 0.01, 11)
    with pytest.raises(ValueError, match='one label per segment'):
        MotifPotential(segs, 60, abar, groups=['A'])
    with pytest.raises(ValueError, match='one label per segment'):
        MotifPotential(segs, 60, abar, groups=['A', 'B', 'C'], align='rigid')
    many = [torch.randn(3, 3, generator=torch.Generator().manual_seed(i)) for i in range(capi.MOTIF_MAX_GROUPS + 1)]
    with pytest.raises(ValueError, match='at most %d' % capi.MOTIF_MAX_GROUPS):
        MotifPotential(many, 60, abar, groups=list(range(len(many))))
    two = torch.tensor([[0.0, 0.0, 0.0], [3.8, 0.0, 0.0]])
    with pytest.raises(ValueError, match="at least 3 motif residues.*group 'B'"):
        MotifPotential([segs[0], two], 60, abar, groups=['A', 'B'], align='rigid')
    line = torch.arange(4.0)[:, None] * torch.tensor([[1.0, 2.0, 3.0]])
    with pytest.raises(ValueError, match="group 'L' are collinear"):
        MotifPotential([line, segs[1]], 60, abar, groups=['L', 'B'], align='rigid')
    # A, B, A: the two short pieces of A make one body of 4 residues that are not collinear
    bent = torch.tensor([[9.0, 1.0, 0.0], [9.0, 5.0, 2.0]])
    with pytest.raises(ValueError, match="group 'B'"):
        MotifPotential([two, two, bent], 60, abar, groups=['A', 'B', 'A'], align='rigid')


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _check_fit(fit, ref, what):
    gap = top_two_gap(ref['score']) if ref['score'].shape[1] > 1 else torch.ones(ref['score'].shape[0])
    best, rmsd = fit['best'].cpu().long(), fit['rmsd'].double().cpu()
    print(what, 'top-two gap', gap.tolist(), 'best', best.tolist(), ref['best'].tolist(), 'rmsd', rmsd.tolist(), ref['rmsd'].tolist())
    assert bool((gap > 1e-4).all()), (what, gap)                     # the argmax is the oracle's to decide, for every particle
    assert torch.equal(best, ref['best']), (what, best, ref['best'])
    assert bool(((rmsd - ref['rmsd']).abs() <= 1e-5 * ref['rmsd'] + 1e-4).all()), (what, rmsd, ref['rmsd'])
    if 'group_rmsd' in fit:
        gr = fit['group_rmsd'].double().cpu()
        print(what, 'group rmsd', gr.tolist(), ref['group_rmsd'].tolist())
        assert gr.shape == ref['group_rmsd'].shape
        assert bool(((gr - ref['group_rmsd']).abs() <= 1e-5 * ref['group_rmsd'] + 1e-4).all()), (what, gr, ref['group_rmsd'])


def _entry(pot, seg_group, x, var, align, want_potential=True, want_fit=True):
    """The C entry itself with every output, or with one set NULL."""
    B, G = x.shape[0], max(seg_group) + 1
    need = pot.lib.genie_motif_potential_grouped_work_bytes(B, pot.P, G, align)
    work = torch.empty(max(need, 16), dtype=torch.uint8, device='cuda')
    v = torch.tensor([var], dtype=torch.float32, device='cuda')
    sg = torch.tensor(seg_group, dtype=torch.int32, device='cuda')
    logp, grad = torch.full((B,), 7.0, device='cuda'), torch.full_like(x, 7.0)
    best, rmsd = torch.full((B,), -7, dtype=torch.int32, device='cuda'), torch.full((B,), 7.0, device='cuda')
    grmsd = torch.full((B, G), 7.0, device='cuda')
    p = lambda t, on=True: C.c_void_p(t.data_ptr()) if on else None      # noqa: E731
    rc = pot.lib.genie_motif_potential_grouped(C.c_void_p(torch.cuda.current_stream().cuda_stream), B, pot.n_res, p(x), pot.P, pot.S,
                                               pot.M, G, p(pot.seg_len_t), p(sg), p(pot.starts), p(pot.target), p(v), align,
                                               p(logp, want_potential), p(grad, want_potential), p(best, want_fit), p(rmsd, want_fit),
                                               p(grmsd, want_fit), p(work, need > 0), work.numel())
    torch.cuda.synchronize()
    assert rc == 0
    return logp, grad, best, rmsd, grmsd


@pytest.mark.gpu
@pytest.mark.parametrize('align', ['rigid', 'translation'])
def test_one_group_is_the_single_motif_three_ways(align):
    abar = _abar()
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    pot = _pot(segs, 20, abar, align=align, groups=['A', 'A'])
    assert pot.P == 36 and pot.groups is None                            # one label: the single-motif entries, as without `groups`
    x0 = walk(2, 20, 3)
    rigid = align == 'rigid'
    ref = _oracle('one', x0, pot.starts.cpu(), lens, [0, 0], pot.target, var, rigid=rigid)
    logp, grad, best, rmsd, grmsd = _entry(pot, [0, 0], x0.cuda().contiguous(), var, int(rigid))
    _check(logp, grad, ref, 'G=1 entry ' + align)
    _check_fit({'best': best, 'rmsd': rmsd, 'group_rmsd': grmsd}, ref, 'G=1 entry ' + align)
    assert torch.equal(grmsd[:, 0], rmsd)
    # the existing entry on the same inputs, held to the same bounds
    lp_old, g_old = _run(pot, x0)
    _check(logp, grad, {'logp': lp_old.double().cpu(), 'grad': g_old.double().cpu()}, 'G=1 entry against the existing ' + align)
    _check(lp_old, g_old, ref, 'existing entry ' + align)
    if rigid:
        fit = pot.locate(x0.cuda())
        assert 'group_rmsd' not in fit and torch.equal(fit['best'], best.long())
        assert bool(((fit['rmsd'] - rmsd).abs() <= 1e-5 * rmsd + 1e-4).all())


@pytest.mark.gpu
@pytest.mark.parametrize('align', ['rigid', 'translation'])
def test_two_groups_match_the_float64_oracle_n20(align):
    abar = _abar()
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    pot = _pot(segs, 20, abar, align=align, groups=['A', 'B'])
    assert pot.P == 36 and pot.groups == ['A', 'B'] and pot.seg_group == [0, 1] and pot.has_fit
    x0 = walk(2, 20, 3)
    ref = _oracle('n20', x0, pot.starts.cpu(), lens, [0, 1], pot.target, var, rigid=align == 'rigid')
    _check(*_run(pot, x0), ref, 'N=20 ' + align)
    fit = pot.locate(x0.cuda())                                         # always the superposed fit
    _check_fit(fit, _oracle('n20', x0, pot.starts.cpu(), lens, [0, 1], pot.target, 1.0, rigid=True, want_grad=False), 'N=20 locate')
    assert fit['groups'] == ['A', 'B'] and fit['group_rmsd'].shape == (2, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('align', ['rigid', 'translation'])
@pytest.mark.parametrize('B', [1, 3])
def test_two_groups_match_the_float64_oracle_every_placement_of_n60(B, align):
    abar = _abar()
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    x0 = walk(B, 60, 10 + B)
    # var of schedule step 500, then one / a few / all placements carrying weight
    for v in (None, 1e-4, 1.0, 30.0, 1e4):
        pot = _pot(segs, 60, abar, align=align, groups=['A', 'B'])
        assert pot.P == 1176
        var = _var500(abar) if v is None else _fix_var(pot, v)
        ref = _oracle('n60b%d' % B, x0, pot.starts.cpu(), lens, [0, 1], pot.target, var, rigid=align == 'rigid')
        w = torch.softmax(ref['score'], dim=1)
        print('var %g: placements with weight > 1e-3: %s' % (var, (w > 1e-3).sum(dim=1).tolist()))
        _check(*_run(pot, x0), ref, 'N=60 B=%d var=%g %s' % (B, var, align))
    if align == 'rigid':
        _check_fit(pot.locate(x0.cuda()), ref, 'N=60 B=%d' % B)


@pytest.mark.gpu
@pytest.mark.parametrize('align', ['rigid', 'translation'])
def test_two_groups_match_the_float64_oracle_two_residue_tiles_n80(align):
    abar = _abar()
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    pot = _pot(segs, 80, abar, align=align, groups=['A', 'B'])
    assert pot.P == 2346
    x0 = walk(2, 80, 81)
    ref = _oracle('n80', x0, pot.starts.cpu(), lens, [0, 1], pot.target, var, rigid=align == 'rigid')
    _check(*_run(pot, x0), ref, 'N=80 ' + align)
    if align == 'rigid':
        _check_fit(pot.locate(x0.cuda()), ref, 'N=80')


@pytest.mark.gpu
@pytest.mark.parametrize('labels,align', [('ABA', 'rigid'), ('ABA', 'translation'), ('ABC', 'rigid')])
def test_groups_of_separate_segments_and_of_three_residues_n24(labels, align):
    """A, B, A: a group whose two segments are not adjacent.  A, B, C: two groups of exactly 3 residues, superposed."""
    abar = _abar()
    segs = segments_343()
    lens = [3, 4, 3]
    var = _var500(abar)
    names, index = canonical(labels)
    pot = _pot(segs, 24, abar, align=align, groups=list(labels))
    assert pot.P == 680 and pot.seg_group == index and pot.groups == names and pot.G == len(names)
    x0 = walk(3, 24, 33)                                                 # (three-residue groups fit almost anywhere: this walk keeps the top two apart)
    ref = _oracle(labels, x0, pot.starts.cpu(), lens, index, pot.target, var, rigid=align == 'rigid')
    _check(*_run(pot, x0), ref, '%s %s' % (labels, align))
    if align == 'rigid':
        _check_fit(pot.locate(x0.cuda()), ref, labels)


@pytest.mark.gpu
@pytest.mark.parametrize('align', ['rigid', 'translation'])
@pytest.mark.parametrize('which', ['cap', 'cap+1'])
def test_two_groups_match_the_float64_oracle_around_the_lds_cap(which, align):
    from genie2_amd import capi
    abar = _abar()
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    a = int(align == 'rigid')
    cap = _lds_cap(lambda P: capi.load_library().genie_motif_potential_grouped_work_bytes(2, P, 2, a))
    P = cap + (which == 'cap+1')
    pot = _pot(segs, 256, abar, P=P, seed=22, align=align, groups=['A', 'B'])
    assert pot.P == P and (pot.lib.genie_motif_potential_grouped_work_bytes(2, P, 2, a) > 0) == (which != 'cap')
    x0 = walk(2, 256, 23)
    ref = _oracle('cap%s%s' % (which, align), x0, pot.starts.cpu(), lens, [0, 1], pot.target, var, rigid=bool(a))
    _check(*_run(pot, x0), ref, 'N=256 B=2 P=%d %s' % (P, align))
    if a:
        _check_fit(pot.locate(x0.cuda()), ref, 'N=256 B=2 P=%d' % P)


@pytest.mark.gpu
def test_planted_groups_are_found_where_the_welded_fit_is_not_and_a_mirror_image_shows_in_its_own_group():
    abar = _abar()
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    pot = _pot(segs, 60, abar, align='rigid', groups=['A', 'B'])
    assert pot.P == 1176
    tc = pot.target.cpu()
    x0 = planted(segs)
    ref = _oracle('planted', x0, pot.starts.cpu(), lens, [0, 1], tc, var)
    _check(*_run(pot, x0), ref, 'planted groups', grad_floor=float(tc.abs().max()) / var)
    fit = pot.locate(x0.cuda())
    _check_fit(fit, ref, 'planted groups')
    print('planted: starts', fit['starts'][0].tolist(), 'group rmsd', fit['group_rmsd'][0].tolist())
    assert fit['starts'][0].tolist() == [5, 30] and fit['ends'][0].tolist() == [10, 36]
    assert float(fit['group_rmsd'][0].max()) <= 1e-3 and float(fit['rmsd'][0]) <= 1e-3

    # the same coordinates without groups: the two motifs welded in the pose of the file
    old = _pot(segs, 60, abar, align='rigid').locate(x0.cuda())
    print('welded: starts', old['starts'][0].tolist(), 'rmsd', float(old['rmsd'][0]))
    assert 'group_rmsd' not in old and old['starts'][0].tolist() != [5, 30] and float(old['rmsd'][0]) > 1.0

    # group B's copy mirrored: at the planted placement B no longer fits, A is as it was
    xm = planted(segs, mirror=1)
    at = int((pot.starts.cpu() == torch.tensor([5, 30], dtype=torch.int32)).all(dim=1).nonzero()[0, 0])
    pot.starts, pot.P = pot.starts[at:at + 1].contiguous(), 1
    fm = pot.locate(xm.cuda())
    want = group_fit_rmsd(xm[0], [5, 30], lens, [0, 1], tc)
    print('mirror image of B at the planted placement: group rmsd', fm['group_rmsd'][0].tolist(), 'oracle', want.tolist())
    assert float(want[1]) > 1.0 and float(want[0]) < 1e-5
    assert bool(((fm['group_rmsd'][0].double().cpu() - want).abs() <= 1e-5 * want + 1e-4).all())
    assert float(fm['group_rmsd'][0, 0]) <= 1e-3 and float(fm['group_rmsd'][0, 1]) > 1.0


@pytest.mark.gpu
def test_grouped_rigid_potential_does_not_depend_on_the_pose_of_a_group_in_the_file():
    abar = _abar()
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    g = torch.Generator().manual_seed(5)
    r = random_rotation(g).float()
    moved = [segs[0], segs[1] @ r.T + torch.tensor([[7.0, -3.0, 11.0]])]
    x0 = walk(2, 60, 71)
    pot = _pot(segs, 60, abar, align='rigid', groups=['A', 'B'])
    ref = _oracle('inv', x0, pot.starts.cpu(), lens, [0, 1], pot.target, var)
    a = _run(pot, x0)
    b = _run(_pot(moved, 60, abar, align='rigid', groups=['A', 'B']), x0)
    _check(*a, ref, 'file pose')
    _check(*b, ref, 'group B rotated and shifted')
    # the single rigid motif does depend on it
    c = _run(_pot(segs, 60, abar, align='rigid'), x0)
    d = _run(_pot(moved, 60, abar, align='rigid'), x0)
    tol = 1e-5 * c[0].abs().clamp(min=1.0)
    print('welded logp', c[0].tolist(), 'with B moved', d[0].tolist())
    assert bool(((c[0] - d[0]).abs() > 100 * tol).all())


@pytest.mark.gpu
def test_grouped_gradient_is_zero_where_no_placement_reaches_and_null_outputs_are_left_alone():
    abar = _abar()
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    var = _var500(abar)
    for align in ('rigid', 'translation'):
        pot = _pot(segs, 60, abar, P=1, seed=3, align=align, groups=['A', 'B'])
        assert pot.P == 1
        st = pot.starts[0].tolist()
        lp, g = _run(pot, walk(2, 60, 3), 400)
        outside = torch.ones(60, dtype=torch.bool)
        for s, n in zip(st, lens):
            outside[s:s + n] = False
        assert bool((g[:, outside] == 0).all()) and bool((g[:, ~outside] != 0).any()), align
    pot = _pot(segs, 80, abar, align='rigid', groups=['A', 'B'])
    x = walk(2, 80, 81).cuda().contiguous()
    logp, grad, best, rmsd, grmsd = _entry(pot, [0, 1], x, var, 1)
    ref = _oracle('n80', x.cpu(), pot.starts.cpu(), lens, [0, 1], pot.target, var, rigid=True)
    _check(logp, grad, ref, 'entry N=80')
    _check_fit({'best': best, 'rmsd': rmsd, 'group_rmsd': grmsd}, ref, 'entry N=80')
    lp2, g2, b2, r2, gr2 = _entry(pot, [0, 1], x, var, 1, want_fit=False)
    assert torch.equal(lp2, logp) and torch.equal(g2, grad) and bool((b2 == -7).all()) and bool((r2 == 7.0).all()) and bool((gr2 == 7.0).all())
    lp3, g3, b3, r3, gr3 = _entry(pot, [0, 1], x, var, 1, want_potential=False)
    assert torch.equal(b3, best) and torch.equal(r3, rmsd) and torch.equal(gr3, grmsd) and bool((lp3 == 7.0).all()) and bool((g3 == 7.0).all())
    lp4, g4 = _run(pot, x.cpu())
    assert torch.equal(lp4, logp) and torch.equal(g4, grad)


@pytest.mark.gpu
@pytest.mark.parametrize('align', ['rigid', 'translation'])
@pytest.mark.parametrize('P', [1000, 3000])
def test_grouped_potential_is_deterministic_and_never_synchronises(P, align):
    abar = _abar()
    pot = _pot(segments_6e6r(), 256, abar, P=P, seed=P, align=align, groups=['A', 'B'])
    assert (pot.lib.genie_motif_potential_grouped_work_bytes(8, P, 2, int(align == 'rigid')) > 0) == (P == 3000)
    x0 = walk(8, 256, 7).cuda()
    a = _run(pot, x0, 400)
    b = _run(pot, x0, 400)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), P
    x = x0.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        lp = pot(x, 400)
        g, = torch.autograd.grad(lp.mean(), x)
        fit = pot.locate(x0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(lp, a[0]) and torch.equal(g, a[1] * 0.125)          # (the backward scales by grad_output = 1/8)
    assert bool((fit['rmsd'] > 0).all()) and bool((fit['group_rmsd'] > 0).all())


@pytest.mark.gpu
def test_locate_needs_three_residues_in_every_group():
    abar = _abar()
    segs = segments_6e6r()
    pot = _pot([segs[0], segs[1][:2]], 40, abar, groups=['A', 'B'])
    assert pot.groups == ['A', 'B'] and not pot.has_fit
    with pytest.raises(ValueError):
        pot.locate(walk(1, 40, 1).cuda())
    lp, g = _run(pot, walk(2, 40, 1))                                    # the translation form guides all the same
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all())


@pytest.mark.gpu
def test_grouped_guidance_pulls_both_motifs_in_and_the_sampler_reports_every_group(tmp_path, base_weights):
    """No numeric bar is set for the pull: the guided mean RMSD has to be below the unguided one on identical noise, and the ratio is
    printed (the single rigid motif's test holds 0.5 for its own ratio)."""
    from genie2_amd import pack
    from genie2_amd.smc import TwistedSampler
    B, N, T = 4, 40, 12
    model = _tiny_model(base_weights, T)
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    abar = pack.schedule_tensors(T)['alphas_cumprod'].cuda()
    noise = torch.randn(T, B, N, 3, generator=torch.Generator().manual_seed(4))
    base = {'length': N, 'scale': 0.6, 'num_samples': B, 'outdir': str(tmp_path), 'prefix': 'x', 'offset': 0, 'noise': noise,
            'last_unguided_steps': 0, 'guidance_alpha': 0.05, 'ess_threshold': 0.0}
    tw = TwistedSampler(model)
    pot = _pot(segs, N, abar, tausq=0.5, align='rigid', groups=['A', 'B'])
    assert pot.P == 406

    out = tw._sample(dict(base, twisting_function=pot))
    xyz = torch.from_numpy(np.stack([r['atom_positions'] for r in out]))
    fit = tw.last_fit
    assert bool(torch.isfinite(xyz).all()) and tw.resampled_at == []
    assert all(not t.is_cuda for t in fit.values() if torch.is_tensor(t)) and fit['groups'] == ['A', 'B']
    assert fit['best'].shape == (B,) and fit['starts'].shape == (B, 2) and fit['group_rmsd'].shape == (B, 2)
    ref = grouped_oracle(xyz, pot.starts.cpu(), lens, [0, 1], pot.target, 1.0, want_grad=False)
    _check_fit(fit, ref, 'last_fit')
    assert torch.equal(fit['starts'], pot.starts.cpu()[fit['best']].long())

    # the same noise without guidance: a potential that does not depend on x0 (and has no locate)
    free = tw._sample(dict(base, twisting_function=lambda x0, step: (x0 * 0).sum(dim=(1, 2))))
    assert tw.last_fit is None
    xyz_free = torch.from_numpy(np.stack([r['atom_positions'] for r in free]))
    rmsd_free = pot.locate(xyz_free.cuda())['rmsd'].cpu()
    print('per-group superposed motif RMSD: guided %s (mean %.3f), unguided %s (mean %.3f), ratio %.3f'
          % (fit['rmsd'].tolist(), float(fit['rmsd'].mean()), rmsd_free.tolist(), float(rmsd_free.mean()),
             float(fit['rmsd'].mean()) / float(rmsd_free.mean())))
    assert float(fit['rmsd'].mean()) < float(rmsd_free.mean())


@pytest.mark.gpu
def test_motif_cli_writes_one_rmsd_line_per_group(tmp_path, base_weights):
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser
    root = str(tmp_path / 'results')
    d = os.path.join(root, 'base')
    os.makedirs(d)
    with open(os.path.join(d, 'configuration'), 'w') as fh:
        fh.write('name base\nnumTimesteps 12\n')
    g = Genie(Config(os.path.join(d, 'configuration')))
    g.model.load_state_dict(base_weights)
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.7.ckpt'), epoch=7)
    out = str(tmp_path / 'out')
    common = ['--name', 'base', '--epoch', '7', '--rootdir', root, '--scale', '0.6', '--motif_file', MOTIF, '--last_unguided_steps', '0',
              '--batch_size', '2', '--num_samples', '2', '--align', 'rigid', '--write_motif_locations']
    args = build_parser().parse_args(common + ['--outdir', out, '--min_length', '40', '--max_length', '56', '--length_step', '16',
                                               '--motif_groups', 'file'])
    np.random.seed(0)
    torch.manual_seed(0)
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    names = sorted('{}_{}'.format(n, i) for n in (56, 40) for i in range(2))
    assert sorted(os.listdir(os.path.join(out, 'pdbs'))) == [n + '.pdb' for n in names]
    assert sorted(os.listdir(os.path.join(out, 'motif_locations'))) == [n + '.txt' for n in names]
    segs = segments_6e6r()
    lens = [len(s) for s in segs]
    for name in names:
        n = int(name.split('_')[0])
        lines = open(os.path.join(out, 'motif_locations', name + '.txt')).read().splitlines()
        assert len(lines) == 5 and lines[2].startswith('# rmsd ') and not lines[2].startswith('# rmsd group'), (name, lines)
        assert [line.split()[:4] for line in lines[3:]] == [['#', 'rmsd', 'group', 'A'], ['#', 'rmsd', 'group', 'B']], lines
        spans = [tuple(int(v) for v in line.split('\t')) for line in lines[:2]]
        assert [e - s + 1 for s, e in spans] == lens and spans[0][0] >= 0 and spans[0][1] < spans[1][0] and spans[1][1] <= n - 1, spans
        xyz = _ca_coordinates(os.path.join(out, 'pdbs', name + '.pdb'))
        assert xyz.shape == (n, 3) and np.isfinite(xyz).all()
        want = group_fit_rmsd(xyz, [s for s, _ in spans], lens, [0, 1], torch.cat(segs))
        print(name, spans, lines[2:], 'oracle on the PDB: %s' % want.tolist())
        for k in (0, 1):
            value = lines[3 + k].split()[4]
            assert len(value.split('.')[1]) == 3 and abs(float(value) - float(want[k])) <= 2e-3, (name, lines[3 + k], want)
        overall = float(torch.sqrt((want ** 2 * torch.tensor(lens)).sum() / sum(lens)))
        assert abs(float(lines[2].split()[2]) - overall) <= 2e-3, (name, lines[2], overall)

    # without --motif_groups the files are as they were: the spans and one `# rmsd` line
    out2 = str(tmp_path / 'out2')
    args = build_parser().parse_args(common + ['--outdir', out2, '--min_length', '40', '--max_length', '40'])
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)
    for name in ('40_0', '40_1'):
        lines = open(os.path.join(out2, 'motif_locations', name + '.txt')).read().splitlines()
        assert len(lines) == 3 and lines[2].startswith('# rmsd ') and 'group' not in lines[2], (name, lines)
