"""The gapped TM alignment on the GPU (genie_tm_align, csrc/tmalign_kernels.hip; TMAlign in genie2_amd/similarity.py) against the
float64 oracle of tests/_tmalign.py, a certificate recomputed from the returned alignment and transform, the floor of the gapless score,
the known answers, the structure of the output, the entry's refusals, and both command lines end to end.

Bounds: the project's bar for a fused kernel, tm and rmsd within 1e-5 max(1, |value|), each widened per case to 4 x the error the
float32 restatement makes on the same input where that is larger; n_aligned, rounds and map exact.  A pair is left out of the parity
check only where the oracle alone calls it ill-posed -- the smallest relative gap between the two largest Horn eigenvalues over its
fits, stage 0's offset margin, the path margin of its tracebacks or the lead of its best stage is below 1e-4 -- and at most 15 % of a
case's pairs may be.  On the CPU the float64 oracle leaves out 4, 6 and 8 of 72 pairs at N = 4, 5 and 8 (nearly all by the eigenvalue
gap: chains of a few residues are close to collinear) and 5, 3, 6 and 10 of 72 at N = 24, 48, 65 and 129 (by the path margin and the
stage lead), with the families' first seeds.  The certificate, the map's structure and the gapless floor leave no pair out."""
import os

import numpy as np
import pytest
import torch

import _similarity as S
import _tmalign as T
from _motif import _ca_coordinates
from _parity import hard_time_limit

pytestmark = pytest.mark.gpu

BAR = 1e-5
_cache = {}


@pytest.fixture(autouse=True)
def _limit():
    with hard_time_limit(300):
        yield


@pytest.fixture(scope='module')
def entry():
    from genie2_amd.similarity import TMAlign
    return TMAlign('cuda:0')


@pytest.fixture(scope='module')
def gapless():
    from genie2_amd.similarity import PairwiseTM
    return PairwiseTM('cuda:0')


def _reference(key, xq, lq, xr, lr, **kw):
    """The oracle and the float32 restatement of an input, computed once and left unchanged."""
    if key not in _cache:
        _cache[key] = (T.all_pairs(xq, lq, xr, lr, **kw), T.all_pairs(xq, lq, xr, lr, dtype=torch.float32, **kw))
    return _cache[key]


def _gapless_floor(gapless, xq, lq, xr, lr, norm):
    """PairwiseTM's tm of every (query, reference) pair under the norm that matches `norm` for that pair: [M, R] float64."""
    M, R, N = len(lq), len(lr), max(xq.shape[1], xr.shape[1])
    x = torch.zeros(M + R, N, 3)
    x[:M, :xq.shape[1]], x[M:, :xr.shape[1]] = xq, xr
    both = {n: gapless(x, list(lq) + list(lr), norm=n)['tm'][:M, M:].double().cpu() for n in ('shorter', 'longer')}
    q, r = torch.tensor(lq)[:, None].expand(M, R), torch.tensor(lr)[None, :].expand(M, R)
    lnorm = {'query': q, 'reference': r, 'shorter': torch.minimum(q, r), 'longer': torch.maximum(q, r)}[norm]
    return torch.where(lnorm == torch.minimum(q, r), both['shorter'], both['longer'])


def _check(what, entry, gapless, xq, lq, xr, lr, ref, r32, norm='query', **kw):
    """The entry against the oracle over the pairs the oracle calls well-posed, then the checks that leave no pair out."""
    out = entry(xq, lq, xr, lr, norm=norm, return_alignment=True, **kw)
    M, R, Nq = len(lq), len(lr), xq.shape[1]
    assert all(tuple(out[k].shape) == (M, R) and out[k].device.type == 'cuda' for k in ('tm', 'rmsd', 'n_aligned', 'rounds'))
    assert out['tm'].dtype == torch.float32 and out['rmsd'].dtype == torch.float32
    assert out['n_aligned'].dtype == torch.int32 and out['rounds'].dtype == torch.int32 and out['map'].dtype == torch.int32
    assert tuple(out['map'].shape) == (M, R, Nq) and tuple(out['rot'].shape) == (M, R, 3, 3) and tuple(out['trans'].shape) == (M, R, 3)
    well = T.well_posed(ref)
    left_out = int((~well).sum())
    print('%s: %d of %d pairs left out' % (what, left_out, M * R))
    assert left_out <= 0.15 * M * R, '%s: %d of %d pairs are ill-posed: take another seed' % (what, left_out, M * R)
    widen = {}
    for k in ('tm', 'rmsd'):
        v, r = out[k].double().cpu(), ref[k]
        assert bool(torch.isfinite(v).all()), (what, k)
        bound = BAR * r.abs().clamp(min=1.0)
        widen[k] = max(1.0, 4.0 * float(((r32[k].double() - r).abs() / bound)[well].max()))
        ratio = ((v - r).abs() / (bound * widen[k]))[well]
        print('%s: %s error / bound %.3f (bar x%.2f)' % (what, k, float(ratio.max()), widen[k]))
        assert float(ratio.max()) <= 1.0, (what, k, float(ratio.max()))
    for k in ('n_aligned', 'rounds'):
        differ = int((out[k].cpu().long() != ref[k])[well].sum())
        print('%s: %d %s differ' % (what, differ, k))
        assert differ == 0, (what, k)
    amap = out['map'].cpu().long()
    assert bool((amap == ref['map'])[well].all()), (what, 'map')
    # the certificate: what the entry returned, recomputed in float64 from its own alignment and transform
    tm64, rmsd64, n = T.rescore(xq, lq, xr, lr, amap, out['rot'].cpu(), out['trans'].cpu(), norm)
    for k, again in (('tm', tm64), ('rmsd', rmsd64)):
        v = out[k].double().cpu()
        ratio = (v - again).abs() / (BAR * again.abs().clamp(min=1.0))             # (the plain bar: no restatement is involved)
        print('%s: certificate %s error / bound %.3f' % (what, k, float(ratio.max())))
        assert float(ratio.max()) <= 1.0, (what, 'certificate', k, float(ratio.max()))
    assert bool((n == out['n_aligned'].cpu().long()).all())
    for m in range(M):
        for r in range(R):
            row = amap[m, r]
            hit = row[row >= 0]
            assert bool((row[lq[m]:] == -1).all()) and bool((hit < lr[r]).all()) and bool((hit[1:] > hit[:-1]).all()), (what, m, r)
    det = torch.linalg.det(out['rot'].double().cpu())
    assert float((det - 1).abs().max()) < 1e-5
    # never below the gapless score
    floor = _gapless_floor(gapless, xq, lq, xr, lr, norm)
    short = float((floor - out['tm'].double().cpu()).max())
    print('%s: gapless tm - gapped tm at most %.2e' % (what, short))
    assert short <= BAR, (what, short)
    return out


# ---- parity with the oracle ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', T.INDEL_N)
def test_indel_families_match_the_float64_oracle(entry, gapless, N):
    xq, lq, xr, lr = T.family(N)
    assert min(lr[:6]) < N < max(lr[:6]) and N in lr[:6]                          # Lq > Lr, Lq = Lr and Lq < Lr all occur
    ref, r32 = _reference(('family', N, 'query'), xq, lq, xr, lr)
    _check('indel-N%d' % N, entry, gapless, xq, lq, xr, lr, ref, r32)
    d = torch.arange(6)
    assert float((ref['tm'][d, d] - ref['stage0'][d, d]).max()) > 0.2             # the gaps are worth finding
    assert int(ref['rounds'].max()) > 2


@pytest.mark.parametrize('N', T.TINY_N)
def test_tiny_families_match_the_float64_oracle(entry, gapless, N):
    xq, lq, xr, lr = T.family(N)
    ref, r32 = _reference(('family', N, 'query'), xq, lq, xr, lr)
    _check('tiny-N%d' % N, entry, gapless, xq, lq, xr, lr, ref, r32)


@pytest.mark.parametrize('norm', T.NORMS)
def test_every_norm_matches_the_float64_oracle(entry, gapless, norm):
    xq, lq, xr, lr = T.family(48)
    ref, r32 = _reference(('family', 48, norm), xq, lq, xr, lr, norm=norm)
    _check('N48-%s' % norm, entry, gapless, xq, lq, xr, lr, ref, r32, norm=norm)


def test_no_rounds_is_the_gapless_score(entry, gapless):
    xq, lq, xr, lr = T.family(65)
    ref, r32 = _reference(('family', 65, 'shorter', 0), xq, lq, xr, lr, norm='shorter', n_rounds=0)
    out = _check('N65-n_rounds0', entry, gapless, xq, lq, xr, lr, ref, r32, norm='shorter', n_rounds=0)
    assert bool((out['rounds'] == 0).all())
    M, N = 6, max(xq.shape[1], xr.shape[1])
    x = torch.zeros(18, N, 3)
    x[:M, :xq.shape[1]], x[M:, :xr.shape[1]] = xq, xr
    plain = gapless(x, lq + lr, norm='shorter')
    d = (out['tm'] - plain['tm'][:M, M:]).abs().double().cpu() / BAR
    print('n_rounds 0 against PairwiseTM: tm difference / bar %.3f' % float(d.max()))
    assert float(d.max()) <= 1.0
    # map is the threading at PairwiseTM's offset
    sure = T.well_posed(ref)
    off = plain['offset'][:M, M:].cpu().long()
    for m in range(M):
        for r in range(12):
            if not bool(sure[m, r]):
                continue
            La = min(lq[m], lr[r])
            want = torch.full((xq.shape[1],), -1, dtype=torch.long)
            if lq[m] <= lr[r]:
                want[:La] = off[m, r] + torch.arange(La)
            else:
                want[off[m, r]:off[m, r] + La] = torch.arange(La)
            assert out['map'][m, r].cpu().long().tolist() == want.tolist(), (m, r)
            assert int(out['n_aligned'][m, r]) == La


def test_the_largest_calls_match_the_float64_oracle(entry, gapless):
    for what, (q, r) in zip(('362x362', '128x1024'), T.limit_pairs()):
        xq, lq = T.pad([q])
        xr, lr = T.pad([r])
        assert lq[0] * lr[0] <= T.MAX_CELLS < (lq[0] + 1) * (lr[0] + 1)
        ref, r32 = _reference(what, xq, lq, xr, lr)
        out = _check(what, entry, gapless, xq, lq, xr, lr, ref, r32)
        assert float(out['tm'][0, 0]) > 0.8
        if lq[0] != lr[0]:                                                        # the long chain as the query: the reference moves
            swapped = _reference(what + '-swapped', xr, lr, xq, lq)
            _check(what + '-swapped', entry, gapless, xr, lr, xq, lq, *swapped)
    assert ref['map'][0, 0, 0] == 500 and int(ref['n_aligned'][0, 0]) == 128     # the excerpt is found where it was cut


# ---- known answers -------------------------------------------------------------------------------------------------------------------

def _one(entry, a, b, **kw):
    out = entry(a[None], [len(a)], b[None], [len(b)], return_alignment=True, **kw)
    return float(out['tm'][0, 0]), int(out['n_aligned'][0, 0]), int(out['rounds'][0, 0]), out['map'][0, 0].cpu().tolist()


def test_known_answers_on_the_device(entry, gapless):
    a = T.walk(1, 70, 7000)[0]
    tm, n, rounds, amap = _one(entry, a, a)
    assert tm > 0.999999 and n == 70 and amap == list(range(70)) and rounds == 1   # a chain against itself
    a, b = S.threading_pair()
    tm, n, rounds, amap = _one(entry, a, b)
    assert tm >= 0.999 and amap == [7 + i for i in range(20)] and rounds == 1
    tm, n, rounds, amap = _one(entry, b, a, norm='reference')                      # the same pair from the long chain's side
    assert tm >= 0.999 and amap == [-1] * 7 + list(range(20)) + [-1] * 20
    a, b = T.insertion_pair()
    x = torch.zeros(2, 74, 3)
    x[0, :64], x[1] = a, b
    assert float(gapless(x, [64, 74])['tm'][0, 1]) < 0.6                           # threading finds one half only
    tm, n, rounds, amap = _one(entry, a, b)
    assert tm >= 0.999 and n == 64 and amap == list(range(32)) + [i + 10 for i in range(32, 64)]


# ---- structure of the output ---------------------------------------------------------------------------------------------------------

def test_determinism_padding_and_the_optional_outputs(entry):
    xq, lq, xr, lr = T.family(65)
    a, b = entry(xq, lq, xr, lr, return_alignment=True), entry(xq, lq, xr, lr, return_alignment=True)
    for k in a:
        assert bool((a[k] == b[k]).all()), k                                      # two calls: the same bits
    plain = entry(xq, lq, xr, lr)
    assert sorted(plain) == ['n_aligned', 'rmsd', 'rounds', 'tm']
    for k in plain:
        assert bool((plain[k] == a[k]).all()), k                                  # with and without the alignment: the same bits
    # what lies beyond a chain's length never reaches the result
    g = torch.Generator().manual_seed(1)
    jq, jr = torch.cat([xq, torch.zeros(6, 9, 3)], dim=1), xr.clone()
    for m, L in enumerate(lq):
        jq[m, L:] = 1e3 * torch.randn(jq.shape[1] - L, 3, generator=g)
    for r, L in enumerate(lr):
        jr[r, L:] = 1e3 * torch.randn(xr.shape[1] - L, 3, generator=g)
    jq[0, lq[0]] = float('nan')
    jr[0, lr[0]] = float('nan')
    jr[1, -1] = float('inf')
    c = entry(jq, lq, jr, lr, return_alignment=True)
    for k in a:
        if k == 'map':
            assert bool((c[k][:, :, :xq.shape[1]] == a[k]).all()) and bool((c[k][:, :, xq.shape[1]:] == -1).all())
        else:
            assert bool((a[k] == c[k]).all()), k
    one = entry(xq[:1], lq[:1], xr[:1], lr[:1], return_alignment=True)             # M = R = 1
    for k in a:
        assert bool((one[k][0, 0] == a[k][0, 0]).all()), k


def test_rigid_motion_of_a_reference(entry):
    xq, lq, xr, lr = T.family(48)
    ref, _ = _reference(('family', 48, 'query'), xq, lq, xr, lr)
    base = entry(xq, lq, xr, lr)
    y = xr.clone()
    y[2, :lr[2]] = S.moved(xr[2, :lr[2]], 77)
    moved = entry(xq, lq, y, lr)
    well = T.well_posed(ref)
    for k in ('tm', 'rmsd'):
        d = ((moved[k] - base[k]).abs().double().cpu() / (BAR * ref[k].abs().clamp(min=1.0)))[well]
        print('rigid motion of one reference: %s change / bar %.3f' % (k, float(d.max())))
        assert float(d.max()) <= 1.0, k
    assert bool((moved['n_aligned'] == base['n_aligned']).cpu()[well].all())


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_entry_refusals_leave_the_next_call_working(entry):
    from genie2_amd import capi
    from genie2_amd.smc import _ptr
    xq, lq, xr, lr = T.family(24)
    xq, xr = xq.cuda().contiguous(), xr.cuda().contiguous()
    lq, lr = torch.tensor(lq, dtype=torch.int32, device='cuda'), torch.tensor(lr, dtype=torch.int32, device='cuda')
    good = entry._launch(xq, lq, xr, lr, 0, 16, 8, -0.6, True)
    outs = [good[k] for k in ('tm', 'rmsd', 'n_aligned', 'rounds', 'map', 'rot', 'trans')]
    ok = dict(M=6, Nq=xq.shape[1], xq=xq, lq=lq, R=12, Nr=xr.shape[1], xr=xr, lr=lr, norm=0, n_iter=16, n_rounds=8, gap_open=-0.6,
              tm=outs[0], rmsd=outs[1], n_aligned=outs[2], rounds=outs[3], map=outs[4], rot=outs[5], trans=outs[6])
    order = ('M', 'Nq', 'xq', 'lq', 'R', 'Nr', 'xr', 'lr', 'norm', 'n_iter', 'n_rounds', 'gap_open', 'tm', 'rmsd', 'n_aligned', 'rounds', 'map',
             'rot', 'trans')
    cases = ((dict(M=0), 'M outside 1..65535'), (dict(M=65536), 'M outside 1..65535'), (dict(R=0), 'R outside 1..65535'),
             (dict(R=65536), 'R outside 1..65535'), (dict(Nq=3), 'Nq outside 4..1024'), (dict(Nq=1025), 'Nq outside 4..1024'),
             (dict(Nr=3), 'Nr outside 4..1024'), (dict(Nr=1025), 'Nr outside 4..1024'), (dict(Nq=363, Nr=362), r'Nq \* Nr above 131072 cells'),
             (dict(norm=4), 'norm outside 0..3'), (dict(norm=-1), 'norm outside 0..3'), (dict(n_iter=0), 'n_iter outside 1..32'),
             (dict(n_iter=33), 'n_iter outside 1..32'), (dict(n_rounds=-1), 'n_rounds outside 0..16'), (dict(n_rounds=17), 'n_rounds outside 0..16'),
             (dict(gap_open=0.1), 'gap_open is not a finite number in -10..0'), (dict(gap_open=-10.5), 'gap_open is not a finite number'),
             (dict(gap_open=float('nan')), 'gap_open is not a finite number'), (dict(gap_open=float('-inf')), 'gap_open is not a finite number'),
             (dict(xq=None), 'xq is NULL'), (dict(lq=None), 'lq is NULL'), (dict(xr=None), 'xr is NULL'), (dict(lr=None), 'lr is NULL'),
             (dict(tm=None), 'tm is NULL'), (dict(rmsd=None), 'rmsd is NULL'), (dict(n_aligned=None), 'n_aligned is NULL'),
             (dict(rounds=None), 'rounds is NULL'), (dict(rot=None), 'rot and trans are given together or not at all'),
             (dict(trans=None), 'rot and trans are given together or not at all'))
    for change, msg in cases:
        a = dict(ok, **change)
        args = [_ptr(a[k]) if k in ('xq', 'lq', 'xr', 'lr', 'tm', 'rmsd', 'n_aligned', 'rounds', 'map', 'rot', 'trans') else a[k] for k in order]
        with pytest.raises(capi.GenieError, match='genie_tm_align: ' + msg):
            entry._call('genie_tm_align', entry._stream(), *args)
    again = entry._launch(xq, lq, xr, lr, 0, 16, 8, -0.6, True)
    for k in good:
        assert bool((again[k] == good[k]).all()), k
    torch.cuda.synchronize()


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

def _write(folder, name, xyz):
    from genie2_amd import features as F
    f = F.create_empty_np_features([len(xyz)])
    f['atom_positions'] = xyz.double().numpy()
    F.save_np_features_to_pdb(f, os.path.join(folder, name + '.pdb'))


def _read(folder, name):
    return torch.tensor(_ca_coordinates(os.path.join(folder, name + '.pdb')), dtype=torch.float32)


def _read_report(path):
    header, rows = {}, []
    for line in open(path):
        if line.startswith('#'):
            _, k, v = line.split()
            header[k] = v
        else:
            rows.append(line.split())
    return header, rows


def test_novelty_cli_end_to_end(tmp_path):
    from genie2_amd import novelty as NV
    run, refs = tmp_path / 'run', tmp_path / 'known'
    os.makedirs(run / 'pdbs')
    os.makedirs(refs)
    xq, lq, xr, lr = T.family(65)
    designs = {'fresh': T.walk(1, 150, 35)[0], 'related': xq[0, :65]}
    known = {'k%d' % k: T.walk(1, 50 + 12 * k, 40 + k)[0] for k in range(4)}
    known['planted'] = xr[0, :lr[0]]                                              # query 0's indel relative
    known['zlong'] = T.walk(1, 900, 50)[0]                                        # 150 x 900 is above the cell limit
    for name, xyz in designs.items():
        _write(str(run / 'pdbs'), name, xyz)
    for name, xyz in known.items():
        _write(str(refs), name, xyz)
    names, ref_names = sorted(designs), sorted(known)
    # the oracle reads the files itself
    q = [_read(str(run / 'pdbs'), n) for n in names]
    r = [_read(str(refs), n) for n in ref_names]
    rows_ref = []
    for m, a in enumerate(q):
        scored = [(T.align(a, b), k) for k, b in enumerate(r) if len(a) * len(b) <= T.MAX_CELLS]
        best = max(scored, key=lambda s: (float(s[0]['tm']), -s[1]))
        top = sorted(float(s[0]['tm']) for s in scored)
        assert top[-1] - top[-2] > 1e-3 and abs(top[-1] - 0.5) > 1e-3              # neither the nearest nor the verdict is a near tie
        assert min(best[0][k] for k in ('gap', 'margin', 'path_margin', 'stage_lead')) >= T.ILL
        rows_ref.append((best, len(r) - len(scored)))
    assert [s for _, s in rows_ref] == [1, 0]

    p = NV.build_parser()
    summary = NV.main(p.parse_args(['--indir', str(run), '--refdir', str(refs), '--write_alignments']))
    header, rows = _read_report(str(run / 'novelty' / 'novelty.txt'))
    assert list(header) == ['designs', 'references', 'norm', 'n_iter', 'n_rounds', 'gap_open', 'threshold', 'novel', 'novelty', 'skipped_pairs']
    assert (header['designs'], header['references'], header['norm'], header['n_iter'], header['n_rounds'], header['gap_open'], header['threshold'],
            header['novel'], header['novelty'], header['skipped_pairs']) == ('2', '6', 'query', '16', '8', '-0.6', '0.500', '1', '0.500', '1')
    assert summary['n_novel'] == 1 and summary['skipped_pairs'] == 1
    for m, row in enumerate(rows):
        (best, k), _ = rows_ref[m]
        assert row[0] == names[m] and int(row[1]) == len(q[m]) and row[2] == ref_names[k] and int(row[3]) == len(r[k]), row
        assert abs(float(row[4]) - float(best['tm'])) <= 1.1e-3 and int(row[5]) == best['n_aligned'], row
        assert abs(float(row[6]) - float(best['rmsd'])) <= 1.1e-3 and int(row[7]) == int(float(best['tm']) < 0.5), row
    assert rows[1][2] == 'planted' and rows[1][7] == '0' and rows[0][7] == '1'
    # the alignment files round-trip: the pairs are the oracle's, the distances follow from the written transform
    for m, name in enumerate(names):
        (best, k), _ = rows_ref[m]
        lines = open(str(run / 'novelty' / 'alignments' / (name + '.txt'))).read().splitlines()
        head = {ln.split()[1]: ln.split()[2:] for ln in lines if ln.startswith('#')}
        assert head['design'] == [name] and head['reference'] == [ref_names[k]] and int(head['n_aligned'][0]) == best['n_aligned']
        rot = torch.tensor([float(v) for v in head['rot']], dtype=torch.float64).reshape(3, 3)
        trans = torch.tensor([float(v) for v in head['trans']], dtype=torch.float64)
        pairs = [ln.split() for ln in lines if not ln.startswith('#')]
        assert [(int(i), int(j)) for i, j, _ in pairs] == [(i, j) for i, j in enumerate(best['map']) if j >= 0]
        for i, j, d in pairs:
            want = float((rot @ q[m][int(i)].double() + trans - r[k][int(j)].double()).norm())
            assert abs(float(d) - want) <= 2e-3, (name, i, j, d, want)
    # scalars out of range and empty folders end the run with a message
    os.makedirs(tmp_path / 'empty')
    with pytest.raises(SystemExit, match='no .pdb files in'):
        NV.main(p.parse_args(['--indir', str(run), '--refdir', str(tmp_path / 'empty')]))


def test_cluster_designs_gapped_merges_an_indel_variant(tmp_path):
    from genie2_amd import cluster_designs as CD
    run = tmp_path / 'run'
    os.makedirs(run / 'pdbs')
    xq, lq, xr, lr = T.family(65)
    for name, xyz in (('a_design', xq[0, :65]), ('b_variant', xr[0, :lr[0]]), ('c_other', T.walk(1, 65, 99)[0])):
        _write(str(run / 'pdbs'), name, xyz)
    names = ['a_design', 'b_variant', 'c_other']
    chains = [_read(str(run / 'pdbs'), n) for n in names]
    x, lengths = T.pad(chains)
    plain = S.all_pairs(x, lengths)['tm']
    one = [[T.align(chains[i], chains[j], norm='shorter') if i != j else None for j in range(3)] for i in range(3)]
    gapped = torch.tensor([[1.0 if i == j else max(float(one[i][j]['tm']), float(one[j][i]['tm'])) for j in range(3)] for i in range(3)],
                          dtype=torch.float64)
    assert all(min(o[k] for k in ('gap', 'margin', 'path_margin', 'stage_lead')) >= T.ILL for o in (one[0][1], one[1][0]))
    off = ~torch.eye(3, dtype=torch.bool)
    assert float((plain[off] - 0.6).abs().min()) > 1e-3 and float((gapped[off] - 0.6).abs().min()) > 1e-3
    assert float(plain[0, 1]) < 0.6 < float(gapped[0, 1])
    p = CD.build_parser()
    CD.main(p.parse_args(['--indir', str(run), '--outdir', str(tmp_path / 'gapless')]))
    header, rows = _read_report(str(tmp_path / 'gapless' / 'clusters.txt'))
    assert list(header) == list(CD.HEADER) and [int(r[2]) for r in rows] == [0, 1, 2]
    CD.main(p.parse_args(['--indir', str(run), '--outdir', str(tmp_path / 'gapped'), '--align', 'gapped', '--write_matrix']))
    header, rows = _read_report(str(tmp_path / 'gapped' / 'clusters.txt'))
    assert list(header) == list(CD.HEADER) + ['align', 'n_rounds', 'gap_open']
    assert (header['align'], header['n_rounds'], header['gap_open'], header['clusters']) == ('gapped', '8', '-0.6', '2')
    assert [int(r[2]) for r in rows] == [0, 0, 1]
    z = np.load(str(tmp_path / 'gapped' / 'tm.npz'))
    assert bool((z['tm'] == z['tm'].T).all()) and bool((np.diag(z['tm']) == 1).all()) and 'n_aligned' in z and 'offset' not in z
    assert abs(float(z['tm'][0, 1]) - float(gapped[0, 1])) <= BAR                   # the well-posed pair: the ordinary bar
    assert float(np.abs(z['tm'] - gapped.numpy()).max()) < 1e-3                    # the others: inside what the verdicts have to spare
