"""The envelope potential without a device: the float64 oracle of tests/_envelope.py against the header's gradient formula written
with loops and against central differences, its behaviour far from the envelope and under rigid motion; load_envelope's,
envelope_shape_points' and EnvelopePotential's host side; both command lines' parsers and constants, the report and the PDB writer;
the C entry's symbols, work sizes and refusals (genie_envelope_potential, include/genie_hip.h).

What holds the kernel to the oracle is tests/test_envelope_gpu.py."""
import ctypes as C
import math
import os

import pytest
import torch

import _envelope as En
from conftest import GOLDEN

MOTIF = os.path.join(GOLDEN, 'motif_problem_6E6R.pdb')
BASE = ['--name', 'base', '--epoch', '40', '--scale', '0.6', '--outdir', 'o']


@pytest.fixture(scope='module')
def lib():
    from genie2_amd import build, capi
    build.build()
    return capi.load_library()


def _small(B, N, seed, M, weighted=False, **kw):
    """A small input with both terms acting: a centred walk and the first M lattice points of a sphere, 2 A apart."""
    return En.centred_walk(B, N, seed).double(), En.case_config((B, N, seed, 'sphere:6', 2.0, M, weighted), **kw)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,M,weighted', [(1, 1, False), (2, 3, False), (5, 9, True), (12, 40, False), (9, 123, True)])
def test_autograd_equals_the_loop_gradient_and_central_differences(N, M, weighted):
    """The header's formula, written out with loops, against autograd of the oracle: 1e-10 of the largest entry; and central
    differences of the oracle's logp with a step of 1e-5 A: 1e-6 of the largest entry (the truncation error of a C^1 function whose
    second derivative is of the gradient's order per Angstrom, 1e-10, and the rounding error 1e-16 |logp| / 1e-5, are both below)."""
    x, cfg = _small(2, N, 10 * N + M, M, weighted, inside=1.0, cover=1.5)
    x = x + 4.0                                                           # (off the lattice and partly outside: every case has both energies)
    ref = En.reference(x, cfg, 0.7)
    scale = float(ref['grad'].abs().max())
    assert scale > 0 and bool((ref['e_envelope_inside'] > 0).all()) and bool((ref['e_envelope_cover'] > 0).all())
    assert float((ref['grad'] - En.loop_gradient(x, cfg, 0.7)).abs().max()) <= 1e-10 * scale
    step, worst = 1e-5, 0.0
    for b in range(2):
        for n in range(N):
            for d in range(3):
                hi, lo = x.clone(), x.clone()
                hi[b, n, d] += step
                lo[b, n, d] -= step
                fd = float(En.logp(hi, cfg, 0.7)[b] - En.logp(lo, cfg, 0.7)[b]) / (2 * step)
                worst = max(worst, abs(fd - float(ref['grad'][b, n, d])))
    assert worst <= 1e-6 * scale, (worst, scale)


def test_each_term_alone_and_the_c1_join_at_the_clamp():
    x, cfg = _small(2, 12, 3, 40, inside=1.0, cover=1.5)
    both = En.reference(x, cfg, 1.0)
    inside, cover = En.reference(x, dict(cfg, cover_weight=0.0), 1.0), En.reference(x, dict(cfg, inside_weight=0.0), 1.0)
    assert torch.equal(inside['e_envelope_inside'], both['e_envelope_inside']) and bool((inside['e_envelope_cover'] == 0).all())
    assert torch.equal(cover['e_envelope_cover'], both['e_envelope_cover']) and bool((cover['e_envelope_inside'] == 0).all())
    assert float((inside['grad'] + cover['grad'] - both['grad']).abs().max()) <= 1e-12 * float(both['grad'].abs().max())
    # a particle lying on the envelope points: every s_n <= 0, a_n = eps, the inside term and its gradient are exactly 0
    on = cfg['points'][None, :12].clone()
    ref = En.reference(on, dict(cfg, cover_weight=0.0), 1.0)
    assert bool((ref['distance'] == En.EPS).all()) and float(ref['e_envelope_inside'][0]) == 0 and float(ref['grad'].abs().max()) == 0


def test_oracle_far_from_the_envelope_and_under_rigid_motion():
    """300 A away every exp(-q / tau) underflows (q / tau > 2e4): logsumexp subtracts the minimum, so the oracle stays finite and a_n
    is the distance to the nearest point to 1e-3 A.  Moving design and envelope together changes nothing."""
    x, cfg = _small(2, 12, 5, 40)
    far = x + torch.tensor([300.0, 0.0, 0.0], dtype=torch.float64)
    ref = En.reference(far, cfg, 1.0)
    assert all(bool(torch.isfinite(ref[k]).all()) for k in ('logp', 'grad', 'distance', 'gap'))
    nearest = torch.cdist(far, cfg['points'][None].expand(2, -1, -1)).min(dim=2).values
    assert float((ref['distance'] - nearest).abs().max()) <= 1e-3 + 1e-2 and float(ref['n_outside'].min()) == 12
    q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1)))
    shift = torch.tensor([3.0, -20.0, 7.5], dtype=torch.float64)
    moved = dict(cfg, points=cfg['points'] @ q.T + shift)
    a, b = En.reference(x, cfg, 1.0), En.reference(x @ q.T + shift, moved, 1.0)
    assert float((a['logp'] - b['logp']).abs().max()) <= 1e-9 * float(a['logp'].abs().max())
    assert float((a['grad'] @ q.T - b['grad']).abs().max()) <= 1e-9 * float(a['grad'].abs().max())


def test_parity_inputs_keep_their_margins():
    """Every parity case of test_envelope_gpu.py from the oracle alone (the longest left to the GPU file, which builds it anyway); the
    first five have the point counts they were specified with."""
    assert [c[5] for c in En.CASES[:5]] == [257, 253, 773, 1375, 4169]
    assert {c[5] for c in En.CASES} >= {1, 3, 64, En.CHUNK - 1, En.CHUNK, En.CHUNK + 1} and {c[1] for c in En.CASES} >= {1, 2, 63, En.CHUNK - 1, En.CHUNK, En.CHUNK + 1}
    from genie2_amd.smc import envelope_shape_points
    groups = [c[0] * (-(-c[1] // 64) - (-c[5] // 64)) for c in En.CASES]             # work-groups of the soft minima's launch
    assert {En.FILL - 2, En.FILL} <= set(groups) and {En.FILL - 1, En.FILL} <= {c[0] for c in En.CASES if c[1] <= 64}
    assert En.CASES[-1][0] * (2 + 17) >= En.FILL and En.CASES[-1][5] > En.CHUNK
    for case in En.CASES[:4] + En.CASES[5:]:
        x, cfg = En.inputs(case)
        assert tuple(x.shape) == (case[0], case[1], 3) and x.dtype == torch.float32 and len(cfg['points']) == case[5]
        assert float(x.mean(dim=1).abs().max()) <= 1e-4 and En.margins(x, cfg) >= 1e-4
    for case in En.CASES[:5]:
        assert len(envelope_shape_points(case[3], case[4])) == case[5]


# ---- the host side of smc.py ---------------------------------------------------------------------------------------------------------

def test_shape_points_counts_order_and_errors():
    from genie2_amd import capi
    from genie2_amd.smc import ENVELOPE_MAX_POINTS, envelope_shape_points
    assert ENVELOPE_MAX_POINTS == capi.ENVELOPE_MAX_POINTS == 16384
    # closed-form lattice counts: the integer points with i^2 + j^2 + k^2 <= (R / h)^2, and (2 floor(A / 2h) + 1) ... of a box
    for R, h in ((12.0, 3.0), (10.0, 2.5), (7.0, 2.0), (40.0, 4.0)):
        r2 = (R / h) ** 2
        k = int(math.floor(R / h))
        want = sum(1 for i in range(-k, k + 1) for j in range(-k, k + 1) for l in range(-k, k + 1) if i * i + j * j + l * l <= r2)
        pts = envelope_shape_points('sphere:%g' % R, h)
        assert len(pts) == want and pts.dtype == torch.float64 and tuple(pts.shape) == (want, 3)
        assert torch.equal(pts, envelope_shape_points('ellipsoid:%g,%g,%g' % (R, R, R), h))
    for (A, B_, C_), h in (((6.0, 6.0, 3.0), 3.0), ((10.0, 4.0, 7.0), 1.0), ((5.0, 5.0, 5.0), 2.0)):
        want = 1
        for edge in (A, B_, C_):
            want *= 2 * int(math.floor(edge / 2 / h)) + 1
        assert len(envelope_shape_points('box:%g,%g,%g' % (A, B_, C_), h)) == want
    # the order: ascending (i, j, k), k fastest; the origin is a lattice point; the solid is symmetric, so its centroid is the origin
    pts = envelope_shape_points('box:6,6,3', 3.0)
    assert pts.tolist() == [[x, y, 0.0] for x in (-3.0, 0.0, 3.0) for y in (-3.0, 0.0, 3.0)]
    pts = envelope_shape_points('ellipsoid:12,6,6', 3.0)
    keys = [tuple(p) for p in (pts / 3.0).round().long().tolist()]
    assert keys == sorted(keys) and (0, 0, 0) in keys and len(set(keys)) == len(keys) == 61
    assert float(pts.sum(dim=0).abs().max()) == 0
    cyl = envelope_shape_points('cylinder:5,10', 2.5)
    assert float(cyl[:, 2].abs().max()) == 5.0 and float((cyl[:, :2] ** 2).sum(dim=1).max()) <= 25.0 and len(cyl) == 13 * 5
    tor = envelope_shape_points('torus:10,3', 1.0)
    rho = torch.sqrt(tor[:, 0] ** 2 + tor[:, 1] ** 2)
    assert bool((((rho - 10.0) ** 2 + tor[:, 2] ** 2) <= 9.0 + 1e-12).all()) and float(rho.min()) >= 7.0 and not any(k == [0.0, 0.0, 0.0] for k in tor.tolist())
    assert torch.equal(tor, envelope_shape_points(' Torus:10,3', 1))                     # deterministic; the name in any case
    for spec, msg in (('ball:3', 'an envelope shape is one of sphere:R, ellipsoid:A,B,C, cylinder:R,L, torus:R,r, box:A,B,C'),
                      ('sphere', 'sphere takes 1 finite sizes above 0, sphere:R'), ('sphere:1,2', 'sphere takes 1'), ('box:1,2', 'box takes 3'),
                      ('sphere:x', 'sphere takes 1'), ('sphere:-3', 'sphere takes 1'), ('ellipsoid:3,0,3', 'ellipsoid takes 3'),
                      ('cylinder:inf,3', 'cylinder takes 2'), ('torus:3', 'torus takes 2')):
        with pytest.raises(ValueError, match=msg):
            envelope_shape_points(spec, 3.0)
    for spacing in (0.0, -1.0, math.inf, math.nan, 'x', None):
        with pytest.raises(ValueError, match='spacing must be finite and > 0'):
            envelope_shape_points('sphere:10', spacing)
    with pytest.raises(ValueError, match='holds no lattice point: use a smaller spacing'):
        envelope_shape_points('torus:10.5,0.01', 1.0)
    with pytest.raises(ValueError, match='more than 16384'):
        envelope_shape_points('sphere:40', 2.0)
    with pytest.raises(ValueError, match='more than 16384 points: use a larger spacing'):
        envelope_shape_points('sphere:4000', 1.0)                                        # refused from the bounding box, nothing allocated


def test_load_envelope(tmp_path):
    from genie2_amd.smc import load_envelope
    path = tmp_path / 'env.txt'
    path.write_text('# a map\n1 2 3\n-4.5 0 1e1 2.5\n\n0 0 0 0.5  # centre\n')
    pts, w = load_envelope(str(path))
    assert pts.tolist() == [[1.0, 2.0, 3.0], [-4.5, 0.0, 10.0], [0.0, 0.0, 0.0]] and w.tolist() == [1.0, 2.5, 0.5]
    assert pts.dtype == w.dtype == torch.float64
    for text, msg in (('1 2\n', r'env.txt:1: expected `x y z \[weight\]`, got 2 fields'), ('# x\n1 2 3 4 5\n', r'env.txt:2: expected'),
                      ('1 2 3\n1 two 3\n', r'env.txt:2: x, y, z and weight are numbers'), ('# nothing\n\n', r'env.txt: no envelope point')):
        path.write_text(text)
        with pytest.raises(ValueError, match=msg):
            load_envelope(str(path))
    with pytest.raises(OSError):
        load_envelope(str(tmp_path / 'none.txt'))
    # a .pdb: every ATOM and HETATM record, whatever the atom
    pts, w = load_envelope(MOTIF)
    records = [ln for ln in open(MOTIF) if ln.startswith(('ATOM', 'HETATM'))]
    assert len(pts) == len(records) > 0 and bool((w == 1).all())
    assert pts[0].tolist() == [float(records[0][30:38]), float(records[0][38:46]), float(records[0][46:54])]
    pdb = tmp_path / 'map.PDB'
    pdb.write_text('REMARK x\nHETATM    1  C   ENV E   1       1.000  -2.500  30.125  1.00  0.00           C\nATOM      2  CA  ALA A   2     -11.000   0.000   0.001\nEND\n')
    assert load_envelope(str(pdb))[0].tolist() == [[1.0, -2.5, 30.125], [-11.0, 0.0, 0.001]]
    pdb.write_text('ATOM      2  CA  ALA A   2     -11.000   x.000   0.001\n')
    with pytest.raises(ValueError, match=r'map.PDB:1: no coordinates in columns 31-54'):
        load_envelope(str(pdb))
    pdb.write_text('REMARK nothing\n')
    with pytest.raises(ValueError, match='no ATOM or HETATM record'):
        load_envelope(str(pdb))


def test_constructor_validates_on_the_host():
    from genie2_amd import capi
    from genie2_amd.smc import EnvelopePotential
    import genie.sampler.envelope as mirror
    assert mirror.EnvelopePotential is EnvelopePotential and mirror.load_envelope and mirror.envelope_shape_points
    abar = torch.linspace(0.999, 0.001, 13)
    inf, nan = math.inf, math.nan
    pts = [[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]]
    for n_res in (0, -1, 4097, 40.0, True):
        with pytest.raises(ValueError, match=r'n_res must be an integer in 1\.\.4096'):
            EnvelopePotential(n_res, abar, pts, device='cpu')
    for points, msg in (([[0.0, 0.0]], r'points must be \[M, 3\]'), ([], r'points must be \[M, 3\]'), (torch.zeros(16385, 3), r'M in 1\.\.16384'),
                        ('abc', r'points must be \[M, 3\] coordinates'), ([[0.0, nan, 0.0]], 'not finite'), ([[inf, 0.0, 0.0]], 'not finite')):
        with pytest.raises(ValueError, match=msg):
            EnvelopePotential(40, abar, points, device='cpu')
    for weights, msg in (([1.0], r'weights must be \[2\]'), ([1.0, 0.0], 'finite and > 0'), ([1.0, -1.0], 'finite and > 0'), ([1.0, inf], 'finite and > 0'),
                         ([nan, 1.0], 'finite and > 0'), ('ab', r'weights must be \[M\] numbers')):
        with pytest.raises(ValueError, match=msg):
            EnvelopePotential(40, abar, pts, weights=weights, device='cpu')
    for name in ('inside_distance', 'cover_distance'):
        for v in (0.0, 0.1, 0.05, -1.0, inf, nan, 'x'):
            with pytest.raises(ValueError, match='%s must be finite and above eps' % name):
                EnvelopePotential(40, abar, pts, device='cpu', **{name: v})
    for name in ('inside_weight', 'cover_weight'):
        for v in (-1.0, inf, nan, 'x'):
            with pytest.raises(ValueError, match='%s must be finite and >= 0' % name):
                EnvelopePotential(40, abar, pts, device='cpu', **{name: v})
    for name in ('softness', 'tausq'):
        for v in (0.0, -1.0, inf, nan, 'x'):
            with pytest.raises(ValueError, match='%s must be finite and > 0' % name):
                EnvelopePotential(40, abar, pts, device='cpu', **{name: v})
    with pytest.raises(ValueError, match='no term enabled'):
        EnvelopePotential(40, abar, pts, inside_weight=0.0, cover_weight=0, device='cpu')
    # what is allowed gets as far as the device: a CPU potential is a GenieError
    for kw in ({}, dict(weights=[0.5, 1.5]), dict(inside_weight=0.0), dict(cover_weight=0.0, center=False), dict(inside_distance=0.2, softness=0.5, tausq=0.012)):
        with pytest.raises(capi.GenieError, match='EnvelopePotential runs on the GPU'):
            EnvelopePotential(40, abar, pts, device='cpu', **kw)
    doc = EnvelopePotential.__doc__
    assert 'design choices' in doc and 'unmeasured' in doc and 'Not built' in doc
    for words in ('rotating or fitting', 'regions of it to residues', "motif's placement", 'density-map file formats'):
        assert words in doc, words
    others = (capi.SHAPE_REPORT, capi.SECSTRUCT_REPORT, capi.SHEET_REPORT, capi.SYMMETRY_REPORT, capi.BINDER_REPORT, capi.FOLD_REPORT,
              capi.DIVERSITY_REPORT, capi.BURIAL_REPORT)
    assert capi.ENVELOPE_REPORT == En.REPORT and capi.ENVELOPE_COUNTS == En.COUNTS == ('n_outside', 'n_uncovered')
    assert capi.ENVELOPE_CHUNK == En.CHUNK and capi.ENVELOPE_EPS == En.EPS and capi.ENVELOPE_FILL == En.FILL
    assert not any(set(capi.ENVELOPE_REPORT) & set(o) for o in others)                 # SumPotential merges the reports


# ---- the command lines ---------------------------------------------------------------------------------------------------------------

FLAGS = ('--envelope_file', '--envelope_shape', '--envelope_spacing', '--envelope_keep_frame', '--envelope_inside_distance',
         '--envelope_inside_weight', '--envelope_cover_distance', '--envelope_cover_weight', '--envelope_softness', '--envelope_tausq',
         '--write_envelope')


def test_parsers_constants_and_the_messages(tmp_path):
    from genie2_amd import sample_unconditional_motif as M
    from genie2_amd import sample_unconditional_shape as Sh
    import genie.sample_unconditional_shape as mirror
    assert mirror.add_envelope_arguments is Sh.add_envelope_arguments and mirror.envelope_potential is Sh.envelope_potential
    assert mirror.envelope_constants is Sh.envelope_constants
    defaults = dict(envelope_file=None, envelope_shape=None, envelope_spacing=3.0, envelope_keep_frame=False, envelope_inside_distance=3.0,
                    envelope_inside_weight=1.0, envelope_cover_distance=5.0, envelope_cover_weight=1.0, envelope_softness=4.0,
                    envelope_tausq=1.0, write_envelope=False)
    assert Sh.ENVELOPE_DEFAULTS == defaults
    from genie2_amd import capi
    assert (Sh.ENVELOPE_EPS, Sh.ENVELOPE_MAX_POINTS) == (capi.ENVELOPE_EPS, capi.ENVELOPE_MAX_POINTS)
    given = ['--envelope_shape', 'ellipsoid:12,6,6', '--envelope_spacing', '2', '--envelope_keep_frame', '--envelope_inside_distance', '2.5',
             '--envelope_inside_weight', '0.5', '--envelope_cover_distance', '4', '--envelope_cover_weight', '2', '--envelope_softness', '3',
             '--envelope_tausq', '0.5', '--write_envelope']
    values = dict(envelope_file=None, envelope_shape='ellipsoid:12,6,6', envelope_spacing=2.0, envelope_keep_frame=True,
                  envelope_inside_distance=2.5, envelope_inside_weight=0.5, envelope_cover_distance=4.0, envelope_cover_weight=2.0,
                  envelope_softness=3.0, envelope_tausq=0.5, write_envelope=True)
    for parser, more in ((Sh.build_parser(), []), (M.build_parser(), ['--motif_file', MOTIF])):
        text = parser.format_help()
        assert all(flag + ' ' in text or flag + '\n' in text for flag in FLAGS)
        a = vars(parser.parse_args(BASE + more))
        assert {k: a[k] for k in defaults} == defaults
        assert a['rog_max'] is None and a['symmetry'] is None and a['bury'] is None      # (the flags that were there)
        a = vars(parser.parse_args(BASE + more + given))
        assert {k: a[k] for k in values} == values

    # constants: an envelope term is enough on its own for the shape CLI
    from genie2_amd.smc import envelope_shape_points
    c = Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + given)))
    assert {k: c[k] for k in values} == values and Sh.has_envelope_terms(c) and c['envelope']['weights'] is None
    assert torch.equal(torch.from_numpy(c['envelope']['points']), envelope_shape_points('ellipsoid:12,6,6', 2.0))
    assert not (Sh.has_shape_terms(c) or Sh.has_secstruct_terms(c) or Sh.has_sheet_terms(c) or Sh.has_symmetry_terms(c) or Sh.has_binder_terms(c)
                or Sh.has_fold_terms(c) or Sh.has_diversity_terms(c) or Sh.has_burial_terms(c))
    path = tmp_path / 'env.txt'
    path.write_text('0 0 0\n3 0 0 2\n')
    c = M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF, '--envelope_file', str(path)])))
    assert c['envelope']['points'].tolist() == [[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]] and c['envelope']['weights'].tolist() == [1.0, 2.0]
    assert c['tausq'] == 0.012 and Sh.has_envelope_terms(c) and c['envelope_keep_frame'] is False
    path.write_text('0 0 0\n3 0 0\n')
    assert Sh.envelope_constants(vars(Sh.build_parser().parse_args(BASE + ['--envelope_file', str(path)])))['envelope']['weights'] is None

    # no envelope flag: no term, and sum_potentials gets None for it
    for c in (M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF]))),
              Sh.GuidedRunner().create_constants(vars(Sh.build_parser().parse_args(BASE))),
              Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + ['--rog_max', '12'])))):
        assert {k: c[k] for k in defaults} == defaults and c['envelope'] is None and not Sh.has_envelope_terms(c)
        pot = Sh.envelope_potential(c, 60, None, 'cuda')                                            # no term: no potential, no device
        assert pot is None
        marker = object()
        assert Sh.sum_potentials(marker, pot) is marker and Sh.sum_potentials(pot) is None

    # every way the flags end a run, in both CLIs
    shape = ['--envelope_shape', 'sphere:10']
    for run in (lambda f: Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE + f))),
                lambda f: M.MotifRunner().create_constants(vars(M.build_parser().parse_args(BASE + ['--motif_file', MOTIF] + f)))):
        for flags in (['--envelope_spacing', '2'], ['--envelope_keep_frame'], ['--envelope_inside_distance', '2'], ['--envelope_inside_weight', '2'],
                      ['--envelope_cover_distance', '4'], ['--envelope_cover_weight', '2'], ['--envelope_softness', '2'], ['--envelope_tausq', '2'],
                      ['--write_envelope']):
            with pytest.raises(SystemExit, match='an envelope flag needs a term: --envelope_file or --envelope_shape'):
                run(flags)
        with pytest.raises(SystemExit, match='--envelope_file and --envelope_shape both name the envelope'):
            run(shape + ['--envelope_file', str(path)])
        for flags, msg in ((['--envelope_inside_distance', '0.1'], 'envelope_inside_distance must be finite and above 0.1'),
                           (['--envelope_cover_distance', 'inf'], 'envelope_cover_distance must be finite and above 0.1'),
                           (['--envelope_inside_weight', '-1'], 'envelope_inside_weight must be finite and >= 0'),
                           (['--envelope_cover_weight', 'nan'], 'envelope_cover_weight must be finite and >= 0'),
                           (['--envelope_spacing', '0'], 'envelope_spacing must be finite and > 0'), (['--envelope_softness', '0'], 'envelope_softness must be'),
                           (['--envelope_tausq', '-1'], 'envelope_tausq must be'),
                           (['--envelope_inside_weight', '0', '--envelope_cover_weight', '0'], 'both 0: nothing to guide')):
            with pytest.raises(SystemExit, match=msg):
                run(shape + flags)
        for flags, msg in ((['--envelope_shape', 'ball:3'], '--envelope_file / --envelope_shape: an envelope shape is one of'),
                           (['--envelope_shape', 'sphere:40', '--envelope_spacing', '1'], 'more than 16384'),
                           (['--envelope_file', str(tmp_path / 'none.txt')], '--envelope_file / --envelope_shape'), ):
            with pytest.raises(SystemExit, match=msg):
                run(flags)
    path.write_text('0 0 0\n3 0\n')
    with pytest.raises(SystemExit, match=r'env.txt:2: expected'):
        Sh.envelope_constants(vars(Sh.build_parser().parse_args(BASE + ['--envelope_file', str(path)])))
    path.write_text('0 0 0\n3 0 0 -1\n')
    with pytest.raises(SystemExit, match='every weight must be finite and > 0'):
        Sh.envelope_constants(vars(Sh.build_parser().parse_args(BASE + ['--envelope_file', str(path)])))

    # the message of a run with no term names the flags, keeps every name it had, and still ends as tests/test_symmetry_host.py reads it
    with pytest.raises(SystemExit, match='no shape term.*--symmetry$') as info:
        Sh.ShapeRunner().create_constants(vars(Sh.build_parser().parse_args(BASE)))
    for name in ('--envelope_file', '--envelope_shape', '--burial_file', '--bury', '--expose_max', '--burial_mean_max', '--diversity_tm_max',
                 '--template_pdb', '--target_pdb', '--rog_max', '--helix_min', '--ladder_file'):
        assert name in str(info.value), name
    for doc in (Sh.__doc__, M.__doc__):
        assert '--envelope_shape' in doc and '--envelope_file' in doc and '--write_envelope' in doc and 'outdir/envelope/' in doc
    assert 'Not built' in Sh.__doc__ and 'outdir/envelope/{length}_{index}.txt' in Sh.__doc__ and 'envelope.pdb' in Sh.__doc__


def test_report_and_pdb_writers(tmp_path):
    from genie2_amd import capi
    from genie2_amd import sample_unconditional_shape as Sh
    from genie2_amd.smc import load_envelope
    merged = {'rog': torch.tensor([12.3, 9.0]), 'n_outside': torch.tensor([2, 0]), 'max_outside': torch.tensor([3.0004, 0.0]),
              'n_uncovered': torch.tensor([1, 0]), 'max_uncovered': torch.tensor([0.25, 0.0]), 'e_envelope_inside': torch.tensor([1234.5678, 0.0]),
              'e_envelope_cover': torch.tensor([0.0625, 0.0])}
    assert list(Sh.report_fields(merged, capi.ENVELOPE_REPORT)) == list(capi.ENVELOPE_REPORT)
    distance = torch.tensor([[0.1, 7.61239, 6.0004], [0.1, 0.1, 2.0]])
    gap = torch.tensor([[5.25, 5.0, 0.1, 1.0], [0.1, 0.2, 0.3, 4.9999]])
    Sh.write_envelope_report(distance, gap, torch.tensor([1.0, 2.0, 0.5, 0.5]), 5.0, Sh.report_fields(merged, capi.ENVELOPE_REPORT),
                             str(tmp_path / 'envelope'), 3, 4)
    assert sorted(os.listdir(tmp_path / 'envelope')) == ['3_4.txt', '3_5.txt']
    assert (tmp_path / 'envelope' / '3_4.txt').read_text() == (
        'residue 0 0.100\nresidue 1 7.612\nresidue 2 6.000\ncovered_fraction 0.750\nn_outside 2\nmax_outside 3.000\nn_uncovered 1\n'
        'max_uncovered 0.250\ne_envelope_inside 1234.568\ne_envelope_cover 0.062\n')
    assert (tmp_path / 'envelope' / '3_5.txt').read_text().splitlines()[2:5] == ['residue 2 2.000', 'covered_fraction 1.000', 'n_outside 0']
    Sh.write_envelope_report(distance, gap, None, 5.0, Sh.report_fields(merged, capi.ENVELOPE_REPORT), str(tmp_path / 'plain'), 3, 0)
    assert (tmp_path / 'plain' / '3_0.txt').read_text().splitlines()[3] == 'covered_fraction 0.750'
    pts = torch.tensor([[1.0, -2.5, 30.125], [-110.0, 0.0, 0.0015], [0.0, 0.0, 0.0]])
    Sh.write_envelope_pdb(pts, torch.tensor([1.0, 0.5, 1.5]), str(tmp_path / 'e' / 'envelope.pdb'))
    lines = (tmp_path / 'e' / 'envelope.pdb').read_text().splitlines()
    assert len(lines) == 4 and lines[-1] == 'END' and all(ln.startswith('HETATM') and len(ln) == 78 for ln in lines[:3])
    assert lines[0] == 'HETATM    1  C   ENV E   1       1.000  -2.500  30.125  1.00  0.00           C'
    back, w = load_envelope(str(tmp_path / 'e' / 'envelope.pdb'))
    assert float((back - pts.double()).abs().max()) <= 5.1e-4 and bool((w == 1).all())


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------

def _work_bytes(B, N, M):
    return 4 * B * (N + 2 * M + 3 * ((N + 63) // 64 + (M + 63) // 64))


def test_symbols_are_declared_and_exported(lib):
    from genie2_amd import build, capi
    assert 'envelope_kernels.hip' in build.SOURCES and os.path.exists(os.path.join(os.path.dirname(build.__file__), 'csrc', 'envelope_kernels.hip'))
    res, args = capi.SYMBOLS['genie_envelope_potential']
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_float] * 5 + \
        [C.c_void_p] * 7 + [C.c_size_t]
    assert capi.SYMBOLS['genie_envelope_potential_work_bytes'] == (C.c_size_t, [C.c_int, C.c_int, C.c_int])
    assert lib.genie_envelope_potential and lib.genie_envelope_potential_work_bytes
    header = open(os.path.join(os.path.dirname(build.__file__), '..', 'include', 'genie_hip.h')).read()
    # the argument list of the header, one C type per ctypes entry
    start = header.index('int genie_envelope_potential(genie_stream_t stream')
    text = header[start:header.index(');', start)]
    import re
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    params = [p.strip() for p in text[text.index('(') + 1:].split(',')]
    kinds = {'genie_stream_t': C.c_void_p, 'int': C.c_int, 'float': C.c_float, 'size_t': C.c_size_t}
    want = [C.c_void_p if '*' in p else kinds[p.split()[0]] for p in params]
    assert want == args and [p.split()[-1].lstrip('*') for p in params] == [
        'stream', 'B', 'N', 'x0', 'M', 'points', 'weights', 'softness', 'inside_distance', 'inside_weight', 'cover_distance', 'cover_weight', 'var',
        'logp_out', 'grad_out', 'report_out', 'distance_out', 'gap_out', 'work', 'work_bytes']
    assert 'size_t genie_envelope_potential_work_bytes(int B, int N, int M);' in header
    assert '#define GENIE_ENVELOPE_REPORT %d ' % len(capi.ENVELOPE_REPORT) in header and '#define GENIE_ENVELOPE_EPS 0.1f' in header
    assert '#define GENIE_ENVELOPE_CHUNK %d' % capi.ENVELOPE_CHUNK in header and '#define GENIE_ENVELOPE_FILL %d ' % capi.ENVELOPE_FILL in header
    assert '#define GENIE_ENVELOPE_MAX_LENGTH %d' % capi.ENVELOPE_MAX_LENGTH in header
    assert '#define GENIE_ENVELOPE_MAX_POINTS %d' % capi.ENVELOPE_MAX_POINTS in header
    for B, N, M in ((8, 256, 2048), (1, 1, 1), (3, 65, 253), (1, 4096, 16384), (65535, 1, 1)):
        assert lib.genie_envelope_potential_work_bytes(B, N, M) == _work_bytes(B, N, M)
    for B, N, M in ((0, 10, 10), (65536, 10, 10), (1, 0, 10), (1, 4097, 10), (1, 10, 0), (1, 10, 16385), (-1, -1, -1)):
        assert lib.genie_envelope_potential_work_bytes(B, N, M) == 0


def test_entry_refuses_bad_arguments_before_the_device(lib):
    """Every refusal names the entry and the argument and comes back before the device is touched: the pointers are made up."""
    inf, nan = math.inf, math.nan
    P = C.c_void_p
    x, var, out, work, pts = P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x5000)
    null = P(0)

    def call(B=2, N=10, x0=x, M=7, points=pts, weights=null, softness=4.0, inside=3.0, iw=1.0, cover=5.0, cw=1.0, v=var, logp=out, grad=out,
             report=null, distance=null, gap=null, wk=work, wbytes=10 ** 6):
        return lib.genie_envelope_potential(null, B, N, x0, M, points, weights, softness, inside, iw, cover, cw, v, logp, grad, report, distance,
                                            gap, wk, wbytes)

    cases = [(dict(B=0), 'B outside'), (dict(B=65536), 'B outside'), (dict(N=0), 'N outside'), (dict(N=4097), 'N outside 1..GENIE_ENVELOPE_MAX_LENGTH'),
             (dict(M=0), 'M outside'), (dict(M=16385), 'M outside 1..GENIE_ENVELOPE_MAX_POINTS'), (dict(x0=null), 'x0 is NULL'),
             (dict(points=null), 'points is NULL'), (dict(v=null), 'var is NULL'), (dict(softness=0.0), 'softness'), (dict(softness=-1.0), 'softness'),
             (dict(softness=inf), 'softness'), (dict(softness=nan), 'softness'), (dict(softness=1e-39), 'softness'),
             (dict(inside=0.1), 'inside_distance'), (dict(inside=0.0), 'inside_distance'), (dict(inside=inf), 'inside_distance'),
             (dict(inside=nan), 'inside_distance'), (dict(cover=0.1), 'cover_distance'), (dict(cover=-5.0), 'cover_distance'),
             (dict(cover=inf), 'cover_distance'), (dict(cover=nan), 'cover_distance'), (dict(iw=-1.0), 'inside_weight'), (dict(iw=inf), 'inside_weight'),
             (dict(iw=nan), 'inside_weight'), (dict(cw=-1.0), 'cover_weight'), (dict(cw=inf), 'cover_weight'), (dict(cw=nan), 'cover_weight'),
             (dict(iw=0.0, cw=0.0), 'no term enabled'), (dict(logp=null, grad=null), 'no output asked for'), (dict(logp=null), 'given together'),
             (dict(grad=null), 'given together'), (dict(wk=null), 'work is NULL'), (dict(wbytes=_work_bytes(2, 10, 7) - 1), 'work_bytes below'),
             (dict(wk=P(0x4002)), 'work not 4-byte aligned')]
    for kw, words in cases:
        assert call(**kw) == -1, kw                                                         # GENIE_E_ARG
        msg = lib.genie_last_error(None).decode()
        assert msg.startswith('genie_envelope_potential: ') and words in msg, (kw, msg)
