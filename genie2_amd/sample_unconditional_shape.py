"""`python -m genie2_amd.sample_unconditional_shape` -- shape-guided twisted-diffusion / SMC sampling (not in the reference): the
unconditional CLI's flags and output layout, outdir/pdbs/{length}_{index}.pdb, with every batch guided by a ShapePotential
(genie2_amd/smc.py, csrc/shape_kernels.hip): `--rog_max` caps the radius of gyration, `--clash_distance` penalises C-alpha pairs
closer than that (residues at least `--clash_separation` apart), `--restraint_file` keeps pairwise distances in given ranges.  At
least one of the three, or a secondary-structure, sheet, symmetry, binder, fold or diversity term (below), or a burial or an envelope
term (below), is needed.

The restraint file has one restraint per line, `i j lo hi [weight]`: residues 0-based like the motif_locations files, distances in
Angstrom, `inf` allowed for hi, weight 1 when omitted; `#` starts a comment.  A length too short for a restrained residue is skipped.

`--write_shape_report` adds outdir/shape/{length}_{index}.txt beside each PDB, one `key value` line per report field of the written
structure: rog, min_distance, n_clash, e_rog, e_clash, e_restraint, n_violated, max_violation (ShapePotential.describe).

`--helix_min` / `--helix_max` and `--extended_min` / `--extended_max` keep the soft helix / extended content (fractions of the
length - 4 five-residue windows) in a range, and `--ss_target STRING|FILE` pulls residues to a blueprint over `H`, `E` and `-` (or `C`:
free; in a file whitespace is ignored and `#` starts a comment): a SecStructPotential (csrc/secstruct_kernels.hip), summed with the
shape terms when both are asked for and enough on its own.  Giving only one of min / max leaves the other at 0 / 1.  "Extended" is
local geometry only, with no strand pairing (the sheet terms below add it).  A length other than the blueprint's is skipped.
`--write_secstruct` adds outdir/secstruct/{length}_{index}.txt: the hard assignment of the written structure as a string over `HEC`,
then one `key value` line per field of SecStructPotential.describe.

`--antiparallel_min` / `--antiparallel_max` and `--parallel_min` / `--parallel_max` keep the soft antiparallel / parallel strand-pairing
content (rungs per residue; an interior strand of a large sheet approaches 1) in a range, and `--ladder_file FILE` pulls listed rungs
together: a SheetPotential (csrc/sheet_kernels.hip), summed after the others and enough on its own.  Giving only a max leaves the min
at 0, only a min leaves the content unbounded above.  The ladder file has one ladder per line, `i j len A|P [weight]`: residues 0-based,
class A pairs i + k with j - k, class P pairs i + k with j + k, k = 0..len-1; `#` starts a comment.  A length that cannot hold the
ladder is skipped.  `--write_sheet` adds outdir/sheet/{length}_{index}.txt: one `i j A|P` line per formed rung of the written
structure (each rung once, i < j), then one `key value` line per field of SheetPotential.describe.

`--symmetry C<n>|D<n>|R<n>` guides the chain to repeat itself: n units around an n-fold axis (a cyclic oligomer, a closed toroid), 2n
units in two rings related by a two-fold, or n units along one screw (an open repeat): a SymmetryPotential
(csrc/symmetry_kernels.hip), summed last and enough on its own.  `--unit_length` (default: the length divided evenly), `--unit_linker`
and `--unit_offset` lay the units out, `--symmetry_weight` and `--symmetry_tausq` scale the term; a length the layout does not fit is
skipped.  `--unit_chains` samples and writes the units as chains A, B, ... (no linker, no offset, units that fill the length).
`--write_symmetry` adds outdir/symmetry/{length}_{index}.txt: the line `symmetry C3 units 3 unit_length 20 linker 0 offset 0`, then
one `key value` line per field of SymmetryPotential.describe.  Units can satisfy the term by lying on top of each other, which
`--clash_distance` prevents; `--rog_max` over the assembly keeps separate chains together.

`--target_pdb FILE` guides the design relative to a structure that is not sampled: a BinderPotential (csrc/binder_kernels.hip) over
the C-alpha atoms of the file's chains (`--target_chains AB`: those chains only), summed after everything else and enough on its own.
`--hotspots A45,A46,B12` (chain letter and residue number; or a file of such tokens, `#` starting a comment) asks every listed target
residue for `--hotspot_contacts` soft contacts with the design (weight `--hotspot_weight`); `--contacts_min` / `--contacts_max` keep
the soft number of design-target contacts within `--contact_distance` (default 8 A) in a range (weight `--contacts_weight`; only a
max leaves the min at 0, only a min leaves the count unbounded above); `--target_clash_distance` pushes design-target pairs closer
than that apart (weight `--target_clash_weight`).  At least one of the three is needed with a target.  `--target_standoff D` moves
the target, without rotating it, so that the origin -- where designs are born -- lies D Angstrom outside the hotspot patch on the
line from the target's centroid through the hotspots'; without it the file's frame is used as it is.  `--binder_tausq` is the
likelihood variance.  `--write_binder` adds outdir/binder/{length}_{index}.txt: a line `hotspot A45 0.873` per hotspot (its soft
contacts with the written design), then one `key value` line per field of BinderPotential.describe.  `--write_complex` adds
outdir/complex/{length}_{index}.pdb: the target's chains followed by the design as the last chain, centred jointly, relative
placement kept (the files under pdbs/ are centred per design); residue numbers restart at 1 in every chain.  A binder flag without
`--target_pdb` ends the run.  Not built: rotating the target, per-design-residue interface masks, all-atom or side-chain terms, and
feeding the target to the denoiser.

`--template_pdb FILE` guides every design towards the fold of a backbone: a FoldPotential (csrc/fold_kernels.hip) keeps the design's
TM-score to the file's C-alpha atoms (the project's gapless score of genie2_amd/similarity.py, the design moving) at or above
`--template_tm_min` (default 0.6; weight `--template_weight`).  `--avoid_dir DIR` guides every design away from known folds: its
TM-score to every backbone of DIR/pdbs/*.pdb (or DIR/*.pdb) is kept at or below `--avoid_tm_max` (default 0.5; weight
`--avoid_weight` each); `--avoid_representatives` keeps of them the designs that DIR/diversity/clusters.txt (python -m
genie2_amd.cluster_designs) names as representatives, and ends the run where that file is missing.  Both may be given; the term is
summed after everything else and enough on its own.  A reference counts for designs of exactly its own length: a template of another
length skips the length, avoided backbones of other lengths are ignored there, and a length left without a reference is skipped;
more than 4096 references of one length end the run.  `--fold_iterations` (default 16) are the ascent steps per seed,
`--fold_tausq` the likelihood variance.  `--write_fold` adds outdir/fold/{length}_{index}.txt: a line `ref NAME TM LO HI` per
reference (the written design's TM-score to it and the range asked for), then one `key value` line per field of
FoldPotential.describe.  `--fold_align gapped` (default `gapless`: all of the above, unchanged) scores under the gapped alignment of
genie2_amd.novelty instead, with an AlignedFoldPotential (csrc/fold_align_kernels.hip): every reference of 4..1024 residues applies
at every design length where length times its own is at most 131072; a template that does not fit a length skips it, avoided
backbones that do not fit are dropped there with a printed count, and more than 1024 applicable references end the run.
`--fold_norm query|reference|shorter|longer` (default query, novelty's), `--fold_rounds` (default 8), `--fold_gap_open` (default
-0.6) and `--fold_offset_stride` (default 1: every offset of the gapless stage) are the alignment's arguments and need
`--fold_align gapped`; the `ref` lines of `--write_fold` become `ref NAME TM LO HI LENGTH N_ALIGNED`.  Not built: gradients across
a change of alignment, per-residue masks on a reference, a best-of-several-templates form.

`--diversity_tm_max T` (with `--num_particles K`, which it needs: the run ends without it; K = 1 is valid and gives single coupled
trajectories) makes the designs of one device batch repel each other while they are sampled: a DiversityPotential
(csrc/diversity_kernels.hip) scores every pair of particles of different designs once with the fold term's score and keeps it at or
below T (weight `--diversity_weight`, default 1, divided by K; `--diversity_iterations`, default 16, ascent steps per seed;
`--diversity_tausq` the likelihood variance).  The particles of one design are resampled copies of each other and do not repel.  The
term is summed last and is enough on its own.  A design's trajectory then depends on the others of its batch, on purpose.  The coupling
is within one device batch only (`--batch_size` designs): across batches, devices and runs use `--avoid_dir` on the outputs so far.
`--write_diversity` adds outdir/batch_diversity/{length}_{index}.txt: a line `design NAME TM` for every other written design of the
same batch, then one `key value` line per field of DiversityPotential.describe (the nearest design of the batch, the mean, the number
above T, the energy), every written design counting as one.  Not built: gapped alignment between particles, coupling across batches
or devices, weighting partners by their SMC weights, a lower hinge.

`--bury RANGES --bury_min C` and `--expose RANGES --expose_max C` (RANGES like `3,10-20,35`: 0-based residues, inclusive) tell inside
from outside: a BurialPotential (csrc/burial_kernels.hip) keeps the half-sphere exposure of the listed residues -- the soft number of
C-alpha atoms within `--burial_radius` (default 10 A) on the side the virtual C-beta direction 2 x_n - x_{n-1} - x_{n+1} points to,
residues closer than `--burial_separation` (default 3) in sequence left out, the half-space `--burial_width` (default 2 A) soft -- at
or above C (a catalytic residue, the hydrophobic face of a helix) or at or below C (an epitope, a binding face).  `--burial_file FILE`
lists residues one per line, `i lo hi [weight]` (0-based, `inf` allowed for hi, `#` starts a comment); `--burial_weight` scales every
per-residue weight.  `--burial_mean_min` / `--burial_mean_max` keep the mean count over the chain in a range (weight
`--burial_mean_weight`; only a max leaves the min at 0, only a min leaves the mean unbounded above): a design with a core, not merely
a small one.  `--burial_tausq` is the likelihood variance.  The term is summed after the sheet term and before symmetry, and is enough
on its own.  `--bury` without `--bury_min`, `--expose` without `--expose_max`, a residue named by two sources, and a burial flag
without a term (`--burial_file`, `--bury`, `--expose`, `--burial_mean_min` or `--burial_mean_max`) end the run; a length too short for
a listed residue is skipped.  `--write_burial` adds outdir/burial/{length}_{index}.txt: a line `residue I C LO HI` per residue of the
written structure (its count, and the range asked of it or `- -`), then one `key value` line per field of BurialPotential.describe.
Not built: tying targets to a motif's placement, chain breaks under `--unit_chains` (the direction stencil crosses them), a full-atom
or C-beta model, counting a binder target's atoms as neighbours.

`--envelope_shape SPEC` or `--envelope_file FILE` (exactly one) says what shape the design should have: an EnvelopePotential
(csrc/envelope_kernels.hip) keeps every residue within `--envelope_inside_distance` (default 3 A, weight `--envelope_inside_weight`) of
the envelope's points and every point within `--envelope_cover_distance` (default 5 A, weight `--envelope_cover_weight`) of the design,
both as soft minima of softness `--envelope_softness` (default 4 A^2), so that the design stays inside the shape and fills it; a weight
of 0 switches a term off.  SPEC is `sphere:R`, `ellipsoid:A,B,C`, `cylinder:R,L`, `torus:R,r` (axis z) or `box:A,B,C` (full edge
lengths) in Angstrom, filled with lattice points `--envelope_spacing` (default 3 A) apart; FILE is a `.pdb` (every ATOM / HETATM record:
a C-alpha trace, a full-atom model, the pseudo-atoms a map tool writes) or text lines `x y z [weight]`, `#` starting a comment.  The
envelope's weighted centroid is moved to the origin, where designs are born; `--envelope_keep_frame` leaves it where it is (with
`--target_pdb`).  `--envelope_tausq` is the likelihood variance.  The term is summed after burial and before symmetry, and is enough
on its own.  Both sources at once and an envelope flag without either end the run.  `--write_envelope` adds
outdir/envelope/{length}_{index}.txt: a line `residue I A` per residue of the written structure (its soft distance to the envelope),
`covered_fraction F` (the weight share of points within the cover distance), then one `key value` line per field of
EnvelopePotential.describe; and once outdir/envelope/envelope.pdb, the points as placed, as HETATM pseudo-atoms.  Not built: rotating
or fitting the envelope to the design, assigning regions of it to residues, envelopes that follow a motif's placement, density-map
file formats.

`--num_particles`, `--num_steps`, `--guidance_alpha`, `--ess_threshold`, `--last_unguided_steps`, `--input_pdb` / `--start_step` /
`--write_start_rmsd` and `--resume` are those of the motif CLI (genie2_amd/sample_unconditional_motif.py), which takes the flags of
add_shape_arguments, add_secstruct_arguments, add_sheet_arguments, add_symmetry_arguments, add_binder_arguments, add_fold_arguments and
add_diversity_arguments, add_burial_arguments and add_envelope_arguments too and then guides
with the sum of the potentials asked for."""
import os

from tqdm import tqdm

from .sample_unconditional import PartialParser, UnconditionalRunner, add_common_arguments, write_start_rmsd

SHAPE_KEYS = ('rog_max', 'rog_weight', 'clash_distance', 'clash_separation', 'clash_weight', 'shape_tausq')
COUNTS = ('n_clash', 'n_violated')
SECSTRUCT_KEYS = ('helix_weight', 'extended_weight', 'ss_target_weight', 'ss_tausq')
SECSTRUCT_COUNTS = ('n_helix', 'n_extended', 'n_target_missed')
SHEET_KEYS = ('antiparallel_weight', 'parallel_weight', 'ladder_weight', 'sheet_tausq')
SYMMETRY_KEYS = ('symmetry', 'unit_length', 'unit_linker', 'unit_offset', 'symmetry_weight', 'symmetry_tausq')
BINDER_DEFAULTS = dict(target_pdb=None, target_chains=None, hotspots=None, hotspot_contacts=1.0, hotspot_weight=1.0, contact_distance=8.0,
                       contacts_min=None, contacts_max=None, contacts_weight=1.0, target_clash_distance=None, target_clash_weight=1.0,
                       target_standoff=None, binder_tausq=1.0, write_binder=False, write_complex=False)


def add_shape_arguments(parser):
    tail = ' (an addition to the reference CLI, like --align)'
    parser.add_argument('--rog_max', type=float, default=None,
                        help='Guide the radius of gyration below this many Angstrom; default: no such term' + tail)
    parser.add_argument('--rog_weight', type=float, default=1.0, help='Weight of the radius-of-gyration term' + tail)
    parser.add_argument('--clash_distance', type=float, default=None,
                        help='Guide C-alpha pairs apart that are closer than this many Angstrom; default: no such term' + tail)
    parser.add_argument('--clash_separation', type=int, default=2,
                        help='Residues at least this far apart in sequence count as a clashing pair' + tail)
    parser.add_argument('--clash_weight', type=float, default=1.0, help='Weight of the clash term' + tail)
    parser.add_argument('--restraint_file', type=str, default=None,
                        help='Distance restraints, one `i j lo hi [weight]` line each (0-based residues, Angstrom)' + tail)
    parser.add_argument('--shape_tausq', type=float, default=1.0, help='Likelihood variance tau^2 of the shape terms, Angstrom^2' + tail)
    parser.add_argument('--write_shape_report', action='store_true',
                        help='Write outdir/shape/{length}_{index}.txt: radius of gyration, closest pair, clashes, energies and '
                             'restraint violations of every written structure' + tail)


def shape_constants(params):
    """The shape keys of a runner's constants: the flags of add_shape_arguments, the restraint file read into 'restraints'."""
    from .smc import load_restraints
    defaults = dict(rog_max=None, rog_weight=1.0, clash_distance=None, clash_separation=2, clash_weight=1.0, shape_tausq=1.0)
    c = {k: params.get(k, defaults[k]) for k in SHAPE_KEYS}
    c['restraints'] = load_restraints(params['restraint_file']) if params.get('restraint_file') else []
    c['write_shape_report'] = bool(params.get('write_shape_report', False))
    return c


def has_shape_terms(constants):
    return constants.get('rog_max') is not None or constants.get('clash_distance') is not None or bool(constants.get('restraints'))


def restrained_lengths(tasks, restraints):
    """The tasks long enough for every restrained residue; the others are skipped with one printed line."""
    need = 1 + max([max(r[0], r[1]) for r in restraints], default=-1)
    short = [t['length'] for t in tasks if t['length'] < need]
    if short:
        print('skipping lengths shorter than the {} residues the restraints name: {}'.format(need, ', '.join(map(str, short))))
    return [t for t in tasks if t['length'] >= need]


def shape_potential(constants, length, abar, device):
    """The ShapePotential the constants ask for at this length, or None when they ask for no term.  (Lengths too short for a
    restrained residue never get here: restrained_lengths drops them when the tasks are made.)"""
    if not has_shape_terms(constants):
        return None
    from .smc import ShapePotential
    return ShapePotential(length, abar, rog_max=constants['rog_max'], rog_weight=constants['rog_weight'],
                          clash_distance=constants['clash_distance'], clash_separation=constants['clash_separation'],
                          clash_weight=constants['clash_weight'], restraints=constants['restraints'] or None,
                          tausq=constants['shape_tausq'], device=device)


def write_report(report, counts, directory, length, offset, headers=None):
    """One file per sample of a batch (so worker processes never share one), {length}_{offset + i}.txt: the line(s) headers[i] when
    there are headers (nothing for an empty one), then a `key value` line per field of `report`, %d for the fields named in `counts`,
    %.3f for the others."""
    os.makedirs(directory, exist_ok=True)
    for i in range(len(next(iter(report.values())))):
        with open(os.path.join(directory, '{}_{}.txt'.format(length, offset + i)), 'w') as fh:
            if headers is not None and headers[i]:
                fh.write(headers[i] + '\n')
            for key, column in report.items():
                fh.write(('{} {:d}\n' if key in counts else '{} {:.3f}\n').format(key, column[i].item()))


def write_shape_report(last_shape, directory, length, offset):
    """write_report of TwistedSampler.last_shape: %.3f for Angstrom and energies, %d for counts."""
    write_report(last_shape, COUNTS, directory, length, offset)


def add_secstruct_arguments(parser):
    tail = ' (an addition to the reference CLI, like --rog_max)'
    for name, word in (('helix', 'helix'),
                       ('extended', 'extended (strand-like, local geometry only: the sheet flags guide strand pairing)')):
        parser.add_argument('--%s_min' % name, type=float, default=None,
                            help='Guide the soft %s content, a fraction of the five-residue windows, above this; default: no such '
                                 'bound' % word + tail)
        parser.add_argument('--%s_max' % name, type=float, default=None,
                            help='Guide the soft %s content below this fraction; default: no such bound' % word + tail)
        parser.add_argument('--%s_weight' % name, type=float, default=1.0, help='Weight of the %s content term' % name + tail)
    parser.add_argument('--ss_target', type=str, default=None,
                        help='Blueprint over H, E and - (or C: free), one character per residue, or a file that holds it' + tail)
    parser.add_argument('--ss_target_weight', type=float, default=1.0, help='Weight of the blueprint term' + tail)
    parser.add_argument('--ss_tausq', type=float, default=1.0,
                        help='Likelihood variance tau^2 of the secondary-structure terms, Angstrom^2' + tail)
    parser.add_argument('--write_secstruct', action='store_true',
                        help='Write outdir/secstruct/{length}_{index}.txt: the H / E / C assignment, soft contents, counts and energies '
                             'of every written structure' + tail)


def secstruct_constants(params):
    """The secondary-structure keys of a runner's constants: the flags of add_secstruct_arguments, each min / max pair as 'helix' /
    'extended' = (min, max) or None (one of the two given: the other is 0 / 1), the blueprint read into 'ss_target'."""
    from .smc import load_ss_target
    defaults = dict(helix_weight=1.0, extended_weight=1.0, ss_target_weight=1.0, ss_tausq=1.0)
    c = {k: params.get(k, defaults[k]) for k in SECSTRUCT_KEYS}
    for name in ('helix', 'extended'):
        lo, hi = params.get(name + '_min'), params.get(name + '_max')
        c[name] = None if lo is None and hi is None else (0.0 if lo is None else lo, 1.0 if hi is None else hi)
    c['ss_target'] = load_ss_target(params['ss_target']) if params.get('ss_target') else None
    c['write_secstruct'] = bool(params.get('write_secstruct', False))
    return c


def has_secstruct_terms(constants):
    return constants.get('helix') is not None or constants.get('extended') is not None or constants.get('ss_target') is not None


def target_lengths(tasks, ss_target):
    """The tasks of the blueprint's length; the others are skipped with one printed line."""
    if ss_target is None:
        return tasks
    other = [t['length'] for t in tasks if t['length'] != len(ss_target)]
    if other:
        print('skipping lengths other than the {} residues of the blueprint: {}'.format(len(ss_target), ', '.join(map(str, other))))
    return [t for t in tasks if t['length'] == len(ss_target)]


def secstruct_potential(constants, length, abar, device):
    """The SecStructPotential the constants ask for at this length, or None when they ask for no term.  (Lengths other than the
    blueprint's never get here: target_lengths drops them when the tasks are made.)"""
    if not has_secstruct_terms(constants):
        return None
    from .smc import SecStructPotential
    return SecStructPotential(length, abar, helix=constants['helix'], helix_weight=constants['helix_weight'],
                              extended=constants['extended'], extended_weight=constants['extended_weight'],
                              target=constants['ss_target'], target_weight=constants['ss_target_weight'],
                              tausq=constants['ss_tausq'], device=device)


def add_sheet_arguments(parser):
    tail = ' (an addition to the reference CLI, like --rog_max)'
    for name in ('antiparallel', 'parallel'):
        parser.add_argument('--%s_min' % name, type=float, default=None,
                            help='Guide the soft %s strand-pairing content, in rungs per residue, above this; default: no such '
                                 'bound' % name + tail)
        parser.add_argument('--%s_max' % name, type=float, default=None,
                            help='Guide the soft %s strand-pairing content below this many rungs per residue; default: no such '
                                 'bound' % name + tail)
        parser.add_argument('--%s_weight' % name, type=float, default=1.0, help='Weight of the %s content term' % name + tail)
    parser.add_argument('--ladder_file', type=str, default=None,
                        help='Rungs to pull together, one `i j len A|P [weight]` line per ladder (0-based residues; A pairs i + k with '
                             'j - k, P with j + k)' + tail)
    parser.add_argument('--ladder_weight', type=float, default=1.0, help='Weight of the ladder term' + tail)
    parser.add_argument('--sheet_tausq', type=float, default=1.0, help='Likelihood variance tau^2 of the sheet terms, Angstrom^2' + tail)
    parser.add_argument('--write_sheet', action='store_true',
                        help='Write outdir/sheet/{length}_{index}.txt: the formed rungs, soft contents, counts and energies of every '
                             'written structure' + tail)


def sheet_constants(params):
    """The sheet keys of a runner's constants: the flags of add_sheet_arguments, each min / max pair as 'antiparallel' / 'parallel' =
    (min, max) or None (one of the two given: the other is 0 / inf), the ladder file read into 'ladder'."""
    import math
    from .smc import load_ladder
    defaults = dict(antiparallel_weight=1.0, parallel_weight=1.0, ladder_weight=1.0, sheet_tausq=1.0)
    c = {k: params.get(k, defaults[k]) for k in SHEET_KEYS}
    for name in ('antiparallel', 'parallel'):
        lo, hi = params.get(name + '_min'), params.get(name + '_max')
        c[name] = None if lo is None and hi is None else (0.0 if lo is None else lo, math.inf if hi is None else hi)
    c['ladder'] = load_ladder(params['ladder_file']) if params.get('ladder_file') else []
    c['write_sheet'] = bool(params.get('write_sheet', False))
    return c


def has_sheet_terms(constants):
    return constants.get('antiparallel') is not None or constants.get('parallel') is not None or bool(constants.get('ladder'))


def ladder_lengths(tasks, ladder):
    """The tasks long enough to hold every rung of the ladder (its highest centre is at most length - 2: check_ladder's rule); the
    others are skipped with one printed line."""
    top = max([max(i + n - 1, j if cls == 'A' else j + n - 1) for i, j, n, cls, *_ in ladder], default=-2)
    need = top + 2
    short = [t['length'] for t in tasks if t['length'] < need]
    if short:
        print('skipping lengths shorter than the {} residues the ladder needs: {}'.format(need, ', '.join(map(str, short))))
    return [t for t in tasks if t['length'] >= need]


def sheet_potential(constants, length, abar, device):
    """The SheetPotential the constants ask for at this length, or None when they ask for no term.  (Lengths that cannot hold the
    ladder never get here: ladder_lengths drops them when the tasks are made.)"""
    if not has_sheet_terms(constants):
        return None
    from .smc import SheetPotential
    return SheetPotential(length, abar, antiparallel=constants['antiparallel'], antiparallel_weight=constants['antiparallel_weight'],
                          parallel=constants['parallel'], parallel_weight=constants['parallel_weight'],
                          ladder=constants['ladder'] or None, ladder_weight=constants['ladder_weight'],
                          tausq=constants['sheet_tausq'], device=device)


def formed_rungs(pairs):
    """One row of TwistedSampler.last_pairs ([N, 2] partners) -> the lines `i j A|P` of its formed rungs, each once with i < j,
    class A first, ascending.  (A residue names only its best partner per class; a rung is listed when either end names the other.)"""
    rows = pairs.tolist()
    found = sorted({(c, min(n, m), max(n, m)) for n, row in enumerate(rows) for c, m in enumerate(row) if m >= 0})
    return ['{} {} {}'.format(i, j, 'AP'[c]) for c, i, j in found]


def write_sheet_report(pairs, report, directory, length, offset):
    """One file per sample of a batch, {length}_{offset + i}.txt: a line `i j A|P` per formed rung of TwistedSampler.last_pairs, then
    a `key value` line per field of `report` (the sheet fields of last_shape), %.3f for contents and energies, %d for counts."""
    from .capi import SHEET_COUNTS
    write_report(report, SHEET_COUNTS, directory, length, offset, ['\n'.join(formed_rungs(row)) for row in pairs])


def add_symmetry_arguments(parser):
    tail = ' (an addition to the reference CLI, like --rog_max)'
    parser.add_argument('--symmetry', type=str, default=None,
                        help='Guide the chain to repeat itself: C<n> (n units around an n-fold axis: a cyclic oligomer or a closed toroid), '
                             'D<n> (2n units, two rings related by a two-fold), R<n> (n units along one screw: an open repeat); default: '
                             'no such term' + tail)
    parser.add_argument('--unit_length', type=int, default=None,
                        help='Residues per unit; default: what is left of the length, divided evenly' + tail)
    parser.add_argument('--unit_linker', type=int, default=0, help='Free residues between two units' + tail)
    parser.add_argument('--unit_offset', type=int, default=0, help='Free residues before the first unit' + tail)
    parser.add_argument('--symmetry_weight', type=float, default=1.0, help='Weight of the symmetry term' + tail)
    parser.add_argument('--symmetry_tausq', type=float, default=1.0, help='Likelihood variance tau^2 of the symmetry term, Angstrom^2' + tail)
    parser.add_argument('--unit_chains', action='store_true',
                        help='Sample and write the units as separate chains A, B, ... (needs --unit_linker 0, --unit_offset 0 and units '
                             'that fill the length)' + tail)
    parser.add_argument('--write_symmetry', action='store_true',
                        help='Write outdir/symmetry/{length}_{index}.txt: the layout, then the symmetry energy, RMSDs, rotation angles and '
                             'rises of every written structure' + tail)


def symmetry_constants(params):
    """The symmetry keys of a runner's constants: the flags of add_symmetry_arguments.  A symbol that does not parse, and
    --unit_chains without --symmetry or with a linker or an offset, end the run here."""
    from .smc import parse_symmetry
    defaults = dict(symmetry=None, unit_length=None, unit_linker=0, unit_offset=0, symmetry_weight=1.0, symmetry_tausq=1.0)
    c = {k: params.get(k, defaults[k]) for k in SYMMETRY_KEYS}
    c['unit_chains'] = bool(params.get('unit_chains', False))
    c['write_symmetry'] = bool(params.get('write_symmetry', False))
    if c['symmetry'] is not None:
        try:
            parse_symmetry(c['symmetry'])
        except ValueError as e:
            raise SystemExit('--symmetry: %s' % e) from None
    if c['unit_chains'] and (c['symmetry'] is None or c['unit_linker'] or c['unit_offset']):
        raise SystemExit('--unit_chains needs --symmetry with --unit_linker 0 and --unit_offset 0: a chain is a unit, nothing else')
    return c


def has_symmetry_terms(constants):
    return constants.get('symmetry') is not None


def symmetric_lengths(tasks, constants):
    """The tasks whose length the symmetric layout fits (symmetry_layout's rules; with --unit_chains the units fill the length); the
    others are skipped with one printed line."""
    if not has_symmetry_terms(constants):
        return tasks
    from .smc import symmetry_layout

    def fits(length):
        try:
            units, m = symmetry_layout(constants['symmetry'], length, constants['unit_length'], constants['unit_linker'], constants['unit_offset'])
        except ValueError:
            return False
        return not constants['unit_chains'] or units * m == length

    other = [t['length'] for t in tasks if not fits(t['length'])]
    if other:
        print('skipping lengths the {} layout does not fit: {}'.format(constants['symmetry'], ', '.join(map(str, other))))
    return [t for t in tasks if fits(t['length'])]


def symmetry_potential(constants, length, abar, device):
    """The SymmetryPotential the constants ask for at this length, or None when they ask for no term.  (Lengths the layout does not
    fit never get here: symmetric_lengths drops them when the tasks are made.)"""
    if not has_symmetry_terms(constants):
        return None
    from .smc import SymmetryPotential
    return SymmetryPotential(length, abar, symmetry=constants['symmetry'], unit_length=constants['unit_length'],
                             linker=constants['unit_linker'], offset=constants['unit_offset'], weight=constants['symmetry_weight'],
                             tausq=constants['symmetry_tausq'], device=device)


def symmetry_header(potential):
    """The first line of a symmetry report: `symmetry C3 units 3 unit_length 20 linker 0 offset 0`."""
    return 'symmetry {} units {} unit_length {} linker {} offset {}'.format(potential.symmetry, potential.units, potential.unit_length,
                                                                            potential.linker, potential.offset)


def write_symmetry_report(report, header, directory, length, offset):
    """One file per sample of a batch, {length}_{offset + i}.txt: the layout line `header`, then a `key value` line per field of
    `report` (the symmetry fields of last_shape), %.3f."""
    write_report(report, (), directory, length, offset, [header] * len(next(iter(report.values()))))


def add_binder_arguments(parser):
    tail = ' (an addition to the reference CLI, like --rog_max)'
    parser.add_argument('--target_pdb', type=str, default=None,
                        help='Guide the design relative to the C-alpha atoms of this structure, which is not sampled; default: no such '
                             'term' + tail)
    parser.add_argument('--target_chains', type=str, default=None, help='Chain letters of the target to use, e.g. AB; default: all' + tail)
    parser.add_argument('--hotspots', type=str, default=None,
                        help='Target residues the design must touch, e.g. A45,A46,B12 (chain letter and residue number), or a file of '
                             'such tokens' + tail)
    parser.add_argument('--hotspot_contacts', type=float, default=1.0, help='Soft contacts asked of every hotspot' + tail)
    parser.add_argument('--hotspot_weight', type=float, default=1.0, help='Weight of the hotspot term' + tail)
    parser.add_argument('--contact_distance', type=float, default=8.0,
                        help='C-alpha distance in Angstrom at which a design-target pair counts half a contact' + tail)
    parser.add_argument('--contacts_min', type=float, default=None,
                        help='Guide the soft number of design-target contacts above this; default: no such bound' + tail)
    parser.add_argument('--contacts_max', type=float, default=None,
                        help='Guide the soft number of design-target contacts below this; default: no such bound' + tail)
    parser.add_argument('--contacts_weight', type=float, default=1.0, help='Weight of the contact-count term' + tail)
    parser.add_argument('--target_clash_distance', type=float, default=None,
                        help='Guide design-target C-alpha pairs apart that are closer than this many Angstrom; default: no such '
                             'term' + tail)
    parser.add_argument('--target_clash_weight', type=float, default=1.0, help='Weight of the target clash term' + tail)
    parser.add_argument('--target_standoff', type=float, default=None,
                        help='Move the target (no rotation) so that the origin, where designs are born, lies this many Angstrom outside '
                             'the hotspot patch; default: the frame of the file' + tail)
    parser.add_argument('--binder_tausq', type=float, default=1.0, help='Likelihood variance tau^2 of the binder terms, Angstrom^2' + tail)
    parser.add_argument('--write_binder', action='store_true',
                        help='Write outdir/binder/{length}_{index}.txt: the soft contacts of every hotspot, then contacts, interface '
                             'size, closest approach, clashes and energies of every written structure' + tail)
    parser.add_argument('--write_complex', action='store_true',
                        help='Write outdir/complex/{length}_{index}.pdb: the target chains and the design as the last chain, placed as '
                             'sampled' + tail)


def binder_constants(params):
    """The binder keys of a runner's constants: the flags of add_binder_arguments; with --target_pdb also 'target', the file read,
    placed (--target_standoff) and ready to travel to a worker process -- 'xyz' float64 numpy [M, 3] in the sampler's frame, 'labels',
    'chain_lengths', 'aatype' numpy [M], 'hotspots' (indices) -- and 'contacts' = (min, max) or None (one of the two given: the other
    is 0 / inf).  A binder flag without --target_pdb, a target with no term, and a file, chain, hotspot or standoff that does not
    hold up end the run here."""
    import math
    from .smc import load_target, parse_hotspots, place_target
    c = {k: params.get(k, v) for k, v in BINDER_DEFAULTS.items()}
    c['write_binder'], c['write_complex'] = bool(c['write_binder']), bool(c['write_complex'])
    c['target'] = c['contacts'] = None
    if c['target_pdb'] is None:
        given = [k for k, v in BINDER_DEFAULTS.items() if c[k] != v]
        if given:
            raise SystemExit('%s: a binder flag needs --target_pdb, the structure it is about' % ', '.join('--' + k for k in given))
        return c
    lo, hi = c['contacts_min'], c['contacts_max']
    c['contacts'] = None if lo is None and hi is None else (0.0 if lo is None else lo, math.inf if hi is None else hi)
    if c['hotspots'] is None and c['contacts'] is None and c['target_clash_distance'] is None:
        raise SystemExit('--target_pdb needs a term: --hotspots, --contacts_min, --contacts_max or --target_clash_distance')
    try:
        xyz, labels, chain_lengths, aatype = load_target(c['target_pdb'], c['target_chains'])
        hotspots = parse_hotspots(c['hotspots'], labels) if c['hotspots'] is not None else []
        xyz = place_target(xyz, hotspots, c['target_standoff'])
    except (OSError, ValueError) as e:
        raise SystemExit('--target_pdb / --hotspots / --target_standoff: %s' % e) from None
    c['target'] = dict(xyz=xyz.numpy(), labels=labels, chain_lengths=chain_lengths, aatype=aatype.numpy(), hotspots=hotspots)
    return c


def has_binder_terms(constants):
    return constants.get('target') is not None


def binder_potential(constants, length, abar, device):
    """The BinderPotential the constants ask for at this length, or None when they name no target."""
    if not has_binder_terms(constants):
        return None
    from .smc import BinderPotential
    t = constants['target']
    return BinderPotential(length, abar, t['xyz'], hotspots=t['hotspots'] or None, clash_distance=constants['target_clash_distance'],
                           clash_weight=constants['target_clash_weight'], contact_distance=constants['contact_distance'],
                           contacts=constants['contacts'], contacts_weight=constants['contacts_weight'],
                           hotspot_contacts=constants['hotspot_contacts'], hotspot_weight=constants['hotspot_weight'],
                           tausq=constants['binder_tausq'], device=device)


def hotspot_names(target):
    """The hotspots of binder_constants' target as the CLI names them: A45, B12, ..."""
    return ['{}{}'.format(*target['labels'][h]) for h in target['hotspots']]


def write_binder_report(hotspot_contacts, names, report, directory, length, offset):
    """One file per sample of a batch, {length}_{offset + i}.txt: a line `hotspot A45 0.873` per hotspot (`names`, and row i of
    `hotspot_contacts` [rows, H], BinderPotential.hotspot_contacts_of of TwistedSampler.last_positions), then a `key value` line per
    field of `report` (the binder fields of last_shape), %.3f for contacts, distances and energies, %d for counts."""
    from .capi import BINDER_COUNTS
    rows = hotspot_contacts.tolist()
    write_report(report, BINDER_COUNTS, directory, length, offset,
                 ['\n'.join('hotspot {} {:.3f}'.format(n, v) for n, v in zip(names, row)) for row in rows])


def write_complex(positions, target, directory, length, offset):
    """One file per sample of a batch, {length}_{offset + i}.pdb, through save_np_features_to_pdb: the target's chains (binder_constants'
    target: coordinates in the sampler's frame, residue types from its file) followed by the design, row i of `positions` [rows, N, 3]
    (TwistedSampler.last_positions), as the last chain.  The writer centres the complex as a whole, so relative placement is kept."""
    import numpy as np
    from . import features as F
    os.makedirs(directory, exist_ok=True)
    M = len(target['xyz'])
    for i, design in enumerate(np.asarray(positions, dtype=float)):
        f = F.create_empty_np_features(list(target['chain_lengths']) + [len(design)])
        f['aatype'][np.arange(M), np.asarray(target['aatype'])] = 1
        f['atom_positions'] = np.concatenate([np.asarray(target['xyz'], dtype=float), design])
        F.save_np_features_to_pdb(f, os.path.join(directory, '{}_{}.pdb'.format(length, offset + i)))


# The context flags of the motif CLI (sample_unconditional_motif.py: a context follows a motif's placement, so the shape CLI's parser
# does not take them).  The defaults -- contact distance 8 A, weights 1, tausq 1 A^2 -- are design choices: no trained checkpoint is
# in the tree, so their effect on sample quality is unmeasured.
CONTEXT_DEFAULTS = dict(context_pdb=None, context_chains=None, context_clash_distance=None, context_clash_weight=1.0, context_contact_distance=8.0,
                        context_contacts_min=None, context_contacts_max=None, context_contacts_weight=1.0, context_group=None, context_tausq=1.0,
                        write_context=False, write_context_complex=False)


def add_context_arguments(parser):
    tail = ' (an addition to the reference CLI, like --motif_groups)'
    parser.add_argument('--context_pdb', type=str, default=None,
                        help='Guide the design relative to the C-alpha atoms of this structure, the binding partner of the motif, which '
                             'follows every particle\'s own placement of the motif; it must be in the frame of the motif file\'s ATOM '
                             'records, typically the complex the motif was cut from; default: no such term' + tail)
    parser.add_argument('--context_chains', type=str, default=None, help='Chain letters of the context to use, e.g. HL; default: all' + tail)
    parser.add_argument('--context_clash_distance', type=float, default=None,
                        help='Guide design-context C-alpha pairs apart that are closer than this many Angstrom (motif residues sit '
                             'out); default: no such term' + tail)
    parser.add_argument('--context_clash_weight', type=float, default=1.0, help='Weight of the context clash term' + tail)
    parser.add_argument('--context_contact_distance', type=float, default=8.0,
                        help='C-alpha distance in Angstrom at which a design-context pair counts half a contact' + tail)
    parser.add_argument('--context_contacts_min', type=float, default=None,
                        help='Guide the soft number of design-context contacts above this; default: no such bound' + tail)
    parser.add_argument('--context_contacts_max', type=float, default=None,
                        help='Guide the soft number of design-context contacts below this; default: no such bound' + tail)
    parser.add_argument('--context_contacts_weight', type=float, default=1.0, help='Weight of the context contact-count term' + tail)
    parser.add_argument('--context_group', type=str, default=None,
                        help='With --motif_groups file: the label of the motif group the context is tied to (required when the file has '
                             'more than one group)' + tail)
    parser.add_argument('--context_tausq', type=float, default=1.0, help='Likelihood variance tau^2 of the context terms, Angstrom^2' + tail)
    parser.add_argument('--write_context', action='store_true',
                        help='Write outdir/context/{length}_{index}.txt: contacts, interface size, closest approach, clashes, the anchor '
                             'RMSD and the energies of every written structure against the context as placed for it' + tail)
    parser.add_argument('--write_context_complex', action='store_true',
                        help='Write outdir/context_complex/{length}_{index}.pdb: the context chains as placed for that design, then the '
                             'design as the last chain' + tail)


def context_constants(params):
    """The context keys of a runner's constants: the flags of add_context_arguments; with --context_pdb also 'context', the file read
    and ready to travel to a worker process -- 'xyz' float64 numpy [C, 3] in the file's frame, 'labels', 'chain_lengths', 'aatype'
    numpy [C] -- and 'context_contacts' = (min, max) or None (one of the two given: the other is 0 / inf).  A context flag without
    --context_pdb, a context with no term, and a file or chain that does not hold up end the run here."""
    import math
    from .smc import load_target
    c = {k: params.get(k, v) for k, v in CONTEXT_DEFAULTS.items()}
    c['write_context'], c['write_context_complex'] = bool(c['write_context']), bool(c['write_context_complex'])
    c['context'] = c['context_contacts'] = None
    if c['context_pdb'] is None:
        given = [k for k, v in CONTEXT_DEFAULTS.items() if c[k] != v]
        if given:
            raise SystemExit('%s: a context flag needs --context_pdb, the structure it is about' % ', '.join('--' + k for k in given))
        return c
    lo, hi = c['context_contacts_min'], c['context_contacts_max']
    c['context_contacts'] = None if lo is None and hi is None else (0.0 if lo is None else lo, math.inf if hi is None else hi)
    if c['context_contacts'] is None and c['context_clash_distance'] is None:
        raise SystemExit('--context_pdb needs a term: --context_clash_distance, --context_contacts_min or --context_contacts_max')
    try:
        xyz, labels, chain_lengths, aatype = load_target(c['context_pdb'], c['context_chains'])
    except (OSError, ValueError) as e:
        raise SystemExit('--context_pdb / --context_chains: %s' % e) from None
    c['context'] = dict(xyz=xyz.numpy(), labels=labels, chain_lengths=chain_lengths, aatype=aatype.numpy())
    return c


def has_context_terms(constants):
    return constants.get('context') is not None


def write_context_report(report, directory, length, offset):
    """One file per sample of a batch, {length}_{offset + i}.txt: a `key value` line per field of `report` (the context fields of
    last_shape), %.3f for contacts, distances and energies, %d for counts."""
    from .capi import CONTEXT_COUNTS
    write_report(report, CONTEXT_COUNTS, directory, length, offset)


def write_context_complex(positions, placed, context, directory, length, offset):
    """write_complex for a context that moves: file {length}_{offset + i}.pdb holds the context's chains (context_constants' context)
    at placed[i] [C, 3], where ContextPotential.placed_context puts them for design i, then positions[i] as the last chain."""
    import numpy as np
    for i, (design, xyz) in enumerate(zip(np.asarray(positions, dtype=float), np.asarray(placed, dtype=float))):
        write_complex(design[None], dict(context, xyz=xyz), directory, length, offset + i)


FOLD_DEFAULTS = dict(template_pdb=None, template_tm_min=0.6, template_weight=1.0, avoid_dir=None, avoid_tm_max=0.5, avoid_weight=1.0,
                     avoid_representatives=False, fold_iterations=16, fold_tausq=1.0, write_fold=False)
FOLD_MAX_REFERENCES = 4096      # capi.FOLD_MAX_REFERENCES: the most references of one length
# the flags of --fold_align gapped (kept apart: FOLD_DEFAULTS is what the gapless form takes)
FOLD_ALIGN_DEFAULTS = dict(fold_align='gapless', fold_norm='query', fold_rounds=8, fold_gap_open=-0.6, fold_offset_stride=1)
FOLD_ALIGN_MAX_REFERENCES = 1024        # capi.FOLD_ALIGN_MAX_REFERENCES: the most references that apply at one length under gapped alignment
FOLD_ALIGN_LENGTHS, FOLD_ALIGN_MAX_CELLS = (4, 1024), 131072       # capi.TM_MIN_LENGTH, TMALIGN_MAX_LENGTH, TMALIGN_MAX_CELLS


def add_fold_arguments(parser):
    tail = ' (an addition to the reference CLI, like --rog_max)'
    parser.add_argument('--template_pdb', type=str, default=None,
                        help='Guide every design to a TM-score of at least --template_tm_min to the C-alpha backbone of this file (same '
                             'length as the design); default: no such term' + tail)
    parser.add_argument('--template_tm_min', type=float, default=0.6, help='TM-score to the template to stay at or above' + tail)
    parser.add_argument('--template_weight', type=float, default=1.0, help='Weight of the template term' + tail)
    parser.add_argument('--avoid_dir', type=str, default=None,
                        help='Guide every design to a TM-score of at most --avoid_tm_max to every backbone of its own length in this '
                             'folder (its pdbs/*.pdb, else its *.pdb); default: no such term' + tail)
    parser.add_argument('--avoid_tm_max', type=float, default=0.5, help='TM-score to every avoided backbone to stay at or below' + tail)
    parser.add_argument('--avoid_weight', type=float, default=1.0, help='Weight of every avoided backbone' + tail)
    parser.add_argument('--avoid_representatives', action='store_true',
                        help='Of --avoid_dir keep the cluster representatives that its diversity/clusters.txt names '
                             '(genie2_amd.cluster_designs writes it)' + tail)
    parser.add_argument('--fold_iterations', type=int, default=16, help='Ascent iterations per seed of the TM-score, 1..32' + tail)
    parser.add_argument('--fold_tausq', type=float, default=1.0, help='Likelihood variance tau^2 of the fold terms, Angstrom^2' + tail)
    parser.add_argument('--write_fold', action='store_true',
                        help='Write outdir/fold/{length}_{index}.txt: the TM-score of every written structure to every reference, the '
                             'nearest reference, the violated bounds and the energy' + tail)
    parser.add_argument('--fold_align', type=str, default='gapless', choices=('gapless', 'gapped'),
                        help='gapless: a reference counts for designs of its own length, under the identity alignment; gapped: every '
                             'reference of 4..1024 residues counts at every length, under the gapped alignment of genie2_amd.novelty' + tail)
    parser.add_argument('--fold_norm', type=str, default='query', choices=('query', 'reference', 'shorter', 'longer'),
                        help='With --fold_align gapped: the length that normalises the TM-score (query: the design)' + tail)
    parser.add_argument('--fold_rounds', type=int, default=8, help='With --fold_align gapped: rounds of dynamic programming, 0..16' + tail)
    parser.add_argument('--fold_gap_open', type=float, default=-0.6, help='With --fold_align gapped: gap opening penalty, -10..0' + tail)
    parser.add_argument('--fold_offset_stride', type=int, default=1,
                        help='With --fold_align gapped: the gapless stage visits every s-th offset and the last one, 1..64' + tail)


def cluster_representatives(path):
    """The names in the `representative` column of a clusters.txt of genie2_amd.cluster_designs, in file order, each once."""
    out = []
    with open(path) as fh:
        for line in fh:
            fields = line.split()
            if fields and not fields[0].startswith('#') and len(fields) >= 4 and fields[3] not in out:
                out.append(fields[3])
    return out


def fold_constants(params):
    """The fold keys of a runner's constants: the flags of add_fold_arguments; with --template_pdb or --avoid_dir also 'fold', the
    references read and ready to travel to a worker process: a list of dicts 'name', 'xyz' (float32 numpy [L, 3]), 'lo', 'hi',
    'weight', 'template' (bool), the template first, then the avoided backbones in file-name order.  A fold flag without either, a
    value out of range, a file or folder that does not hold up and --avoid_representatives without a clusters.txt end the run here."""
    import math
    from .cluster_designs import design_files
    from .similarity import load_designs
    c = {k: params.get(k, v) for k, v in FOLD_DEFAULTS.items()}
    c['avoid_representatives'], c['write_fold'] = bool(c['avoid_representatives']), bool(c['write_fold'])
    c.update({k: params.get(k, v) for k, v in FOLD_ALIGN_DEFAULTS.items()})
    c['fold'] = None
    if c['fold_align'] not in ('gapless', 'gapped'):
        raise SystemExit('--fold_align must be gapless or gapped, got %r' % (c['fold_align'],))
    if c['fold_align'] != 'gapped':
        given = [k for k, v in FOLD_ALIGN_DEFAULTS.items() if k != 'fold_align' and c[k] != v]
        if given:
            raise SystemExit('%s: an alignment flag needs --fold_align gapped' % ', '.join('--' + k for k in given))
    if c['template_pdb'] is None and c['avoid_dir'] is None:
        given = [k for k, v in list(FOLD_DEFAULTS.items()) + list(FOLD_ALIGN_DEFAULTS.items()) if c[k] != v]
        if given:
            raise SystemExit('%s: a fold flag needs --template_pdb or --avoid_dir, the backbones it is about' % ', '.join('--' + k for k in given))
        return c
    if c['avoid_representatives'] and c['avoid_dir'] is None:
        raise SystemExit('--avoid_representatives needs --avoid_dir, the folder whose clusters it reads')
    if not (0.0 < c['template_tm_min'] <= 1.0):
        raise SystemExit('--template_tm_min must be above 0 and at most 1, got %r' % (c['template_tm_min'],))
    if not (0.0 <= c['avoid_tm_max'] < 1.0):
        raise SystemExit('--avoid_tm_max must be at least 0 and below 1, got %r' % (c['avoid_tm_max'],))
    for k in ('template_weight', 'avoid_weight'):
        if not (math.isfinite(c[k]) and c[k] >= 0):
            raise SystemExit('--%s must be finite and >= 0, got %r' % (k, c[k]))
    if not 1 <= c['fold_iterations'] <= 32:
        raise SystemExit('--fold_iterations must be in 1..32, got %r' % (c['fold_iterations'],))
    if not (math.isfinite(c['fold_tausq']) and c['fold_tausq'] > 0):
        raise SystemExit('--fold_tausq must be finite and > 0, got %r' % (c['fold_tausq'],))
    if c['fold_norm'] not in ('query', 'reference', 'shorter', 'longer'):
        raise SystemExit('--fold_norm must be query, reference, shorter or longer, got %r' % (c['fold_norm'],))
    if not 0 <= c['fold_rounds'] <= 16:
        raise SystemExit('--fold_rounds must be in 0..16, got %r' % (c['fold_rounds'],))
    if not -10.0 <= c['fold_gap_open'] <= 0.0:
        raise SystemExit('--fold_gap_open must be in -10..0, got %r' % (c['fold_gap_open'],))
    if not 1 <= c['fold_offset_stride'] <= 64:
        raise SystemExit('--fold_offset_stride must be in 1..64, got %r' % (c['fold_offset_stride'],))
    refs = []

    def read(files, lo, hi, weight, template):
        try:
            x, lengths, names = load_designs(files)
        except (OSError, ValueError) as e:
            raise SystemExit('--template_pdb / --avoid_dir: %s' % e) from None
        for m, name in enumerate(names):
            refs.append(dict(name=name, xyz=x[m, :lengths[m]].numpy().copy(), lo=float(lo), hi=float(hi), weight=float(weight), template=template))

    if c['template_pdb'] is not None:
        read([c['template_pdb']], c['template_tm_min'], math.inf, c['template_weight'], True)
    if c['avoid_dir'] is not None:
        files = design_files(c['avoid_dir'])
        if c['avoid_representatives']:
            table = os.path.join(c['avoid_dir'], 'diversity', 'clusters.txt')
            if not os.path.isfile(table):
                raise SystemExit('--avoid_representatives needs %s: run python -m genie2_amd.cluster_designs --indir %s first'
                                 % (table, c['avoid_dir']))
            keep = set(cluster_representatives(table))
            files = [f for f in files if os.path.basename(f)[:-4] in keep]
            if not files:
                raise SystemExit('%s names no design of %s' % (table, c['avoid_dir']))
        read(files, 0.0, c['avoid_tm_max'], c['avoid_weight'], False)
    if not any(r['weight'] > 0 for r in refs):
        raise SystemExit('--template_weight / --avoid_weight: every fold reference has weight 0')
    c['fold'] = refs
    return c


def has_fold_terms(constants):
    return constants.get('fold') is not None


def fold_gapped(constants):
    return constants.get('fold_align', 'gapless') == 'gapped'


def fold_fits(n_ref, length):
    """Whether a reference of n_ref residues can be aligned to a design of `length`: both of 4..1024 residues, at most 131072 cells."""
    lo, hi = FOLD_ALIGN_LENGTHS
    return lo <= n_ref <= hi and lo <= length <= hi and n_ref * length <= FOLD_ALIGN_MAX_CELLS


def fold_references(constants, length):
    """The fold references that apply at this length: those of exactly `length` residues -- none at all where the template is of
    another length (a template of another length skips the length, as a blueprint does) or every one left has weight 0.  With
    --fold_align gapped: those that fit the length (fold_fits) -- none at all where the template does not or every one left has
    weight 0."""
    refs = constants.get('fold') or []
    if fold_gapped(constants):
        if any(r['template'] and not fold_fits(len(r['xyz']), length) for r in refs):
            return []
        refs = [r for r in refs if fold_fits(len(r['xyz']), length)]
        return refs if any(r['weight'] > 0 for r in refs) else []
    if any(r['template'] and len(r['xyz']) != length for r in refs):
        return []
    refs = [r for r in refs if len(r['xyz']) == length]
    return refs if any(r['weight'] > 0 for r in refs) else []


def fold_lengths(tasks, constants):
    """The tasks whose length has a fold reference (fold_references); the others are skipped with one printed line.  More than
    FOLD_MAX_REFERENCES references of one length end the run."""
    if not has_fold_terms(constants):
        return tasks
    if fold_gapped(constants):
        return fold_lengths_gapped(tasks, constants)
    count = {t['length']: len(fold_references(constants, t['length'])) for t in tasks}
    for length, n in count.items():
        if n > FOLD_MAX_REFERENCES:
            raise SystemExit('%d fold references of %d residues: at most %d of one length (--avoid_representatives keeps one per cluster)'
                             % (n, length, FOLD_MAX_REFERENCES))
    other = [t['length'] for t in tasks if not count[t['length']]]
    if other:
        print('skipping lengths without a fold reference of their own length: {}'.format(', '.join(map(str, other))))
    return [t for t in tasks if count[t['length']]]


def fold_lengths_gapped(tasks, constants):
    """fold_lengths under --fold_align gapped: a length is skipped where the template does not fit it or nothing with a weight does,
    with one printed line; avoided backbones that do not fit a kept length are dropped there, with a printed count per length; more
    than FOLD_ALIGN_MAX_REFERENCES applicable references end the run."""
    refs = constants.get('fold') or []
    count = {t['length']: len(fold_references(constants, t['length'])) for t in tasks}
    for length, n in count.items():
        if n > FOLD_ALIGN_MAX_REFERENCES:
            raise SystemExit('%d fold references apply at %d residues: at most %d under --fold_align gapped (--avoid_representatives '
                             'keeps one per cluster)' % (n, length, FOLD_ALIGN_MAX_REFERENCES))
    other = [t['length'] for t in tasks if not count[t['length']]]
    if other:
        print('skipping lengths without a fold reference that fits them: {}'.format(', '.join(map(str, other))))
    for length in sorted({t['length'] for t in tasks if count[t['length']]}):
        dropped = sum(1 for r in refs if not r['template'] and not fold_fits(len(r['xyz']), length))
        if dropped:
            print('length {}: {} avoided backbones dropped (outside 4..1024 residues or above 131072 cells)'.format(length, dropped))
    return [t for t in tasks if count[t['length']]]


def fold_potential(constants, length, abar, device):
    """The FoldPotential the constants ask for at this length (its references' names as `.names`), or None when they name no
    reference; with --fold_align gapped an AlignedFoldPotential (the references' lengths as `.lengths`).  (Lengths without a
    reference never get here: fold_lengths drops them when the tasks are made.)"""
    if not has_fold_terms(constants):
        return None
    import numpy as np
    from .smc import AlignedFoldPotential, FoldPotential
    refs = fold_references(constants, length)
    if fold_gapped(constants):
        pot = AlignedFoldPotential(length, abar, [r['xyz'] for r in refs], [(r['lo'], r['hi'], r['weight']) for r in refs],
                                   norm=constants['fold_norm'], n_iter=constants['fold_iterations'], n_rounds=constants['fold_rounds'],
                                   gap_open=constants['fold_gap_open'], offset_stride=constants['fold_offset_stride'],
                                   tausq=constants['fold_tausq'], device=device)
        pot.names, pot.ranges = [r['name'] for r in refs], [(r['lo'], r['hi']) for r in refs]
        return pot
    pot = FoldPotential(length, abar, np.stack([r['xyz'] for r in refs]), [(r['lo'], r['hi'], r['weight']) for r in refs],
                        n_iter=constants['fold_iterations'], tausq=constants['fold_tausq'], device=device)
    pot.names, pot.ranges = [r['name'] for r in refs], [(r['lo'], r['hi']) for r in refs]
    return pot


def write_fold_report(tm, names, ranges, report, directory, length, offset, lengths=None, n_aligned=None):
    """One file per sample of a batch, {length}_{offset + i}.txt: a line `ref <name> <tm %.3f> <lo> <hi>` per reference (`names`,
    `ranges`, and row i of `tm` [rows, R], FoldPotential.tm_of of TwistedSampler.last_positions), then a `key value` line per field
    of `report` (the fold fields of last_shape), %.3f for TM-scores and the energy, %d for counts.  With `lengths` (per reference)
    and `n_aligned` [rows, R] (AlignedFoldPotential.alignment_of) the lines are `ref <name> <tm> <lo> <hi> <length> <n_aligned>`."""
    from .capi import FOLD_COUNTS
    rows = tm.tolist()
    if lengths is None:
        heads = ['\n'.join('ref {} {:.3f} {:g} {:g}'.format(n, v, lo, hi) for n, v, (lo, hi) in zip(names, row, ranges)) for row in rows]
    else:
        heads = ['\n'.join('ref {} {:.3f} {:g} {:g} {:d} {:d}'.format(n, v, lo, hi, int(L), int(k))
                           for n, v, (lo, hi), L, k in zip(names, row, ranges, lengths, counts))
                 for row, counts in zip(rows, n_aligned.tolist())]
    write_report(report, FOLD_COUNTS, directory, length, offset, heads)


DIVERSITY_DEFAULTS = dict(diversity_tm_max=None, diversity_weight=1.0, diversity_iterations=16, diversity_tausq=1.0, write_diversity=False)


def add_diversity_arguments(parser):
    tail = ' (an addition to the reference CLI, like --rog_max)'
    parser.add_argument('--diversity_tm_max', type=float, default=None,
                        help='With --num_particles: guide the designs of one device batch to a TM-score of at most this to each other '
                             'while they are sampled (across batches and runs: --avoid_dir); default: no such term' + tail)
    parser.add_argument('--diversity_weight', type=float, default=1.0, help='Weight of the diversity term (divided by --num_particles)' + tail)
    parser.add_argument('--diversity_iterations', type=int, default=16,
                        help='Ascent iterations per seed of the TM-score between particles, 1..32' + tail)
    parser.add_argument('--diversity_tausq', type=float, default=1.0, help='Likelihood variance tau^2 of the diversity term, Angstrom^2' + tail)
    parser.add_argument('--write_diversity', action='store_true',
                        help='Write outdir/batch_diversity/{length}_{index}.txt: the TM-score of every written structure to the others '
                             'of its batch, the nearest of them, their mean, the number above --diversity_tm_max and the energy' + tail)


def diversity_constants(params):
    """The diversity keys of a runner's constants: the flags of add_diversity_arguments.  A diversity flag without
    --diversity_tm_max, --diversity_tm_max without --num_particles and a value out of range end the run here."""
    import math
    c = {k: params.get(k, v) for k, v in DIVERSITY_DEFAULTS.items()}
    c['write_diversity'] = bool(c['write_diversity'])
    if c['diversity_tm_max'] is None:
        given = [k for k, v in DIVERSITY_DEFAULTS.items() if c[k] != v]
        if given:
            raise SystemExit('%s: a diversity flag needs --diversity_tm_max, the TM-score to stay below' % ', '.join('--' + k for k in given))
        return c
    if params.get('num_particles') is None:
        raise SystemExit('--diversity_tm_max needs --num_particles: the designs of a batch repel each other as particle systems '
                         '(--num_particles 1 gives single coupled trajectories)')
    if not 0 < c['diversity_tm_max'] <= 1:
        raise SystemExit('--diversity_tm_max must be in (0, 1], got %r' % (c['diversity_tm_max'],))
    if not (math.isfinite(c['diversity_weight']) and c['diversity_weight'] > 0):
        raise SystemExit('--diversity_weight must be finite and > 0, got %r' % (c['diversity_weight'],))
    if not 1 <= c['diversity_iterations'] <= 32:
        raise SystemExit('--diversity_iterations must be in 1..32, got %r' % (c['diversity_iterations'],))
    if not (math.isfinite(c['diversity_tausq']) and c['diversity_tausq'] > 0):
        raise SystemExit('--diversity_tausq must be finite and > 0, got %r' % (c['diversity_tausq'],))
    return c


def has_diversity_terms(constants):
    return constants.get('diversity_tm_max') is not None


def diversity_potential(constants, length, abar, device):
    """The DiversityPotential the constants ask for at this length, over systems of --num_particles, or None when they ask for no
    such term."""
    if not has_diversity_terms(constants):
        return None
    from .smc import DiversityPotential
    return DiversityPotential(length, abar, constants['num_particles'], tm_max=constants['diversity_tm_max'],
                              weight=constants['diversity_weight'], n_iter=constants['diversity_iterations'],
                              tausq=constants['diversity_tausq'], device=device)


def write_diversity_report(tm, names, report, directory, length, offset):
    """One file per sample of a batch, {length}_{offset + i}.txt: a line `design <name> <tm %.3f>` for every other design of the batch
    (`names`, and row i of `tm` [rows, rows], DiversityPotential.tm_of of TwistedSampler.last_positions), then a `key value` line per
    field of `report` (the diversity fields of last_shape), %.3f for TM-scores and the energy, %d for counts."""
    from .capi import DIVERSITY_COUNTS
    heads = ['\n'.join('design {} {:.3f}'.format(n, v) for k, (n, v) in enumerate(zip(names, row)) if k != i) for i, row in enumerate(tm.tolist())]
    write_report(report, DIVERSITY_COUNTS, directory, length, offset, heads)


BURIAL_DEFAULTS = dict(burial_file=None, bury=None, bury_min=None, expose=None, expose_max=None, burial_mean_min=None, burial_mean_max=None,
                       burial_weight=1.0, burial_mean_weight=1.0, burial_radius=10.0, burial_width=2.0, burial_separation=3, burial_tausq=1.0,
                       write_burial=False)
BURIAL_TERM_FLAGS = ('burial_file', 'bury', 'expose', 'burial_mean_min', 'burial_mean_max')     # any of them makes a term


def add_burial_arguments(parser):
    tail = ' (an addition to the reference CLI, like --rog_max)'
    parser.add_argument('--burial_file', type=str, default=None,
                        help='Half-sphere exposure targets, one `i lo hi [weight]` line per residue (0-based; hi may be inf); default: '
                             'no such term' + tail)
    parser.add_argument('--bury', type=str, default=None,
                        help='Residues to bury, e.g. 3,10-20,35 (0-based, inclusive): their soft half-sphere count is guided to at least '
                             '--bury_min' + tail)
    parser.add_argument('--bury_min', type=float, default=None, help='The count --bury asks for at least' + tail)
    parser.add_argument('--expose', type=str, default=None,
                        help='Residues to keep solvent-exposed, e.g. 30-41: their soft half-sphere count is guided to at most '
                             '--expose_max' + tail)
    parser.add_argument('--expose_max', type=float, default=None, help='The count --expose allows at most' + tail)
    parser.add_argument('--burial_mean_min', type=float, default=None,
                        help='Guide the mean soft half-sphere count over the chain above this; default: no such bound' + tail)
    parser.add_argument('--burial_mean_max', type=float, default=None,
                        help='Guide the mean soft half-sphere count over the chain below this; default: no such bound' + tail)
    parser.add_argument('--burial_weight', type=float, default=1.0, help='Scales the weight of every per-residue burial target' + tail)
    parser.add_argument('--burial_mean_weight', type=float, default=1.0, help='Weight of the mean-burial term' + tail)
    parser.add_argument('--burial_radius', type=float, default=10.0,
                        help='C-alpha distance in Angstrom at which a residue counts half a neighbour' + tail)
    parser.add_argument('--burial_width', type=float, default=2.0, help='Softness of the half-space in Angstrom' + tail)
    parser.add_argument('--burial_separation', type=int, default=3,
                        help='Residues at least this far apart in sequence count as neighbours' + tail)
    parser.add_argument('--burial_tausq', type=float, default=1.0, help='Likelihood variance tau^2 of the burial terms' + tail)
    parser.add_argument('--write_burial', action='store_true',
                        help='Write outdir/burial/{length}_{index}.txt: the soft half-sphere count of every residue of every written '
                             'structure with the range asked of it, then the mean, extremes, violations and energies' + tail)


def burial_constants(params):
    """The burial keys of a runner's constants: the flags of add_burial_arguments, and 'burial_targets', the residues of --burial_file,
    --bury and --expose as one list [(i, lo, hi, weight), ...] sorted by residue, every weight scaled by --burial_weight, and
    'burial_mean' = (min, max) or None (one of the two given: the other is 0 / inf).  --bury or --expose without its threshold (or
    the threshold without its list), a residue named by two sources, a burial flag without a term, a value out of range and a file or
    a list that does not hold up end the run here."""
    import math
    from .smc import check_burial_targets, load_burial_targets, parse_residue_ranges
    c = {k: params.get(k, v) for k, v in BURIAL_DEFAULTS.items()}
    c['write_burial'] = bool(c['write_burial'])
    c['burial_targets'], c['burial_mean'] = [], None
    if all(c[k] is None for k in BURIAL_TERM_FLAGS):
        given = [k for k, v in BURIAL_DEFAULTS.items() if c[k] != v]
        if given:
            raise SystemExit('%s: a burial flag needs a term: --burial_file, --bury, --expose, --burial_mean_min or --burial_mean_max'
                             % ', '.join('--' + k for k in given))
        return c
    for ranges, bound in (('bury', 'bury_min'), ('expose', 'expose_max')):
        if c[ranges] is not None and c[bound] is None:
            raise SystemExit('--%s needs --%s, the count to stay %s' % (ranges, bound, 'at or above' if ranges == 'bury' else 'at or below'))
        if c[bound] is not None and c[ranges] is None:
            raise SystemExit('--%s needs --%s, the residues it is about' % (bound, ranges))
    for k in ('bury_min', 'expose_max', 'burial_mean_min', 'burial_mean_max', 'burial_weight', 'burial_mean_weight'):
        if c[k] is not None and not (math.isfinite(c[k]) and c[k] >= 0):
            raise SystemExit('--%s must be finite and >= 0, got %r' % (k, c[k]))
    for k in ('burial_radius', 'burial_width', 'burial_tausq'):
        if not (math.isfinite(c[k]) and c[k] > 0):
            raise SystemExit('--%s must be finite and > 0, got %r' % (k, c[k]))
    if c['burial_separation'] < 1:
        raise SystemExit('--burial_separation must be at least 1, got %r' % (c['burial_separation'],))
    targets = []
    try:
        if c['burial_file'] is not None:
            targets += load_burial_targets(c['burial_file'])
        if c['bury'] is not None:
            targets += [(i, c['bury_min'], math.inf, 1.0) for i in parse_residue_ranges(c['bury'])]
        if c['expose'] is not None:
            targets += [(i, 0.0, c['expose_max'], 1.0) for i in parse_residue_ranges(c['expose'])]
        seen = set()
        for t in targets:
            if t[0] in seen:
                raise ValueError('residue %d is named twice (by --burial_file, --bury or --expose)' % t[0])
            seen.add(t[0])
        top = 1 + max([t[0] for t in targets if isinstance(t[0], int)], default=0)
        targets = check_burial_targets([(i, lo, hi, w * c['burial_weight']) for i, lo, hi, w in targets], top)
    except (OSError, ValueError) as e:
        raise SystemExit('--burial_file / --bury / --expose: %s' % e) from None
    c['burial_targets'] = targets
    lo, hi = c['burial_mean_min'], c['burial_mean_max']
    if lo is not None or hi is not None:
        c['burial_mean'] = (0.0 if lo is None else lo, math.inf if hi is None else hi)
        if c['burial_mean'][1] < c['burial_mean'][0]:
            raise SystemExit('--burial_mean_max is below --burial_mean_min: %r < %r' % (hi, lo))
    if not targets and (c['burial_mean'] is None or c['burial_mean_weight'] == 0):
        raise SystemExit('the burial flags name no residue and no mean with a weight: nothing to guide')
    return c


def has_burial_terms(constants):
    return bool(constants.get('burial_targets')) or constants.get('burial_mean') is not None


def burial_lengths(tasks, targets):
    """The tasks long enough for every listed residue; the others are skipped with one printed line."""
    need = 1 + max([t[0] for t in targets], default=-1)
    short = [t['length'] for t in tasks if t['length'] < need]
    if short:
        print('skipping lengths shorter than the {} residues the burial targets name: {}'.format(need, ', '.join(map(str, short))))
    return [t for t in tasks if t['length'] >= need]


def burial_potential(constants, length, abar, device):
    """The BurialPotential the constants ask for at this length, or None when they ask for no term.  (Lengths too short for a listed
    residue never get here: burial_lengths drops them when the tasks are made.)"""
    if not has_burial_terms(constants):
        return None
    from .smc import BurialPotential
    return BurialPotential(length, abar, targets=constants['burial_targets'] or None, mean=constants['burial_mean'],
                           mean_weight=constants['burial_mean_weight'], radius=constants['burial_radius'], width=constants['burial_width'],
                           separation=constants['burial_separation'], tausq=constants['burial_tausq'], device=device)


def write_burial_report(burial, targets, report, directory, length, offset):
    """One file per sample of a batch, {length}_{offset + i}.txt: a line `residue I C LO HI` per residue (row i of `burial` [rows, N],
    BurialPotential.burial_of of TwistedSampler.last_positions, %.3f; LO and HI from `targets` [(i, lo, hi, weight), ...], `-` where
    the residue has none), then a `key value` line per field of `report` (the burial fields of last_shape), %.3f for counts of
    neighbours and energies, %d for the number of violations."""
    from .capi import BURIAL_COUNTS
    ranges = {t[0]: ('{:g}'.format(t[1]), '{:g}'.format(t[2])) for t in targets}
    heads = ['\n'.join('residue {} {:.3f} {} {}'.format(n, v, *ranges.get(n, ('-', '-'))) for n, v in enumerate(row)) for row in burial.tolist()]
    write_report(report, BURIAL_COUNTS, directory, length, offset, heads)


ENVELOPE_DEFAULTS = dict(envelope_file=None, envelope_shape=None, envelope_spacing=3.0, envelope_keep_frame=False,
                         envelope_inside_distance=3.0, envelope_inside_weight=1.0, envelope_cover_distance=5.0, envelope_cover_weight=1.0,
                         envelope_softness=4.0, envelope_tausq=1.0, write_envelope=False)
ENVELOPE_EPS, ENVELOPE_MAX_POINTS = 0.1, 16384      # capi.ENVELOPE_EPS, capi.ENVELOPE_MAX_POINTS


def add_envelope_arguments(parser):
    tail = ' (an addition to the reference CLI, like --rog_max)'
    parser.add_argument('--envelope_file', type=str, default=None,
                        help='Guide the design to stay inside and to fill the shape these points outline: a .pdb (every ATOM / HETATM '
                             'record) or text lines `x y z [weight]`; default: no such term' + tail)
    parser.add_argument('--envelope_shape', type=str, default=None,
                        help='The same with a solid: sphere:R, ellipsoid:A,B,C, cylinder:R,L, torus:R,r (axis z) or box:A,B,C (full edge '
                             'lengths), in Angstrom, filled with lattice points --envelope_spacing apart' + tail)
    parser.add_argument('--envelope_spacing', type=float, default=3.0, help='Lattice spacing of --envelope_shape in Angstrom' + tail)
    parser.add_argument('--envelope_keep_frame', action='store_true',
                        help='Leave the envelope where its coordinates put it (with --target_pdb, say); default: its weighted centroid is '
                             'moved to the origin, where designs are born' + tail)
    parser.add_argument('--envelope_inside_distance', type=float, default=3.0,
                        help='Soft distance in Angstrom from the nearest envelope points a residue may have' + tail)
    parser.add_argument('--envelope_inside_weight', type=float, default=1.0, help='Weight of the stay-inside term; 0: off' + tail)
    parser.add_argument('--envelope_cover_distance', type=float, default=5.0,
                        help='Soft distance in Angstrom from the nearest residues an envelope point may have' + tail)
    parser.add_argument('--envelope_cover_weight', type=float, default=1.0, help='Weight of the fill-it term; 0: off' + tail)
    parser.add_argument('--envelope_softness', type=float, default=4.0, help='Softness tau of the two soft minima, Angstrom^2' + tail)
    parser.add_argument('--envelope_tausq', type=float, default=1.0, help='Likelihood variance tau^2 of the envelope terms' + tail)
    parser.add_argument('--write_envelope', action='store_true',
                        help='Write outdir/envelope/{length}_{index}.txt: the soft distance of every residue of every written structure '
                             'to the envelope, the covered fraction, then counts, worst excesses and energies; and once '
                             'outdir/envelope/envelope.pdb, the points as placed' + tail)


def envelope_constants(params):
    """The envelope keys of a runner's constants: the flags of add_envelope_arguments; with --envelope_file or --envelope_shape also
    'envelope', the points read or generated and ready to travel to a worker process: 'points' float64 numpy [M, 3] as the file or the
    solid gives them (EnvelopePotential centres them unless --envelope_keep_frame) and 'weights' float64 numpy [M] or None.  Both
    sources at once, an envelope flag without either, a value out of range, both weights 0 and a file or a specification that does not
    hold up end the run here."""
    import math
    from .smc import envelope_shape_points, load_envelope
    c = {k: params.get(k, v) for k, v in ENVELOPE_DEFAULTS.items()}
    c['write_envelope'], c['envelope_keep_frame'] = bool(c['write_envelope']), bool(c['envelope_keep_frame'])
    c['envelope'] = None
    if c['envelope_file'] is None and c['envelope_shape'] is None:
        given = [k for k, v in ENVELOPE_DEFAULTS.items() if c[k] != v]
        if given:
            raise SystemExit('%s: an envelope flag needs a term: --envelope_file or --envelope_shape' % ', '.join('--' + k for k in given))
        return c
    if c['envelope_file'] is not None and c['envelope_shape'] is not None:
        raise SystemExit('--envelope_file and --envelope_shape both name the envelope: give one of them')
    for k in ('envelope_inside_distance', 'envelope_cover_distance'):
        if not (math.isfinite(c[k]) and c[k] > ENVELOPE_EPS):
            raise SystemExit('--%s must be finite and above %g, got %r' % (k, ENVELOPE_EPS, c[k]))
    for k in ('envelope_inside_weight', 'envelope_cover_weight'):
        if not (math.isfinite(c[k]) and c[k] >= 0):
            raise SystemExit('--%s must be finite and >= 0, got %r' % (k, c[k]))
    for k in ('envelope_spacing', 'envelope_softness', 'envelope_tausq'):
        if not (math.isfinite(c[k]) and c[k] > 0):
            raise SystemExit('--%s must be finite and > 0, got %r' % (k, c[k]))
    if c['envelope_inside_weight'] == 0 and c['envelope_cover_weight'] == 0:
        raise SystemExit('--envelope_inside_weight and --envelope_cover_weight are both 0: nothing to guide')
    try:
        if c['envelope_file'] is not None:
            points, weights = load_envelope(c['envelope_file'])
            if len(points) > ENVELOPE_MAX_POINTS:
                raise ValueError('%s has %d points, at most %d fit' % (c['envelope_file'], len(points), ENVELOPE_MAX_POINTS))
            if not bool((weights > 0).all()) or not bool((weights < math.inf).all()):
                raise ValueError('%s: every weight must be finite and > 0' % c['envelope_file'])
            weights = None if bool((weights == 1).all()) else weights.numpy()
        else:
            points, weights = envelope_shape_points(c['envelope_shape'], c['envelope_spacing']), None
    except (OSError, ValueError) as e:
        raise SystemExit('--envelope_file / --envelope_shape: %s' % e) from None
    c['envelope'] = dict(points=points.numpy(), weights=weights)
    return c


def has_envelope_terms(constants):
    return constants.get('envelope') is not None


def envelope_potential(constants, length, abar, device):
    """The EnvelopePotential the constants ask for at this length, or None when they name no envelope."""
    if not has_envelope_terms(constants):
        return None
    from .smc import EnvelopePotential
    e = constants['envelope']
    return EnvelopePotential(length, abar, e['points'], weights=e['weights'], inside_distance=constants['envelope_inside_distance'],
                             inside_weight=constants['envelope_inside_weight'], cover_distance=constants['envelope_cover_distance'],
                             cover_weight=constants['envelope_cover_weight'], softness=constants['envelope_softness'],
                             tausq=constants['envelope_tausq'], center=not constants['envelope_keep_frame'], device=device)


def write_envelope_report(distance, gap, weights, cover_distance, report, directory, length, offset):
    """One file per sample of a batch, {length}_{offset + i}.txt: a line `residue I A` per residue (row i of `distance` [rows, N],
    EnvelopePotential.distance_of of TwistedSampler.last_positions, %.3f), then `covered_fraction F`, the weight share of the envelope
    points whose soft distance to the design (row i of `gap` [rows, M], gap_of) is at most `cover_distance` (`weights` [M] or None:
    all 1), then a `key value` line per field of `report` (the envelope fields of last_shape), %.3f for Angstrom and energies, %d for
    counts."""
    from .capi import ENVELOPE_COUNTS
    covered = (gap <= cover_distance).double()
    share = covered.mean(dim=1) if weights is None else (covered * weights.double()[None]).sum(dim=1) / weights.double().sum()
    heads = ['\n'.join(['residue {} {:.3f}'.format(n, v) for n, v in enumerate(row)] + ['covered_fraction {:.3f}'.format(f)])
             for row, f in zip(distance.tolist(), share.tolist())]
    write_report(report, ENVELOPE_COUNTS, directory, length, offset, heads)


def write_envelope_pdb(points, weights, path):
    """The envelope as placed, [M, 3] with weights [M] or None, as HETATM pseudo-atoms (the weight in the occupancy column), so that a
    viewer shows design and envelope together; residue numbers wrap at 10000."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        for m, (x, y, z) in enumerate(points.tolist()):
            w = 1.0 if weights is None else float(weights[m])
            fh.write('HETATM{:5d}  C   ENV E{:4d}    {:8.3f}{:8.3f}{:8.3f}{:6.2f}{:6.2f}           C\n'.format((m + 1) % 100000, (m + 1) % 10000,
                                                                                                             x, y, z, w, 0.0))
        fh.write('END\n')


def sum_potentials(*potentials):
    """The potentials that are not None, in that order: the one there is, their SumPotential, or None."""
    from .smc import SumPotential
    members = [p for p in potentials if p is not None]
    return None if not members else members[0] if len(members) == 1 else SumPotential(*members)


def report_fields(report, names):
    """The fields `names` of a sampler's merged report, in that order."""
    return {k: report[k] for k in names}


def write_secstruct_report(assignment, report, directory, length, offset):
    """One file per sample of a batch, {length}_{offset + i}.txt: the assignment of TwistedSampler.last_secstruct as a string over
    HEC, then a `key value` line per field of `report` (the secondary-structure fields of last_shape), %.3f for contents and
    energies, %d for counts."""
    from .smc import ss_string
    write_report(report, SECSTRUCT_COUNTS, directory, length, offset, [ss_string(row) for row in assignment.tolist()])


GUIDANCE_FLAGS = {
    'guidance_alpha': dict(type=float, default=0.012, help='Guidance gradient regulariser alpha'),
    'ess_threshold': dict(type=float, default=0.5, help='Resample when the effective sample size falls below this fraction of the batch'),
    'last_unguided_steps': dict(type=int, default=50, help='Steps below this one are not guided'),
    'num_steps': dict(type=int, default=None, help='Run the reverse process on this many of the n_timestep steps, with the ancestral '
                                                   'kernel between them; default: all'),
    'num_particles': dict(type=int, default=None,
                          help='Guide every design as a particle system of its own with this many particles (1..64) and write its best '
                               'particle: --num_samples and --batch_size then count designs; default: one system per batch, every '
                               'particle written'),
    'resume': dict(action='store_true', help='Skip batches whose PDB files already exist'),
}


def add_guidance_arguments(parser, tail, *names):
    """The guidance flags `names` of a guided CLI (all of GUIDANCE_FLAGS when none are named), in that order, each help text ending
    in `tail`: a CLI that words its tails differently, or lists other flags between these, calls this once per run of flags."""
    for name in names or GUIDANCE_FLAGS:
        kw = GUIDANCE_FLAGS[name]
        parser.add_argument('--' + name, **dict(kw, help=kw['help'] + tail))


class GuidedRunner(UnconditionalRunner):
    """The runner of the guided CLIs: every batch sampled by a TwistedSampler under the sum of the potentials of `batch_potentials`
    (a subclass's own, made per batch; none here) and the shape, secondary-structure, sheet, burial, envelope, symmetry, binder, fold and diversity
    potentials the constants ask for, in that order; `after_batch` writes a subclass's own reports.  With --unit_chains the features hold the units as chains."""

    def guided_lengths(self, tasks, params):
        """The tasks whose length the restraints, the blueprint, the ladder, the burial targets, the symmetric layout and the fold
        references allow."""
        tasks = target_lengths(restrained_lengths(tasks, shape_constants(params)['restraints']), secstruct_constants(params)['ss_target'])
        tasks = burial_lengths(ladder_lengths(tasks, sheet_constants(params)['ladder']), burial_constants(params)['burial_targets'])
        tasks = symmetric_lengths(tasks, symmetry_constants(params))
        return fold_lengths(tasks, fold_constants(params))

    def create_tasks(self, params):
        return self.guided_lengths(super().create_tasks(params), params)

    def create_constants(self, params):
        c = super().create_constants(params)
        c.update({k: params[k] for k in ('guidance_alpha', 'ess_threshold', 'last_unguided_steps')})
        c['num_particles'] = params.get('num_particles')
        c.update(shape_constants(params))
        c.update(secstruct_constants(params))
        c.update(sheet_constants(params))
        c.update(burial_constants(params))
        c.update(envelope_constants(params))
        c.update(symmetry_constants(params))
        c.update(binder_constants(params))
        c.update(fold_constants(params))
        c.update(diversity_constants(params))
        return c

    def batch_potentials(self, constants, length, abar, device):
        return ()

    def after_batch(self, constants, sampler, length, offset):
        pass

    def execute(self, constants, tasks, device):
        from . import capi, pack
        from .smc import TwistedSampler
        model = self.load_model(constants, device)
        sampler = TwistedSampler(model)
        abar = pack.schedule_tensors(model.config.diffusion['n_timestep'])['alphas_cumprod'].to(device)
        # (with --num_particles: `batch` systems, each returning its best particle)
        systems = {} if constants.get('num_particles') is None else {'num_particles': constants['num_particles'], 'return_particles': 'best'}
        for task in tqdm(tasks, desc=device):
            length, outdir = task['length'], constants['outdir']
            shape = shape_potential(constants, length, abar, device)
            secstruct = secstruct_potential(constants, length, abar, device)
            sheet = sheet_potential(constants, length, abar, device)
            burial = burial_potential(constants, length, abar, device)
            envelope = envelope_potential(constants, length, abar, device)
            if constants['write_envelope'] and envelope is not None and not os.path.exists(os.path.join(outdir, 'envelope', 'envelope.pdb')):
                write_envelope_pdb(envelope.points.cpu(), None if envelope.weights is None else envelope.weights.cpu(),
                                   os.path.join(outdir, 'envelope', 'envelope.pdb'))
            symmetry = symmetry_potential(constants, length, abar, device)
            binder = binder_potential(constants, length, abar, device)
            fold = fold_potential(constants, length, abar, device)
            diversity = diversity_potential(constants, length, abar, device)
            chains = {'chain_lengths': symmetry.chain_lengths()} if constants['unit_chains'] else {}
            for batch, offset in self.batches(constants, outdir, length):
                sampler.sample({
                    'length': length, 'scale': constants['scale'], 'num_samples': batch,
                    'outdir': outdir, 'prefix': str(length), 'offset': offset,
                    'twisting_function': sum_potentials(*self.batch_potentials(constants, length, abar, device), shape, secstruct, sheet,
                                                        burial, envelope, symmetry, binder, fold, diversity),
                    'guidance_alpha': constants['guidance_alpha'],
                    'ess_threshold': constants['ess_threshold'], 'last_unguided_steps': constants['last_unguided_steps'],
                    'num_steps': constants.get('num_steps'), **systems, **chains, **self.partial_params(constants)})
                if constants.get('write_start_rmsd'):
                    write_start_rmsd(sampler.last_start_rmsd, os.path.join(outdir, 'start_rmsd'),
                                     ['{}_{}'.format(length, offset + i) for i in range(batch)])
                self.after_batch(constants, sampler, length, offset)
                if constants['write_shape_report'] and shape is not None:
                    write_shape_report(report_fields(sampler.last_shape, capi.SHAPE_REPORT), os.path.join(outdir, 'shape'), length, offset)
                if constants['write_secstruct'] and secstruct is not None:
                    write_secstruct_report(sampler.last_secstruct, report_fields(sampler.last_shape, capi.SECSTRUCT_REPORT),
                                           os.path.join(outdir, 'secstruct'), length, offset)
                if constants['write_sheet'] and sheet is not None:
                    write_sheet_report(sampler.last_pairs, report_fields(sampler.last_shape, capi.SHEET_REPORT),
                                       os.path.join(outdir, 'sheet'), length, offset)
                if constants['write_burial'] and burial is not None:
                    write_burial_report(burial.burial_of(sampler.last_positions.to(burial.device)).cpu(), constants['burial_targets'],
                                        report_fields(sampler.last_shape, capi.BURIAL_REPORT), os.path.join(outdir, 'burial'), length, offset)
                if constants['write_envelope'] and envelope is not None:
                    at = sampler.last_positions.to(envelope.device)
                    write_envelope_report(envelope.distance_of(at).cpu(), envelope.gap_of(at).cpu(),
                                          None if envelope.weights is None else envelope.weights.cpu(), envelope.cover_distance,
                                          report_fields(sampler.last_shape, capi.ENVELOPE_REPORT), os.path.join(outdir, 'envelope'), length, offset)
                if constants['write_symmetry'] and symmetry is not None:
                    write_symmetry_report(report_fields(sampler.last_shape, capi.SYMMETRY_REPORT), symmetry_header(symmetry),
                                          os.path.join(outdir, 'symmetry'), length, offset)
                if constants['write_binder'] and binder is not None:
                    write_binder_report(binder.hotspot_contacts_of(sampler.last_positions.to(binder.device)).cpu(),
                                        hotspot_names(constants['target']), report_fields(sampler.last_shape, capi.BINDER_REPORT),
                                        os.path.join(outdir, 'binder'), length, offset)
                if constants['write_complex'] and binder is not None:
                    write_complex(sampler.last_positions.numpy(), constants['target'], os.path.join(outdir, 'complex'), length, offset)
                if constants['write_fold'] and fold is not None and fold_gapped(constants):
                    found = fold.alignment_of(sampler.last_positions.to(fold.device))
                    write_fold_report(found['tm'].cpu(), fold.names, fold.ranges, report_fields(sampler.last_shape, capi.FOLD_REPORT),
                                      os.path.join(outdir, 'fold'), length, offset, fold.lengths, found['n_aligned'].cpu())
                elif constants['write_fold'] and fold is not None:
                    write_fold_report(fold.tm_of(sampler.last_positions.to(fold.device)).cpu(), fold.names, fold.ranges,
                                      report_fields(sampler.last_shape, capi.FOLD_REPORT), os.path.join(outdir, 'fold'), length, offset)
                if constants['write_diversity'] and diversity is not None:
                    write_diversity_report(diversity.tm_of(sampler.last_positions.to(diversity.device)).cpu(),
                                           ['{}_{}'.format(length, offset + i) for i in range(len(sampler.last_positions))],
                                           report_fields(sampler.last_shape, capi.DIVERSITY_REPORT),
                                           os.path.join(outdir, 'batch_diversity'), length, offset)


class ShapeRunner(GuidedRunner):
    def create_constants(self, params):
        c = super().create_constants(params)
        if not (has_shape_terms(c) or has_secstruct_terms(c) or has_sheet_terms(c) or has_symmetry_terms(c) or has_binder_terms(c)
                or has_fold_terms(c) or has_diversity_terms(c) or has_burial_terms(c) or has_envelope_terms(c)):
            raise SystemExit('no shape term asked for: give --rog_max, --clash_distance or --restraint_file, a secondary-structure '
                             'term (--helix_min, --helix_max, --extended_min, --extended_max, --ss_target), a sheet term '
                             '(--antiparallel_min, --antiparallel_max, --parallel_min, --parallel_max, --ladder_file), a binder term (--target_pdb '
                             'with --hotspots, --contacts_min, --contacts_max or --target_clash_distance), a fold term (--template_pdb, --avoid_dir), '
                             'a diversity term (--diversity_tm_max with --num_particles), a burial term (--burial_file, --bury with --bury_min, '
                             '--expose with --expose_max, --burial_mean_min, --burial_mean_max), an envelope term (--envelope_file, --envelope_shape) '
                             'or --symmetry')
        return c


def build_parser():
    p = PartialParser('input_pdb', 'Structure file whose C-alpha backbone every particle starts from')
    add_common_arguments(p)
    add_guidance_arguments(p, '', 'resume', 'guidance_alpha', 'ess_threshold', 'last_unguided_steps', 'num_steps', 'num_particles')
    add_shape_arguments(p)
    add_secstruct_arguments(p)
    add_sheet_arguments(p)
    add_symmetry_arguments(p)
    add_binder_arguments(p)
    add_fold_arguments(p)
    add_diversity_arguments(p)
    add_burial_arguments(p)
    add_envelope_arguments(p)
    return p


def main(args):
    ShapeRunner().run(vars(args), args.num_devices, args.sequential_order)


if __name__ == '__main__':
    main(build_parser().parse_args())
