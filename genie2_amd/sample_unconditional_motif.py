"""`python -m genie2_amd.sample_unconditional_motif` -- motif-guided twisted-diffusion / SMC sampling, the fork's
genie/sample_unconditional_motif.py (:131-166 flags; its runner drives genie/sampler/unconditional_smc.py) with the reference's
flags and the unconditional CLI's output layout, outdir/pdbs/{length}_{index}.pdb.

The reference hard-codes its motif (sampler/smc_sampler_new.py:155-157); here it is an explicit `--motif_file` in the REMARK 999
format of the scaffold CLI.  Its motif entries, in file order, are the segments; their C-alpha coordinates come from the file's
ATOM records.  Each batch is one particle system of `batch_size` particles guided by the fused motif potential (MotifPotential,
csrc/smc_kernels.hip) over every placement of the segments in a structure of that length.

`--align rigid` guides with the superposed form of the potential, which does not depend on the orientation the motif file is written
in.  `--write_motif_locations` adds outdir/motif_locations/{length}_{index}.txt beside each PDB: one `start\tend` line per segment
(0-based, end inclusive: the format of the reference's motif_location.txt, unconditional_smc.py:334-343) for the placement that fits
the sample best after optimal superposition, then a last line `# rmsd <motif RMSD of that fit in Angstrom>`.

`--motif_groups file` reads the motif group of every segment from the problem file (column 29 of REMARK 999 INPUT, as the scaffold
CLI does): segments of one group keep their relative pose, different groups are guided as independent bodies, and the location files
end with one more line per group, `# rmsd group <label> <that group's own RMSD>`.  The default, `joint`, treats all segments as one
rigid motif.

`--num_particles K` makes every design a particle system of its own: `--num_samples` then counts designs, `--batch_size` designs per
sampler call (a device batch of batch_size * K particles), and each system's best particle (the largest accumulated weight) is the
one written, one PDB and one location file per design.  Without it a batch is one system and every particle is written.

`--input_pdb FILE --start_step T0` starts every particle from the file's backbone noised to step T0 (partial diffusion, as in the
unconditional CLI: one length, `--write_start_rmsd`); it combines with `--align`, `--motif_groups`, `--num_particles` and `--num_steps`.

`--rog_max`, `--clash_distance` and `--restraint_file` (with their weights, `--clash_separation` and `--shape_tausq`: the flags of
genie2_amd/sample_unconditional_shape.py) add shape guidance: the potential is then SumPotential(MotifPotential, ShapePotential), and
`--write_shape_report` writes outdir/shape/{length}_{index}.txt as that CLI does.  Lengths too short for a restrained residue are
skipped.

`--helix_min` / `--helix_max`, `--extended_min` / `--extended_max` and `--ss_target` (with their weights and `--ss_tausq`: the flags
of add_secstruct_arguments in the same module) add secondary-structure guidance: the potentials asked for are summed in the order
motif, shape, secondary structure, `--write_secstruct` writes outdir/secstruct/{length}_{index}.txt as that CLI does, and lengths
other than the blueprint's are skipped.

`--antiparallel_min` / `--antiparallel_max`, `--parallel_min` / `--parallel_max` and `--ladder_file` (with their weights and
`--sheet_tausq`: the flags of add_sheet_arguments in the same module) add strand-pairing guidance, summed after them; `--write_sheet`
writes outdir/sheet/{length}_{index}.txt as that CLI does, and lengths that cannot hold the ladder are skipped.

`--symmetry C<n>|D<n>|R<n>` (with `--unit_length`, `--unit_linker`, `--unit_offset`, `--symmetry_weight`, `--symmetry_tausq`,
`--unit_chains` and `--write_symmetry`: the flags of add_symmetry_arguments in the same module) adds symmetry guidance, summed last;
`--write_symmetry` writes outdir/symmetry/{length}_{index}.txt as that CLI does, and lengths the layout does not fit are skipped.

`--target_pdb` (with `--target_chains`, `--hotspots`, `--hotspot_contacts`, `--hotspot_weight`, `--contact_distance`, `--contacts_min`,
`--contacts_max`, `--contacts_weight`, `--target_clash_distance`, `--target_clash_weight`, `--target_standoff`, `--binder_tausq`,
`--write_binder` and `--write_complex`: the flags of add_binder_arguments in the same module) adds binder guidance against a fixed
target, summed after all the others; `--write_binder` writes outdir/binder/{length}_{index}.txt and `--write_complex`
outdir/complex/{length}_{index}.pdb as that CLI does.

`--template_pdb` and `--avoid_dir` (with `--template_tm_min`, `--template_weight`, `--avoid_tm_max`, `--avoid_weight`,
`--avoid_representatives`, `--fold_iterations`, `--fold_tausq` and `--write_fold`: the flags of add_fold_arguments in the same module)
add fold guidance towards a template backbone or away from known ones, summed after all the others; `--write_fold` writes
outdir/fold/{length}_{index}.txt as that CLI does, and lengths without a reference of their own length are skipped.  `--fold_align
gapped` (with `--fold_norm`, `--fold_rounds`, `--fold_gap_open`, `--fold_offset_stride`) scores under gapped alignment instead, so
that references of any length apply, exactly as that CLI describes.

`--diversity_tm_max T` (with `--diversity_weight`, `--diversity_iterations`, `--diversity_tausq` and `--write_diversity`: the flags of
add_diversity_arguments in the same module; it needs `--num_particles`) makes the designs of one device batch repel each other while
they are sampled, summed last; `--write_diversity` writes outdir/batch_diversity/{length}_{index}.txt as that CLI does.  The coupling
is within one device batch only: across batches and runs use `--avoid_dir`.

`--bury RANGES --bury_min C`, `--expose RANGES --expose_max C`, `--burial_file`, `--burial_mean_min` / `--burial_mean_max` (with
`--burial_weight`, `--burial_mean_weight`, `--burial_radius`, `--burial_width`, `--burial_separation`, `--burial_tausq` and
`--write_burial`: the flags of add_burial_arguments in the same module) add burial guidance by half-sphere exposure, summed after the
sheet term and before symmetry; `--write_burial` writes outdir/burial/{length}_{index}.txt as that CLI does.  The listed residues are
positions of the design, not of the motif: a motif's placement moves per particle and the targets do not follow it.

`--envelope_shape SPEC` or `--envelope_file FILE` (with `--envelope_spacing`, `--envelope_keep_frame`, `--envelope_inside_distance`,
`--envelope_inside_weight`, `--envelope_cover_distance`, `--envelope_cover_weight`, `--envelope_softness`, `--envelope_tausq` and
`--write_envelope`: the flags of add_envelope_arguments in the same module) add envelope guidance -- the design stays inside a given 3D
shape and fills it -- summed after burial and before symmetry; `--write_envelope` writes outdir/envelope/ as that CLI does.  The
envelope does not follow the motif's placement either.

`--context_pdb FILE` (with `--context_chains`, `--context_clash_distance`, `--context_clash_weight`, `--context_contact_distance`,
`--context_contacts_min`, `--context_contacts_max`, `--context_contacts_weight`, `--context_group`, `--context_tausq`, `--write_context`
and `--write_context_complex`: the flags of add_context_arguments in the same module, which this CLI alone takes) adds the one term
that does follow the motif: the C-alpha atoms of the motif's binding partner, given in the frame of the motif file's ATOM records
(typically the complex the motif was cut from), are placed for every particle by the superposition of the motif on that particle's
best placement and kept clear of, or in contact with, the rest of the design (ContextPotential, csrc/context_kernels.hip), summed
right after the motif term.  It works with either `--align`: the fit it uses is always the superposed one, so the motif needs three
residues that are not on a line.  With `--motif_groups file` the context is tied to one group, `--context_group LABEL` (required when
there is more than one).  `--write_context` writes outdir/context/{length}_{index}.txt, one `key value` line per report field, and
`--write_context_complex` outdir/context_complex/{length}_{index}.pdb: the context's chains as placed for that design, then the design
as the last chain.  The defaults are design choices whose effect on sample quality is unmeasured (no trained checkpoint is in the
tree)."""
import os

from . import capi
from .motif import load_motif_spec
from .sample_unconditional import PartialParser, UnconditionalRunner, add_common_arguments
from .sample_unconditional_shape import (GuidedRunner, add_binder_arguments, add_burial_arguments, add_context_arguments, add_diversity_arguments, add_envelope_arguments,
                                         add_fold_arguments, add_guidance_arguments, add_secstruct_arguments, add_shape_arguments, add_sheet_arguments,
                                         add_symmetry_arguments, context_constants, has_context_terms, report_fields, write_context_complex, write_context_report)


def load_motif_segments(filepath):
    """The motif entries of a problem file, in file order, as [n_i, 3] lists of C-alpha coordinates (chain, residue index from
    the ATOM records' columns 22 and 23-26, coordinates from 31-54, as features.parse_pdb reads them)."""
    ca = {}
    with open(filepath) as fh:
        for line in fh:
            if line.startswith('ATOM') and line[13:15].strip() == 'CA':
                ca[(line[21], int(line[22:26]))] = [float(line[30:38]), float(line[38:46]), float(line[46:54])]
    segments = []
    for st in load_motif_spec(filepath)['structures']:
        if st['type'] != 'motif':
            continue
        missing = [i for i in range(st['start_index'], st['end_index'] + 1) if (st['chain'], i) not in ca]
        if missing:
            raise ValueError('%s: no CA record for chain %s residue(s) %s' % (filepath, st['chain'], missing))
        segments.append([ca[(st['chain'], i)] for i in range(st['start_index'], st['end_index'] + 1)])
    if not segments:
        raise ValueError('%s: no motif segment (REMARK 999 INPUT with a chain)' % filepath)
    return segments


def load_motif_groups(filepath):
    """The motif group label of every segment load_motif_segments returns, in the same order (column 29 of REMARK 999 INPUT)."""
    return [st['group'] for st in load_motif_spec(filepath)['structures'] if st['type'] == 'motif']


def write_motif_locations(fit, directory, length, offset):
    """One file per sample of a batch (so worker processes never share one), {length}_{offset + i}.txt: the segments' `start\tend`
    lines of TwistedSampler.last_fit, then `# rmsd`; with motif groups one `# rmsd group <label>` line per group after it."""
    os.makedirs(directory, exist_ok=True)
    for i, (starts, ends, rmsd) in enumerate(zip(fit['starts'].tolist(), fit['ends'].tolist(), fit['rmsd'].tolist())):
        with open(os.path.join(directory, '{}_{}.txt'.format(length, offset + i)), 'w') as fh:
            for st, end in zip(starts, ends):
                fh.write('{}\t{}\n'.format(st, end))
            fh.write('# rmsd {:.3f}\n'.format(rmsd))
            if 'group_rmsd' in fit:
                for label, value in zip(fit['groups'], fit['group_rmsd'][i].tolist()):
                    fh.write('# rmsd group {} {:.3f}\n'.format(label, value))


def context_segments(constants):
    """The indices of the motif segments a context is tied to: all of them, or with --motif_groups file those of --context_group
    (of the only group when there is one).  A label the file does not have, a missing label with several groups, a label without
    --motif_groups file and segments a superposition cannot use (fewer than 3 residues, or all on one line) end the run here."""
    import torch
    from .smc import _check_superposable, canonical_groups
    segments, groups, label = constants['segments'], constants.get('groups'), constants.get('context_group')
    if groups is None:
        if label is not None:
            raise SystemExit('--context_group needs --motif_groups file')
        chosen = list(range(len(segments)))
    else:
        labels, index = canonical_groups(groups, len(segments))
        if label is None and len(labels) > 1:
            raise SystemExit('--context_pdb with --motif_groups file needs --context_group, one of %s' % ', '.join(map(str, labels)))
        if label is not None and label not in [str(v) for v in labels]:
            raise SystemExit('--context_group %s: the motif file has the groups %s' % (label, ', '.join(map(str, labels))))
        g = 0 if label is None else [str(v) for v in labels].index(label)
        chosen = [s for s, k in enumerate(index) if k == g]
    try:
        _check_superposable(torch.tensor([xyz for s in chosen for xyz in segments[s]], dtype=torch.float64), ' the context is tied to')
    except ValueError as e:
        raise SystemExit('--context_pdb: %s' % e) from None
    return chosen


class MotifRunner(GuidedRunner):
    def create_tasks(self, params):
        total = sum(len(s) for s in load_motif_segments(params['motif_file']))
        tasks = UnconditionalRunner.create_tasks(self, params)
        short = [t['length'] for t in tasks if t['length'] < total]
        if short:
            print('skipping lengths shorter than the {}-residue motif: {}'.format(total, ', '.join(map(str, short))))
        return self.guided_lengths([t for t in tasks if t['length'] >= total], params)

    def create_constants(self, params):
        c = super().create_constants(params)
        c.update({k: params[k] for k in ('tausq', 'max_offsets')})
        c['align'] = params.get('align', 'translation')
        c['write_motif_locations'] = bool(params.get('write_motif_locations', False))
        c['segments'] = load_motif_segments(params['motif_file'])
        c['motif_groups'] = params.get('motif_groups', 'joint')
        c['groups'] = load_motif_groups(params['motif_file']) if c['motif_groups'] == 'file' else None
        c.update(context_constants(params))
        c['context_segments'] = context_segments(c) if has_context_terms(c) else None
        return c

    def batch_potentials(self, constants, length, abar, device):
        # one MotifPotential per batch; its placements drawn from numpy's global generator, as the reference does
        from .smc import ContextPotential, MotifPotential
        motif = MotifPotential(constants['segments'], length, abar, tausq=constants['tausq'], max_offsets=constants['max_offsets'],
                               device=device, align=constants['align'], groups=constants.get('groups'))
        self.context = None                                             # (the batch's own: after_batch reports with it)
        if not has_context_terms(constants):
            return (motif,)
        anchors = [xyz for s in constants['context_segments'] for xyz in constants['segments'][s]]
        self.context = ContextPotential(length, abar, anchors, constants['context']['xyz'], motif=motif, segments=constants['context_segments'],
                                        clash_distance=constants['context_clash_distance'], clash_weight=constants['context_clash_weight'],
                                        contact_distance=constants['context_contact_distance'], contacts=constants['context_contacts'],
                                        contacts_weight=constants['context_contacts_weight'], tausq=constants['context_tausq'], device=device)
        return (motif, self.context)

    def after_batch(self, constants, sampler, length, offset):
        if constants['write_motif_locations']:
            write_motif_locations(sampler.last_fit, os.path.join(constants['outdir'], 'motif_locations'), length, offset)
        context = getattr(self, 'context', None)
        if constants.get('write_context') and context is not None:
            write_context_report(report_fields(sampler.last_shape, capi.CONTEXT_REPORT), os.path.join(constants['outdir'], 'context'), length, offset)
        if constants.get('write_context_complex') and context is not None:
            placed = context.placed_context(sampler.last_positions.to(context.device)).cpu().numpy()
            write_context_complex(sampler.last_positions.numpy(), placed, constants['context'], os.path.join(constants['outdir'], 'context_complex'),
                                  length, offset)


def build_parser():
    p = PartialParser('input_pdb', 'Structure file whose C-alpha backbone every particle starts from')
    add_common_arguments(p)
    tail = ' (not in the reference CLI)'
    p.add_argument('--motif_file', type=str, required=True,
                   help='Motif problem file (REMARK 999 format, as the scaffold CLI reads); its motif segments guide sampling' + tail)
    p.add_argument('--tausq', type=float, default=0.012, help='Motif likelihood variance tau^2' + tail)
    add_guidance_arguments(p, tail, 'guidance_alpha', 'ess_threshold', 'last_unguided_steps')
    p.add_argument('--max_offsets', type=int, default=1000,
                   help='Placements of the motif kept (a random subset when there are more)' + tail)
    add_guidance_arguments(p, tail, 'resume')
    p.add_argument('--align', type=str, choices=('translation', 'rigid'), default='translation',
                   help='Compare placements to the motif as the file orients it (translation) or after optimal superposition (rigid)')
    p.add_argument('--motif_groups', type=str, choices=('joint', 'file'), default='joint',
                   help='Treat all motif segments as one rigid motif (joint) or guide every motif group of the problem file as a body '
                        'of its own (file)')
    p.add_argument('--write_motif_locations', action='store_true',
                   help='Write outdir/motif_locations/{length}_{index}.txt: start and end residue of every motif segment in the '
                        'best-fitting placement (0-based, inclusive) and the superposed motif RMSD')
    add_guidance_arguments(p, ' (an addition to the reference CLI, like --align)', 'num_steps', 'num_particles')
    add_shape_arguments(p)
    add_secstruct_arguments(p)
    add_sheet_arguments(p)
    add_symmetry_arguments(p)
    add_binder_arguments(p)
    add_fold_arguments(p)
    add_diversity_arguments(p)
    add_burial_arguments(p)
    add_envelope_arguments(p)
    add_context_arguments(p)
    return p


def main(args):
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)


if __name__ == '__main__':
    main(build_parser().parse_args())
