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
other than the blueprint's are skipped."""
import os

from tqdm import tqdm

from .diffusion import load_pretrained_model
from .motif import load_motif_spec
from .sample_unconditional import PartialParser, UnconditionalRunner, write_start_rmsd
from .sample_unconditional_shape import (add_secstruct_arguments, add_shape_arguments, report_fields, restrained_lengths,
                                         secstruct_constants, secstruct_potential, shape_constants, shape_potential, sum_potentials,
                                         target_lengths, write_secstruct_report, write_shape_report)


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


class MotifRunner(UnconditionalRunner):
    def create_tasks(self, params):
        total = sum(len(s) for s in load_motif_segments(params['motif_file']))
        tasks = super().create_tasks(params)
        short = [t['length'] for t in tasks if t['length'] < total]
        if short:
            print('skipping lengths shorter than the {}-residue motif: {}'.format(total, ', '.join(map(str, short))))
        tasks = [t for t in tasks if t['length'] >= total]
        return target_lengths(restrained_lengths(tasks, shape_constants(params)['restraints']), secstruct_constants(params)['ss_target'])

    def create_constants(self, params):
        c = super().create_constants(params)
        c.update({k: params[k] for k in ('tausq', 'guidance_alpha', 'ess_threshold', 'last_unguided_steps', 'max_offsets')})
        c['align'] = params.get('align', 'translation')
        c['write_motif_locations'] = bool(params.get('write_motif_locations', False))
        c['segments'] = load_motif_segments(params['motif_file'])
        c['motif_groups'] = params.get('motif_groups', 'joint')
        c['groups'] = load_motif_groups(params['motif_file']) if c['motif_groups'] == 'file' else None
        c['num_particles'] = params.get('num_particles')
        c.update(shape_constants(params))
        c.update(secstruct_constants(params))
        return c

    def execute(self, constants, tasks, device):
        from . import capi, pack
        from .smc import MotifPotential, TwistedSampler
        model = load_pretrained_model(constants['rootdir'], constants['name'], constants['epoch']).eval().to(device)
        sampler = TwistedSampler(model)
        abar = pack.schedule_tensors(model.config.diffusion['n_timestep'])['alphas_cumprod'].to(device)
        for task in tqdm(tasks, desc=device):
            shape = shape_potential(constants, task['length'], abar, device)
            secstruct = secstruct_potential(constants, task['length'], abar, device)
            remaining = constants['num_samples']
            while remaining > 0:
                batch = min(constants['batch_size'], remaining)
                offset = constants['num_samples'] - remaining
                if constants.get('resume') and all(
                        os.path.exists(os.path.join(constants['outdir'], 'pdbs', '{}_{}.pdb'.format(task['length'], offset + i)))
                        for i in range(batch)):
                    remaining -= batch           # this batch was written by an earlier (interrupted) run
                    continue
                # one particle system per batch; its placements drawn from numpy's global generator, as the reference does
                potential = MotifPotential(constants['segments'], task['length'], abar, tausq=constants['tausq'],
                                           max_offsets=constants['max_offsets'], device=device, align=constants['align'],
                                           groups=constants.get('groups'))
                potential = sum_potentials(potential, shape, secstruct)
                # (with --num_particles: `batch` systems, each returning its best particle)
                systems = {} if constants.get('num_particles') is None else {'num_particles': constants['num_particles'],
                                                                             'return_particles': 'best'}
                sampler.sample({
                    'length': task['length'], 'scale': constants['scale'], 'num_samples': batch,
                    'outdir': constants['outdir'], 'prefix': str(task['length']), 'offset': offset,
                    'twisting_function': potential, 'guidance_alpha': constants['guidance_alpha'],
                    'ess_threshold': constants['ess_threshold'], 'last_unguided_steps': constants['last_unguided_steps'],
                    'num_steps': constants.get('num_steps'), **systems, **self.partial_params(constants)})
                if constants.get('write_start_rmsd'):
                    write_start_rmsd(sampler.last_start_rmsd, os.path.join(constants['outdir'], 'start_rmsd'),
                                     ['{}_{}'.format(task['length'], offset + i) for i in range(batch)])
                if constants['write_motif_locations']:
                    write_motif_locations(sampler.last_fit, os.path.join(constants['outdir'], 'motif_locations'), task['length'], offset)
                if constants['write_shape_report'] and shape is not None:
                    write_shape_report(report_fields(sampler.last_shape, capi.SHAPE_REPORT), os.path.join(constants['outdir'], 'shape'),
                                       task['length'], offset)
                if constants['write_secstruct'] and secstruct is not None:
                    write_secstruct_report(sampler.last_secstruct, report_fields(sampler.last_shape, capi.SECSTRUCT_REPORT),
                                           os.path.join(constants['outdir'], 'secstruct'), task['length'], offset)
                remaining -= batch


def build_parser():
    p = PartialParser('input_pdb', 'Structure file whose C-alpha backbone every particle starts from')
    p.add_argument('--name', type=str, help='Model name', required=True)
    p.add_argument('--epoch', type=int, help='Model epoch', required=True)
    p.add_argument('--rootdir', type=str, help='Root directory', default='results')
    p.add_argument('--scale', type=float, help='Sampling noise scale', required=True)
    p.add_argument('--outdir', type=str, help='Output directory', required=True)
    p.add_argument('--num_samples', type=int, help='Number of samples per length', default=5)
    p.add_argument('--batch_size', type=int, help='Batch size', default=4)
    p.add_argument('--min_length', type=int, help='Minimum sequence length', default=50)
    p.add_argument('--max_length', type=int, help='Maximum sequence length', default=256)
    p.add_argument('--length_step', type=int, help='Length step size', default=1)
    p.add_argument('--num_devices', type=int, help='Number of GPU devices', default=1)
    p.add_argument('--sequential_order', action='store_true', help='Run in increasing order of length')
    p.add_argument('--motif_file', type=str, required=True,
                   help='Motif problem file (REMARK 999 format, as the scaffold CLI reads); its motif segments guide sampling '
                        '(not in the reference CLI)')
    p.add_argument('--tausq', type=float, default=0.012, help='Motif likelihood variance tau^2 (not in the reference CLI)')
    p.add_argument('--guidance_alpha', type=float, default=0.012, help='Guidance gradient regulariser alpha (not in the reference CLI)')
    p.add_argument('--ess_threshold', type=float, default=0.5,
                   help='Resample when the effective sample size falls below this fraction of the batch (not in the reference CLI)')
    p.add_argument('--last_unguided_steps', type=int, default=50,
                   help='Steps below this one are not guided (not in the reference CLI)')
    p.add_argument('--max_offsets', type=int, default=1000,
                   help='Placements of the motif kept (a random subset when there are more) (not in the reference CLI)')
    p.add_argument('--resume', action='store_true', help='Skip batches whose PDB files already exist (not in the reference CLI)')
    p.add_argument('--align', type=str, choices=('translation', 'rigid'), default='translation',
                   help='Compare placements to the motif as the file orients it (translation) or after optimal superposition (rigid)')
    p.add_argument('--motif_groups', type=str, choices=('joint', 'file'), default='joint',
                   help='Treat all motif segments as one rigid motif (joint) or guide every motif group of the problem file as a body '
                        'of its own (file)')
    p.add_argument('--write_motif_locations', action='store_true',
                   help='Write outdir/motif_locations/{length}_{index}.txt: start and end residue of every motif segment in the '
                        'best-fitting placement (0-based, inclusive) and the superposed motif RMSD')
    p.add_argument('--num_steps', type=int, default=None,
                   help='Run the reverse process on this many of the n_timestep steps, with the ancestral kernel between them; default: all '
                        '(an addition to the reference CLI, like --align)')
    p.add_argument('--num_particles', type=int, default=None,
                   help='Guide every design as a particle system of its own with this many particles (1..64) and write its best '
                        'particle: --num_samples and --batch_size then count designs; default: one system per batch, every particle '
                        'written (an addition to the reference CLI, like --align)')
    add_shape_arguments(p)
    add_secstruct_arguments(p)
    return p


def main(args):
    MotifRunner().run(vars(args), args.num_devices, args.sequential_order)


if __name__ == '__main__':
    main(build_parser().parse_args())
