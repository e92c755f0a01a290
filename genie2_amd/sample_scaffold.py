"""`python -m genie2_amd.sample_scaffold` -- same flags and output layout as the reference CLI
(genie/sample_scaffold.py): outdir/motif=<name>/{pdbs,motif_pdbs}/<name>_<index>.pdb.

`--input_dir DIR --start_step T0` (not in the reference CLI) re-scaffolds a previous run's designs by partial diffusion: DIR is that
run's outdir (its motif=<name> folders, or one of them); for every pdbs/X.pdb that has a motif_pdbs/X.pdb the design is noised to
step T0 and denoised under the conditioning features it was generated with (features.create_np_features_from_design), and
`--num_samples` variants are written as outdir/motif=<name>/{pdbs,motif_pdbs}/X_{i}.pdb.  The problem file is
<datadir>/<name>.pdb with <name> = X without its trailing _<index>, the reference's naming.  `--write_start_rmsd` adds
outdir/motif=<name>/start_rmsd/X_{i}.txt with the line `# rmsd <C-alpha RMSD to the design after optimal superposition, Angstrom>`."""
import glob
import os

from tqdm import tqdm

from .diffusion import load_pretrained_model
from .multiprocessor import MultiProcessor
from .sample_unconditional import PartialParser, UnconditionalRunner, check_start_step_flag, write_start_rmsd
from .sampler import ScaffoldSampler


def pair_designs(input_dir):
    """The designs of a previous scaffold run: [(X, pdbs/X.pdb, motif_pdbs/X.pdb)] sorted by X, over `input_dir` itself and its
    motif=* folders.  A pdbs/X.pdb without its motif_pdbs/X.pdb cannot be re-scaffolded: it is skipped, with a notice."""
    found = []
    for base in [input_dir] + sorted(glob.glob(os.path.join(input_dir, 'motif=*'))):
        for design in sorted(glob.glob(os.path.join(base, 'pdbs', '*.pdb'))):
            x = os.path.basename(design)[:-len('.pdb')]
            motif = os.path.join(base, 'motif_pdbs', x + '.pdb')
            if os.path.exists(motif):
                found.append((x, design, motif))
            else:
                print('skipping {}: no {}'.format(design, motif))
    return found


class ScaffoldRunner(MultiProcessor):
    def create_tasks(self, params):
        if params.get('input_dir') is not None:
            # (X = <motif name>_<index>, sample_scaffold.py's own naming)
            return [{'motif_name': x.rsplit('_', 1)[0], 'design': x, 'design_filepath': d, 'motif_filepath': m}
                    for x, d, m in pair_designs(params['input_dir'])
                    if params.get('motif_name') is None or x.rsplit('_', 1)[0] == params['motif_name']]
        # (the reference reads the global `args` here, sample_scaffold.py:34-49; same values)
        if params.get('motif_name') is not None:
            names = [params['motif_name']]
        else:
            names = [p.split('/')[-1].split('.')[0] for p in glob.glob(os.path.join(params['datadir'], '*.pdb'))]
        return [{'motif_name': n} for n in names]

    def create_constants(self, params):
        c = {k: params[k] for k in ('rootdir', 'name', 'epoch', 'scale', 'strength', 'outdir', 'num_samples',
                                    'batch_size', 'datadir')}
        c.update({k: params[k] for k in ('num_steps', 'sampler', 'eta') if params.get(k) is not None})      # few-step sampling, when asked for
        check_start_step_flag(params)
        if params.get('input_dir') is not None:
            c.update(start_step=params['start_step'], write_start_rmsd=bool(params.get('write_start_rmsd')))
        return c

    def load_model(self, constants, device):
        return load_pretrained_model(constants['rootdir'], constants['name'], constants['epoch']).eval().to(device)

    def execute(self, constants, tasks, device):
        sampler = ScaffoldSampler(self.load_model(constants, device))
        for task in tqdm(tasks, desc=device):
            outdir = os.path.join(constants['outdir'], 'motif={}'.format(task['motif_name']))
            prefix = task.get('design', task['motif_name'])
            for batch, offset in UnconditionalRunner.batches(constants, outdir, prefix):      # (no --resume here: every batch)
                partial = {} if 'design' not in task else {'design_filepath': task['design_filepath'], 'motif_filepath': task['motif_filepath'],
                                                           'start_step': constants['start_step']}
                sampler.sample({
                    'filepath': os.path.join(constants['datadir'], '{}.pdb'.format(task['motif_name'])),
                    'scale': constants['scale'], 'strength': constants['strength'], 'num_samples': batch,
                    'outdir': outdir, 'prefix': prefix, 'offset': offset,
                    'num_steps': constants.get('num_steps'), 'sampler': constants.get('sampler'), 'eta': constants.get('eta'), **partial})
                if partial and constants.get('write_start_rmsd'):
                    write_start_rmsd(sampler.last_start_rmsd, os.path.join(outdir, 'start_rmsd'),
                                     ['{}_{}'.format(prefix, offset + i) for i in range(batch)])


def build_parser():
    p = PartialParser('input_dir', 'Outdir of a previous scaffold run whose designs are re-scaffolded')
    p.add_argument('--name', type=str, help='Model name', required=True)
    p.add_argument('--epoch', type=int, help='Model epoch', required=True)
    p.add_argument('--rootdir', type=str, help='Root directory', default='results')
    p.add_argument('--scale', type=float, help='Sampling noise scale', required=True)
    p.add_argument('--outdir', type=str, help='Output directory', required=True)
    p.add_argument('--strength', type=float, help='Sampling classifier-free strength', default=0)
    p.add_argument('--num_samples', type=int, help='Number of samples per length', default=100)
    p.add_argument('--batch_size', type=int, help='Batch size', default=4)
    p.add_argument('--motif_name', type=str, help='Motif name', default=None)
    p.add_argument('--datadir', type=str, help='Data directory', default='data/design25')
    p.add_argument('--num_devices', type=int, help='Number of GPU devices', default=1)
    p.add_argument('--num_steps', type=int, default=None,
                   help='Run the reverse process on this many of the n_timestep steps; default: all (not in the reference CLI)')
    p.add_argument('--sampler', type=str, choices=('ancestral', 'ddim'), default=None,
                   help='Reverse step used with --num_steps; default: ancestral (not in the reference CLI)')
    p.add_argument('--eta', type=float, default=None,
                   help='DDIM noise level in [0, 1], 0 = deterministic; with --sampler ddim only (not in the reference CLI)')
    return p


def main(args):
    ScaffoldRunner().run(vars(args), args.num_devices)


if __name__ == '__main__':
    main(build_parser().parse_args())
