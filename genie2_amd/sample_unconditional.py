"""`python -m genie2_amd.sample_unconditional` -- same flags and output layout as
the reference CLI (genie/sample_unconditional.py:132-159):
outdir/pdbs/{length}_{index}.pdb.

`--input_pdb FILE --start_step T0` (not in the reference CLI) is partial diffusion: the file's C-alpha backbone is noised to step T0
and denoised from there (the sampler module's docstring), `--num_samples` variants of it written as outdir/pdbs/{length}_{i}.pdb for
the file's one length; `--min_length`, `--max_length` and `--length_step` are then ignored.  `--write_start_rmsd` adds
outdir/start_rmsd/{length}_{i}.txt with one line, `# rmsd <C-alpha RMSD to the start after optimal superposition, Angstrom>`."""
import argparse
import os

from tqdm import tqdm

from .diffusion import load_pretrained_model
from .multiprocessor import MultiProcessor
from .sampler import UnconditionalSampler


class PartialParser(argparse.ArgumentParser):
    """An ArgumentParser whose flags `start_from` (--input_pdb or --input_dir) and --start_step come together: either without the
    other is a usage error (SystemExit), and --write_start_rmsd needs them."""

    def __init__(self, start_from, what, **kw):
        super().__init__(**kw)
        self.start_from = start_from
        self.add_argument('--' + start_from, type=str, default=None, help=what + ' (partial diffusion; not in the reference CLI)')
        self.add_argument('--start_step', type=int, default=None,
                          help='Noise the start to this timestep (1..n_timestep) and denoise from there; with --%s' % start_from)
        self.add_argument('--write_start_rmsd', action='store_true',
                          help='Write outdir/start_rmsd/{name}.txt: C-alpha RMSD of every sample to its start after optimal superposition')

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        given = getattr(ns, self.start_from) is not None
        if given != (ns.start_step is not None):
            self.error('--%s and --start_step come together: %s is missing'
                       % (self.start_from, '--start_step' if given else '--' + self.start_from))
        if ns.write_start_rmsd and not given:
            self.error('--write_start_rmsd needs --%s and --start_step' % self.start_from)
        return ns


def check_start_step_flag(params):
    """--start_step against the model's n_timestep as soon as its configuration can be read: in the parent process, before a
    checkpoint is loaded or a device touched.  A missing model directory is left to load_pretrained_model's own message."""
    if params.get('start_step') is None:
        return
    from .config import Config
    from .sampler import check_start_step
    path = os.path.join(params['rootdir'], params['name'], 'configuration')
    if os.path.exists(path):
        try:
            check_start_step(params['start_step'], Config(path).diffusion['n_timestep'])
        except ValueError as e:
            raise SystemExit('--start_step: %s' % e)


def load_backbone(filepath):
    """The C-alpha coordinates [N, 3] of a structure file, all chains in file order (features.parse_pdb)."""
    import numpy as np
    from .features import parse_pdb
    _, coords = parse_pdb(filepath)
    if not coords:
        raise SystemExit('%s: no C-alpha ATOM record' % filepath)
    return np.concatenate(coords).astype(float)


def write_start_rmsd(rmsd, directory, names):
    """One file per sample, {name}.txt with the line `# rmsd <%.3f>` (BaseSampler.last_start_rmsd of the batch)."""
    os.makedirs(directory, exist_ok=True)
    for name, value in zip(names, rmsd.tolist()):
        with open(os.path.join(directory, name + '.txt'), 'w') as fh:
            fh.write('# rmsd {:.3f}\n'.format(value))


class UnconditionalRunner(MultiProcessor):
    def create_tasks(self, params):
        if params.get('input_pdb') is not None:
            length = len(load_backbone(params['input_pdb']))
            print('--input_pdb: one length, {} residues; --min_length, --max_length and --length_step are ignored'.format(length))
            return [{'length': length}]
        # downward from max_length (sample_unconditional.py:33-44)
        return [{'length': length}
                for length in range(params['max_length'], params['min_length'] - 1, -params['length_step'])]

    def create_constants(self, params):
        check_start_step_flag(params)
        c = {k: params.get(k) for k in ('rootdir', 'name', 'epoch', 'scale', 'outdir', 'num_samples', 'batch_size', 'resume',
                                          'num_steps', 'sampler', 'eta')}
        if params.get('input_pdb') is not None:
            c.update(init_structure=load_backbone(params['input_pdb']), start_step=params['start_step'],
                     write_start_rmsd=bool(params.get('write_start_rmsd')))
        return c

    @staticmethod
    def partial_params(constants):
        """The sampler params of partial diffusion, when asked for."""
        return {k: constants[k] for k in ('init_structure', 'start_step') if constants.get(k) is not None}

    def load_model(self, constants, device):
        return load_pretrained_model(constants['rootdir'], constants['name'], constants['epoch']).eval().to(device)

    @staticmethod
    def batches(constants, outdir, prefix):
        """(batch, offset) of every sampler call that constants['num_samples'] in batches of constants['batch_size'] need; with
        constants['resume'] without the batches whose outdir/pdbs/{prefix}_{offset + i}.pdb all exist (written by an earlier,
        interrupted run)."""
        remaining = constants['num_samples']
        while remaining > 0:
            batch = min(constants['batch_size'], remaining)
            offset = constants['num_samples'] - remaining
            remaining -= batch
            if not (constants.get('resume') and all(os.path.exists(os.path.join(outdir, 'pdbs', '{}_{}.pdb'.format(prefix, offset + i)))
                                                    for i in range(batch))):
                yield batch, offset

    def execute(self, constants, tasks, device):
        sampler = UnconditionalSampler(self.load_model(constants, device))
        for task in tqdm(tasks, desc=device):
            for batch, offset in self.batches(constants, constants['outdir'], task['length']):
                sampler.sample({
                    'length': task['length'], 'scale': constants['scale'], 'num_samples': batch,
                    'outdir': constants['outdir'], 'prefix': str(task['length']), 'offset': offset,
                    'num_steps': constants.get('num_steps'), 'sampler': constants.get('sampler'), 'eta': constants.get('eta'),
                    **self.partial_params(constants)})
                if constants.get('write_start_rmsd'):
                    write_start_rmsd(sampler.last_start_rmsd, os.path.join(constants['outdir'], 'start_rmsd'),
                                     ['{}_{}'.format(task['length'], offset + i) for i in range(batch)])


def add_common_arguments(p):
    """The model, output and length flags every sampling CLI of the package shares."""
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


def build_parser():
    p = PartialParser('input_pdb', 'Structure file whose C-alpha backbone every sample starts from')
    add_common_arguments(p)
    p.add_argument('--resume', action='store_true', help='Skip batches whose PDB files already exist (not in the reference CLI)')
    p.add_argument('--num_steps', type=int, default=None,
                   help='Run the reverse process on this many of the n_timestep steps; default: all (not in the reference CLI)')
    p.add_argument('--sampler', type=str, choices=('ancestral', 'ddim'), default=None,
                   help='Reverse step used with --num_steps; default: ancestral (not in the reference CLI)')
    p.add_argument('--eta', type=float, default=None,
                   help='DDIM noise level in [0, 1], 0 = deterministic; with --sampler ddim only (not in the reference CLI)')
    return p


def main(args):
    UnconditionalRunner().run(vars(args), args.num_devices, args.sequential_order)


if __name__ == '__main__':
    main(build_parser().parse_args())
