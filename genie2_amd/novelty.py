"""python genie/novelty.py --indir out --refdir known_pdbs [--outdir out/novelty] [--tm_threshold 0.5] [--norm query] [--n_iter 16]
       [--n_rounds 8] [--gap_open -0.6] [--write_alignments] [--device cuda:0]

How many of the designs a sampler wrote are new: reads <indir>/pdbs/*.pdb (or <indir>/*.pdb where there is no pdbs folder) and every
*.pdb of --refdir, aligns every design to every reference with the HIP entry (similarity.TMAlign: the project's gapped TM alignment, a
lower bound of TM-align's score), and writes <outdir>/novelty.txt:

    # designs 100            '# key value' lines: designs, references, norm, n_iter, n_rounds, gap_open, threshold, novel, novelty,
    ...                      skipped_pairs
    name length nearest_ref ref_length tm n_aligned rmsd novel        one line per design, in file-name order; TM values as %.3f

`nearest_ref` is the reference with the highest TM-score ('-' where none was scored), `novel` is 1 when that score is below the
threshold, and novelty = novel / designs.  The references are sorted by length and scored in chunks, so that each call stays inside the
entry's limit (longest query x longest reference <= 131072 cells) with little padding; a reference too long for a design under that
limit is skipped for it and counted in skipped_pairs.  --write_alignments aligns every design to its nearest reference once more and
writes alignments/<name>.txt: the transform (rot x_design + trans ~ x_reference) and one `i j distance` line per aligned pair
(0-based residue indices)."""
import argparse
import glob
import math
import os

import numpy as np

from . import capi
from .cluster_designs import design_files
from .similarity import ALIGN_NORMS, TMAlign, align_sets, load_designs

HEADER = ('designs', 'references', 'norm', 'n_iter', 'n_rounds', 'gap_open', 'threshold', 'novel', 'novelty', 'skipped_pairs')


def build_parser():
    p = argparse.ArgumentParser(description='Novelty of a folder of designs: the highest gapped TM-score (HIP) against known structures')
    p.add_argument('--indir', type=str, required=True, help='a sampler output folder (its pdbs/ is read) or a folder of .pdb files')
    p.add_argument('--refdir', type=str, required=True, help='a folder of .pdb files: the known structures')
    p.add_argument('--outdir', type=str, default=None, help='where novelty.txt goes (default: <indir>/novelty)')
    p.add_argument('--tm_threshold', type=float, default=0.5, help='a design whose highest TM-score is below this is novel (0 < t <= 1)')
    p.add_argument('--norm', type=str, default='query', choices=ALIGN_NORMS, help='normalising length of a pair')
    p.add_argument('--n_iter', type=int, default=16, help='ascent steps per fit, 1..%d' % capi.TM_MAX_ITER)
    p.add_argument('--n_rounds', type=int, default=8, help='rounds of dynamic programming, 0..%d' % capi.TMALIGN_MAX_ROUNDS)
    p.add_argument('--gap_open', type=float, default=-0.6, help='gap opening penalty, -10..0')
    p.add_argument('--write_alignments', action='store_true', help='also write alignments/<name>.txt against the nearest reference')
    p.add_argument('--device', type=str, default='cuda:0')
    return p


def check_align_args(args):
    """The alignment's scalars that argparse cannot judge: SystemExit with a message."""
    if not 1 <= args.n_iter <= capi.TM_MAX_ITER:
        raise SystemExit('--n_iter must be in 1..%d, got %d' % (capi.TM_MAX_ITER, args.n_iter))
    if not 0 <= args.n_rounds <= capi.TMALIGN_MAX_ROUNDS:
        raise SystemExit('--n_rounds must be in 0..%d, got %d' % (capi.TMALIGN_MAX_ROUNDS, args.n_rounds))
    if not -10.0 <= args.gap_open <= 0.0:
        raise SystemExit('--gap_open must be in -10..0, got %r' % (args.gap_open,))


def check_args(args):
    if not (args.tm_threshold > 0.0 and args.tm_threshold <= 1.0):
        raise SystemExit('--tm_threshold must be above 0 and at most 1, got %r' % (args.tm_threshold,))
    check_align_args(args)


def reference_files(refdir):
    if not os.path.isdir(refdir):
        raise SystemExit('%s is not a directory' % refdir)
    files = sorted(glob.glob(os.path.join(refdir, '*.pdb')))
    if not files:
        raise SystemExit('no .pdb files in %s' % refdir)
    return files


def check_lengths(names, lengths, what):
    for name, L in zip(names, lengths):
        if not capi.TM_MIN_LENGTH <= L <= capi.TMALIGN_MAX_LENGTH:
            raise SystemExit('%s has %d residues: a %s needs %d..%d' % (name, L, what, capi.TM_MIN_LENGTH, capi.TMALIGN_MAX_LENGTH))


def nearest_references(tm, scored):
    """Per design the index of the scored reference with the highest tm (ties to the lowest index), -1 where none was scored."""
    tm, scored = np.asarray(tm, dtype=np.float64), np.asarray(scored, dtype=bool)
    if tm.ndim != 2 or tm.shape != scored.shape:
        raise ValueError('tm and scored must be [M, R] alike, got %s and %s' % (tm.shape, scored.shape))
    near = np.where(scored, tm, -np.inf).argmax(axis=1)
    return np.where(scored.any(axis=1), near, -1).astype(np.int64)


def write_report(path, names, lengths, ref_names, ref_lengths, out, scored, skipped, norm, n_iter, n_rounds, gap_open, threshold):
    """Writes novelty.txt from the [M, R] matrices of `out` ('tm', 'n_aligned', 'rmsd'); returns {'n_designs', 'n_references',
    'n_novel', 'novelty', 'skipped_pairs', 'nearest' int64 [M], 'novel' bool [M]}."""
    near = nearest_references(out['tm'], scored)
    M = len(names)
    best = np.array([float(out['tm'][m, near[m]]) if near[m] >= 0 else 0.0 for m in range(M)])
    novel = best < threshold
    values = (M, len(ref_names), norm, n_iter, n_rounds, '%g' % gap_open, '%.3f' % threshold, int(novel.sum()), '%.3f' % (novel.sum() / M),
              skipped)
    with open(path, 'w') as fh:
        for k, v in zip(HEADER, values):
            fh.write('# %s %s\n' % (k, v))
        for m, name in enumerate(names):
            r = int(near[m])
            if r < 0:
                fh.write('%s %d - 0 %.3f 0 %.3f 1\n' % (name, lengths[m], 0.0, 0.0))
            else:
                fh.write('%s %d %s %d %.3f %d %.3f %d\n' % (name, lengths[m], ref_names[r], ref_lengths[r], out['tm'][m, r],
                                                           out['n_aligned'][m, r], out['rmsd'][m, r], int(novel[m])))
    return {'n_designs': M, 'n_references': len(ref_names), 'n_novel': int(novel.sum()), 'novelty': float(novel.sum() / M),
            'skipped_pairs': int(skipped), 'nearest': near, 'novel': novel}


def write_alignment(path, name, ref_name, xq, xr, one):
    """One alignments/<name>.txt from a 1 x 1 call with return_alignment: xq [Lq, 3], xr [Lr, 3] numpy, `one` the call's dict."""
    rot = one['rot'][0, 0].double().cpu().numpy()
    trans = one['trans'][0, 0].double().cpu().numpy()
    amap = one['map'][0, 0].cpu().numpy()
    with open(path, 'w') as fh:
        fh.write('# design %s\n# reference %s\n' % (name, ref_name))
        fh.write('# tm %.6f\n# n_aligned %d\n# rmsd %.6f\n' % (float(one['tm'][0, 0]), int(one['n_aligned'][0, 0]), float(one['rmsd'][0, 0])))
        fh.write('# rot %s\n' % ' '.join('%.8f' % v for v in rot.reshape(-1)))
        fh.write('# trans %s\n' % ' '.join('%.6f' % v for v in trans))
        for i in range(len(xq)):
            j = int(amap[i])
            if j >= 0:
                fh.write('%d %d %.3f\n' % (i, j, math.sqrt(float(((rot @ xq[i] + trans - xr[j]) ** 2).sum()))))


def main(args):
    check_args(args)
    x, lengths, names = load_designs(design_files(args.indir))
    xr, ref_lengths, ref_names = load_designs(reference_files(args.refdir))
    check_lengths(names, lengths, 'design')
    check_lengths(ref_names, ref_lengths, 'reference')
    entry = TMAlign(args.device)
    kw = dict(norm=args.norm, n_iter=args.n_iter, n_rounds=args.n_rounds, gap_open=args.gap_open)
    out, scored, skipped = align_sets(entry, x, lengths, xr, ref_lengths, **kw)
    outdir = args.outdir if args.outdir is not None else os.path.join(args.indir, 'novelty')
    os.makedirs(outdir, exist_ok=True)
    summary = write_report(os.path.join(outdir, 'novelty.txt'), names, lengths, ref_names, ref_lengths, out, scored, skipped, args.norm,
                           args.n_iter, args.n_rounds, args.gap_open, args.tm_threshold)
    if args.write_alignments:
        os.makedirs(os.path.join(outdir, 'alignments'), exist_ok=True)
        for m, name in enumerate(names):
            r = int(summary['nearest'][m])
            if r < 0:
                continue
            one = entry(x[m:m + 1], [lengths[m]], xr[r:r + 1], [ref_lengths[r]], return_alignment=True, **kw)
            write_alignment(os.path.join(outdir, 'alignments', name + '.txt'), name, ref_names[r], x[m, :lengths[m]].double().numpy(),
                            xr[r, :ref_lengths[r]].double().numpy(), one)
    print('%d designs against %d references: %d novel at TM %.3f (novelty %.3f), %d pairs skipped -> %s'
          % (summary['n_designs'], summary['n_references'], summary['n_novel'], args.tm_threshold, summary['novelty'],
             summary['skipped_pairs'], os.path.join(outdir, 'novelty.txt')))
    return summary


if __name__ == '__main__':
    main(build_parser().parse_args())
