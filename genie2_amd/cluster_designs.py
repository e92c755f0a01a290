"""python genie/cluster_designs.py --indir out [--outdir out/diversity] [--tm_threshold 0.6] [--linkage single|leader]
       [--norm shorter|longer] [--n_iter 16] [--same_length_only] [--write_matrix] [--device cuda:0]
       [--align gapless|gapped] [--n_rounds 8] [--gap_open -0.6]

How many of the designs a sampler wrote are different: reads <indir>/pdbs/*.pdb (or <indir>/*.pdb where there is no pdbs folder),
scores every pair with the HIP entry (similarity.PairwiseTM: the project's gapless TM-score, a lower bound of TM-align's), clusters
the matrix on the host and writes <outdir>/clusters.txt:

    # designs 100            '# key value' lines: designs, threshold, norm, linkage, n_iter, clusters, diversity, mean_tm, max_tm
    ...
    name length cluster representative nearest nearest_tm        one line per design, in file-name order; TM values as %.3f

`representative` is the name of the design that stands for the cluster, `nearest` the most similar other design ('-' where no other
design was scored against it).  --same_length_only scores and clusters the designs of each length on their own, one call per length,
and leaves cross-length pairs out (their tm is stored as 0); --write_matrix adds tm.npz (names, lengths, tm, rmsd, offset, scored).
--align gapped scores the pairs with the gapped alignment instead (similarity.TMAlign of the designs against themselves under --norm,
--n_rounds rounds of dynamic programming with the gap opening penalty --gap_open): designs that differ by an inserted loop or a deleted
turn then score as the relatives they are.  Both directions of a pair are lower bounds, so the matrix is their element-wise maximum
with a diagonal of 1; the header gains align, n_rounds and gap_open after its other keys, tm.npz holds n_aligned in place of offset, and
the longest design squared has to stay inside the entry's 131072 cells (362 residues).
The number of clusters at TM 0.6 under single linkage is the diversity figure Genie 2 reports; designability is not computed here."""
import argparse
import glob
import os

import numpy as np

from . import capi
from .similarity import NORMS, PairwiseTM, TMAlign, cluster_leader, cluster_single, diversity_summary, load_designs

LINKAGES = {'single': cluster_single, 'leader': cluster_leader}
HEADER = ('designs', 'threshold', 'norm', 'linkage', 'n_iter', 'clusters', 'diversity', 'mean_tm', 'max_tm')
GAPPED_HEADER = ('align', 'n_rounds', 'gap_open')       # appended under --align gapped
ALIGNS = ('gapless', 'gapped')


def build_parser():
    p = argparse.ArgumentParser(description='Cluster a folder of designs by pairwise TM-score (HIP) and report its diversity')
    p.add_argument('--indir', type=str, required=True, help='a sampler output folder (its pdbs/ is read) or a folder of .pdb files')
    p.add_argument('--outdir', type=str, default=None, help='where clusters.txt goes (default: <indir>/diversity)')
    p.add_argument('--tm_threshold', type=float, default=0.6, help='designs at or above this TM-score are linked (0 < t <= 1)')
    p.add_argument('--linkage', type=str, default='single', choices=sorted(LINKAGES))
    p.add_argument('--norm', type=str, default='shorter', choices=NORMS, help='normalising length of a pair of unequal lengths')
    p.add_argument('--n_iter', type=int, default=16, help='ascent steps per seed, 1..%d' % capi.TM_MAX_ITER)
    p.add_argument('--same_length_only', action='store_true', help='cluster each length on its own; cross-length pairs are skipped')
    p.add_argument('--write_matrix', action='store_true', help='also write tm.npz')
    p.add_argument('--device', type=str, default='cuda:0')
    p.add_argument('--align', type=str, default='gapless', choices=ALIGNS, help='gapless threading, or dynamic programming (gapped)')
    p.add_argument('--n_rounds', type=int, default=8, help='--align gapped: rounds of dynamic programming, 0..%d' % capi.TMALIGN_MAX_ROUNDS)
    p.add_argument('--gap_open', type=float, default=-0.6, help='--align gapped: gap opening penalty, -10..0')
    return p


def check_args(args):
    """The parser's values that argparse cannot judge: SystemExit with a message."""
    if not (args.tm_threshold > 0.0 and args.tm_threshold <= 1.0):
        raise SystemExit('--tm_threshold must be above 0 and at most 1, got %r' % (args.tm_threshold,))
    if not 1 <= args.n_iter <= capi.TM_MAX_ITER:
        raise SystemExit('--n_iter must be in 1..%d, got %d' % (capi.TM_MAX_ITER, args.n_iter))
    if getattr(args, 'align', 'gapless') == 'gapped':
        if not 0 <= args.n_rounds <= capi.TMALIGN_MAX_ROUNDS:
            raise SystemExit('--n_rounds must be in 0..%d, got %d' % (capi.TMALIGN_MAX_ROUNDS, args.n_rounds))
        if not -10.0 <= args.gap_open <= 0.0:
            raise SystemExit('--gap_open must be in -10..0, got %r' % (args.gap_open,))


def design_files(indir):
    """The .pdb files of a run, sorted by name: <indir>/pdbs/*.pdb where that folder exists, else <indir>/*.pdb."""
    if not os.path.isdir(indir):
        raise SystemExit('%s is not a directory' % indir)
    sub = os.path.join(indir, 'pdbs')
    files = sorted(glob.glob(os.path.join(sub if os.path.isdir(sub) else indir, '*.pdb')))
    if not files:
        raise SystemExit('no .pdb files in %s' % (sub if os.path.isdir(sub) else indir))
    return files


def symmetrise(out):
    """The gapped scores of a set against itself as a symmetric matrix: per pair the direction with the higher tm (both are lower
    bounds; ties to the upper triangle) gives tm, rmsd and n_aligned, and the diagonal is (1, 0, the length)."""
    tm = out['tm']
    take = (tm.T > tm) | ((tm.T == tm) & np.tril(np.ones(tm.shape, dtype=bool), -1))
    sym = {k: np.where(take, out[k].T, out[k]) for k in ('tm', 'rmsd', 'n_aligned')}
    np.fill_diagonal(sym['tm'], 1.0)
    np.fill_diagonal(sym['rmsd'], 0.0)
    return sym


def score_gapped(x, lengths, args):
    """score() under --align gapped: {'tm', 'rmsd', 'n_aligned'}."""
    if max(lengths) ** 2 > capi.TMALIGN_MAX_CELLS:
        raise SystemExit('--align gapped: the longest design has %d residues, and its square is above the %d cells of one call'
                         % (max(lengths), capi.TMALIGN_MAX_CELLS))
    entry = TMAlign(args.device)
    kw = dict(norm=args.norm, n_iter=args.n_iter, n_rounds=args.n_rounds, gap_open=args.gap_open)
    M = len(lengths)
    if not args.same_length_only:
        out = entry(x, lengths, x, lengths, **kw)
        return symmetrise({k: v.cpu().numpy() for k, v in out.items()}), np.ones((M, M), dtype=bool)
    out = {'tm': np.zeros((M, M), dtype=np.float32), 'rmsd': np.zeros((M, M), dtype=np.float32), 'n_aligned': np.zeros((M, M), dtype=np.int32)}
    scored = np.zeros((M, M), dtype=bool)
    for L in sorted(set(lengths)):
        idx = np.array([m for m, v in enumerate(lengths) if v == L])
        part = symmetrise({k: v.cpu().numpy() for k, v in entry(x[idx, :L], None, x[idx, :L], None, **kw).items()})
        for k, v in part.items():
            out[k][np.ix_(idx, idx)] = v
        scored[np.ix_(idx, idx)] = True
    return out, scored


def score(x, lengths, args):
    """({'tm', 'rmsd', 'offset'} as numpy [M, M], scored bool [M, M]): all pairs in one call, or one call per length with
    --same_length_only (cross-length pairs are left at tm 0, rmsd 0, offset 0 and marked unscored)."""
    if getattr(args, 'align', 'gapless') == 'gapped':
        return score_gapped(x, lengths, args)
    entry = PairwiseTM(args.device)
    M = len(lengths)
    if not args.same_length_only:
        out = entry(x, lengths, norm=args.norm, n_iter=args.n_iter)
        return {k: v.cpu().numpy() for k, v in out.items()}, np.ones((M, M), dtype=bool)
    out = {'tm': np.zeros((M, M), dtype=np.float32), 'rmsd': np.zeros((M, M), dtype=np.float32), 'offset': np.zeros((M, M), dtype=np.int32)}
    scored = np.zeros((M, M), dtype=bool)
    for L in sorted(set(lengths)):
        idx = np.array([m for m, v in enumerate(lengths) if v == L])
        part = entry(x[idx, :L], None, norm=args.norm, n_iter=args.n_iter)
        for k, v in part.items():
            out[k][np.ix_(idx, idx)] = v.cpu().numpy()
        scored[np.ix_(idx, idx)] = True
    return out, scored


def main(args):
    check_args(args)
    files = design_files(args.indir)
    x, lengths, names = load_designs(files)
    for name, L in zip(names, lengths):
        if not capi.TM_MIN_LENGTH <= L <= capi.TM_MAX_LENGTH:
            raise SystemExit('%s has %d residues: a design needs %d..%d' % (name, L, capi.TM_MIN_LENGTH, capi.TM_MAX_LENGTH))
    out, scored = score(x, lengths, args)
    labels, reps = LINKAGES[args.linkage](out['tm'], args.tm_threshold)
    summary = diversity_summary(out['tm'], labels, scored)
    outdir = args.outdir if args.outdir is not None else os.path.join(args.indir, 'diversity')
    os.makedirs(outdir, exist_ok=True)
    values = (summary['n_designs'], '%.3f' % args.tm_threshold, args.norm, args.linkage, args.n_iter, summary['n_clusters'],
              '%.3f' % summary['diversity'], '%.3f' % summary['mean_tm'], '%.3f' % summary['max_tm'])
    header = HEADER
    if args.align == 'gapped':
        header, values = HEADER + GAPPED_HEADER, values + ('gapped', args.n_rounds, '%g' % args.gap_open)
    with open(os.path.join(outdir, 'clusters.txt'), 'w') as fh:
        for k, v in zip(header, values):
            fh.write('# %s %s\n' % (k, v))
        for m, name in enumerate(names):
            near = int(summary['nearest'][m])
            fh.write('%s %d %d %s %s %.3f\n' % (name, lengths[m], labels[m], names[reps[labels[m]]], names[near] if near >= 0 else '-',
                                                 summary['nearest_tm'][m]))
    if args.write_matrix:
        np.savez(os.path.join(outdir, 'tm.npz'), names=np.array(names), lengths=np.array(lengths, dtype=np.int64), scored=scored, **out)
    print('%d designs, %d clusters at TM %.3f (%s linkage): diversity %.3f, mean TM %.3f, max TM %.3f -> %s'
          % (summary['n_designs'], summary['n_clusters'], args.tm_threshold, args.linkage, summary['diversity'], summary['mean_tm'],
             summary['max_tm'], os.path.join(outdir, 'clusters.txt')))
    return summary


if __name__ == '__main__':
    main(build_parser().parse_args())
