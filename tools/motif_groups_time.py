"""GPU tool (not a test): what one call of the group-wise motif potential costs beside the single-motif entries, on the same inputs:
N = 256, B = 8, the 6E6R motif (tests/golden/motif_problem_6E6R.pdb, segments of 6 and 7 residues, groups A and B) thinned to
P = 1000 placements, var of schedule step 500.

    python tools/motif_groups_time.py [--reps 50] [--warmup 20]     one JSON line: median ms per launch (device events)

Timed are the C entries themselves (forward + gradient in one launch, as MotifPotential calls them), after a warm-up, in batches of
20 launches between two events (the median batch, per launch): genie_motif_potential, genie_motif_potential_rigid, genie_motif_potential_grouped with G = 2 and
either align, and the two fits (best, rmsd and, grouped, group_rmsd without a gradient: what MotifPotential.locate launches)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MOTIF = os.path.join(ROOT, 'tests', 'golden', 'motif_problem_6E6R.pdb')


def median_ms(fn, reps, warmup, batch=20):
    """Median over `reps` event pairs of the time of `batch` back-to-back launches, per launch: the launches queue up faster than
    they run, so this is device time, not the host's cost of a call."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        for _ in range(batch):
            fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[reps // 2] / batch


def entry_call(pot, x, var, fit):
    """A zero-argument launch of the C entry `pot` uses (MotifPotential._entry), with its outputs allocated once."""
    import ctypes as C
    name, need, args, outs = pot._entry(x, var, fit)
    assert need == 0                                            # (P = 1000: every record stays in LDS, one launch per call)
    fn, null = getattr(pot.lib, name), C.c_void_p(0)

    def launch(keep=outs):
        rc = fn(*args, null, 0)
        assert rc == 0
    return launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    from genie2_amd import pack
    from genie2_amd.sample_unconditional_motif import load_motif_groups, load_motif_segments
    from genie2_amd.smc import MotifPotential
    B, N, P, step, dev = 8, 256, 1000, 500, 'cuda:0'
    abar = pack.schedule_tensors(1000)['alphas_cumprod'].to(dev)
    segs = [torch.tensor(s, dtype=torch.float32) for s in load_motif_segments(MOTIF)]
    groups = load_motif_groups(MOTIF)
    g = torch.Generator().manual_seed(0)
    v = torch.randn(B, N, 3, generator=g)
    x = torch.cumsum(3.8 * v / v.norm(dim=-1, keepdim=True), dim=1).to(dev).contiguous()
    pots = {}
    for name, kw in (('translation', {}), ('rigid', {'align': 'rigid'}), ('grouped_translation', {'groups': groups}),
                     ('grouped_rigid', {'groups': groups, 'align': 'rigid'})):
        pots[name] = MotifPotential(segs, N, abar, max_offsets=P, rng=np.random.RandomState(0), device=dev, **kw)      # the same placements
        assert pots[name].P == P
    var = pots['rigid'].variance(step)
    res = {'tool': 'motif_groups_time', 'B': B, 'N': N, 'P': P, 'G': 2, 'step': step, 'reps': args.reps, 'warmup': args.warmup,
           'motif': '6E6R (6 + 7 residues, groups A, B)', 'device': torch.cuda.get_device_name(0)}
    for name, pot in pots.items():
        res[name + '_ms'] = median_ms(entry_call(pot, x, var, False), args.reps, args.warmup)
    res['rigid_fit_ms'] = median_ms(entry_call(pots['rigid'], x, var, True), args.reps, args.warmup)
    res['grouped_fit_ms'] = median_ms(entry_call(pots['grouped_rigid'], x, var, True), args.reps, args.warmup)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
