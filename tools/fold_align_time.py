"""GPU tool (not a test): what one forward + gradient of the aligned fold potential costs (AlignedFoldPotential,
csrc/fold_align_kernels.hip) inside a guided step, and what a stride over the gapless stage's offsets saves and loses: N = 256, B = 8,
3.8 A random walks, var of schedule step 500, at (a) R = 1, a 300-residue template, and (b) R = 64 references of 200..400 residues
(indel relatives of the designs and unrelated walks, tests/_fold_align.py: references, bounds_of), each at offset_stride 1 and 4.

    python tools/fold_align_time.py [--reps 10] [--warmup 3]     one JSON line: median ms per call (device events) per case and stride;
                                                                   the same line goes to profiles/fold_align_time.json

The protocol is tools/fold_potential_time.py's: each timing is taken after a warm-up, in batches of `batch` calls between two events
(the median batch, per call; the calls queue up faster than they run, so the figure is device time), `rounds` times with the strides
alternating, and the median round is reported with the spread (min, max) beside it.  `guided_step_ms` repeats the 88 ms of one guided
step at N = 256, B = 8 so that a reader sees beside it what the potential adds to a step.  For stride 4 against
stride 1 the largest and the mean drop of `tm_of` over the pairs are reported, and the number of pairs whose map changed.

Before anything is timed the entry must agree with the float64 oracle started from its own alignment (the certificate of
tests/test_fold_align_gpu.py, coarsely: no restatement widens a bar here): every TM-score within 2e-5, logp within 1e-4 max(1, |logp|),
every particle's gradient within 1e-3 of its largest entry; the tool stops with an AssertionError otherwise.  No time is a pass
condition."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

GUIDED_STEP_MS = 88.0       # one guided step (denoiser forward + VJP + potential) at N = 256, B = 8


def median_ms(fn, reps, warmup, batch):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'fold_align_time.json'))
    args = ap.parse_args()
    import torch
    import _fold_align as Fa
    from genie2_amd import pack
    from genie2_amd.smc import AlignedFoldPotential
    B, N, step, dev = 8, 256, 500, 'cuda:0'
    abar = pack.schedule_tensors(1000)['alphas_cumprod'].to(dev)
    res = {'tool': 'fold_align_time', 'B': B, 'N': N, 'n_iter': 16, 'n_rounds': 8, 'norm': 'query', 'step': step, 'reps': args.reps,
           'warmup': args.warmup, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0), 'guided_step_ms': GUIDED_STEP_MS}
    designs = Fa.particles(B, N)
    x = designs.to(dev).contiguous()
    cases = {'a_R1_L300': [300], 'b_R64_L200_400': [200 + (200 * r) // 63 for r in range(64)]}
    for key, lengths in cases.items():
        refs, bounds = Fa.references(designs, lengths), Fa.bounds_of(len(lengths))
        pots = {s: AlignedFoldPotential(N, abar, refs, bounds, offset_stride=s, device=dev) for s in (1, 4)}
        var = pots[1].variance(step)
        res[key] = {'R': len(lengths), 'lengths': [min(lengths), max(lengths)]}
        found = {}
        for s, pot in pots.items():
            # the entry agrees with the oracle started from its own alignment before it is timed
            lp, g = pot._launch(x, var)
            al = found[s] = pot.alignment_of(x)
            r64 = Fa.evaluate(designs, refs, bounds, float(var), al['map'].cpu(), al['rot0'].cpu().double(), al['trans0'].cpu().double())
            d_tm = (al['tm'].cpu().double() - r64['tm']).abs()
            d_lp = (lp.cpu().double() - r64['logp']).abs() / r64['logp'].abs().clamp(min=1)
            d_g = (g.cpu().double() - r64['grad']).abs().amax(dim=(1, 2)) / r64['grad'].abs().amax(dim=(1, 2)).clamp(min=1e-30)
            res[key]['stride%d' % s] = {'tm_diff': float(d_tm.max()), 'logp_rel_diff': float(d_lp.max()), 'grad_rel_diff': float(d_g.max()),
                                        'guided_particles': int((r64['logp'] != 0).sum())}
            assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), 'the entry is not finite'
            assert float(lp.abs().max()) > 0 and float(g.abs().max()) > 0, 'no hinge is active on the timed inputs'
            assert float(d_tm.max()) <= 2e-5, 'a TM-score differs by %.3e from the oracle' % float(d_tm.max())
            assert float(d_lp.max()) <= 1e-4, 'logp differs by %.3e of max(1, |logp|) from the oracle' % float(d_lp.max())
            assert float(d_g.max()) <= 1e-3, "the gradient differs by %.3e of a particle's largest entry" % float(d_g.max())
        drop = (found[1]['tm'] - found[4]['tm']).double()
        res[key]['stride4_tm_drop_max'], res[key]['stride4_tm_drop_mean'] = float(drop.max()), float(drop.mean())
        res[key]['stride4_maps_changed'] = int((found[1]['map'] != found[4]['map']).any(dim=2).sum())
        times = {s: [] for s in pots}
        for _ in range(args.rounds):                             # alternately: both see the same neighbours on the host
            for s, pot in pots.items():
                times[s].append(median_ms(lambda: pot._launch(x, var), args.reps, args.warmup, 5))
        for s, t in times.items():
            t.sort()
            res[key]['stride%d' % s].update(fused_ms=t[len(t) // 2], fused_ms_range=[t[0], t[-1]],
                                            fused_share_of_guided_step=t[len(t) // 2] / GUIDED_STEP_MS)
        res[key]['stride1_over_stride4'] = res[key]['stride1']['fused_ms'] / res[key]['stride4']['fused_ms']
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
