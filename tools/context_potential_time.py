"""GPU tool (not a test): what one forward + gradient of the context potential costs as the fused HIP entry (ContextPotential,
csrc/context_kernels.hip) at the benchmark's shape, N = 256, B = 8, with A = 13 anchors and a context of C = 300 atoms, both terms on,
3.8 A random walks, var of schedule step 500 -- next to
  BinderPotential at M = 300 on the same designs in the same process: the same pair walk without the fit, the moments and the
  anchors' shares, so what the new kernels are measured against;
  the float32 PyTorch restatement with autograd.grad through torch.linalg.eigh (tests/_context.py) on the same device and inputs;
  the motif mode on the 6E6R motif (13 residues, 1000 placements in 256 residues, the motif CLI's default): the motif's superposed
  placement search that precedes every call there, alone and with the entry, and the motif potential's own call beside them.

    python tools/context_potential_time.py [--reps 30] [--warmup 10]     one JSON line: median ms per call (device events);
                                                                           the same line goes to profiles/context_potential_time.json

Each timing is taken after a warm-up, in batches of `batch` calls between two events (the median batch, per call): the calls queue up
faster than they run for the fused entries, so that figure is device time.  The candidates are measured alternately, `rounds` times,
and the median round is reported with the spread (min, max) beside it.

Before anything is timed the fused entry must agree with the float64 oracle on the timed inputs, to the project's bars for a fused
potential: logp within 1e-5 max(1, |logp|), every particle's gradient within 1e-5 of its largest entry, each widened to 4 x the
float32 restatement's own error where that is larger; the tool stops with an AssertionError otherwise."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


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
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'context_potential_time.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    import _binder as Bd
    import _context as Cx
    from _motif import segments_6e6r
    from genie2_amd import pack
    from genie2_amd.smc import ContextPotential, MotifPotential
    case, step, dev = (8, 256, 13, 300, 20.0, 2), 500, 'cuda:0'
    B, N, A, C = case[:4]
    abar = pack.schedule_tensors(1000)['alphas_cumprod'].to(dev)
    res = {'tool': 'context_potential_time', 'B': B, 'N': N, 'A': A, 'C': C, 'offset': case[4], 'seed': case[5], 'step': step, 'reps': args.reps,
           'warmup': args.warmup, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0)}
    x, idx, t, y, cfg = Cx.inputs(case)                           # checked: every term active, every fit well conditioned
    pot = Cx.potential(cfg, N, idx[0], t, y, abar)
    var = pot.variance(step)
    ref = Cx.reference(x, idx, t, y, cfg, float(var))
    xd, td, yd = x.to(dev).contiguous(), t.to(dev), y.to(dev)
    rows = idx.to(dev)

    # the binder potential against the same atoms where the oracle places them for particle 0: the same number of pairs
    placed = ref['placed'][0].float()
    bcfg = Bd.config(clash_distance=cfg['clash_distance'], clash_weight=1.0, contacts_min=cfg['contacts_min'], contacts_max=cfg['contacts_max'],
                     contacts_weight=1.0)
    binder = Bd.potential(bcfg, N, placed, abar)

    # the motif mode: the 6E6R motif over 1000 placements, the same context
    segs = segments_6e6r()
    motif = MotifPotential(segs, N, abar, max_offsets=1000, rng=np.random.RandomState(0), device=dev, align='rigid')
    moving = ContextPotential(N, abar, torch.cat(segs), y, motif=motif, clash_distance=cfg['clash_distance'],
                              contacts=(cfg['contacts_min'], cfg['contacts_max']), device=dev)
    res['motif_placements'] = motif.P

    def restated():
        xg = xd.detach().requires_grad_(True)
        return torch.autograd.grad(Cx.logp(xg, rows, td, yd, cfg, var).sum(), xg)

    # the fused entry agrees with the oracle on these inputs before anything is timed
    lp, g = pot._launch(xd, var)
    r32 = Cx.restatement32(xd, rows, td, yd, cfg, float(var))
    lp, g = lp.double().cpu(), g.double().cpu()
    lp_b, g_b = 1e-5 * ref['logp'].abs().clamp(min=1), 1e-5 * ref['grad'].abs().amax(dim=(1, 2))
    wide_lp = max(1.0, 4.0 * float(((r32['logp'].double().cpu() - ref['logp']).abs() / lp_b).max()))
    wide_g = max(1.0, 4.0 * float(((r32['grad'].double().cpu() - ref['grad']).abs().amax(dim=(1, 2)) / g_b).max()))
    d_lp, d_g = (lp - ref['logp']).abs() / lp_b, (g - ref['grad']).abs().amax(dim=(1, 2)) / g_b
    res['logp_error_over_bound'], res['grad_error_over_bound'] = float(d_lp.max()), float(d_g.max())
    res['bars_widened'] = [wide_lp, wide_g]
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), 'the fused entry is not finite'
    assert float(d_lp.max()) <= wide_lp, 'logp is %.3f of its bar from the oracle' % float(d_lp.max())
    assert float(d_g.max()) <= wide_g, 'the gradient is %.3f of its bar from the oracle' % float(d_g.max())

    timed = {'fused': (lambda: pot._launch(xd, var), 50), 'binder': (lambda: binder._launch(xd, var), 50), 'torch': (restated, 5),
             'motif_search': (lambda: motif._launch(xd, motif._one, fit=True), 50), 'motif_mode': (lambda: moving._launch(xd, var), 50),
             'motif_potential': (lambda: motif._launch(xd, var), 50)}
    got = {k: [] for k in timed}
    for _ in range(args.rounds):                                 # alternately: all see the same neighbours on the host
        for k, (fn, batch) in timed.items():
            got[k].append(median_ms(fn, args.reps, args.warmup, batch))
    for k, v in got.items():
        v.sort()
        res[k + '_ms'], res[k + '_ms_range'] = v[len(v) // 2], [v[0], v[-1]]
    res['fused_over_binder'] = res['fused_ms'] / res['binder_ms']
    res['torch_over_fused'] = res['torch_ms'] / res['fused_ms']
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
