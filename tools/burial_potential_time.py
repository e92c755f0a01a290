"""GPU tool (not a test): what one forward + gradient of the burial potential costs as the fused HIP entry (BurialPotential,
csrc/burial_kernels.hip) and as its float32 PyTorch restatement with autograd.grad (tests/_burial.py) on the same device and inputs:
N = 256 at B = 8 and B = 128, targets on a third of the residues and the mean term on (tests/_burial.walk_config), 3.8 A random
walks, var of schedule step 500.

    python tools/burial_potential_time.py [--reps 30] [--warmup 10]     one JSON line: median ms per call (device events) per shape;
                                                                          the same line goes to profiles/burial_potential_time.json

Each timing is taken after a warm-up, in batches of `batch` calls between two events (the median batch, per call): the calls queue up
faster than they run for the fused entry, so that figure is device time; the restatement's dozens of launches over [B, N, N] tensors
are what a user of it pays inside the sampling loop.  The two are measured alternately, `rounds` times, and the median round is
reported with the spread (min, max) beside it.

Before either is timed the two must agree on the timed inputs, to the project's bars for a fused potential: logp within 1e-5
max(1, |logp|), every particle's gradient within 1e-5 of its largest entry; the tool stops with an AssertionError otherwise."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = ((8, 256), (128, 256))


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


def measure(B, N, args, abar, dev, step=500):
    import torch
    import _burial as Bu
    from _motif import walk
    x = walk(B, N, 100 * N + B)
    cfg = Bu.walk_config(x, N)
    x = x.to(dev).contiguous()
    pot = Bu.potential(cfg, N, abar)
    var = pot.variance(step)

    def fused():
        pot._launch(x, var)                                      # logp and gradient, as BurialPotential's forward takes them

    def restated():
        xg = x.detach().requires_grad_(True)
        torch.autograd.grad(Bu.logp(xg, cfg, var).sum(), xg)

    # the two agree on these inputs before either is timed
    lp, g = pot._launch(x, var)
    xg = x.detach().requires_grad_(True)
    lp_t = Bu.logp(xg, cfg, var)
    g_t, = torch.autograd.grad(lp_t.sum(), xg)
    lp_t = lp_t.detach()
    d_lp = (lp - lp_t).abs() / lp_t.abs().clamp(min=1)
    d_g = (g - g_t).abs().amax(dim=(1, 2)) / g_t.abs().amax(dim=(1, 2))
    res = {'B': B, 'N': N, 'targets': len(cfg['targets']), 'logp_rel_diff': float(d_lp.max()), 'grad_rel_diff': float(d_g.max())}
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), 'the fused entry is not finite'
    assert float(lp_t.abs().min()) > 0, 'a particle of the timed input has no energy'
    assert float(d_lp.max()) <= 1e-5, 'logp differs by %.3e of max(1, |logp|) from the restatement' % float(d_lp.max())
    assert float(d_g.max()) <= 1e-5, "the gradient differs by %.3e of a particle's largest entry" % float(d_g.max())

    f, t = [], []
    for _ in range(args.rounds):                                 # alternately: both see the same neighbours on the host
        f.append(median_ms(fused, args.reps, args.warmup, 50))
        t.append(median_ms(restated, args.reps, args.warmup, 5))
    f.sort()
    t.sort()
    res['fused_ms'], res['fused_ms_range'] = f[len(f) // 2], [f[0], f[-1]]
    res['torch_ms'], res['torch_ms_range'] = t[len(t) // 2], [t[0], t[-1]]
    res['torch_over_fused'] = res['torch_ms'] / res['fused_ms']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'burial_potential_time.json'))
    args = ap.parse_args()
    import torch
    from genie2_amd import pack
    dev = 'cuda:0'
    abar = pack.schedule_tensors(1000)['alphas_cumprod'].to(dev)
    res = {'tool': 'burial_potential_time', 'step': 500, 'reps': args.reps, 'warmup': args.warmup, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(0), 'shapes': [measure(B, N, args, abar, dev) for B, N in SHAPES]}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
