"""GPU tool (not a test): what one forward + gradient of the symmetry potential costs as the fused HIP entry (SymmetryPotential,
csrc/symmetry_kernels.hip) and as its float32 PyTorch restatement with an SVD fit and autograd.grad (tests/_symmetry.py) on the same
device and inputs: N = 256, C4 with units of 64 residues, 3.8 A random walks, var of schedule step 500, at B = 8 and B = 128.

    python tools/symmetry_potential_time.py [--reps 30] [--warmup 10]     one JSON line: median ms per call (device events)

Each timing is taken after a warm-up, in batches of `batch` calls between two events (the median batch, per call): the calls queue up
faster than they run for the fused entry, so that figure is device time; the restatement's dozens of launches and its batched SVD
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
    args = ap.parse_args()
    import torch
    import _symmetry as S
    from _motif import walk
    from genie2_amd.smc import SymmetryPotential
    from genie2_amd import pack
    N, step, dev = 256, 500, 'cuda:0'
    abar = pack.schedule_tensors(1000)['alphas_cumprod'].to(dev)
    res = {'tool': 'symmetry_potential_time', 'symmetry': 'C4', 'unit_length': 64, 'N': N, 'step': step, 'reps': args.reps, 'warmup': args.warmup, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(0)}
    for B in (8, 128):
        x = walk(B, N, 1).to(dev).contiguous()
        cfg = S.on_device(S.generators('C4', 64, N), dev)
        pot = SymmetryPotential(N, abar, symmetry='C4', unit_length=64, device=dev)
        var = pot.variance(step)

        def fused(x=x, pot=pot, var=var):
            pot._launch(x, var)                                  # logp and gradient, as SymmetryPotential's forward takes them

        def restated(x=x, cfg=cfg, var=var):
            xg = x.detach().requires_grad_(True)
            torch.autograd.grad(S.logp32(xg, cfg, var).sum(), xg)

        # the two agree on these inputs before either is timed
        lp, g = pot._launch(x, var)
        xg = x.detach().requires_grad_(True)
        lp_t = S.logp32(xg, cfg, var)
        g_t, = torch.autograd.grad(lp_t.sum(), xg)
        lp_t = lp_t.detach()
        d_lp = (lp - lp_t).abs() / lp_t.abs().clamp(min=1)
        d_g = (g - g_t).abs().amax(dim=(1, 2)) / g_t.abs().amax(dim=(1, 2))
        res['B%d_logp_rel_diff' % B], res['B%d_grad_rel_diff' % B] = float(d_lp.max()), float(d_g.max())
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), 'B = %d: the fused entry is not finite' % B
        assert float(d_lp.max()) <= 1e-5, 'B = %d: logp differs by %.3e of max(1, |logp|) from the restatement' % (B, float(d_lp.max()))
        assert float(d_g.max()) <= 1e-5, "B = %d: the gradient differs by %.3e of a particle's largest entry" % (B, float(d_g.max()))

        f, t = [], []
        for _ in range(args.rounds):                             # alternately: both see the same neighbours on the host
            f.append(median_ms(fused, args.reps, args.warmup, 50))
            t.append(median_ms(restated, args.reps, args.warmup, 5))
        f.sort()
        t.sort()
        res['B%d_fused_ms' % B], res['B%d_fused_ms_range' % B] = f[len(f) // 2], [f[0], f[-1]]
        res['B%d_torch_ms' % B], res['B%d_torch_ms_range' % B] = t[len(t) // 2], [t[0], t[-1]]
        res['B%d_torch_over_fused' % B] = res['B%d_torch_ms' % B] / res['B%d_fused_ms' % B]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
