"""GPU tool (not a test): what one forward + gradient of the shape potential costs as the fused HIP entry (ShapePotential,
csrc/shape_kernels.hip) and as its float32 PyTorch restatement with autograd.grad (tests/_shape.py) on the same device and inputs,
beside eng.denoise at the same length: N = 256, 3.8 A random walks, all three terms on (rog cap, clashes below 4 A, 40 restraints),
var of schedule step 500, at B = 128 and B = 8.  The denoiser is timed at B = 8 and at B = 32, the largest batch the test suite runs
it at; the B = 128 ratios are against four B = 32 calls.

    python tools/shape_potential_time.py [--reps 30] [--warmup 10]     one JSON line: median ms per call (device events)

Each timing is taken after a warm-up, in batches of `batch` calls between two events (the median batch, per call): the calls queue up
faster than they run for the fused entry, so that figure is device time; the restatement's dozens of small launches are bound by the
host's launch rate, which is what a user of it pays inside the sampling loop."""
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
    args = ap.parse_args()
    import torch
    import _shape as S
    from _motif import walk
    from genie2_amd import pack
    from genie2_amd.engine import GenieEngine
    from oracle import genie_oracle as O
    N, step, dev = 256, 500, 'cuda:0'
    abar = pack.schedule_tensors(1000)['alphas_cumprod'].to(dev)
    res = {'tool': 'shape_potential_time', 'N': N, 'restraints': 40, 'step': step, 'reps': args.reps, 'warmup': args.warmup,
           'device': torch.cuda.get_device_name(0)}
    dims = dict(O.BASE_DIMS)
    eng = GenieEngine(dims, O.synthetic_state_dict(dims, seed=0), dev)
    for B in (128, 8):
        x = walk(B, N, 1).to(dev).contiguous()
        cfg = S.walk_config(x.cpu(), 40, 1)
        pot = S.potential(cfg, N, abar)
        var = pot.variance(step)

        def fused(x=x, pot=pot, var=var):
            pot._launch(x, var)                                  # logp and gradient, as ShapePotential's forward takes them

        def restated(x=x, cfg=cfg, var=var):
            xg = x.detach().requires_grad_(True)
            torch.autograd.grad(S.logp(xg, cfg, var).sum(), xg)

        # the two agree on these inputs before either is timed
        lp, g = pot._launch(x, var)
        xg = x.detach().requires_grad_(True)
        lp_t = S.logp(xg, cfg, var)
        g_t, = torch.autograd.grad(lp_t.sum(), xg)
        res['B%d_logp_rel_diff' % B] = float(((lp - lp_t.detach()).abs() / lp_t.detach().abs().clamp(min=1)).max())
        res['B%d_grad_rel_diff' % B] = float((g - g_t).abs().max() / g_t.abs().max())

        Bd = min(B, 32)
        eng.bind_features(O.empty_features([N] * Bd))
        trans = x[:Bd].contiguous()
        rots = eng.frenet(trans)
        ts = torch.full((Bd,), step, dtype=torch.int32, device=dev)
        res['B%d_fused_ms' % B] = median_ms(fused, args.reps, args.warmup, 20)
        res['B%d_torch_ms' % B] = median_ms(restated, args.reps, args.warmup, 5)
        res['B%d_denoise_batch' % B] = Bd
        res['B%d_denoise_ms' % B] = (B // Bd) * median_ms(lambda: eng.denoise(trans, rots, ts), max(args.reps // 3, 5), 2, 2)
        res['B%d_fused_over_denoise' % B] = res['B%d_fused_ms' % B] / res['B%d_denoise_ms' % B]
        res['B%d_torch_over_denoise' % B] = res['B%d_torch_ms' % B] / res['B%d_denoise_ms' % B]
        res['B%d_torch_over_fused' % B] = res['B%d_torch_ms' % B] / res['B%d_fused_ms' % B]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
