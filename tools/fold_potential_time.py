"""GPU tool (not a test): what one forward + gradient of the fold potential costs as the fused HIP entry (FoldPotential,
csrc/fold_kernels.hip) and as its float32 PyTorch restatement with autograd.grad (tests/_fold.py: logp) on the same device and
inputs: N = 256, B = 8, 3.8 A random walks, var of schedule step 500, at R = 1 (one template) and at R = 256 (a template and 255
avoided backbones: moved, noised copies of the designs and unrelated walks, tests/_fold.py: references, bounds_of).

    python tools/fold_potential_time.py [--reps 30] [--warmup 10]     one JSON line: median ms per call (device events) per R;
                                                                        the same line goes to profiles/fold_potential_time.json

Each timing is taken after a warm-up, in batches of `batch` calls between two events (the median batch, per call): the calls queue up
faster than they run for the fused entry, so that figure is device time; the restatement's hundreds of launches (16 batched `eigh`
calls among them) are what a user of it pays inside the sampling loop.  The two are measured alternately, `rounds` times, and the
median round is reported with the spread (min, max) beside it.  `guided_step_ms` repeats the 88 ms of one guided step at N = 256,
B = 8 so that a reader sees beside it what an avoid set of that size adds to a step.

Before either is timed the two must agree on the timed inputs.  Both are float32 and may settle on different seeds of one basin for
a far pair, which the test suite handles with the float64 oracle's rule; here the check is the coarse one that needs
no oracle: every TM-score within 2e-5 (two float32 results, each held to 1e-5 elsewhere), logp within 1e-4 max(1, |logp|), every
particle's gradient within 1e-3 of its largest entry; the tool stops with an AssertionError otherwise.  No time is a pass
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
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'fold_potential_time.json'))
    args = ap.parse_args()
    import torch
    import _fold as Fd
    from genie2_amd import pack
    from genie2_amd.smc import FoldPotential
    B, N, step, dev = 8, 256, 500, 'cuda:0'
    abar = pack.schedule_tensors(1000)['alphas_cumprod'].to(dev)
    res = {'tool': 'fold_potential_time', 'B': B, 'N': N, 'n_iter': 16, 'step': step, 'reps': args.reps, 'warmup': args.warmup,
           'rounds': args.rounds, 'device': torch.cuda.get_device_name(0), 'guided_step_ms': GUIDED_STEP_MS}
    designs = Fd.designs(B, N)
    for R in (1, 256):
        ref, bounds = Fd.references(designs, R), Fd.bounds_of(R)
        x, y = designs.to(dev).contiguous(), ref.to(dev).contiguous()
        pot = FoldPotential(N, abar, ref, bounds, device=dev)
        var = pot.variance(step)

        def fused():
            pot._launch(x, var)                                  # logp and gradient, as FoldPotential's forward takes them

        def restated():
            xg = x.detach().requires_grad_(True)
            torch.autograd.grad(Fd.logp(xg, y, bounds, var).sum(), xg)

        # the two agree on these inputs before either is timed
        lp, g = pot._launch(x, var)
        xg = x.detach().requires_grad_(True)
        lp_t = Fd.logp(xg, y, bounds, var)
        g_t, = torch.autograd.grad(lp_t.sum(), xg)
        lp_t = lp_t.detach()
        tm_t = Fd.restatement32(x, y, bounds, float(var))['tm'].to(dev)
        d_tm = (pot.tm_of(x) - tm_t).abs()
        d_lp = (lp - lp_t).abs() / lp_t.abs().clamp(min=1)
        d_g = (g - g_t).abs().amax(dim=(1, 2)) / g_t.abs().amax(dim=(1, 2)).clamp(min=1e-30)
        key = 'R%d' % R
        res[key] = {'R': R, 'tm_diff': float(d_tm.max()), 'logp_rel_diff': float(d_lp.max()), 'grad_rel_diff': float(d_g.max()),
                    'guided_particles': int((lp_t != 0).sum())}
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), 'the fused entry is not finite'
        assert float(lp.abs().max()) > 0 and float(g.abs().max()) > 0, 'no hinge is active on the timed inputs'
        assert float(d_tm.max()) <= 2e-5, 'a TM-score differs by %.3e from the restatement' % float(d_tm.max())
        assert float(d_lp.max()) <= 1e-4, 'logp differs by %.3e of max(1, |logp|) from the restatement' % float(d_lp.max())
        assert float(d_g.max()) <= 1e-3, "the gradient differs by %.3e of a particle's largest entry" % float(d_g.max())

        f, t = [], []
        for _ in range(args.rounds):                             # alternately: both see the same neighbours on the host
            f.append(median_ms(fused, args.reps, args.warmup, 50 if R == 1 else 10))
            t.append(median_ms(restated, max(3, args.reps // 6), 2, 1))
        f.sort()
        t.sort()
        res[key].update(fused_ms=f[len(f) // 2], fused_ms_range=[f[0], f[-1]], torch_ms=t[len(t) // 2], torch_ms_range=[t[0], t[-1]])
        res[key]['torch_over_fused'] = res[key]['torch_ms'] / res[key]['fused_ms']
        res[key]['fused_share_of_guided_step'] = res[key]['fused_ms'] / GUIDED_STEP_MS
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
