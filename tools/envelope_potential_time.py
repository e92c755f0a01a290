"""GPU tool (not a test): what one forward + gradient of the envelope potential costs as the fused HIP entry (EnvelopePotential,
csrc/envelope_kernels.hip) and as its float32 PyTorch restatement with autograd.grad (tests/_envelope.py) on the same device and
inputs: N = 256 against M = 2048 points, the first 2048 of the 2109 lattice points of a 24 A sphere, 3 A apart, at B = 8
and B = 128, both terms on with the defaults (tau 4, inside 3, cover 5, weights 1), centred 3.8 A random walks, var of schedule step
500.

    python tools/envelope_potential_time.py [--reps 30] [--warmup 10]   one JSON line: median ms per call (device events) per shape;
                                                                          the same line goes to profiles/envelope_potential_time.json

Each timing is taken after a warm-up, in batches of `batch` calls between two events (the median batch, per call): the calls queue up
faster than they run for the fused entry, so that figure is device time; the restatement's dozens of launches over [B, N, M] tensors
are what a user of it pays inside the sampling loop.  The two are measured alternately, `rounds` times, and the median round is
reported with the spread (min, max) beside it.

Before either is timed the fused entry is held to the float64 oracle (tests/_envelope.reference, on the CPU) on the timed inputs, to
the project's bars for a fused potential as tests/test_envelope_gpu.py uses them: logp within 1e-5 max(1, |logp|), every particle's
gradient within 1e-5 of its largest entry, each widened to 4 x the restatement's own error where that is larger; the tool stops with
an AssertionError otherwise, and records error / bar of both."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = ((8, 256), (128, 256))
SOLID, SPACING, POINTS = 'sphere:24', 3.0, 2048


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
    import _envelope as En
    x = En.centred_walk(B, N, 100 * N + B)
    cfg = En.case_config((B, N, 0, SOLID, SPACING, POINTS, False))
    x = x.to(dev).contiguous()
    pot = En.potential(cfg, N, abar)
    var = pot.variance(step)

    def fused():
        pot._launch(x, var)                                      # logp and gradient, as EnvelopePotential's forward takes them

    def restated():
        xg = x.detach().requires_grad_(True)
        torch.autograd.grad(En.logp(xg, cfg, var).sum(), xg)

    # both are held to the float64 oracle on these inputs before either is timed (eight particles at a time on the CPU)
    lp, g = pot._launch(x, var)
    xg = x.detach().requires_grad_(True)
    lp_t = En.logp(xg, cfg, var)
    g_t, = torch.autograd.grad(lp_t.sum(), xg)
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), 'the fused entry is not finite'
    ratios = {'logp': [0.0, 0.0], 'grad': [0.0, 0.0]}                  # error / unwidened bar: [fused, restatement]
    for b0 in range(0, B, 8):
        ref = En.reference(x[b0:b0 + 8].cpu(), cfg, float(var))
        assert float(ref['logp'].abs().min()) > 0, 'a particle of the timed input has no energy'
        lp_b = 1e-5 * ref['logp'].abs().clamp(min=1.0)
        g_b = 1e-5 * ref['grad'].abs().amax(dim=(1, 2))
        for k, (a, t) in enumerate(((lp, g), (lp_t.detach(), g_t))):
            ratios['logp'][k] = max(ratios['logp'][k], float(((a[b0:b0 + 8].double().cpu() - ref['logp']).abs() / lp_b).max()))
            ratios['grad'][k] = max(ratios['grad'][k], float(((t[b0:b0 + 8].double().cpu() - ref['grad']).abs().amax(dim=(1, 2)) / g_b).max()))
    res = {'B': B, 'N': N, 'M': POINTS, 'exponentials': [2 * B * N * POINTS, 4 * B * N * POINTS],
           'logp_error_over_bar': ratios['logp'][0], 'grad_error_over_bar': ratios['grad'][0],
           'torch_logp_error_over_bar': ratios['logp'][1], 'torch_grad_error_over_bar': ratios['grad'][1]}
    for k in ('logp', 'grad'):
        wide = max(1.0, 4.0 * ratios[k][1])
        assert ratios[k][0] <= wide, '%s: error %.3f of the bar (widened x%.2f by the restatement\'s own error)' % (k, ratios[k][0], wide)

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
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'envelope_potential_time.json'))
    args = ap.parse_args()
    import torch
    from genie2_amd import pack
    dev = 'cuda:0'
    abar = pack.schedule_tensors(1000)['alphas_cumprod'].to(dev)
    res = {'tool': 'envelope_potential_time', 'step': 500, 'reps': args.reps, 'warmup': args.warmup, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(0), 'shapes': [measure(B, N, args, abar, dev) for B, N in SHAPES]}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
