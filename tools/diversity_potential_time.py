"""GPU tool (not a test): what one forward + gradient of the diversity potential costs as the fused HIP entry (DiversityPotential,
csrc/diversity_kernels.hip) and as its float32 PyTorch restatement with autograd.grad (tests/_diversity.py: logp) on the same device
and inputs: N = 256, var of schedule step 500, tm_max 0.5, at (S, K) = (8, 1), (8, 16) and (32, 4) -- 28, 7168 and 7936 scored pairs;
the particles are tests/_diversity.py's inputs (moved, noised copies of one 3.8 A walk and unrelated walks).

    python tools/diversity_potential_time.py [--reps 30] [--warmup 10]     one JSON line: median ms per call (device events) per
                                                                             (S, K); the same line goes to
                                                                             profiles/diversity_potential_time.json

DESIGN.md 7.7's protocol, as tools/fold_potential_time.py follows it: each timing is taken after a warm-up, in batches of `batch`
calls between two events (the median batch, per call) -- the calls queue up faster than they run for the fused entry, so that figure
is device time; the restatement's hundreds of launches (16 batched `eigh` calls among them) are what a user of it pays inside the
sampling loop.  The two are measured alternately, `rounds` times, and the median round is reported with the spread (min, max) beside
it.  `guided_step_ms` repeats the 88 ms of one guided step at N = 256, B = 8; `us_per_pair` is the fused time over
the scored pairs, beside the 1.4 us per pair DESIGN.md 7.9 measured for the fold potential's kernels.

Before either is timed the two must agree on the timed inputs.  Both are float32 and may settle on different seeds of one basin for a
far pair; a far pair is idle (its hinge is 0) and gives exactly nothing to logp or to the gradient, so the check is:
every TM-score of a pair above tm_max within 2e-5 (two float32 results, each held to 1e-5 elsewhere) and of the others within 1e-3,
logp within 1e-4 max(1, |logp|), every particle's gradient within 1e-3 of its largest entry; the tool stops with an AssertionError
otherwise.  No time is a pass condition."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

GUIDED_STEP_MS = 88.0       # one guided step (denoiser forward + VJP + potential) at N = 256, B = 8
FOLD_US_PER_PAIR = 1.4      # the fold potential's kernels at N = 256 with the device full


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
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'diversity_potential_time.json'))
    args = ap.parse_args()
    import torch
    import _diversity as Dv
    from genie2_amd import pack
    from genie2_amd.smc import DiversityPotential
    N, step, dev = 256, 500, 'cuda:0'
    abar = pack.schedule_tensors(1000)['alphas_cumprod'].to(dev)
    res = {'tool': 'diversity_potential_time', 'N': N, 'n_iter': 16, 'tm_max': Dv.TM_MAX, 'step': step, 'reps': args.reps,
           'warmup': args.warmup, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0), 'guided_step_ms': GUIDED_STEP_MS,
           'fold_us_per_pair': FOLD_US_PER_PAIR}
    for S, K in ((8, 1), (8, 16), (32, 4)):
        x = Dv.inputs((S, K, N)).to(dev).contiguous()
        pot = DiversityPotential(N, abar, K, tm_max=Dv.TM_MAX, device=dev)
        var = pot.variance(step)
        pairs = len(Dv.pair_index(S * K, K)[0])

        def fused():
            pot._launch(x, var)                                  # logp and gradient, as DiversityPotential's forward takes them

        def restated():
            xg = x.detach().requires_grad_(True)
            torch.autograd.grad(Dv.logp(xg, K, var).sum(), xg)

        # the two agree on these inputs before either is timed
        lp, g = pot._launch(x, var)
        xg = x.detach().requires_grad_(True)
        lp_t = Dv.logp(xg, K, var)
        g_t, = torch.autograd.grad(lp_t.sum(), xg)
        lp_t = lp_t.detach()
        tm = pot._launch(x, pot._one, want='tm')[0]              # (systems of K: what the timed call scores)
        r32 = Dv.restatement32(x, K, float(var))
        tm_t, active = r32['tm'].to(dev), (r32['a'] > 0).to(dev)
        d_tm = (tm - tm_t).abs()
        d_lp = (lp - lp_t).abs() / lp_t.abs().clamp(min=1)
        d_g = (g - g_t).abs().amax(dim=(1, 2)) / g_t.abs().amax(dim=(1, 2)).clamp(min=1e-30)
        key = 'S%d_K%d' % (S, K)
        res[key] = {'S': S, 'K': K, 'pairs': pairs, 'active_pairs': int(active.sum()) // 2, 'tm_diff_active': float(d_tm[active].max()),
                    'tm_diff_idle': float(d_tm[~active].max()), 'logp_rel_diff': float(d_lp.max()), 'grad_rel_diff': float(d_g.max()),
                    'guided_particles': int((lp_t != 0).sum())}
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all()), 'the fused entry is not finite'
        assert float(lp.abs().max()) > 0 and float(g.abs().max()) > 0, 'no hinge is active on the timed inputs'
        assert float(d_tm[active].max()) <= 2e-5, 'a TM-score above tm_max differs by %.3e from the restatement' % float(d_tm[active].max())
        assert float(d_tm[~active].max()) <= 1e-3, 'an idle TM-score differs by %.3e from the restatement' % float(d_tm[~active].max())
        assert float(d_lp.max()) <= 1e-4, 'logp differs by %.3e of max(1, |logp|) from the restatement' % float(d_lp.max())
        assert float(d_g.max()) <= 1e-3, "the gradient differs by %.3e of a particle's largest entry" % float(d_g.max())

        f, t = [], []
        for _ in range(args.rounds):                             # alternately: both see the same neighbours on the host
            f.append(median_ms(fused, args.reps, args.warmup, 50 if pairs < 100 else 5))
            t.append(median_ms(restated, max(3, args.reps // 10), 1, 1))
        f.sort()
        t.sort()
        res[key].update(fused_ms=f[len(f) // 2], fused_ms_range=[f[0], f[-1]], torch_ms=t[len(t) // 2], torch_ms_range=[t[0], t[-1]])
        res[key]['torch_over_fused'] = res[key]['torch_ms'] / res[key]['fused_ms']
        res[key]['us_per_pair'] = 1e3 * res[key]['fused_ms'] / pairs
        res[key]['fused_share_of_guided_step'] = res[key]['fused_ms'] / GUIDED_STEP_MS
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
