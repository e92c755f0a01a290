"""GPU tool (not a test): what independent particle systems cost in one step of motif-guided twisted-diffusion / SMC sampling, at the
setting of tools/smc_step_time.py: N = 256, a device batch of 8, step 500 of 1000, the rigid 6E6R potential thinned to P = 1000
placements, random-init base weights.

    python tools/smc_particles_time.py [--batches 10] [--steps 3] [--warmup 3]      one JSON line (device events, one process)

Per-step time, the median over --batches event-timed batches of --steps steps each, after --warmup steps, of
    (a) today's loop body (tools/smc_step_time.twisted_step: torch bookkeeping, one ESS read per step), B = 8
    (b) the body of TwistedSampler's num_particles path (per-system norm cap, one genie_smc_reweight call, no host read), S = 1, K = 8
    (c) the same with S = 2, K = 4        (d) the same with S = 8, K = 1
run in the order (a) (b) (a) (c) (d); the two (a) runs give the spread to read (b) against.  Then genie_smc_reweight alone for the
three shapes: device events around batches of 20 launches, median of 50 batches after 20 warm-up launches."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def systems_step(ctx, twist, S, K, reweight, state, alpha=0.012, scale=1.0, ess_fraction=0.5):
    """One iteration of TwistedSampler._sample's loop with num_particles (genie2_amd/smc.py: guided_step, then one SmcReweight call)
    at ctx['step'], the state left unchanged."""
    import torch
    import smc_step_time as base
    from genie2_amd.smc import guided_step
    mean_t, mean_u, sigma, log_prob = guided_step(base.guided_state(ctx, twist, S, alpha), 0, ctx['step'], ctx['trans'], ctx['rots'])
    new = (mean_t + scale * sigma * ctx['noise']) * ctx['mask']
    u = torch.rand(S, device=ctx['trans'].device) / K
    state['log_proposal'].zero_()
    state['log_w_acc'].zero_()
    x_out, _ = reweight(new, mean_t, mean_u, sigma, log_prob, u, ess_fraction, state['log_proposal'], state['log_w_acc'])
    return ctx['eng'].frenet(x_out)


def median_step_ms(fn, batches, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return statistics.median(out), min(out), max(out)


def entry_ms(S, K, N, dev, launches=20, batches=50, warmup=20):
    import torch
    from genie2_amd.smc import SmcReweight
    g = torch.Generator().manual_seed(S * 100 + K)
    B = S * K
    mean_u = torch.cumsum(3.0 * torch.randn(B, N, 3, generator=g), dim=1).to(dev)
    mean_t = mean_u + 0.01 * torch.randn(B, N, 3, generator=g).to(dev)
    new = mean_t + 0.1 * torch.randn(B, N, 3, generator=g).to(dev)
    sigma = torch.tensor([0.1], device=dev)
    log_prob, u = torch.randn(B, generator=g).to(dev), (torch.rand(S, generator=g) / K).to(dev)
    log_proposal, log_w_acc = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    rw, x_out = SmcReweight(S, K, N, dev), torch.empty_like(new)
    call = lambda: rw(new, mean_t, mean_u, sigma, log_prob, u, 0.5, log_proposal, log_w_acc, x_out=x_out)      # noqa: E731
    med, lo, hi = median_step_ms(call, batches, launches, warmup)
    return {'S': S, 'K': K, 'ms_per_launch_median': med, 'min': lo, 'max': hi}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=10)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--step', type=int, default=500)
    args = ap.parse_args()
    import torch
    import smc_step_time as base
    from genie2_amd.smc import SmcReweight
    ctx = base.setup(step=args.step)
    B, N, dev = ctx['B'], ctx['N'], ctx['trans'].device
    twist = ctx['potentials']['rigid']
    state = {'log_proposal': torch.zeros(B, device=dev), 'log_w_acc': torch.zeros(B, device=dev)}
    res = {'tool': 'smc_particles_time', 'B': B, 'N': N, 'P': ctx['P'], 'step': args.step, 'potential': 'rigid', 'batches': args.batches,
           'steps_per_batch': args.steps, 'warmup_steps': args.warmup, 'motif': '6E6R (6 + 7 residues)',
           'device': torch.cuda.get_device_name(0), 'runs': []}

    def today():
        return base.twisted_step(ctx, twist)

    def systems(S, K):
        rw = SmcReweight(S, K, N, dev)
        return lambda: systems_step(ctx, twist, S, K, rw, state)

    for name, fn in (('a', today), ('b S=1 K=8', systems(1, 8)), ('a again', today), ('c S=2 K=4', systems(2, 4)),
                     ('d S=8 K=1', systems(8, 1))):
        med, lo, hi = median_step_ms(fn, args.batches, args.steps, args.warmup)
        res['runs'].append({'run': name, 'step_ms_median': med, 'min': lo, 'max': hi})
    a1, b, a2 = (res['runs'][i]['step_ms_median'] for i in range(3))
    res['a_spread_ms'] = abs(a1 - a2)
    res['b_minus_a_mean_ms'] = b - 0.5 * (a1 + a2)
    res['entry'] = [entry_ms(S, K, N, dev) for S, K in ((1, 8), (2, 4), (8, 1))]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
