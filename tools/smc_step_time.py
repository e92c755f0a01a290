"""GPU tool (not a test): what one step of motif-guided twisted-diffusion / SMC sampling costs at N = 256, B = 8, with the 6E6R
motif (tests/golden/motif_problem_6E6R.pdb, segments of 6 and 7 residues) thinned to P = 1000 placements, at a mid-trajectory step.

    python tools/smc_step_time.py [--reps 50] [--warmup 5] [--step 500]     one JSON line of ms per call (device events)
    python tools/smc_step_time.py --align rigid   the same line for the superposed potential (MotifPotential(align='rigid')) beside
                                                  the fused translation one, without the PyTorch potential
    python tools/smc_step_time.py --trace K       K twisted steps with each potential, each run between two torch.cuda._sleep
                                                  marker kernels (for rocprofv3 --kernel-trace --stats)
    python tools/smc_step_time.py --digest DIR    launches and kernel time per step from the kernel_trace.csv under DIR

Timed, each after a warm-up and over --reps calls: eng.denoise, eng.denoise_vjp, the PyTorch potential (motif_twisting_function
+ torch.autograd.grad, genie2_amd/smc.py:58-69), the fused potential (MotifPotential + torch.autograd.grad), and one whole twisted
step with each potential, as TwistedSampler._sample runs it (its ESS read included).  Random-init base weights."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MOTIF = os.path.join(ROOT, 'tests', 'golden', 'motif_problem_6E6R.pdb')
MARKER = 'spin_kernel'


def setup(B=8, N=256, P=1000, step=500, dev='cuda:0'):
    import numpy as np
    import torch
    from genie2_amd import features as F, pack
    from genie2_amd.engine import GenieEngine
    from genie2_amd.sample_unconditional_motif import load_motif_segments
    from genie2_amd.smc import MotifPotential, generate_motif_index_mask, motif_twisting_function, placement_masks
    dims = dict(pack.BASE_DIMS)
    T = dims['n_timestep']
    sd = pack.random_state_dict(dims, seed=0)
    eng = GenieEngine(dims, sd, dev)
    eng.bind_features(F.convert_np_features_to_tensor(
        F.batchify_np_features([F.create_empty_np_features([N]) for _ in range(B)]), dev))
    w = pack.flatten_state_dict(sd, dims).to(dev)
    sched = {k: v.to(dev) for k, v in pack.schedule_tensors(T).items()}
    abar = sched['alphas_cumprod']
    g = torch.Generator().manual_seed(0)
    v = torch.randn(B, N, 3, generator=g)
    x0 = torch.cumsum(3.8 * v / v.norm(dim=-1, keepdim=True), dim=1)
    x0 = x0 - x0.mean(dim=1, keepdim=True)
    trans = (abar[step].sqrt().cpu() * x0 + (1 - abar[step]).sqrt().cpu() * torch.randn(B, N, 3, generator=g)).to(dev)
    segs = [torch.tensor(s, dtype=torch.float32) for s in load_motif_segments(MOTIF)]
    np.random.seed(0)
    pm = placement_masks(generate_motif_index_mask(segs, N, P)).to(dev)
    tgt = torch.cat(segs).to(dev)
    tgt = tgt - tgt.mean(dim=0, keepdim=True)
    np.random.seed(0)                                        # the same placements
    pot = MotifPotential(segs, N, abar, max_offsets=P, device=dev)
    assert pot.P == pm.shape[0] == P
    np.random.seed(0)
    rigid = MotifPotential(segs, N, abar, max_offsets=P, device=dev, align='rigid')
    potentials = {'torch': lambda x, s: motif_twisting_function(x, pm, tgt, abar[s], 0.012), 'fused': pot, 'rigid': rigid}
    return dict(eng=eng, w=w, sched=sched, trans=trans, rots=eng.frenet(trans), step=step, B=B, N=N, P=P, potentials=potentials,
                noise=torch.randn(B, N, 3, generator=g).to(dev), mask=torch.ones(B, N, 1, device=dev))


def potential_call(ctx, twist):
    import torch
    x0 = ctx['trans'].detach().clone().requires_grad_(True)
    lp = twist(x0, ctx['step'])
    return torch.autograd.grad(lp.mean(), x0)[0]


def guided_state(ctx, twist, S=None, alpha=0.012):
    """What genie2_amd.smc.guided_step reads of a sampler's state, from `ctx`: the full schedule, every step guided."""
    import types
    return types.SimpleNamespace(eng=ctx['eng'], w=ctx['w'], sched=ctx['sched'], tw_coef=None, twist=twist, alpha=alpha, unguided=0, S=S)


def twisted_step(ctx, twist, alpha=0.012, scale=1.0):
    """One iteration of TwistedSampler._sample's loop for one system (genie2_amd/smc.py: guided_step, then the weights and the ESS
    read of _host_update) at ctx['step'], the state left unchanged."""
    from genie2_amd.smc import compute_ess_from_log_w, guided_step, log_normal_density
    mean_t, mean_u, sigma, log_prob = guided_step(guided_state(ctx, twist, None, alpha), 0, ctx['step'], ctx['trans'], ctx['rots'])
    new = (mean_t + scale * sigma * ctx['noise']) * ctx['mask']
    log_rev = log_normal_density(new, mean_u, sigma ** 2).sum(dim=(1, 2))
    log_tw = log_normal_density(new, mean_t, sigma ** 2).sum(dim=(1, 2))
    log_w = log_rev + log_prob - log_tw
    float(compute_ess_from_log_w(log_w))                     # the sampler's per-step host read (ess_trace)
    return ctx['eng'].frenet(new)


def time_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def timing(args):
    import torch
    ctx = setup(step=args.step)
    eng, B, N = ctx['eng'], ctx['B'], ctx['N']
    ts = torch.full((B,), args.step, dtype=torch.int32, device=ctx['trans'].device)
    dz = torch.randn(B, N, 3, device=ctx['trans'].device)
    pt = ctx['potentials']
    res = {'tool': 'smc_step_time', 'B': B, 'N': N, 'P': ctx['P'], 'step': args.step, 'reps': args.reps, 'warmup': args.warmup,
           'motif': '6E6R (6 + 7 residues)', 'device': torch.cuda.get_device_name(0)}
    res['denoise_ms'] = time_ms(lambda: eng.denoise(ctx['trans'], ctx['rots'], ts), args.reps, args.warmup)
    res['denoise_vjp_ms'] = time_ms(lambda: eng.denoise_vjp(ctx['w'], ctx['trans'], ctx['rots'], ts, dz), args.reps, args.warmup)
    if args.align == 'rigid':
        res['align'] = 'rigid'
        for k in ('fused', 'rigid'):
            res[k + '_potential_ms'] = time_ms(lambda: potential_call(ctx, pt[k]), args.reps, args.warmup)
        res['rigid_locate_ms'] = time_ms(lambda: pt['rigid'].locate(ctx['trans']), args.reps, args.warmup)
        for k in ('fused', 'rigid'):
            res[k + '_step_ms'] = time_ms(lambda: twisted_step(ctx, pt[k]), args.reps, args.warmup)
        print(json.dumps(res))
        return
    for k in ('torch', 'fused'):
        res[k + '_potential_ms'] = time_ms(lambda: potential_call(ctx, pt[k]), args.reps, args.warmup)
    for k in ('torch', 'fused'):
        res[k + '_step_ms'] = time_ms(lambda: twisted_step(ctx, pt[k]), args.reps, args.warmup)
    res['potential_speedup'] = res['torch_potential_ms'] / res['fused_potential_ms']
    res['step_speedup'] = res['torch_step_ms'] / res['fused_step_ms']
    # agreement of the two potentials at this state (the timed calls compute the same thing)
    g_t, g_f = potential_call(ctx, pt['torch']), potential_call(ctx, pt['fused'])
    res['grad_max_rel_diff'] = float((g_t - g_f).abs().max() / g_t.abs().max())
    print(json.dumps(res))


def trace(args):
    import torch
    ctx = setup(step=args.step)
    for k in ('torch', 'fused'):                             # warm both paths outside the marked windows
        twisted_step(ctx, ctx['potentials'][k])
    torch.cuda.synchronize()
    order = ['torch', 'fused']
    torch.cuda._sleep(1000)
    for k in order:
        for _ in range(args.trace):
            twisted_step(ctx, ctx['potentials'][k])
        torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    print(json.dumps({'trace_steps': args.trace, 'windows': order, 'marker': MARKER}))


def digest(args):
    import csv
    files = sorted(glob.glob(os.path.join(args.digest, '**', '*kernel_trace.csv'), recursive=True))
    if not files:
        raise SystemExit('no kernel_trace.csv under ' + args.digest)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    marks = [i for i, r in enumerate(rows) if MARKER in r['Kernel_Name']]
    if len(marks) != 3:
        raise SystemExit('expected 3 marker kernels, found %d' % len(marks))
    out = {'trace_steps': args.steps}
    for name, (lo, hi) in zip(('torch', 'fused'), zip(marks[:-1], marks[1:])):
        win = rows[lo + 1:hi]
        kt = sum(int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in win) * 1e-6
        by = {}
        for r in win:
            e = by.setdefault(r['Kernel_Name'].split('(')[0][:80], [0, 0.0])
            e[0] += 1
            e[1] += (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-6
        span = (int(rows[hi]['Start_Timestamp']) - int(rows[lo]['End_Timestamp'])) * 1e-6
        top = sorted(by.items(), key=lambda kv: -kv[1][1])[:8]
        out[name] = {'launches_per_step': len(win) / args.steps, 'kernel_ms_per_step': kt / args.steps,
                     'wall_ms_per_step': span / args.steps,
                     'top_kernels': [{'name': k, 'launches_per_step': v[0] / args.steps, 'ms_per_step': v[1] / args.steps}
                                     for k, v in top]}
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--step', type=int, default=500)
    ap.add_argument('--align', choices=('translation', 'rigid'), default='translation')
    ap.add_argument('--trace', type=int, default=0)
    ap.add_argument('--digest', type=str, default=None)
    ap.add_argument('--steps', type=int, default=3, help='(--digest) steps per window of the traced run')
    args = ap.parse_args()
    if args.digest:
        digest(args)
    elif args.trace:
        trace(args)
    else:
        timing(args)


if __name__ == '__main__':
    main()
