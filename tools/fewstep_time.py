"""GPU tool (not a test): what few-step sampling costs at the benchmark shape (N = 256, B = 8, T = 1000, random-init base weights).

    python tools/fewstep_time.py [--num_steps 100] [--repeats 3]      one JSON line (device events, one process, warm-up first)

Timed, each as one device-resident call between two events:
  * `sample_loop` over --num_steps consecutive steps (T, T-1, ...), --repeats times: the per-iteration cost of the schedule-table loop
    and its run-to-run spread (max - min of the repeats);
  * `sample_loop_steps` over the --num_steps timesteps of pack.respaced_steps (ancestral), --repeats times: the per-iteration cost of
    the strided loop, which should sit inside that spread -- the loop body is the same but for the step kernel's mode -- and at the same
    time the whole few-step run;
  * the whole T-step `sample_loop`, once."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--num_steps', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--scale', type=float, default=0.6)
    args = ap.parse_args()
    import torch
    from genie2_amd import features as F, pack
    from genie2_amd.engine import GenieEngine
    dev, B, N, K = 'cuda:0', 8, 256, args.num_steps
    dims = dict(pack.BASE_DIMS)
    T = dims['n_timestep']
    eng = GenieEngine(dims, pack.random_state_dict(dims, seed=0), dev)
    eng.bind_features(F.convert_np_features_to_tensor(
        F.batchify_np_features([F.create_empty_np_features([N]) for _ in range(B)]), dev))
    noise = torch.randn(T, B, N, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    steps = pack.respaced_steps(T, K)
    coef = pack.reverse_coefficients(T, steps)
    few_noise = noise[:K].contiguous()
    consecutive = lambda: eng.sample_loop(noise, args.scale, first_step=T, last_step=T - K + 1)      # noqa: E731
    strided = lambda: eng.sample_loop_steps(few_noise, args.scale, steps, coef)                      # noqa: E731
    consecutive()
    strided()
    torch.cuda.synchronize()
    base, few = [], []
    for _ in range(args.repeats):                 # interleaved, so that a drift of the clocks falls on both alike
        base.append(timed_ms(consecutive) / K)
        few.append(timed_ms(strided) / K)
    full = timed_ms(lambda: eng.sample_loop(noise, args.scale))
    final = eng.sample_loop_steps(few_noise, args.scale, steps, coef)[0]
    mean = lambda v: sum(v) / len(v)              # noqa: E731
    res = {'tool': 'fewstep_time', 'B': B, 'N': N, 'T': T, 'num_steps': K, 'sampler': 'ancestral', 'repeats': args.repeats,
           'math': eng.math, 'device': torch.cuda.get_device_name(0),
           'consecutive_ms_per_iteration': base, 'strided_ms_per_iteration': few,
           'consecutive_ms_per_iteration_mean': mean(base), 'strided_ms_per_iteration_mean': mean(few),
           'consecutive_spread_ms': max(base) - min(base), 'strided_minus_consecutive_ms': mean(few) - mean(base),
           'full_T_run_ms': full, 'few_step_run_ms': mean(few) * K, 'run_speedup': full / (mean(few) * K),
           'few_step_result_finite': bool(torch.isfinite(final).all())}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
