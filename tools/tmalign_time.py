"""GPU tool (not a test): what the gapped TM alignment costs as the HIP entry (TMAlign, csrc/tmalign_kernels.hip) and as the float32
PyTorch restatement of the same definition (tests/_tmalign.py: all_pairs on the device, `eigh` on Horn's matrices, the offsets and seeds
of a pair's stage 0 in one batch, the table one anti-diagonal at a time) on the same GPU and inputs, at two sets:

    novelty  M = 64 walks of 100..256 residues against R = 256 walks of 60..400 (16 384 pairs, one call of 256 x 400 cells)
    self     M = 256 designs of N = 128 residues against themselves: 128 walks and a moved, noised copy of each (65 536 pairs)

    python tools/tmalign_time.py [--reps 20] [--warmup 3]     one JSON line; the same line goes to profiles/tmalign_time.json

The entry is timed after a warm-up with device events around every call (the median call), once with the default 8 rounds and once with
n_rounds = 0, which is stage 0 alone: the difference is what the dynamic programming stages cost.  The restatement runs one pair at a
time and reads back from the device as it goes, so it is timed with the host clock on --torch_pairs pairs spread evenly over the set
and reported per pair and scaled to the set (`torch_ms_scaled`); the whole set would take it the better part of an hour.  Before either
is timed the two must agree on those pairs: their tm may differ by more than 2e-5 (both carry the project's 1e-5 bar) on at most 15 % of
them, the share the tests allow to be ill-posed (a near tie in the table takes another path); the tool stops with an AssertionError
otherwise."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def fused_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[reps // 2], [t[0], t[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch_pairs', type=int, default=24)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'tmalign_time.json'))
    args = ap.parse_args()
    import torch
    import _similarity as S
    import _tmalign as T
    from genie2_amd.similarity import TMAlign
    dev = 'cuda:0'
    entry = TMAlign(dev)
    res = {'tool': 'tmalign_time', 'norm': 'query', 'n_iter': 16, 'n_rounds': 8, 'gap_open': -0.6, 'reps': args.reps, 'warmup': args.warmup,
           'device': torch.cuda.get_device_name(0), 'sets': {}}
    lq = [100 + (156 * m) // 63 for m in range(64)]
    lr = [60 + (340 * r) // 255 for r in range(256)]
    xq, _ = T.pad([S.walk(1, L, 51200 + m)[0] for m, L in enumerate(lq)])
    xr, _ = T.pad([S.walk(1, L, 52200 + r)[0] for r, L in enumerate(lr)])
    own = S.designs(128, M=256)
    sets = (('novelty', xq, lq, xr, lr), ('self', own, [128] * 256, own, [128] * 256))
    small = T.family(8)
    T.all_pairs(small[0][:1].to(dev), small[1][:1], small[2][:2].to(dev), small[3][:2], dtype=torch.float32)     # the restatement's kernels are loaded
    for name, xq, lq, xr, lr in sets:
        xq, xr = xq.to(dev).contiguous(), xr.to(dev).contiguous()
        M, R = len(lq), len(lr)
        lqd, lrd = torch.tensor(lq, dtype=torch.int32, device=dev), torch.tensor(lr, dtype=torch.int32, device=dev)

        def fused(n_rounds=8):
            return entry._launch(xq, lqd, xr, lrd, 0, 16, n_rounds, -0.6)

        got = fused()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got['tm']).all()) and bool(torch.isfinite(got['rmsd']).all()), 'the entry is not finite'
        # the restatement on a sample of the pairs: it agrees with the entry, then its time per pair
        step = max(1, (M * R) // args.torch_pairs)
        sample = [divmod(k, R) for k in range(step // 2, M * R, step)][:args.torch_pairs]
        diffs, t_pair = [], []
        for m, r in sample:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = T.align(xq[m, :lq[m]], xr[r, :lr[r]], dtype=torch.float32)
            torch.cuda.synchronize()
            t_pair.append(1e3 * (time.perf_counter() - t0))
            diffs.append(abs(float(want['tm']) - float(got['tm'][m, r])))
        frac = sum(d > 2e-5 for d in diffs) / len(diffs)
        one = {'M': M, 'R': R, 'query_lengths': '%d..%d' % (min(lq), max(lq)), 'reference_lengths': '%d..%d' % (min(lr), max(lr)), 'pairs': M * R,
               'torch_pairs': len(sample), 'tm_median_diff': sorted(diffs)[len(diffs) // 2], 'tm_max_diff': max(diffs),
               'tm_fraction_above_2e-5': frac, 'mean_rounds': float(got['rounds'].float().mean()), 'mean_tm': float(got['tm'].mean())}
        assert frac <= 0.15, '%s: tm differs from the restatement by more than 2e-5 on %.0f %% of the sampled pairs' % (name, 100 * frac)
        one['fused_ms'], one['fused_ms_range'] = fused_ms(fused, args.reps, args.warmup)
        one['fused_stage0_ms'], one['fused_stage0_ms_range'] = fused_ms(lambda: fused(0), args.reps, args.warmup)
        one['stage0_share'] = one['fused_stage0_ms'] / one['fused_ms']
        t_pair.sort()
        one['torch_ms_per_pair'], one['torch_ms_per_pair_range'] = t_pair[len(t_pair) // 2], [t_pair[0], t_pair[-1]]
        one['torch_ms_scaled'] = sum(t_pair) / len(t_pair) * M * R
        one['torch_over_fused'] = one['torch_ms_scaled'] / one['fused_ms']
        print('%s: entry %.3f ms (stage 0 alone %.3f ms), restatement %.1f ms a pair on %d pairs, %.0f ms scaled to the set, ratio %.0f'
              % (name, one['fused_ms'], one['fused_stage0_ms'], one['torch_ms_per_pair'], len(sample), one['torch_ms_scaled'],
                 one['torch_over_fused']), flush=True)
        res['sets'][name] = one
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
