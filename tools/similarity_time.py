"""GPU tool (not a test): what the TM-score of every pair of a design set costs as the HIP entry (PairwiseTM,
csrc/similarity_kernels.hip) and as the batched float32 PyTorch restatement of the same definition (tests/_similarity.py: all_pairs on
the device, `eigh` on Horn's matrices, pairs of equal length in batches of 4096, the offsets and seeds of an unequal pair in one
batch) on the same GPU and inputs, at two sets:

    equal    M = 256 designs of N = 128 residues: 128 random walks and a moved, noised copy of each (32 640 pairs, one offset each)
    mixed    M = 64 walks with lengths spread evenly over 50..256 (2 016 pairs, 1..207 offsets each)

    python tools/similarity_time.py [--reps 20] [--warmup 3]     one JSON line; the same line goes to profiles/similarity_time.json

The entry is timed after a warm-up with device events around every call (the median call); the restatement, which reads back from the
device as it goes, with the host clock around calls that end in a synchronise (the median of up to --torch_reps calls, fewer when
one call takes long: its budget is --torch_seconds per set).  Before either is timed the two must agree on the timed inputs: their tm
may differ by more than 2e-5 (both carry the project's 1e-5 bar) on at most 0.1 % of the pairs, the near-degenerate ones; the tool
stops with an AssertionError otherwise."""
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


def host_ms(fn, reps, budget_s):
    """Median wall time of fn() (which ends synchronised), of at most `reps` calls inside `budget_s` seconds; at least one."""
    import torch
    t = []
    start = time.perf_counter()
    while len(t) < reps and (not t or time.perf_counter() - start + t[-1] / 1e3 <= budget_s):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    t.sort()
    return t[len(t) // 2], [t[0], t[-1]], len(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch_reps', type=int, default=5)
    ap.add_argument('--torch_seconds', type=float, default=120.0)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'similarity_time.json'))
    args = ap.parse_args()
    import torch
    import _similarity as S
    from genie2_amd.similarity import PairwiseTM
    dev = 'cuda:0'
    entry = PairwiseTM(dev)
    res = {'tool': 'similarity_time', 'n_iter': 16, 'norm': 'shorter', 'reps': args.reps, 'warmup': args.warmup,
           'device': torch.cuda.get_device_name(0), 'sets': {}}
    mixed_lengths = [50 + (206 * m) // 63 for m in range(64)]
    mixed = torch.zeros(64, 256, 3)
    for m, L in enumerate(mixed_lengths):
        mixed[m, :L] = S.walk(1, L, 25600 + m)[0]
    sets = (('equal', S.designs(128, M=256), None), ('mixed', mixed, mixed_lengths))
    S.all_pairs(S.designs(16, M=4).to(dev), dtype=torch.float32)            # the restatement's kernels are loaded before it is timed
    for name, x, lengths in sets:
        x = x.to(dev).contiguous()
        M, N = x.shape[0], x.shape[1]
        ln = torch.tensor([N] * M if lengths is None else lengths, dtype=torch.int32, device=dev)

        def fused():
            return entry._launch(x, ln, 0, 16)

        def restated():
            return S.all_pairs(x, lengths, dtype=torch.float32)

        # the two agree on these inputs before either is timed (this call of the restatement is its warm-up)
        t0 = time.perf_counter()
        want = restated()
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        print('%s: first call of the restatement %.1f s' % (name, first), flush=True)
        got = fused()
        d = (got['tm'] - want['tm']).abs()
        frac = float((d > 2e-5).double().mean())
        one = {'M': M, 'N': N, 'lengths': 'all %d' % N if lengths is None else '%d..%d' % (min(lengths), max(lengths)),
               'pairs': M * (M - 1) // 2, 'tm_max_diff': float(d.max()), 'tm_fraction_above_2e-5': frac,
               'offsets_differing': int((got['offset'].long() != want['offset']).sum()) // 2}
        assert bool(torch.isfinite(got['tm']).all()) and bool(torch.isfinite(got['rmsd']).all()), 'the entry is not finite'
        assert frac <= 1e-3, '%s: tm differs from the restatement by more than 2e-5 on %.2f %% of the entries' % (name, 100 * frac)
        one['fused_ms'], one['fused_ms_range'] = fused_ms(fused, args.reps, args.warmup)
        one['torch_ms'], one['torch_ms_range'], one['torch_calls'] = host_ms(restated, args.torch_reps, args.torch_seconds)
        one['torch_over_fused'] = one['torch_ms'] / one['fused_ms']
        print('%s: entry %.3f ms, restatement %.1f ms (%d calls), ratio %.0f' % (name, one['fused_ms'], one['torch_ms'], one['torch_calls'],
                                                                                  one['torch_over_fused']), flush=True)
        res['sets'][name] = one
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
