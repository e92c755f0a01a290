"""Helpers shared by test_lengths.py and test_dims.py: seeded inputs, the oracle in either precision, and the comparison
of the engine's taps with it under the project's bar (SURVEY.md 8c / BASELINE.md 4): 1e-4 * max(1, |ref|_inf)."""
import torch

from oracle import genie_oracle as O

MATH_MODES = ['hx', 'f32']
TAPS = ('z', 'states', 'p_init', 'p')
BAR = 1e-4
FRAME_TOL = 2e-6          # the bound of every existing Frenet test


def ragged(N):
    """the two lengths of the sweep's batch: a full row and a half-empty one"""
    return [N, max(2, N // 2 + 1)]


def seeded_inputs(features, n_timestep, seed):
    """(coordinates 3 * randn, one timestep per entry) for a bound feature dict"""
    B, N = features['residue_mask'].shape
    g = torch.Generator().manual_seed(seed)
    trans = 3.0 * torch.randn(B, N, 3, generator=g)
    ts = torch.randint(1, n_timestep + 1, (B,), generator=g).int()
    return trans, ts


def as64(x):
    return x.double() if torch.is_tensor(x) and x.is_floating_point() else x


def oracle_taps(sd, dims, features, rots, trans, ts, double=False):
    """z, states, p_init, p of the oracle (canonical quaternion signs, as the kernels); float64 arithmetic on the same float32
    values when `double`."""
    cast = as64 if double else (lambda x: x)
    taps = {}
    with torch.no_grad():
        o = O.denoiser_forward({k: cast(v) for k, v in sd.items()}, dims, cast(rots.cpu()), cast(trans), ts, features, 'closed', None, taps)
    return dict(z=o['z'], states=taps['states'], p_init=taps['p_init'], p=o['p'])


def compare_taps(out, ref, residue_mask, tol=None):
    """[(tap, error, bound)] for z and states on valid residues and p_init and p on all elements, plus ('p_padding', max |p| on
    padded pairs, 0) and ('finite', number of non-finite values, 0).  `tol[tap]` replaces the bar's 1e-4.  Runs on the device
    the engine's tensors live on, in float64."""
    dev = out['z'].device
    m = residue_mask.to(dev).double().unsqueeze(-1)                 # [B,N,1]
    res = []
    bad = 0
    for tap in TAPS:
        got, want = out[tap].double(), ref[tap].to(dev).double()
        bad += int((~torch.isfinite(out[tap])).sum())
        if tap in ('z', 'states'):
            got, want = got * m, want * m
        bound = (tol[tap] if tol else BAR) * max(1.0, float(want.abs().max()))
        res.append((tap, float((got - want).abs().max()), bound))
    pm = m.unsqueeze(1) * m.unsqueeze(2)                            # [B,N,N,1]
    res.append(('p_padding', float((out['p'].double() * (1.0 - pm)).abs().max()), 0.0))
    res.append(('finite', float(bad), 0.0))
    return res


def failures(tag, results):
    """the entries of compare_taps that miss their bound (a NaN error misses it)"""
    return [(tag, tap, err, bound) for tap, err, bound in results if not err <= bound]


def worst(results, frames=False):
    """(tap, error / bound) with the smallest margin among the denoiser's bounded taps, or among the frame checks"""
    pick = [(tap, err / bound) for tap, err, bound in results if bound > 0 and (tap in ('frenet', 'p_sample_frames')) == frames]
    return max(pick, key=lambda x: x[1]) if pick else (None, 0.0)


def conditioned_inputs(features, n_timestep, seed):
    """seeded_inputs, redrawn (seed + 100000, ...) until the float32 oracle's own Frenet frames are within a quarter of
    FRAME_TOL of its float64 frames.  The frames' bound is absolute, and among tens of thousands of random triples some are so
    close to collinear that float32 rounding of the binormal is amplified past it in the reference itself (6.2e-6 at N = 84
    with seed 1084, and above 2.3e-6 for every one of 40 seed bases tried over the sweep); the bound means something only on
    draws where the reference is well inside it.  Decided by the oracle alone, never by the kernels' result."""
    fr = O.prepare_features(features)
    for k in range(64):
        trans, ts = seeded_inputs(features, n_timestep, seed + 100000 * k)
        a = O.compute_frenet_frames(trans, fr['chain_index'], fr['residue_mask'])
        b = O.compute_frenet_frames(trans.double(), fr['chain_index'], fr['residue_mask'])
        if float((a.double() - b).abs().max()) <= FRAME_TOL / 4:
            return trans, ts
    raise AssertionError('no well-conditioned draw in 64 tries')


def hard_time_limit(seconds):
    """Context manager: the process is ended with a traceback if the block runs longer (a hung GPU call never returns to
    Python, so an exception could not end it)."""
    import contextlib
    import faulthandler

    @contextlib.contextmanager
    def cm():
        faulthandler.dump_traceback_later(seconds, exit=True)
        try:
            yield
        finally:
            faulthandler.cancel_dump_traceback_later()
    return cm()
