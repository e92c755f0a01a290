"""The gradient gather of the motif potentials (k_motif<Form, SPILL>, csrc/smc_kernels.hip) where many placements carry weight: the
inputs, the case table and a replica of the gather's dispatch, shared by tests/test_motif_gather_host.py (which decides every case's
regime on the CPU, from the float64 oracle alone) and tests/test_motif_gather_gpu.py (which runs the kernels).  Nothing here calls
the library.

The four forms: 'translate' and 'rigid' on the 6E6R segments (6 + 7 residues), 'grouped' and 'grouped_rigid' on segments_343 with
groups A, B, A.  `oracle(form, ...)` is the float64 reference of each (tests/test_motif_potential.py's `_reference`, restated here
with a `dtype`; rigid_oracle; grouped_oracle), and with dtype=torch.float32 its float32 restatement.

The activity count.  The kernel lists placement p when float32 expf(score_p - max) != 0.  Where that flips (88 to 104, by whether
denormals are flushed) must not decide a case, so a case is accepted only when, for every particle, every placement has
max - score < ON = 50 (surely listed) or > OFF = 200 (surely not), by the float64 oracle.  A walk's placements have a continuous
spread of q, so no variance leaves such a gap among them unless all are on one side: a case with *some* of its placements active is
made by displacing the tail of the walk by 500 A.  A placement is then far off (q above 1e5) exactly when one of its bodies (the whole
motif, or a group) has residues on both sides of the cut, and as close as any other when every body is intact, so the count of
active placements is known by construction and `activity` confirms it.

The replica.  `replica()` restates what k_motif does after the scores: cap = mp_act_cap(P) = min(P, 2048); listed when the count is
at most cap; K = count when listed, else P; wave w takes k in [K w / 4, K (w + 1) / 4), in chunks of 64; ceil(N / 64) residue tiles.
It and k_motif's gather move together: a change to one without the other makes the host file's coverage assertions describe a
kernel that no longer exists."""
import numpy as np
import torch

from _motif import segments_6e6r, walk
from _motif_groups import grouped_oracle, segments_343
from _motif_rigid import rigid_oracle

FORMS = ('translate', 'rigid', 'grouped', 'grouped_rigid')
ACT_CAP = 2048                     # mp_act_cap(P) = min(P, ACT_CAP)
TILE, WAVES, CHUNK = 64, 4, 64     # MP_TILE, MP_WAVES, MP_CHUNK
ON, OFF = 50.0, 200.0
SHIFT = 500.0                      # the displacement of a walk's tail, in A
INSTANCE = {'translate': 'Translate', 'rigid': 'Rigid', 'grouped': 'Grouped<false>', 'grouped_rigid': 'Grouped<true>'}


# ---- the forms ---------------------------------------------------------------------------------------------------------------------

def motif(form):
    """(segments, seg_len, seg_group or None) of a form."""
    if form in ('translate', 'rigid'):
        segs = segments_6e6r()
        return segs, [len(s) for s in segs], None
    return segments_343(), [3, 4, 3], [0, 1, 0]


def pot_kwargs(form):
    """What MotifPotential takes to run the form."""
    kw = {'align': 'rigid' if form.endswith('rigid') else 'translation'}
    if form.startswith('grouped'):
        kw['groups'] = ['A', 'B', 'A']
    return kw


def centred_target(form):
    t = torch.cat(motif(form)[0])
    return t - t.mean(dim=0, keepdim=True)


def translate_oracle(x0, starts, seg_len, target, var, want_grad=True, dtype=torch.float64):
    """tests/test_motif_potential.py's `_reference` as a dict, in `dtype`: {'logp' [B], 'grad' [B,N,3] (or None), 'score' [B,P]}."""
    x = x0.detach().to(dtype).cpu().requires_grad_(want_grad)
    idx = torch.cat([starts[:, s:s + 1].long() + torch.arange(n) for s, n in enumerate(seg_len)], dim=1)     # [P, M]
    sel = x[:, idx]                                                                                        # [B, P, M, 3]
    sel = sel - sel.mean(dim=-2, keepdim=True)
    score = -((sel - target.to(dtype).cpu()[None, None]) ** 2).sum(dim=(2, 3)) / (2 * var)
    logp = torch.logsumexp(score, dim=1) - np.log(score.shape[1])
    grad = torch.autograd.grad(logp.sum(), x)[0] if want_grad else None
    return {'logp': logp.detach(), 'grad': grad, 'score': score.detach()}


def oracle(form, x0, starts, target, var, want_grad=True, dtype=torch.float64):
    """The form's reference on the CPU: a dict with at least 'logp', 'grad', 'score' (float64, or the `dtype` restatement)."""
    _, lens, seg_group = motif(form)
    starts = starts.cpu()
    if form == 'translate':
        return translate_oracle(x0, starts, lens, target, var, want_grad, dtype)
    if form == 'rigid':
        return rigid_oracle(x0, starts, lens, target, var, want_grad=want_grad, dtype=dtype)
    return grouped_oracle(x0, starts, lens, seg_group, target, var, rigid=form == 'grouped_rigid', want_grad=want_grad, dtype=dtype)


# ---- placement lists ---------------------------------------------------------------------------------------------------------------

_EVERY = {}


def every_start(n_res, lens):
    """int32 [C(n_res - M + S, S), S]: every placement (segments in order, not overlapping, inside 0..n_res-1), sorted."""
    key = (n_res, tuple(lens))
    if key not in _EVERY:
        grids = np.meshgrid(*[np.arange(n_res, dtype=np.int32)] * len(lens), indexing='ij')
        st = np.stack([g.ravel() for g in grids], axis=1)
        ok = st[:, -1] + lens[-1] <= n_res
        for s in range(len(lens) - 1):
            ok &= st[:, s] + lens[s] <= st[:, s + 1]
        _EVERY[key] = torch.from_numpy(st[ok].copy())
    return _EVERY[key]


def thinned(rows, P, seed=0):
    """P rows of a placement list in the order of one choice() draw: without replacement, or, where the list has fewer than P
    rows, with it (duplicated placements are legal)."""
    return rows[torch.from_numpy(np.random.RandomState(seed).choice(len(rows), P, replace=P > len(rows)))].contiguous()


def straddles(starts, lens, seg_group, cut):
    """bool [P]: some body of the placement (the whole motif, or one group) has residues on both sides of `cut`."""
    groups = [0] * len(lens) if seg_group is None else seg_group
    out = torch.zeros(len(starts), dtype=torch.bool)
    for g in set(groups):
        first = min(s for s in range(len(lens)) if groups[s] == g)
        last = max(s for s in range(len(lens)) if groups[s] == g)
        out |= (starts[:, first] < cut) & (starts[:, last] + lens[last] > cut)
    return out


def displaced_walk(B, n_res, seed, cut):
    x = walk(B, n_res, seed)
    x[:, cut:, 0] += SHIFT
    return x


def mixed_list(n_res, lens, seg_group, cut, n_on, P, seed=0, on_below_cut=True):
    """P placements of n_res residues of which exactly n_on have every body intact about `cut` (all of them below it when
    `on_below_cut`), in a shuffled order, so the intact ones are scattered through the list."""
    rows = every_start(n_res, lens)
    off = rows[straddles(rows, lens, seg_group, cut)]
    on = every_start(cut, lens) if on_below_cut else rows[~straddles(rows, lens, seg_group, cut)]
    both = torch.cat([thinned(on, n_on, seed), thinned(off, P - n_on, seed + 1)])
    return both[torch.from_numpy(np.random.RandomState(seed + 2).permutation(P))].contiguous()


def with_ties(form, x0, base, K, seed):
    """`base` with K - 1 rows, chosen by `seed`, overwritten by the row that scores best for particle 0 (the argmax does not depend on
    the variance): K placements of exactly equal score.  Returns (starts, the sorted indices of the K equal rows).  (A `base` drawn
    with replacement may hold the best row more than once: its other copies are first overwritten by a row that is not the best.)"""
    score = oracle(form, x0[:1], base, centred_target(form), 1.0, want_grad=False)['score'][0]
    best = int(score.argmax())
    same = (base == base[best]).all(dim=1)
    st = base.clone()
    st[same] = base[int((~same).nonzero()[0, 0])]
    st[best] = base[best]
    others = [i for i in np.random.RandomState(seed).permutation(len(base)).tolist() if i != best][:K - 1]
    st[others] = base[best]
    return st.contiguous(), sorted(others + [best])


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# name -> (n_res, B, var, x0(), starts(form, x0)).  `expect`: what the case is there to reach, checked by the host file against the
# replica: ('all',) every placement active; ('count', n) exactly n active for every particle; ('counts', [...]) per particle.

def _case_table():
    t = {}

    def add(name, n_res, B, var, x0, starts, expect):
        t[name] = dict(name=name, n_res=n_res, B=B, var=var, x0=x0, starts=starts, expect=expect)

    def lens_of(form):
        return motif(form)[1]

    # all-N80: every placement of 6E6R (2346; the 62196 of 3 + 4 + 3 thinned to as many), B = 3, two tiles; all active
    def n80(form, x0):
        rows = every_start(80, lens_of(form))
        return rows if len(rows) == 2346 else thinned(rows, 2346)
    for var in (100.0, 1e4):
        add('n80-all-var%g' % var, 80, 3, var, lambda: walk(3, 80, 81), n80, ('all',))
    # the same list on a walk whose last 30 residues are displaced: the intact placements (on either side) are active
    add('n80-some-var100', 80, 3, 100.0, lambda: displaced_walk(3, 80, 81, 50), n80, ('intact', 50))

    # N = 129: three tiles, the last with one live lane; P at and past the list's cap and Translate's record cap
    for P in (2048, 2049, 4100):
        add('n129-all-P%d' % P, 129, 3, 100.0, lambda: walk(3, 129, 129),
            lambda form, x0, P=P: thinned(every_start(129, lens_of(form)), P), ('all',))
        add('n129-some-P%d' % P, 129, 3, 100.0, lambda: displaced_walk(3, 129, 129, 89),
            lambda form, x0, P=P: mixed_list(129, lens_of(form), motif(form)[2], 89, 137, P), ('count', 137))

    # the exact boundary of the list: cnt == cap with P > cap (a strict subset, with gaps), cnt == cap + 1 (unlisted, zeros skipped)
    for n_on in (2048, 2049):
        for k in (1, 300):
            add('n129-cnt%d-P%d' % (n_on, 2049 + k), 129, 2, 100.0, lambda: displaced_walk(2, 129, 130, 89),
                lambda form, x0, n_on=n_on, k=k: mixed_list(129, lens_of(form), motif(form)[2], 89, n_on, 2049 + k), ('count', n_on))

    # small K: the best placement duplicated, var 1e-4; some waves get nothing, quarters are uneven
    # (P = 2500 spills the records of every form but Grouped<false>, which keeps 2730 placements in LDS: P = 3000 is there for it)
    for P in (300, 2500, 3000):
        for K in (1, 2, 3, 5, 7):
            add('n65-K%d-P%d' % (K, P), 65, 1, 1e-4, lambda: walk(1, 65, 65),
                lambda form, x0, K=K, P=P: with_ties(form, x0, thinned(every_start(65, lens_of(form)), P), K, 10 * K + P)[0],
                ('count', K))

    # chunk and grid edges: the 256-placement ballot chunk, k_motif_records' grid, quarters of 63.75; all active
    for n_res in (64, 63):
        for P in (255, 256, 257):
            add('n%d-all-P%d' % (n_res, P), n_res, 2, 1e4, lambda n_res=n_res: walk(2, n_res, n_res),
                lambda form, x0, n_res=n_res, P=P: thinned(every_start(n_res, lens_of(form)), P), ('all',))

    # mixed particles in one launch: particle 0 a 0.3 A blob (every placement active, unlisted), particles 1 and 2 displaced walks
    # (100 active, listed): `listed` differs between work-groups of one grid, and under SPILL each particle reads its own records
    def blob_and_walks():
        x = displaced_walk(3, 129, 131, 89)
        x[0] = 0.3 * torch.randn(129, 3, generator=torch.Generator().manual_seed(5))
        return x
    add('n129-mixed-P4100', 129, 3, 100.0, blob_and_walks,
        lambda form, x0: mixed_list(129, lens_of(form), motif(form)[2], 89, 100, 4100, seed=7), ('counts', [4100, 100, 100]))
    return t


CASES = _case_table()
_INPUTS = {}


def inputs(name, form):
    """(x0 [B,N,3] float32, starts int32 [P,S]) of a case for a form, built once and left unchanged."""
    if (name, form) not in _INPUTS:
        c = CASES[name]
        x0 = c['x0']()
        starts = c['starts'](form, x0)
        assert x0.shape == (c['B'], c['n_res'], 3) and starts.dtype == torch.int32
        _INPUTS[name, form] = (x0, starts)
    return _INPUTS[name, form]


def expected_counts(name, form):
    """The number of active placements of every particle that the case was built to have."""
    c = CASES[name]
    x0, starts = inputs(name, form)
    kind = c['expect']
    if kind[0] == 'all':
        return [len(starts)] * c['B']
    if kind[0] == 'count':
        return [kind[1]] * c['B']
    if kind[0] == 'counts':
        return list(kind[1])
    _, lens, seg_group = motif(form)
    return [int((~straddles(starts, lens, seg_group, kind[1])).sum())] * c['B']


# ---- regime ------------------------------------------------------------------------------------------------------------------------

def activity(score):
    """Of float64 scores [B, P]: {'count' [B]: placements with max - score < ON, 'between' [B]: those neither below ON nor above
    OFF, 'on_max' [B]: the largest max - score among the active, 'off_min' [B]: the smallest among the rest (inf when none)}."""
    d = score.max(dim=1, keepdim=True).values - score
    on, off = d < ON, d > OFF
    inf = torch.full_like(d, float('inf'))
    return {'count': on.sum(dim=1).tolist(), 'between': (~on & ~off).sum(dim=1).tolist(),
            'on_max': torch.where(on, d, -inf).max(dim=1).values.tolist(), 'off_min': torch.where(on, inf, d).min(dim=1).values.tolist()}


def replica(form, n_res, P, count, spill):
    """What k_motif does for one particle with `count` active placements out of P (the records spilled or not): the instantiation,
    listed or not, K, the quarters of the four waves, the chunks of the longest quarter and the residue tiles."""
    cap = min(P, ACT_CAP)
    listed = count <= cap
    K = count if listed else P
    quarters = [(K * w // WAVES, K * (w + 1) // WAVES) for w in range(WAVES)]
    return {'kernel': 'k_motif<%s, %s>' % (INSTANCE[form], 'true' if spill else 'false'), 'spill': bool(spill), 'cap': cap, 'listed': listed,
            'K': K, 'quarters': quarters, 'chunks': max(-(-(b - a) // CHUNK) for a, b in quarters), 'tiles': -(-n_res // TILE),
            'live_in_last_tile': n_res - (-(-n_res // TILE) - 1) * TILE}


def work_bytes(lib, form, B, P):
    """The form's host-side *_work_bytes (no device needed): above 0 the records spill."""
    if form == 'translate':
        return lib.genie_motif_potential_work_bytes(B, P)
    if form == 'rigid':
        return lib.genie_motif_potential_rigid_work_bytes(B, P)
    return lib.genie_motif_potential_grouped_work_bytes(B, P, 2, int(form == 'grouped_rigid'))


# ---- the reference of a case and how far its bar may widen ------------------------------------------------------------------------

BAR = 1e-5
_REFS = {}


def error_ratios(logp, grad, ref):
    """{'logp', 'grad'}: the largest error over the particles in units of the project's bar: logp against BAR max(1, |logp|), the
    gradient against BAR times the particle's largest gradient entry (both of the reference)."""
    lp, g = logp.detach().double().cpu(), grad.detach().double().cpu()
    rl = float(((lp - ref['logp']).abs() / (BAR * ref['logp'].abs().clamp(min=1.0))).max())
    rg = max(float((g[b] - ref['grad'][b]).abs().max() / (BAR * ref['grad'][b].abs().max())) for b in range(g.shape[0]))
    return {'logp': rl, 'grad': rg}


def reference(name, form, target):
    """(the float64 oracle of a case, the error ratios of its float32 restatement), computed once per target and left unchanged."""
    key = (name, form, tuple(target.flatten().tolist()))
    if key not in _REFS:
        x0, starts = inputs(name, form)
        ref = oracle(form, x0, starts, target, float(np.float32(CASES[name]['var'])))
        r32 = oracle(form, x0, starts, target, float(np.float32(CASES[name]['var'])), dtype=torch.float32)
        _REFS[key] = (ref, error_ratios(r32['logp'], r32['grad'], ref))
    return _REFS[key]


def restatement_ratios(name, form, target):
    return reference(name, form, target)[1]


def widen(r32):
    """The factor on the bar, per output: 4 x the float32 restatement's own error where that is above the bar, at most 10; a
    restatement that is itself more than 10 bars off says nothing about the kernel and widens nothing."""
    return {k: 1.0 if v > 10.0 else min(10.0, max(1.0, 4.0 * v)) for k, v in r32.items()}
