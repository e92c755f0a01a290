"""Helpers of test_train_paths_host.py and test_train_paths_gpu.py: the five smallest batches that reach each row of the training
path's kernel dispatch (by the number of pair rows P = B N^2), a Python replica of that dispatch, and the autograd references in
either precision.  No tests here."""
import functools

import torch

from oracle import genie_oracle as O

# name -> lengths, seed of _build's generator, one timestep per entry, condition_loss_weight.  A 4-residue motif sits on entry 0.
# In descending P, so that a shared engine allocates its training workspace once.
# Seeds: 7 unless the float32 oracle itself then misses 1e-3 against the float64 oracle (test_train_paths_host.py) -- the three-entry
# batch does with 7, 8 and 9 (5.3e-3, 9.7e-3, 1.4e-3 on a transition weight: rows at a ReLU threshold) and is at 4e-5 with 10.  Decided by
# the oracle alone, never by the kernels' result.
CASES = {
    'n92_60': dict(lengths=[92, 60], seed=7, timesteps=[37, 5], weight=1.0),
    'n64_33': dict(lengths=[64, 33], seed=7, timesteps=[37, 5], weight=3.0),
    'n56_40': dict(lengths=[56, 40], seed=7, timesteps=[37, 5], weight=1.0),
    'n40_33_21': dict(lengths=[40, 33, 21], seed=10, timesteps=[37, 5, 81], weight=1.0),
    'n47_31': dict(lengths=[47, 31], seed=7, timesteps=[37, 5], weight=2.0),
}
SUITE_SHAPES = [[21, 14], [128, 101]]          # what test_training.py already runs gradients at (the second on the base model)


@functools.lru_cache(maxsize=None)
def dims():
    return O.small_dims()


@functools.lru_cache(maxsize=None)
def weights():
    return O.synthetic_state_dict(dims(), seed=4)


# ------------------------------------------------------------------------------------------------------------------------------
# The dispatch, replayed.  gemm_kernel_choice / gemm_splits below and the functions of the same names in
# genie2_amd/csrc/train_kernels.hip MOVE TOGETHER: a change on either side without the other makes test_train_paths_host.py's
# coverage statement false.
GM_BK = 32
GM_SPLIT_WGS = 512
GENERIC, TILE64, TILE128 = 'generic', '64-tile', '128-tile'


def gemm_kernel_choice(M, N, K, batch=1, nsplit=1, unit_a=True, unit_b=True, max_stride=0):
    """unit_a / unit_b: the operand has a unit stride in one of its two dimensions; max_stride: its largest stride"""
    ks = ((K + nsplit - 1) // nsplit + GM_BK - 1) // GM_BK * GM_BK
    fast = (unit_a and unit_b and M % 64 == 0 and N % 64 == 0 and K % GM_BK == 0 and ks % GM_BK == 0 and max_stride < (1 << 24)
            and batch * nsplit < 65536 and M // 64 < 65536)
    if not fast:
        return GENERIC
    big_tiles = (M // 128) * (N // 128) * batch * nsplit
    use_big = M % 128 == 0 and N % 128 == 0 and (big_tiles >= 256 or (big_tiles >= 192 and (M // 128) * (N // 128) >= 2))
    return TILE128 if use_big else TILE64


def gemm_splits_branch(M, N, K, batch=1):
    """(nsplit, 'long_k' | 'fill'): the split-K factor and which of gemm_splits' two branches gave it"""
    if batch == 1 and M % 128 == 0 and N % 128 == 0 and 2 <= (M // 128) * (N // 128) <= 32 and K >= 16384:
        t = (M // 128) * (N // 128)
        return max(8, GM_SPLIT_WGS // t // 8 * 8), 'long_k'
    tiles = ((M + 63) // 64) * ((N + 63) // 64) * batch
    s = (768 + tiles - 1) // tiles
    smax = (K + 127) // 128
    s = min(s, smax, 512)
    if s >= 8 and batch == 1:
        s = min((s + 7) // 8 * 8, smax // 8 * 8 if smax // 8 * 8 > 0 else s)
    return max(1, s), 'fill'


def gemm_splits(M, N, K, batch=1):
    return gemm_splits_branch(M, N, K, batch)[0]
# ------------------------------------------------------------------------------------------------------------------------------


def empty_k_ranges(K, nsplit):
    """K ranges of a split-K launch that start at or past K (the kernels return early on them)"""
    ks = ((K + nsplit - 1) // nsplit + GM_BK - 1) // GM_BK * GM_BK
    return sum(1 for sp in range(nsplit) if sp * ks >= K)


def _wgrad(O_, Kin, P, cblk=0):
    """a weight gradient dW[O][Kin] += dY[P][O]^T X[P][Kin] as lin_bwd_w* launches it; cblk: rows per separately placed block"""
    ns, branch = gemm_splits_branch(O_, Kin, P)
    kern = gemm_kernel_choice(O_, Kin, P, nsplit=ns)
    placed = None
    if cblk:
        placed = 'table' if (kern != GENERIC and cblk % 128 == 0) else 'fallback'
        if placed == 'fallback':          # one GEMM per block, each with its own split factor
            ns, branch = gemm_splits_branch(cblk, Kin, P)
            kern = gemm_kernel_choice(cblk, Kin, P, nsplit=ns)
    return dict(kernel=kern, nsplit=ns, empty=empty_k_ranges(P, ns), branch=branch, xcd=kern != GENERIC and ns >= 8 and ns % 8 == 0,
                row_sums='gemm' if kern != GENERIC else 'k_colsum', cblk=placed)


def dispatch_row(lengths, d=None):
    """One row of the dispatch table for a batch of these lengths (padded to the longest) on a model of dims d: which kernel each
    class of GEMM of the training step runs on, the split-K launches of the weight gradients, the LayerNorm kernels."""
    d = d or dims()
    B, N = len(lengths), max(lengths)
    P, M = B * N * N, B * N
    cp, ch, nh, cs = d['c_p'], d['c_hidden_mul'], d['c_p'] * d['pair_transition_n'], d['c_s']
    cat5 = ch == cp
    fwd = {}
    k5 = gemm_kernel_choice(P, 5 * ch, cp) if cat5 else gemm_kernel_choice(P, ch, cp)
    cblk_fwd = ('table' if k5 != GENERIC and ch % 128 == 0 else 'fallback') if cat5 else None
    fwd['stack5'] = k5 if cblk_fwd != 'fallback' else gemm_kernel_choice(P, ch, cp)
    fwd['u'] = gemm_kernel_choice(P, cp, ch)
    fwd['transition1'] = gemm_kernel_choice(P, nh, cp)
    fwd['transition2'] = gemm_kernel_choice(P, cp, nh)
    dx_w2 = gemm_kernel_choice(P, nh, cp)
    # gemm_takes_mask on both the Linear + ReLU and the ReLU's backward GEMM (neither is placed in blocks or batched)
    mask = nh % 32 == 0 and fwd['transition1'] == TILE128 and dx_w2 == TILE128
    wg = {'stack5': _wgrad(5 * ch, cp, P, cblk=ch) if cat5 else _wgrad(ch, cp, P), 'transition1': _wgrad(nh, cp, P),
          'transition2': _wgrad(cp, nh, P), 'z': _wgrad(cp, ch, P)}
    return dict(lengths=list(lengths), P=P, fwd=fwd, cblk_fwd=cblk_fwd, dx_w2=dx_w2, mask=mask,
                contraction=gemm_kernel_choice(N, N, N, batch=B * ch), wgrad=wg,
                ln128=cp == 128 and P >= 4096, P_mod8=P % 8, P_mod32=P % 32, structure=gemm_kernel_choice(M, cs, cs))


# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(name):
    """features, noise target and noised inputs of a case (as _case of test_training.py builds them)"""
    c = CASES[name]
    g = torch.Generator().manual_seed(c['seed'])
    f = O.empty_features(c['lengths'])
    B, N = f['residue_mask'].shape
    O.add_motif(f, 0, torch.randn(4, 3, generator=g) * 4, [1, 2, 3, 9])
    f['atom_positions'] = f['atom_positions'] + 0.0
    x0 = torch.randn(B, N, 3, generator=g) * 4 * f['residue_mask'].unsqueeze(-1)
    f['atom_positions'] = torch.where(f['fixed_sequence_mask'].unsqueeze(-1), f['atom_positions'], x0)
    z = torch.randn(B, N, 3, generator=g) * f['residue_mask'].unsqueeze(-1)
    fr = O.prepare_features(f)
    s = torch.tensor(c['timesteps'])
    trans, rots = O.q_sample(f['atom_positions'], s, z, fr['chain_index'], fr['residue_mask'], O.training_schedule(dims()['n_timestep']))
    # the VJP's inputs: coordinates of their own, their Frenet frames, a cotangent on valid residues
    x = torch.randn(B, N, 3, generator=g) * 4
    v = torch.randn(B, N, 3, generator=g) * fr['residue_mask'].unsqueeze(-1)
    return dict(name=name, features=f, prepared=fr, z=z, trans=trans, rots=rots, ts=s.int(), weight=c['weight'], B=B, N=N,
                mask=fr['residue_mask'].unsqueeze(-1).float(), x=x, x_rots=O.compute_frenet_frames(x, fr['chain_index'], fr['residue_mask']), v=v)


def _cast(x, dtype):
    return x.to(dtype) if torch.is_tensor(x) and x.is_floating_point() else x


@functools.lru_cache(maxsize=None)
def oracle_grads(name, dtype, dropout=None):
    """torch autograd over O.denoiser_forward + O.training_loss in `dtype` on the same float32 values: dict(z, weighted_loss,
    unweighted_loss, grads).  dropout: (seed, tri, ipa, transition) -- the same-mask train-mode step.  Shared and never modified."""
    c, d = build(name), dims()
    sdg = {k: v.to(dtype).clone().requires_grad_(True) for k, v in weights().items()}
    kw = {}
    if dropout:
        masks = O.train_dropout_masks(d, c['B'], c['N'], dropout[0], *dropout[1:])
        kw['dropout_masks'] = {k: _cast(m, dtype) for k, m in masks.items()}
    o = O.denoiser_forward(sdg, d, c['rots'].to(dtype), c['trans'].to(dtype), c['ts'], c['features'], 'closed', None, None, **kw)
    lo = O.training_loss(o['z'], c['z'].to(dtype), c['prepared'], c['weight'])
    lo['weighted_loss'].backward()
    return dict(z=o['z'].detach(), weighted_loss=float(lo['weighted_loss'].detach()), unweighted_loss=float(lo['unweighted_loss'].detach()),
                grads={k: v.grad for k, v in sdg.items()})


@functools.lru_cache(maxsize=None)
def vjp_ref(name, dtype):
    """d <v, z> / d x with the frames held fixed, by autograd through the oracle in `dtype`: dict(z, dtrans)"""
    c, d = build(name), dims()
    sd = {k: v.to(dtype) for k, v in weights().items()}
    xg = c['x'].to(dtype).clone().requires_grad_(True)
    zo = O.denoiser_forward(sd, d, c['x_rots'].to(dtype), xg, c['ts'], c['features'], 'closed')['z']
    (zo * c['v'].to(dtype)).sum().backward()
    return dict(z=zo.detach(), dtrans=xg.grad)


def grad_floor(ref):
    """check_grads' floor: 1e-5 of the largest gradient entry of all tensors"""
    return 1e-5 * max(float(r.abs().max()) for r in ref.values())


def worst_tensor(got, ref):
    """(ratio, key): the largest max |got - ref| / max(|ref|_inf, floor) over the tensors -- check_grads' measure"""
    floor = grad_floor(ref)
    return max((float((got[k].double().cpu() - r.double()).abs().max()) / max(float(r.abs().max()), floor), k) for k, r in ref.items())


def rel_l2(got, ref):
    """relative L2 error over the whole gradient vector (dicts of tensors with the same keys)"""
    num = sum(float(((got[k].double().cpu() - r.double()) ** 2).sum()) for k, r in ref.items())
    den = sum(float((r.double() ** 2).sum()) for r in ref.values())
    return (num / den) ** 0.5
