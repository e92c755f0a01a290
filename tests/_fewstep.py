"""Restatements for the few-step sampling tests, written from the formulas and not from genie2_amd.pack: the float64 schedule, the
coefficient rows of a strided ancestral / DDIM step, and the strided reverse loop over the oracle's denoiser."""
import math

import torch

from oracle import genie_oracle as O


def abar64(T):
    """abar_0..abar_T in float64 from the oracle's float32 betas."""
    abar = [1.0]
    for b in O.cosine_beta_schedule(T).tolist()[1:]:
        abar.append(abar[-1] * (1.0 - b))
    return abar


def coefficient_rows(T, steps, sampler, eta=0.0):
    """[(A, Bz, C)] per iteration: t = steps[i] -> s = steps[i + 1], s = 0 after the last."""
    abar = abar64(T)
    rows = []
    for t, s in zip(steps, list(steps[1:]) + [0]):
        at, as_ = abar[t], abar[s]
        if sampler == 'ancestral':
            ap = at / as_
            bp = 1.0 - ap
            rows.append((1.0 / math.sqrt(ap), -bp / (math.sqrt(1.0 - at) * math.sqrt(ap)), math.sqrt(bp)))
        else:
            sigma = eta * math.sqrt((1.0 - as_) / (1.0 - at)) * math.sqrt(1.0 - at / as_)
            a = math.sqrt(as_ / at)
            rows.append((a, math.sqrt(max(0.0, 1.0 - as_ - sigma * sigma)) - a * math.sqrt(1.0 - at), sigma))
    return rows


def reverse_step(row, scale, x, z, eps, mask):
    """x <- ((A x + Bz z) mask + scale C eps) mask in float64; eps None: no noise."""
    a, bz, c = row
    m = mask.unsqueeze(-1).double()
    v = (a * x.double() + bz * z.double()) * m
    if eps is not None:
        v = (v + scale * c * eps.double()) * m
    return v


def strided_loop(sd, dims, features, noise, scale, steps, rows):
    """The strided reverse loop over the oracle ('closed' quaternions): the state after every iteration, float32 [K,B,N,3]."""
    f = O.prepare_features(features)
    trans = noise[0].clone()
    rots = O.compute_frenet_frames(trans, f['chain_index'], f['residue_mask'])
    B = trans.shape[0]
    states = []
    for it, step in enumerate(steps):
        ts = torch.full((B,), step, dtype=torch.int32)
        z = O.denoiser_forward(sd, dims, rots, trans, ts, f, 'closed')['z']
        eps = None if it == len(steps) - 1 else noise[it + 1]
        trans = reverse_step(rows[it], scale, trans, z, eps, f['residue_mask']).float()
        rots = O.compute_frenet_frames(trans, f['chain_index'], f['residue_mask'])
        states.append(trans.clone())
    return torch.stack(states)
