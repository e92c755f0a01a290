"""Triangular attention through the C ABI (libgenie_hip.so, csrc/pair_triatt_kernels.hip) against the reference's recorded call and
against the torch composition of tests/_triatt.py (test_triatt_host.py pins that composition to the reference).  GPU only.

Bar, as everywhere: 1e-4 * max(1, |ref|_inf) per tap (z and states on valid residues, p_init and p on all elements, p_tri_att0 on
valid pairs -- what the attention leaves at padded pairs is free), p exactly 0 at padded pairs, no non-finite value."""
import os

import pytest
import torch

import _parity as P
import _triatt as TA
from conftest import golden_features, load_golden
from oracle import genie_oracle as O

pytestmark = pytest.mark.gpu

SWEEP = [2, 3, 15, 16, 17, 31, 32, 33, 50, 63, 64, 65, 100, 128, 129, 200, 256]
_ENG, _REF = {}, {}


def engine(tag, dims, seed, math):
    """one engine per (dims tag, weights seed), switched between the arithmetic modes"""
    from genie2_amd.engine import GenieEngine
    key = (tag, seed)
    if key not in _ENG:
        sd = TA.full_state_dict(dims, seed)
        _ENG[key] = (GenieEngine(dims, sd, 'cuda:0'), sd)
    eng, sd = _ENG[key]
    eng.set_math(math)
    return eng, sd


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for eng, _ in _ENG.values():
        eng.close()
    _ENG.clear()
    _REF.clear()


def check(tag, out, ref, residue_mask):
    res = P.compare_taps(out, ref, residue_mask)
    err, scale = TA.tap_error(out['p_tri_att0'], ref['p_tri_att0'], residue_mask)
    res.append(('p_tri_att0', err, P.BAR * scale))
    res.append(('p_tri_att0_finite', float((~torch.isfinite(out['p_tri_att0'])).sum()), 0.0))
    print(tag, ' '.join(f'{t}={e:.2e}/{b:.1e}' for t, e, b in res))
    assert not P.failures(tag, res)


@pytest.mark.parametrize('math', P.MATH_MODES)
def test_reference_golden_call(math):
    g = load_golden(TA.GOLDEN)
    dims = TA.tri_dims(O.small_dims(), int(g['dims_c_hidden_tri_att']), int(g['dims_n_head_tri']))
    eng, _ = engine('small', dims, int(g['seed']), math)
    f = golden_features(g)
    eng.bind_features(f)
    out = eng.denoise(torch.from_numpy(g['trans']), torch.from_numpy(g['rots']), torch.from_numpy(g['timesteps']),
                      torch.from_numpy(g['quat_codes']), taps=('states', 'p', 'p_tri_att0'))
    rm = f['residue_mask']
    m3 = rm.unsqueeze(-1).double().cuda()
    pm = (m3.unsqueeze(1) * m3.unsqueeze(2))
    res = []
    for tap, mask in (('z', m3), ('states', m3), ('p', 1.0), ('p_tri_att0', pm)):
        got, want = out[tap].double() * mask, torch.from_numpy(g[tap]).cuda().double() * mask
        res.append((tap, float((got - want).abs().max()), P.BAR * max(1.0, float(want.abs().max()))))
    res.append(('p_padding', float((out['p'].double() * (1.0 - pm)).abs().max()), 0.0))
    res.append(('finite', float(sum(int((~torch.isfinite(v)).sum()) for v in out.values())), 0.0))
    print(math, ' '.join(f'{t}={e:.2e}/{b:.1e}' for t, e, b in res))
    assert not P.failures(math, res)


def sweep_features(N):
    if N == 50:       # the motif and two-chain case
        f = O.empty_features([50, 26], chains_per_sample=[[30, 20], [26]])
        ca = 3.0 * torch.randn(6, 3, generator=torch.Generator().manual_seed(5))
        O.add_motif(f, 0, ca - ca.mean(0, keepdim=True), [7, 8, 9, 33, 34, 35])
        return f
    return O.empty_features(P.ragged(N))


def sweep_case(tag, dims, seed, N, math):
    eng, sd = engine(tag, dims, seed, math)
    f = sweep_features(N)
    fr = O.prepare_features(f)
    trans, ts = P.conditioned_inputs(f, dims['n_timestep'], 2000 + N)
    eng.bind_features(f)
    rots = eng.frenet(trans)
    if (tag, N) not in _REF:        # one float64 composition per case: both arithmetics of a case follow each other
        _REF.clear()
        _REF[(tag, N)] = TA.composed_taps(sd, dims, f, rots, trans, ts, double=True)
    out = eng.denoise(trans, rots, ts, None, taps=('states', 'p_init', 'p', 'p_tri_att0'))
    check(f'{tag} N={N} {math}', out, _REF[(tag, N)], fr['residue_mask'])


@pytest.mark.parametrize('N', SWEEP)
def test_ragged_batches_against_float64(N):
    with P.hard_time_limit(900):
        for math in P.MATH_MODES:
            sweep_case('small', TA.tri_dims(O.small_dims()), 1, N, math)


@pytest.mark.parametrize('N', [33, 100])
def test_eight_heads_of_sixteen(N):
    with P.hard_time_limit(600):
        for math in P.MATH_MODES:
            sweep_case('h8', TA.tri_dims(O.small_dims(), 16, 8), 4, N, math)


def test_base_depth_n256():
    """Five layers, base dims plus (32, 4), N = 256, B = 2 (the second entry half padded), against the float32 composition."""
    with P.hard_time_limit(1500):
        dims = TA.tri_dims(O.BASE_DIMS)
        N = 256
        f = O.empty_features(P.ragged(N))
        fr = O.prepare_features(f)
        trans, ts = P.conditioned_inputs(f, dims['n_timestep'], 77)
        ref = None
        for math in P.MATH_MODES:
            eng, sd = engine('base', dims, 0, math)
            eng.bind_features(f)
            rots = eng.frenet(trans)
            if ref is None:
                ref = TA.composed_taps(sd, dims, f, rots, trans, ts)
            out = eng.denoise(trans, rots, ts, None, taps=('states', 'p_init', 'p', 'p_tri_att0'))
            check(f'base N={N} {math}', out, ref, fr['residue_mask'])
            del out
        eng.close()
        del _ENG[('base', 0)]


@pytest.mark.parametrize('math', P.MATH_MODES)
def test_reverse_loop_t20_n40(math):
    """genie_sample_loop over T = 20 steps against the composed loop on identical noise; the bound of
    test_trajectory_matches_reference_golden: max |dCa| <= 1e-4 * coordinate RMS."""
    T, N = 20, 40
    dims = TA.tri_dims(O.small_dims(n_timestep=T))
    eng, sd = engine('t20', dims, 1, math)
    f = O.empty_features([N, 31])
    noise = torch.randn(T, 2, N, 3, generator=torch.Generator().manual_seed(9))
    if 'loop' not in _REF:
        _REF['loop'] = TA.sample_loop(sd, dims, f, noise, 0.6)[0]
    ref = _REF['loop']
    eng.bind_features(f)
    final, _, _ = eng.sample_loop(noise, 0.6)
    assert torch.isfinite(final).all()
    rms = float(ref.pow(2).mean().sqrt())
    d = float((final.cpu() - ref).abs().max())
    print(f'{math}: max|dCa| {d:.3e}, coordinate RMS {rms:.2f}, ratio {d / rms:.2e}')
    assert d <= 1e-4 * rms


def parent_workspace_bytes(d, B, N):
    """genie_prepare_features' carve plan without triangular attention (csrc/genie_api.hip), every segment rounded up to 256 B."""
    NP = (N + 31) // 32 * 32
    M = B * N
    Pn = M * N
    cs, cp = d['c_s'], d['c_p']
    H, C, Pq, Pv = d['n_head_ipa'], d['c_hidden_ipa'], d['n_qk_point'], d['n_v_point']
    ldx = (d['c_pos_emb'] + d['c_chain_emb'] + d['c_timestep_emb'] + 23 + 7) // 8 * 8
    proj = H * (3 * C + 3 * Pq + 3 * (Pq + Pv))
    cat = H * (cp + C + 4 * Pv)
    is_base = (H, C, Pq, Pv, cp) == (12, 16, 4, 8, 128)
    vf = B * H * (1 + (3 * Pv + 15) // 16) * ((N + 31) // 32) * 512 if is_base else 64
    segs = [Pn * cp * 4] * 2 + [B * cp * NP * NP * 4] * 3 + [d['n_structure_layer'] * H * Pn * 4, M * ldx * 4] + [M * cs * 4] * 6 \
        + [M * 2 * cp * 4, M * proj * 4, M * cat * 4] + [M * H * C * 4] * 2 + [M * H * Pq * 3 * 4] * 2 + [M * H * Pv * 3 * 4] \
        + [vf * 4, M * 2 * 4, M * 9 * 4, M * 3 * 4, M * 3 * 4, B * 4, M * 4, 4, 3 * M * cs * 4] \
        + [M * 20 * 4, M * 4, M * 4, M * 4, M * 3 * 4, M, Pn, M]
    return sum((s + 255) // 256 * 256 for s in segs)


@pytest.mark.parametrize('B,N,c,H', [(1, 2, 32, 4), (2, 3, 32, 4), (2, 24, 32, 4), (3, 100, 16, 8), (2, 256, 32, 4), (8, 256, 32, 4)])
def test_workspace_stays_under_the_cap(B, N, c, H):
    """Two fresh handles of equal dims bound to the same (B, N), with and without the option: the difference is at most one
    module's q, k, v, g in f32 plus one bias tensor; without the option the workspace is the parent's, byte for byte."""
    from genie2_amd.engine import GenieEngine
    base = O.small_dims()
    tri = TA.tri_dims(base, c, H)
    f = O.empty_features([N] * B)
    e0 = GenieEngine(base, O.synthetic_state_dict(base, 1), 'cuda:0')
    e1 = GenieEngine(tri, TA.full_state_dict(tri, 1), 'cuda:0')
    try:
        e0.bind_features(f)
        e1.bind_features(f)
        w0, w1 = e0.workspace_bytes(), e1.workspace_bytes()
    finally:
        e0.close()
        e1.close()
    cap = 4 * B * N * N * base['c_p'] * 4 + B * H * N * N * 4
    print(f'B={B} N={N}: without {w0}, with {w1}, difference {w1 - w0} = {(w1 - w0) / cap:.3f} of the cap {cap}')
    assert w0 == parent_workspace_bytes(base, B, N)
    assert 0 < w1 - w0 <= cap


@pytest.mark.parametrize('math', P.MATH_MODES)
def test_two_calls_are_bitwise_equal(math):
    dims = TA.tri_dims(O.small_dims())
    eng, _ = engine('small', dims, 1, math)
    f = O.empty_features([70, 41])
    trans, ts = P.seeded_inputs(f, dims['n_timestep'], 3)
    eng.bind_features(f)
    rots = eng.frenet(trans)
    a = eng.denoise(trans, rots, ts, None, taps=('p',))
    b = eng.denoise(trans, rots, ts, None, taps=('p',))
    assert torch.equal(a['z'], b['z']) and torch.equal(a['p'], b['p'])


def test_backward_entry_points_refuse_and_leave_the_handle_usable():
    from genie2_amd import capi, pack
    dims = TA.tri_dims(O.small_dims())
    eng, sd = engine('small', dims, 1, 'hx')
    f = O.empty_features([24, 19])
    trans, ts = P.seeded_inputs(f, dims['n_timestep'], 4)
    eng.bind_features(f)
    rots = eng.frenet(trans)
    z0 = eng.denoise(trans, rots, ts)['z']
    w = pack.flatten_state_dict(sd, dims).cuda()
    with pytest.raises(capi.GenieError, match=r'rc=-1.*triangular attention'):
        eng.train_forward_backward(w, trans, rots, ts, torch.zeros(2, 24, 3), 1.0, train_mode=False)
    with pytest.raises(capi.GenieError, match=r'rc=-1.*triangular attention'):
        eng.denoise_vjp(w, trans, rots, ts, torch.ones(2, 24, 3))
    assert torch.equal(eng.denoise(trans, rots, ts)['z'], z0)


def test_unconditional_runner_with_the_option(tmp_path):
    """A configuration with includeTriangularAttention True and a random checkpoint through UnconditionalRunner
    (modelled on test_unconditional_runner_end_to_end): PDB files for two lengths."""
    from genie2_amd import pack
    from genie2_amd.config import Config
    from genie2_amd.diffusion import Genie, save_checkpoint
    from genie2_amd.sample_unconditional import UnconditionalRunner, build_parser
    root = str(tmp_path / 'results')
    d = os.path.join(root, 'triatt')
    os.makedirs(d)
    TA.write_config(os.path.join(d, 'configuration'), numTimesteps=8, numPairTransformLayers=2, numStructureLayers=2)
    g = Genie(Config(os.path.join(d, 'configuration')))
    assert any('tri_att_end' in k for k in g.model.state_dict())
    g.model.load_state_dict(pack.random_state_dict(g.model.dims, seed=3))
    save_checkpoint(g, os.path.join(d, 'checkpoints', 'epoch.2.ckpt'), epoch=2)
    out = str(tmp_path / 'out')
    args = build_parser().parse_args(['--name', 'triatt', '--epoch', '2', '--rootdir', root, '--scale', '0.6', '--outdir', out,
                                      '--min_length', '40', '--max_length', '56', '--length_step', '16', '--batch_size', '2',
                                      '--num_samples', '2', '--num_devices', '1'])
    torch.manual_seed(7)
    UnconditionalRunner().run(vars(args), args.num_devices, args.sequential_order)
    files = sorted(os.listdir(os.path.join(out, 'pdbs')))
    assert files == sorted('{}_{}.pdb'.format(n, i) for n in (56, 40) for i in range(2))
    for n in (56, 40):
        lines = open(os.path.join(out, 'pdbs', '{}_1.pdb'.format(n))).read().splitlines()
        assert len(lines) == n and lines[-1].startswith('ATOM') and 'CA' in lines[-1]
        xyz = [float(x) for ln in lines for x in (ln[30:38], ln[38:46], ln[46:54])]
        assert all(abs(v) < 1e4 for v in xyz)
