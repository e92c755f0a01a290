"""What test_conditioned_gpu.py rests on, decided by the oracle and the helpers alone (CPU): the float32 oracle is well inside
the bounds on exactly the inputs the GPU tests use, every conditioning ingredient of those inputs moves the compared taps by many
bars (so the GPU test cannot pass with one of them ignored), and the features have the shape of a scaffolding problem."""
import pytest
import torch

import _conditioned as CD
from _parity import FRAME_TOL, compare_taps, oracle_taps
from oracle import genie_oracle as O

SENSITIVITY_LENGTHS = [130, 65]
_FULL = {}


@pytest.fixture(scope='module')
def model():
    dims = O.small_dims()
    return dims, O.synthetic_state_dict(dims, seed=3)


@pytest.mark.parametrize('N,style', [(n, s) for n in CD.LENGTHS for s in CD.STYLES])
def test_float32_oracle_is_inside_a_quarter_of_every_bound(model, N, style):
    """z, states, p_init, p (the bar) and the Frenet frames (FRAME_TOL): float32 oracle against float64 oracle on the GPU
    tests' own inputs, at every length and in both coordinate styles, within a quarter of the bound.  Measured: at most 0.085 of
    the bar on the taps and 0.20 of FRAME_TOL on the frames (the draws are selected for a quarter of it).

    The single representation s is the exception and is only held inside its bound 2e-5 here: the reference evaluates the
    sinusoidal encodings in float32, where the argument v * pi of residue_index v = 206 carries a rounding of 3e-5, so the
    float32 oracle's s is 1.73e-5 from the float64 oracle's at N >= 128 (0.87 of the bound), 8.3e-6 at N = 63 .. 65 (index up
    to 141) and 4.6e-6 at N = 5 (no offset: the timestep's encoding).  The engine uploads tables made with the reference's float32 expression
    (pack.sinusoidal_table), so the GPU test also compares s with the float32 oracle's under the same 2e-5."""
    dims, sd = model
    f, mask, trans, ts, rots = CD.case(N, style)
    r32 = CD.reference(sd, dims, f, rots, trans, ts, double=False)
    r64 = CD.reference(sd, dims, f, rots, trans, ts, double=True)
    res = CD.compare(r32, r64, mask) + [('frenet', CD.frame_margin(f, trans), FRAME_TOL)]
    print('N=%d %s: float32 oracle error / bound %s' % (N, style, {k: round(v, 4) for k, v in CD.ratios(res).items()}))
    assert [r[0] for r in res] == ['s', 'z', 'states', 'p_init', 'p', 'p_padding', 'finite', 'frenet']
    late = [(tap, err, bound) for tap, err, bound in res if not err <= (1.0 if tap == 's' else 0.25) * bound]
    assert not late, late


@pytest.mark.parametrize('N,without', [(n, w) for n in SENSITIVITY_LENGTHS for w in CD.INGREDIENTS])
def test_every_ingredient_moves_the_taps(model, N, without):
    """Float64 oracle: leaving out the structure mask, the sequence mask, the motif coordinates, aatype, the interface mask,
    the chain split or the index offset moves p_init by at least 100 bars and z by at least 10 bars."""
    dims, sd = model
    f, mask, trans, ts, rots = CD.case(N)
    if N not in _FULL:
        _FULL[N] = oracle_taps(sd, dims, f, rots, trans, ts, double=True)
    g = CD.scaffold_like(N, without=without)
    assert any(not torch.equal(f[k], g[k]) for k in f)
    moved = CD.ratios(compare_taps(oracle_taps(sd, dims, g, rots, trans, ts, double=True), _FULL[N], mask))
    print('N=%d without %s: moved by (bars) %s' % (N, without, {k: round(v, 1) for k, v in moved.items()}))
    assert moved['p_init'] >= 100.0 and moved['z'] >= 10.0, moved


@pytest.mark.parametrize('N', CD.LENGTHS)
def test_features_are_scaffold_shaped(N):
    f = CD.scaffold_like(N)
    lengths = CD.entry_lengths(N)
    B = len(lengths)
    assert f['residue_mask'].shape == (B, N) and f['residue_mask'].sum(1).tolist() == lengths
    fstm, fsm = f['fixed_structure_mask'], f['fixed_sequence_mask']
    assert torch.equal(fstm, fstm.transpose(1, 2))
    assert torch.equal(fsm, torch.diagonal(fstm, dim1=1, dim2=2))
    assert torch.equal(fstm, fsm[:, :, None] & fsm[:, None, :])           # true only inside the (one) motif of an entry
    valid = f['residue_mask'].bool()
    assert not (fsm & ~valid).any() and not (f['interface_mask'] & ~valid).any()
    motif = CD.motif_index(N)
    for b in range(B):
        want = motif[b] if b < len(motif) else []
        assert len(set(want)) == len(want) and torch.nonzero(fsm[b]).flatten().tolist() == want
        assert torch.equal(f['aatype'][b].sum(-1).bool(), fsm[b])          # one-hot on the motif, zero elsewhere
    assert torch.nonzero(f['interface_mask']).tolist() == [[0, n] for n in CD.interface_index(N)]
    assert not fsm[2].any() and not fstm[2].any() and not f['atom_positions'][2].any()
    if N >= 70:       # the motif and the chain break cross tile edges, in entry 0 and in an entry with b > 0
        assert {63, 64} <= set(motif[0]) and N - 1 in motif[0]
        assert (N - CD.TAIL_CHAIN) % 64 != 0 and f['chain_index'][0].tolist() == [0] * (N - CD.TAIL_CHAIN) + [1] * CD.TAIL_CHAIN
        d = f['residue_index'][0, :, None] - f['residue_index'][0, None, :]
        same = f['chain_index'][0, :, None] == f['chain_index'][0, None, :]
        k = O.small_dims()['relpos_k']
        assert int(d[same].max()) > k and int(d[same].min()) < -k         # both clamps inside one chain
        assert int(f['residue_index'].max()) >= N and int(f['residue_index'].max()) < CD.N_POS
    if N == 130:
        assert {63, 64} & set(motif[1]) == {64} and 65 in motif[1]          # entry 1 (length 66): its last two sit past the edge
