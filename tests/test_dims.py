"""Supported model dims that the sampling path had never run.  GPU only.

INTEGRATION.md: c_p = c_hidden_mul = 128, c_s a multiple of 8 up to 512, up to 40 distance bins, up to 16 IPA heads.  Only the
base widths select the specialised kernels; everything else goes through other launches:

  k_ipa_attn (run-time shapes), k_ipa_prep     any n_head_ipa / c_hidden_ipa / n_qk_point / n_v_point other than 12 / 16 / 4 / 8
  unfused structure tail in hx                 c_s != 384
  pair stack skipped                           n_pair_transform_layer = 0
  k_pair_transition_hx with n_hb != 16         pair_transition_n != 4
  k_pair_static<true> past 40 motif columns    template_dist_n_bin = 39, 40 with a motif (linear_motif_template has n_bin + 2 columns)

Each case: its own engine and weights, a motif-conditioned ragged batch [37, 30] and a plain structure of 130, both arithmetics,
z / states (valid residues) and p_init / p (all elements) against the float32 oracle under the project's bar
1e-4 * max(1, |ref|_inf).  The cases off the base IPA dims also run N = 700 once.
"""
import pytest
import torch

from _parity import MATH_MODES, compare_taps, conditioned_inputs, failures, hard_time_limit, oracle_taps, worst
from oracle import genie_oracle as O

pytestmark = pytest.mark.gpu

DIM_CASES = {
    'heads16': dict(n_head_ipa=16), 'heads5': dict(n_head_ipa=5), 'ipa_hidden8': dict(c_hidden_ipa=8),
    'points2_4': dict(n_qk_point=2, n_v_point=4),
    'cs256': dict(c_s=256), 'cs512': dict(c_s=512), 'cs136': dict(c_s=136),
    'no_pair_stack': dict(n_pair_transform_layer=0), 'transition2': dict(pair_transition_n=2), 'transition1': dict(pair_transition_n=1),
    'bins40': dict(template_dist_n_bin=40), 'bins39': dict(template_dist_n_bin=39), 'bins1': dict(template_dist_n_bin=1), 'relpos0': dict(relpos_k=0), 'relpos8': dict(relpos_k=8),
    'narrow_embeddings': dict(c_pos_emb=64, c_chain_emb=32, c_timestep_emb=128), 'chains4': dict(max_n_chain=4),
}
NON_BASE_IPA = ('heads16', 'heads5', 'ipa_hidden8', 'points2_4')
assert len(DIM_CASES) == 17
_CASE = {}


@pytest.fixture(autouse=True)
def _time_limit():
    with hard_time_limit(1800):
        yield


def case_dims(name):
    over = dict(DIM_CASES[name])
    if name in NON_BASE_IPA:
        over['max_n_res'] = 2048             # the position table covers N = 700; the oracle takes the same dims
    return O.small_dims(**over)


def case_batches(name):
    """[(tag, features)]: motif-conditioned ragged batch, plain N = 130, and N = 700 off the base IPA dims; three chains in the
    first two where the model has a chain table of four"""
    g = torch.Generator().manual_seed(21)
    multi = name == 'chains4'
    f1 = O.empty_features([37, 30], chains_per_sample=[[10, 15, 12], [30]] if multi else None)
    O.add_motif(f1, 0, torch.randn(6, 3, generator=g) * 4, [3, 4, 5, 20, 21, 22])
    out = [('motif_37_30', f1), ('plain_130', O.empty_features([130], chains_per_sample=[[40, 50, 40]] if multi else None))]
    if name in NON_BASE_IPA:
        out.append(('plain_700', O.empty_features([700])))
    return out


def _case(name):
    """engine, weights and the oracle's results of a case, kept while its two arithmetics run"""
    if name not in _CASE:
        for c in _CASE.values():
            c['engine'].close()
        _CASE.clear()
        from genie2_amd.engine import GenieEngine
        dims = case_dims(name)
        sd = O.synthetic_state_dict(dims, seed=3)
        _CASE[name] = dict(dims=dims, sd=sd, engine=GenieEngine(dims, sd, 'cuda:0'), runs={})
    return _CASE[name]


@pytest.mark.parametrize('name,math', [(n, m) for n in DIM_CASES for m in MATH_MODES])
def test_supported_dims_match_oracle(name, math):
    c = _case(name)
    eng, dims, sd = c['engine'], c['dims'], c['sd']
    eng.set_math(math)
    bad, lines = [], []
    n_runs = 0
    for k, (tag, f) in enumerate(case_batches(name)):
        fr = O.prepare_features(f)
        trans, ts = conditioned_inputs(f, dims['n_timestep'], 300 + k)
        eng.bind_features(f)
        rots = eng.frenet(trans)
        if tag not in c['runs']:
            c['runs'][tag] = oracle_taps(sd, dims, f, rots, trans, ts)
        out = eng.denoise(trans, rots, ts, None, taps=('states', 'p_init', 'p'))
        res = compare_taps(out, c['runs'][tag], fr['residue_mask'])
        del out
        bad += failures((name, tag), res)
        lines.append('%s (%s, %.3f)' % ((tag,) + worst(res)))
        n_runs += 1
    assert n_runs == (3 if name in NON_BASE_IPA else 2)
    print('dims %s %s: worst (tap, error / bound): %s' % (name, math, '; '.join(lines)))
    assert not bad, bad


def test_runtime_shape_attention_lds_limit():
    """k_ipa_attn keeps H * N logits and 8 * H * c_p + 3 * H * n_v_point floats in LDS: 64 N + 67072 bytes at 16 heads, which
    meets the 160 KiB of a CU at N = 1512 exactly.  1512 binds and runs, 1513 is refused with the attention kernel's message,
    and the handle stays usable."""
    from genie2_amd.capi import GenieError
    from genie2_amd.engine import GenieEngine
    dims = O.small_dims(n_head_ipa=16, max_n_res=2048, n_pair_transform_layer=1, n_structure_layer=1)
    assert 64 * 1512 + 67072 == 160 * 1024
    eng = GenieEngine(dims, O.synthetic_state_dict(dims, seed=3), 'cuda:0')
    try:
        with pytest.raises(GenieError, match='attention'):
            eng.bind_features(O.empty_features([1513]))
        eng.bind_features(O.empty_features([1512]))
        torch.cuda.synchronize()
        assert eng.N == 1512
        # the launch at exactly 160 KiB goes through
        f = O.empty_features([1512])
        trans, ts = conditioned_inputs(f, dims['n_timestep'], 5)
        z = eng.denoise(trans, eng.frenet(trans), ts)['z']
        assert torch.isfinite(z).all() and float(z.abs().max()) > 0
        eng.bind_features(O.empty_features([16]))
    finally:
        eng.close()


@pytest.mark.parametrize('over,word', [(dict(c_s=132), 'c_s'), (dict(n_head_ipa=17), 'n_head_ipa'), (dict(template_dist_n_bin=41), 'template_dist_n_bin'),
                                       (dict(c_p=64), 'c_p')])
def test_unsupported_dims_are_refused_with_their_message(over, word):
    """what INTEGRATION.md says genie_create refuses, through the engine as a user meets it"""
    from genie2_amd.capi import GenieError
    from genie2_amd.engine import GenieEngine
    dims = O.small_dims(**over)
    with pytest.raises(GenieError, match=word):
        GenieEngine(dims, {}, 'cuda:0')
