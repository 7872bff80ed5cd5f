"""``attn_probs_first`` (the attention probabilities of one query row per sequence) without a GPU.

1. ``attention_probs_ref.emulate_probs`` -- the kernel's documented fp32 arithmetic in its summation order -- stays within
   ``check_probs`` of the float64 ``reference_probs`` on every case of ``attention_probs_ref.CASES``.  Measured: at most 1.40 u (L1) and
   2.02 u max p (elementwise), both at the headline set; PHI = 4 is about twice the larger, so the emulation uses at most 0.51 of the bound.
2. Five mutations of the float64 reference are REJECTED on the blocks they touch and leave every other block at ratio exactly 0: one
   unmasked key dropped, a mask moved to its neighbour, the query taken from position 1, the softmax scale x (1 + 2^-5), the denominator
   summed over the first 128 keys only (a lost group merge).  A block is touched when its float64 probabilities change at all; it must
   be rejected unless fp32 cannot hold the change: rows with fewer than three unmasked keys (query, scale: one key is one-hot whatever
   they are, two can be saturated to 1e-10) and fully masked sequences (lost merge: u = 6e-4 there).  Smallest ratio error / bound over the
   blocks that must be rejected, at PHI = 4: dropped key 3.1e4, moved mask inf (a masked key gets weight: the exact-zero rule), query
   row 3.6e2, scale 7.8 (edge lengths, 12 heads; 3.6e4 at the headline set), lost merge 5.2e3 -- the smallest margin is the scale
   mutation's 7.8, on a short row of the edge lengths.
3. The entry point exists in every layer, ``attention_modality_mass`` is right on a hand-made tensor and ``predict`` refuses an
   unknown ``return_attention``."""
import os
import re

import pytest
import torch

from tests import attention_probs_ref as P
from tests import attention_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def _ref(case):
    """(qkv, bias, reference probabilities, reference scores) of a case: computed once, shared, never written to."""
    if case[0] not in _REF:
        qkv, bias = P.inputs(case)
        _REF[case[0]] = (qkv, bias) + P.reference_probs(qkv, bias, case[1], case[2])
    return _REF[case[0]]


def _by_name(name):
    return next(c for c in P.CASES if c[0] == name)


def _query_matters(case, bias):
    """bool [sequences, heads]: the sequences with three or more unmasked keys (or, fully masked, three or more keys) -- where the query
    and the scale decide how the weight is shared.  With one such key the row is one-hot whatever they are (untouched); with two, a
    large score gap leaves a change below anything fp32 can hold (edge lengths at score scale 2.83: 1e-10)."""
    lens, heads = case[1], case[2]
    n = []
    for s0, S in zip(A._starts(lens), lens):
        un = int((bias[s0:s0 + S] > A.MASKED).sum())
        n.append(un if un else S)
    return (torch.tensor(n) >= 3)[:, None].expand(len(lens), heads)


def _not_fully_masked(case, bias):
    """bool [sequences, heads]: the sequences with an unmasked key.  In a fully masked one |s| ~ 10000, u = 6e-4 and the bound PHI u =
    2.4e-3 is the resolution of fp32 there: a change of one key's weight among 129 can stay below it."""
    lens, heads = case[1], case[2]
    any_un = [bool((bias[s0:s0 + S] > A.MASKED).any()) for s0, S in zip(A._starts(lens), lens)]
    return torch.tensor(any_un)[:, None].expand(len(lens), heads)


@pytest.mark.parametrize("case", P.CASES, ids=[c[0] for c in P.CASES])
def test_emulated_kernel_arithmetic_passes_the_check(case):
    name, lens, heads = case[:3]
    qkv, bias, rp, rs = _ref(case)
    got = P.emulate_probs(qkv, bias, lens, heads)
    l1, el = P.check_probs(got, rp, rs, name)
    print(name, "L1 %.3f u, elementwise %.3f u max p" % (l1, el))
    assert max(l1, el) <= 0.6 * P.PHI, (l1, el)                 # as for the other kernels: the bound sits at about 2x the emulation
    assert bool((got.sum(-1) - 1.0).abs().max() < 1e-5)


def _rejected(name, rp, rs, mutated, expect=None, must=None):
    """The mutated reference against the reference: every touched block out of bound (``must``, a bool [sequences, heads]: those of the
    touched blocks), every untouched block at exactly 0.  ``expect``: the set of blocks that must be the touched ones.  Returns the
    smallest ratio of a block that has to be rejected."""
    r = P.ratios_probs(mutated, rp, rs)
    ratio = torch.maximum(r["l1"], r["elem"])
    touched = (mutated != rp).any(-1)
    if expect is not None:
        assert {(int(s), int(h)) for s, h in touched.nonzero()} == set(expect), name
    assert bool((ratio[~touched] == 0).all()), name
    need = touched if must is None else (touched & must)
    assert int(need.sum()) > 0, name
    low = float(ratio[need].min())
    print(name, int(touched.sum()), "of", touched.numel(), "blocks touched,", int(need.sum()), "must be rejected, smallest ratio %.3g;" % low,
          int((touched & (ratio <= 1.0)).sum()), "touched blocks stay in bound")
    assert low > 1.0, (name, low, [(int(s), int(h)) for s, h in ((ratio <= 1.0) & need).nonzero()])
    with pytest.raises(AssertionError, match="out of bound"):
        P.check_probs(mutated, rp, rs, name)
    return low


def _lost_key_inputs():
    lens, heads = [550, 129, 65], 12
    qkv, bias, _ = A.make_inputs(lens, heads, ["random", "none", "none"], seed=77)
    starts = A._starts(lens)
    for s, k in ((0, 63), (0, 549), (1, 128), (2, 64)):
        bias[starts[s] + k] = 0.0
    return lens, heads, qkv, bias


def test_a_dropped_key_is_rejected():
    lens, heads, qkv, bias = _lost_key_inputs()
    rp, rs = P.reference_probs(qkv, bias, lens, heads)
    for mut in (A.drop_key(0, 5, 63), A.drop_key(0, 0, 549), A.drop_key(1, 7, 128), A.drop_key(2, 11, 64)):
        _rejected(mut.name, rp, rs, P.reference_probs(qkv, bias, lens, heads, mutation=mut)[0], expect=mut.blocks)


def test_a_mask_moved_to_its_neighbour_is_rejected():
    lens, heads, qkv, bias = _lost_key_inputs()
    rp, rs = P.reference_probs(qkv, bias, lens, heads)
    b0 = bias[:lens[0]]
    keys = [k for k in range(lens[0] - 1) if float(b0[k]) <= A.MASKED and float(b0[k + 1]) > A.MASKED]
    assert len(keys) > 10
    for key in (keys[0], keys[len(keys) // 2], keys[-1]):
        mut = A.move_mask(0, key, heads)
        _rejected(mut.name, rp, rs, P.reference_probs(qkv, bias, lens, heads, mutation=mut)[0], expect=mut.blocks)


@pytest.mark.parametrize("name", ["edge-h12-s1.0", "edge-h16-s2.83", "headline-h12", "long-h2"])
def test_the_query_from_position_1_is_rejected(name):
    case = _by_name(name)
    qkv, bias, rp, rs = _ref(case)
    _rejected(name + " query row", rp, rs, P.reference_probs(qkv, bias, case[1], case[2], q_pos=1)[0], must=_query_matters(case, bias))
    with pytest.raises(AssertionError, match="out of bound"):              # ... and so is the emulation of the same mistake
        P.check_probs(P.emulate_probs(qkv, bias, case[1], case[2], q_pos=1), rp, rs, name)


@pytest.mark.parametrize("name", ["edge-h12-s1.0", "edge-h16-s1.0", "headline-h12", "long-h2"])
def test_a_softmax_scale_off_by_2_to_the_minus_5_is_rejected(name):
    """At score scale 1 (the model's): at scale 2.83 the short rows are saturated -- one key holds all the weight to 1e-10 -- and a 3 %
    change of the scale moves nothing that fp32 can hold (25 of the 192 touched blocks of edge-h16-s2.83)."""
    case = _by_name(name)
    qkv, bias, rp, rs = _ref(case)
    _rejected(name + " scale", rp, rs, P.reference_probs(qkv, bias, case[1], case[2], mutation=A.softmax_scale())[0], must=_query_matters(case, bias))


@pytest.mark.parametrize("name", ["edge-h12-s1.0", "headline-h12", "long-h2"])
def test_a_denominator_from_the_first_128_keys_is_rejected(name):
    """A lost group merge: only sequences longer than 128 keys with weight behind key 127 can show it."""
    case = _by_name(name)
    qkv, bias, rp, rs = _ref(case)
    mutated = P.reference_probs(qkv, bias, case[1], case[2], denom_keys=128)[0]
    expect = {(s, h) for s, n in enumerate(case[1]) for h in range(case[2]) if n > 128 and bool((rp[s, h, 128:] > 0).any())}
    assert expect
    _rejected(name + " lost merge", rp, rs, mutated, expect=expect, must=_not_fully_masked(case, bias))


def test_the_entry_point_exists_in_every_layer():
    from msa_amd import _lib, build, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmbert_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmmbert_attn_probs_first\s*\(", text)
    assert "mmbert_attn_probs_first" in _lib.SIGNATURES and len(_lib.SIGNATURES["mmbert_attn_probs_first"][1]) == 13
    if not os.path.exists(_lib.LIB_PATH):
        if not os.path.exists(build.HIPCC):
            pytest.skip("no prebuilt library and no hipcc on this machine")
        build.build(verbose=False)
    assert hasattr(_lib.load(), "mmbert_attn_probs_first")
    assert callable(ops.attn_probs_first)
    assert ops._UNWRAPPED["attn_probs_first"] is ops.attn_probs_first      # launch spies see it (ops.launches_unwrapped)
    assert ops.launches_unwrapped()


def test_attention_modality_mass_on_a_hand_made_tensor():
    from msa_amd.model import attention_modality_mass
    att = torch.tensor([[[0.1, 0.2, 0.3, 0.25, 0.15], [1.0, 0.0, 0.0, 0.0, 0.0]],
                        [[0.0, 0.0, 0.0, 0.5, 0.5], [0.2, 0.2, 0.2, 0.2, 0.2]]])           # [2, 2, 5]: T = 3 text keys, 2 pair keys
    mass = attention_modality_mass(att, 3)
    assert mass.shape == (2, 2, 2) and mass.device.type == "cpu"
    want = torch.tensor([[[0.6, 0.4], [1.0, 0.0]], [[0.0, 1.0], [0.6, 0.4]]])
    assert torch.allclose(mass, want, rtol=0, atol=1e-7)
    assert torch.allclose(mass.sum(-1), att.sum(-1), rtol=0, atol=1e-7)
    assert attention_modality_mass(att, 5)[..., 1].abs().max() == 0 and attention_modality_mass(att, 0)[..., 0].abs().max() == 0
    with pytest.raises(ValueError):
        attention_modality_mass(att, 6)


def test_predict_refuses_an_unknown_return_attention():
    import inspect
    from msa_amd import trainer
    from msa_amd.model import MMBertForPretraining
    from tests.test_predict_cpu import _cpu_inputs, _tiny
    assert inspect.signature(MMBertForPretraining.predict).parameters["return_attention"].default is None
    p = inspect.signature(trainer.predict_epoch).parameters["return_attention"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    m = _tiny()
    for bad in ("bogus", True, 1, "TOP"):
        with pytest.raises(ValueError, match="return_attention"):
            m.predict(*_cpu_inputs(), return_attention=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):                 # a valid value goes on to the usual error on CPU tensors
        m.predict(*_cpu_inputs(), return_attention="top")
