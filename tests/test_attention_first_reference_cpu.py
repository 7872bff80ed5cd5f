"""``attn_fwd_first`` (attention forward for one query row per sequence) against the float64 reference, without a GPU.

1. An fp32 emulation of the kernel's documented arithmetic (tests/attention_first_ref.py: fp32 scores / softmax / P.V, one bf16
   rounding at the store) passes ``attention_ref.check(..., rows=first rows)`` at the module's existing ``TAU["ctx"]`` / ``KAPPA["ctx"]``
   on every case of ``attention_first_ref.CASES``.  Measured: largest ratio 0.46 of the bound (edge lengths, 16 heads), 0.45 at the
   headline set -- the project's bounds are the bounds, no new tolerance.
2. Two mutations FAIL the check: the query taken from row 1 instead of row 0 (132 - 192 of 180 - 240 blocks out of bound at 12 / 16
   heads; every block that stays in bound belongs to a sequence with at most two unmasked keys, where the query can hardly matter),
   and one lost key (``attention_ref.drop_key``)."""
import pytest
import torch

from tests import attention_first_ref as F
from tests import attention_ref as A


def test_the_entry_point_exists_in_every_layer():
    from msa_amd import _lib, ops
    assert "mmbert_attn_fwd_first" in _lib.SIGNATURES
    assert callable(ops.attn_fwd_first)
    assert ops._UNWRAPPED["attn_fwd_first"] is ops.attn_fwd_first          # launch spies see it (ops.launches_unwrapped)


@pytest.mark.parametrize("case", F.CASES, ids=[c[0] for c in F.CASES])
def test_emulated_kernel_arithmetic_passes_the_check(case):
    name, lens, heads = case[:3]
    qkv, bias = F.inputs(*case)
    ref = A.reference(qkv, bias, lens, heads)
    worst = A.check(F.emulate_first(qkv, bias, lens, heads), ref, lens, heads, name, rows=F.first_rows(lens))
    print(name, "largest ratio", round(worst["ctx"], 4))
    assert worst["ctx"] <= 0.6, worst                        # as for the other kernels: the bounds sit at about 2x the emulation


@pytest.mark.parametrize("case", [c for c in F.CASES if c[2] in (12, 16)], ids=[c[0] for c in F.CASES if c[2] in (12, 16)])
def test_query_from_the_wrong_row_fails_the_check(case):
    name, lens, heads, pats, _ = case
    qkv, bias = F.inputs(*case)
    ref = A.reference(qkv, bias, lens, heads)
    rows = F.first_rows(lens)
    got = F.emulate_first(qkv, bias, lens, heads, q_pos=1)
    with pytest.raises(AssertionError, match="out of bound"):
        A.check(got, ref, lens, heads, name, rows=rows)
    res = A.ratios(got, ref, lens, heads, rows)
    starts = A._starts(lens)
    unmasked = [int((bias[s0:s0 + n] > A.MASKED).sum()) for s0, n in zip(starts, lens)]
    bad = {(s, h) for (s, h, _), w in res.items() if not w.ratio <= 1.0}
    print(name, len(bad), "of", len(res), "blocks out of bound")
    assert len(bad) > len(res) // 2
    for (s, h, _), w in res.items():
        if lens[s] > 1 and unmasked[s] > 2:                  # the query decides the weights of three or more keys
            assert (s, h) in bad, (name, s, h, lens[s], pats[s], w)
        if lens[s] == 1 or unmasked[s] == 1:                 # one key carries all the weight whatever the query is
            assert (s, h) not in bad, (name, s, h, lens[s], pats[s], w)


def test_a_lost_key_fails_the_check():
    lens, heads = [550, 129, 65], 12
    qkv, bias, _ = A.make_inputs(lens, heads, ["random", "none", "none"], seed=77)
    starts = A._starts(lens)
    for s, k in ((0, 63), (0, 549), (1, 128), (2, 64)):
        bias[starts[s] + k] = 0.0
    ref = A.reference(qkv, bias, lens, heads)
    rows = F.first_rows(lens)
    for mut in (A.drop_key(0, 5, 63), A.drop_key(0, 0, 549), A.drop_key(1, 7, 128), A.drop_key(2, 11, 64)):
        got = A.reference(qkv, bias, lens, heads, mutation=mut)
        res = A.ratios(got, ref, lens, heads, rows)
        hit = [w.ratio for (s, h, kind), w in res.items() if (s, h) in mut.blocks and kind == "ctx"]
        print(mut.name, hit)
        rest = max(w.ratio for (s, h, _), w in res.items() if (s, h) not in mut.blocks)
        assert hit and min(hit) > 1.0, (mut.name, hit)
        assert rest == 0.0, (mut.name, rest)
        with pytest.raises(AssertionError, match="out of bound"):
            A.check(got, ref, lens, heads, mut.name, rows=rows)
