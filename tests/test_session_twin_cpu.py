"""CPU-only checks of tests/session_twin.py: ``assert_same_bits`` fails on a one-ulp change of any single entry and on a missing key, and
the committed scripts really contain the cache transitions they are there for -- computed from the shapes alone, so that nobody shrinks
them later.  Also the host-side invariant the main script's "same lengths, other batch size" item stands for: a plan is a plan of ONE
batch size."""
import pytest
import torch

from tests import session_twin as ST


def _result():
    g = torch.Generator().manual_seed(5)
    return {"out0": torch.randn((), generator=g), "logits": torch.randn(3, 1, generator=g), "out7": torch.randn(2, 5, 7, generator=g).bfloat16(),
            "grads": torch.randn(1024, generator=g), "half": torch.randn(1024, generator=g).bfloat16(), "top_ids": torch.randint(0, 99, (4, 5), generator=g),
            "m": torch.zeros(1024), "label_rank": torch.randint(0, 9, (4,), generator=g)}


LAYOUT = [(0, 300, "a.weight"), (512, 256, "b.weight"), (768, 200, "c.bias")]


def _one_ulp(t, index):
    t = t.clone()
    flat = t.view(-1) if t.dim() else t.view(1)
    if t.is_floating_point():
        bits = flat.view({2: torch.int16, 4: torch.int32}[t.element_size()])
        bits[index] += 1                                       # the next representable value (away from zero): one ulp
    else:
        flat[index] += 1
    return t


def test_equal_results_pass_and_the_sign_of_zero_does_not_count():
    a, b = _result(), _result()
    b["m"][7] = -0.0
    ST.assert_same_bits(a, b, "item 0 (train)", LAYOUT)


@pytest.mark.parametrize("key", sorted(_result()))
def test_one_ulp_in_any_single_entry_fails(key):
    a, b = _result(), _result()
    n = a[key].numel()
    index = min(600, n - 1)
    b[key] = _one_ulp(b[key], index)
    with pytest.raises(AssertionError) as e:
        ST.assert_same_bits(a, b, "item 3 (accumulate (5, 24, 200, 170))", LAYOUT)
    msg = str(e.value)
    assert "item 3 (accumulate" in msg and repr(key) in msg and f"flat index {index}" in msg and "1 of %d" % n in msg, msg
    if key in ST.FLAT_KEYS:
        assert "owned by b.weight[88]" in msg, msg                     # 600 - 512
    else:
        assert "owned by" not in msg, msg


def test_the_owner_of_an_element_between_parameters_is_named_as_padding():
    a, b = _result(), _result()
    b["grads"] = _one_ulp(b["grads"], 400)
    with pytest.raises(AssertionError, match="padding between parameters"):
        ST.assert_same_bits(a, b, "item 1 (train)", LAYOUT)


def test_a_missing_key_a_shape_or_a_dtype_fails():
    a, b = _result(), _result()
    del b["grads"]
    with pytest.raises(AssertionError, match=r"only in the first \['grads'\]"):
        ST.assert_same_bits(a, b, "item 1 (train)")
    with pytest.raises(AssertionError, match=r"only in the second \['grads'\]"):
        ST.assert_same_bits(b, a, "item 1 (train)")
    b = _result()
    b["logits"] = b["logits"].view(1, 3)
    with pytest.raises(AssertionError, match="'logits'"):
        ST.assert_same_bits(a, b, "item 1 (train)")
    b = _result()
    b["half"] = b["half"].float()                                       # the same values in another dtype are not the same bits
    with pytest.raises(AssertionError, match="'half'"):
        ST.assert_same_bits(a, b, "item 1 (train)")
    b = _result()
    b["out0"] = torch.tensor(float("nan"))
    with pytest.raises(AssertionError, match="'out0'"):
        ST.assert_same_bits(a, b, "item 1 (train)")


def test_row_totals_of_the_main_script():
    rows = [ST.shape_facts(s)["rows"] for s in ST.MAIN_SHAPES]
    assert rows == [480, 2210, 192, 2210, 2640, 1608, 40, 2210, 480, 1206], rows
    script = ST.main_script()
    assert [it[0] for it in script] == ["accumulate", "train"] * 5
    assert len({it[2] for it in script}) == len(script)                 # every item its own batch, also where the shape repeats


def test_the_main_script_contains_every_transition_it_is_there_for():
    tr = ST.transitions(ST.main_script())
    assert all(tr.values()), {k: v for k, v in tr.items() if not v}
    # ... and where: item numbers as in the table of DESIGN.md (1-based)
    one = {k: [i + 1 for i in v] for k, v in tr.items()}
    assert one["grows_past_everything"] == [2, 5]
    assert one["shrinks_right_after_the_largest"] == [6]
    assert one["exact_repeat"] == [4, 9]
    assert one["same_lens_other_batch"] == [10]
    assert one["pair_lengths_exchanged"] == [8]
    assert one["longer_than_256"] == [5]
    assert one["one_sample_labels_on_pair_rows"] == [7]
    assert one["full_length"] == [10]
    # what the float64 items of the default-mode test are: the step_stages batch right after growth and shrinkage, the smallest, a repeat
    assert ST.MAIN_SHAPES[5] == (4, 24, 200, 130) and 6 in one["shrinks_right_after_the_largest"] and 7 in one["one_sample_labels_on_pair_rows"] \
        and 9 in one["exact_repeat"]


def test_the_transitions_are_computed_not_assumed():
    """Each condition goes missing when the item that carries it does."""
    s = ST.main_script()
    drop = lambda *idx: [it for i, it in enumerate(s) if i + 1 not in idx]
    assert not ST.transitions(drop(10))["same_lens_other_batch"] and not ST.transitions(drop(10))["full_length"]
    assert not ST.transitions(drop(8))["pair_lengths_exchanged"]
    assert not ST.transitions(drop(5))["longer_than_256"]
    assert not ST.transitions(drop(7))["one_sample_labels_on_pair_rows"]
    assert not ST.transitions(s[:5])["shrinks_right_after_the_largest"]          # (the largest item last: nothing follows it)
    assert ST.transitions(drop(4, 9))["exact_repeat"] == []
    assert ST.transitions(s[:1])["grows_past_everything"] == []


def test_the_shape_changes_at_every_item_of_the_modes_script():
    s = ST.MODES_SCRIPT
    assert [it[0] for it in s] == ["train", "predict", "train", "predict_tokens", "eval", "ema_eval", "predict_attention", "train"]
    assert all(a[1] != b[1] for a, b in zip(s, s[1:]))
    assert set(it[0] for it in s) | {"accumulate"} == set(ST.KINDS)


def test_a_plan_is_the_plan_of_one_batch_size():
    """``_plan`` at the same lengths and another batch size gives another plan (the library loads without a GPU; the plan's tensors are
    built on the CPU here)."""
    from msa_amd import _lib, build
    import os
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    m = MMBertForPretraining(MMBertConfig(vocab_size=64, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64))
    lens = list(ST.shape_facts(ST.MAIN_SHAPES[5])["lens"])
    p4, p3 = m._plan(lens, 4, "cpu"), m._plan(lens, 3, "cpu")
    assert p4 is m._plan(lens, 4, "cpu") and p4 is not p3
    for p, B in ((p4, 4), (p3, 3)):
        assert p["first"].numel() == 3 * B and p["bounds"][-1] == B * sum(lens) == p["layout"].tokens and len(p["layout"].lens) == 3 * B
