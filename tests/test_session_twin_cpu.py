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


# ------------------------------------------------------------------------------------------------ the fine-tuning lifecycle scripts
_BATCH_CFG = dict(vocab=4096, dataset="mosei")                  # what both configurations of tests/test_lifecycle_twin_gpu.py share
_FREEZE_FACTS = ("stop_rises", "stop_is_top_layer_without_input_gradient", "bias_only_layer", "frozen_layer_between_trainable_ones",
                 "unfreeze_behind_steps", "unfreeze_without_a_step_since_the_freeze")
_LORA_FACTS = ("stop_rises", "unfreeze_behind_steps", "no_encoder_layer_trainable", "adapters_on_frozen_base", "adapters_on_trainable_base",
               "adapters_on_a_subset_of_layers", "rank_changes", "targets_change", "merge", "remove", "reload")
_DENSE_FACTS = ("dense_targets", "ffn_up_adapter", "dense_only_layer", "adapters_on_frozen_base", "adapters_on_trainable_base",
                "adapters_on_a_subset_of_layers", "rank_changes", "targets_change", "merge", "remove", "reload", "no_encoder_layer_trainable")


def _names(L):
    """The parameter names of a CPU-built model of L layers (no adapters), as tests/test_freeze_cpu.py takes them."""
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    m = MMBertForPretraining(MMBertConfig(vocab_size=64, hidden_size=32, num_hidden_layers=L, num_attention_heads=2, intermediate_size=64))
    m.bert.set_joint_embeddings("mosei")
    return [n for n, _ in m.named_parameters()]


@pytest.mark.parametrize("L", [3, 4])
def test_the_lifecycle_scripts_contain_every_transition_they_are_there_for(L):
    """Between them the two scripts contain every transition of ``ST.LIFECYCLE`` (the freeze script has no adapters, the adapter script
    freezes through ``add_lora`` alone: each is held to its own list), and each the shape transitions it is to cross."""
    names = _names(L)
    fz, lo = ST.lifecycle_facts(ST.freeze_script(L), names, L), ST.lifecycle_facts(ST.lora_script(L), names, L)
    de = ST.lifecycle_facts(ST.dense_lora_script(L), names, L)
    assert set(fz) == set(lo) == set(de) == set(ST.LIFECYCLE) == set(_FREEZE_FACTS) | set(_LORA_FACTS) | set(_DENSE_FACTS)
    assert all(fz[k] for k in _FREEZE_FACTS), {k: fz[k] for k in _FREEZE_FACTS}
    assert all(lo[k] for k in _LORA_FACTS), {k: lo[k] for k in _LORA_FACTS}
    assert all(de[k] for k in _DENSE_FACTS), {k: de[k] for k in _DENSE_FACTS}
    assert all(fz[k] or lo[k] for k in ST.LIFECYCLE if k not in ("dense_targets", "ffn_up_adapter", "dense_only_layer"))
    assert not any(fz[k] or lo[k] for k in ("dense_targets", "ffn_up_adapter", "dense_only_layer"))        # (the older scripts know no dense target)
    # where, as the scripts are written down in tests/session_twin.py
    assert fz["stop_rises"] == [2, 6] and fz["stop_is_top_layer_without_input_gradient"] == [6, 9, 10] and fz["bias_only_layer"] == [9, 10]
    assert fz["unfreeze_behind_steps"] == [12, 19] and fz["frozen_layer_between_trainable_ones"] == [15]
    assert fz["unfreeze_without_a_step_since_the_freeze"] == [19] and not lo["unfreeze_without_a_step_since_the_freeze"]
    assert lo["adapters_on_frozen_base"] == [2, 3, 5, 8] and lo["reload"] == [7] and lo["merge"] == [10] and lo["no_encoder_layer_trainable"] == [11]
    assert lo["rank_changes"] == lo["targets_change"] == [14] and lo["adapters_on_trainable_base"] == lo["adapters_on_a_subset_of_layers"] == [15]
    assert lo["remove"] == [17]
    for script, under in ((ST.freeze_script(L), fz["stop_is_top_layer_without_input_gradient"]),
                          (ST.lora_script(L), lo["adapters_on_frozen_base"] + lo["adapters_on_trainable_base"]),
                          (ST.dense_lora_script(L), de["dense_targets"])):
        tr = ST.transitions(script)
        for k in ("grows_past_everything", "shrinks_right_after_the_largest", "longer_than_256", "one_sample_labels_on_pair_rows"):
            assert tr[k], k
        shapes = [it[1] for it in script if it[0] not in ST.MUTATIONS]
        assert (1, 8, 8, 8) in shapes and (6, 30, 260, 90) in shapes and set(shapes) <= set(ST.MAIN_SHAPES)
        # the sparse and the dense top-layer backward each occur there, decided from the batches
        assert {ST.top_layer_is_dense(script[i], _BATCH_CFG) for i in under} == {False, True}
        kinds = {it[0] for it in script}
        assert set(ST.TRAINING) <= kinds and len(kinds & set(ST.KINDS)) >= 5
        assert len({it[2] for it in script if it[0] not in ST.MUTATIONS}) == len(shapes)


@pytest.mark.parametrize("L", [3, 4])
def test_the_dense_adapter_script_holds_what_it_is_there_for(L):
    """``ST.dense_lora_script`` from the names alone: where each fact happens, as the script is written down; the adapter records in the
    canonical order of ops.lora_split_targets with the dense targets' module paths; an ``accumulate`` + ``train`` pair under all six
    targets; the one-sample shape at a ``DENSE_TOP_SEEDS`` seed; every inference kind while dense adapters are live; a targets change
    from a set with dense targets to one without and back."""
    from msa_amd import ops
    names = _names(L)
    script = ST.dense_lora_script(L)
    assert ST.misplaced_mutations(script) == []
    de = ST.lifecycle_facts(script, names, L)
    assert de["adapters_on_frozen_base"] == [2, 3, 6, 9] and de["adapters_on_trainable_base"] == de["adapters_on_a_subset_of_layers"] == [16, 19]
    assert de["dense_targets"] == de["ffn_up_adapter"] == [2, 3, 6, 9, 19] and de["dense_only_layer"] == [19]
    assert de["rank_changes"] == de["targets_change"] == [15, 18] and de["reload"] == [8] and de["merge"] == [12] and de["remove"] == [17, 21]
    assert de["no_encoder_layer_trainable"] == [13] and de["unfreeze_behind_steps"] == [14]
    states = ST.lifecycle_states(script, names, L)
    recs = [states[i][1] for i, it in enumerate(script) if it[0] == "add_lora"]
    assert [r["targets"] for r in recs] == [ops.LORA_ALL_TARGETS, ("key",), ("intermediate", "ffn_output")]
    assert [r["r"] for r in recs] == [8, 4, 16] and [r["layers"] for r in recs] == [tuple(range(L)), (0,), (L - 1,)]
    has_dense = [any(t in ops.LORA_DENSE_TARGETS for t in r["targets"]) for r in recs]
    assert has_dense == [True, False, True]                           # with dense targets -> without -> with
    assert ST._lora_record(dict(targets=("ffn_output", "value", "attention_output")), L)["targets"] == ("value", "attention_output", "ffn_output")
    assert ST.LORA_DENSE_PATHS == ops.LORA_DENSE_MODULES and ST.LORA_QKV == ops.LORA_TARGETS
    with pytest.raises(ValueError):
        ST._lora_record(dict(targets=("output",)), L)
    # the flags name the adapters where add_lora puts them, and the base follows freeze_base
    flags = states[2][0]
    lora_names = sorted(n for n in flags if ".lora_" in n)
    assert len(lora_names) == 2 * 6 * L and all(flags[n] for n in lora_names) and ST.base_frozen(flags)
    for t, path in (("query", "attention.self.query"), ("attention_output", "attention.output.dense"), ("intermediate", "intermediate.dense"),
                    ("ffn_output", "output.dense")):
        assert ST.lora_module_path(t) == path and f"bert.encoder.layer.{L - 1}.{path}.lora_B" in flags
    flags = states[19][0]
    assert sorted(n for n in flags if ".lora_" in n) == sorted(f"bert.encoder.layer.{L - 1}.{p}.lora_{m}" for p in ("intermediate.dense", "output.dense") for m in "AB")
    assert not ST.base_frozen(flags) and states[19][2] is None
    # an accumulate + train pair under all six targets; the one-sample shape at a dense-top seed
    assert script[2][0] == "accumulate" and script[3][0] == "train" and states[2][1]["targets"] == states[3][1]["targets"] == ops.LORA_ALL_TARGETS
    assert script[3][1] == (1, 8, 8, 8) and script[3][2] in ST.DENSE_TOP_SEEDS and ST.top_layer_is_dense(script[3], _BATCH_CFG)
    live = {it[0] for it, (_f, lora, _p) in zip(script, states) if it[0] in ST.KINDS and lora is not None and any(t in ops.LORA_DENSE_TARGETS for t in lora["targets"])}
    assert live == set(ST.KINDS), sorted(set(ST.KINDS) - live)
    # ``predict`` runs the [CLS]-only top layer: once under all six targets, once on a top layer with dense adapters and no Q/K/V ones
    assert [states[i][1]["targets"] for i, it in enumerate(script) if it[0] == "predict"] == [ops.LORA_ALL_TARGETS, ("intermediate", "ffn_output")]
    assert len([it for it in script if it[0] not in ST.MUTATIONS]) == 15 and len([it for it in script if it[0] == "train"]) == 8


def test_the_lifecycle_facts_are_computed_not_assumed():
    """Each fact goes missing when the mutation that carries it does."""
    L = 3
    names = _names(L)
    fs, ls = ST.freeze_script(L), ST.lora_script(L)
    drop = lambda s, *idx: [it for i, it in enumerate(s) if i not in idx]           # noqa: E731
    assert not ST.lifecycle_facts(drop(fs, 5), names, L)["stop_is_top_layer_without_input_gradient"]
    assert not ST.lifecycle_facts(drop(fs, 8), names, L)["bias_only_layer"]
    assert not ST.lifecycle_facts(drop(fs, 14), names, L)["frozen_layer_between_trainable_ones"]
    assert ST.lifecycle_facts(drop(fs, 12), names, L)["unfreeze_behind_steps"] == [18]
    assert not ST.lifecycle_facts(drop(fs, 12, 19), names, L)["unfreeze_behind_steps"]
    assert not ST.lifecycle_facts(drop(fs, 18), names, L)["unfreeze_without_a_step_since_the_freeze"]          # (no forward read the frozen flags)
    f = ST.lifecycle_facts(drop(ls, 10, 14), names, L)                               # no merge (and no second add_lora): the first adapters stay
    assert not f["merge"] and not f["no_encoder_layer_trainable"]
    f = ST.lifecycle_facts(drop(ls, 13), names, L)                                   # no unfreeze in front of the second adapters: the base stays frozen
    assert not f["adapters_on_trainable_base"] and not f["unfreeze_behind_steps"] and f["adapters_on_a_subset_of_layers"]
    ds = ST.dense_lora_script(L)
    f = ST.lifecycle_facts(drop(ds, 18, 21), names, L)                               # no third adapter set: no layer with dense adapters alone
    assert not f["dense_only_layer"] and f["dense_targets"] == f["ffn_up_adapter"] == [2, 3, 6, 9]
    f = ST.lifecycle_facts([it if it[0] != "add_lora" or it[3]["seed"] != 81 else ST._mut("add_lora", **dict(it[3], targets=("query", "ffn_output"))) for it in ds], names, L)
    assert f["dense_targets"] == [2, 3, 6, 9, 19] and f["ffn_up_adapter"] == f["dense_only_layer"] == [19]


@pytest.mark.parametrize("L", [3, 4])
def test_mutations_sit_only_at_optimizer_step_boundaries(L):
    for script in (ST.freeze_script(L), ST.lora_script(L), ST.dense_lora_script(L), ST.main_script(), ST.MODES_SCRIPT):
        assert ST.misplaced_mutations(script) == []
        for kind, shape, _seed, options in script:
            assert (shape is None) == (kind in ST.MUTATIONS) and kind in ST.KINDS + ST.MUTATIONS
            assert kind != "add_lora" or "seed" in options
    s = ST.freeze_script(L)
    # ... and the check sees a mutation behind a pending micro-batch, one with a shape, an add_lora without a seed
    assert ST.misplaced_mutations(s[:3] + [ST._mut("unfreeze")] + s[3:]) == [3]
    assert ST.misplaced_mutations([("accumulate", (1, 8, 8, 8), 1, {}), ("predict", (1, 8, 8, 8), 2, {}), ST._mut("freeze", layers=1)]) == [2]
    assert ST.misplaced_mutations([("freeze", (1, 8, 8, 8), None, {})]) == [0]
    assert ST.misplaced_mutations([ST._mut("add_lora", r=4)]) == [0]


@pytest.mark.parametrize("L", [3, 4])
def test_the_gradient_mask_is_empty_where_nothing_is_frozen_and_the_plans_frozen_names_elsewhere(L):
    names = _names(L)
    seen = {"empty": 0, "frozen": 0}
    for script in (ST.freeze_script(L), ST.lora_script(L)):
        for item, (flags, lora, plan) in zip(script, ST.lifecycle_states(script, names, L)):
            if item[0] not in ST.TRAINING:
                assert plan is None
                continue
            off = frozenset(n for n, t in flags.items() if not t)
            mask = ST.grad_mask(plan)
            assert mask == off == (frozenset() if plan is None else plan.frozen)
            assert (lora is None) == (not any(".lora_" in n for n in flags))
            seen["frozen" if mask else "empty"] += 1
    assert seen["empty"] >= 5 and seen["frozen"] >= 9, seen
    assert ST.grad_mask(None) == frozenset()


def test_one_ulp_inside_a_trainable_span_of_a_masked_buffer_still_fails():
    """The mask zero-fills the frozen parameters' spans on both clones and nothing else: garbage there passes, one ulp in a trainable
    span, or in the padding behind the frozen span, does not."""
    offset, numel = {n: o for o, _k, n in LAYOUT}, {n: k for o, k, n in LAYOUT}
    a, b = _result(), _result()
    b["grads"][520:700] = 7.0                                            # what a dropped, then frozen weight gradient leaves behind
    with pytest.raises(AssertionError, match=r"owned by b.weight\[8\]"):
        ST.assert_same_bits(a, b, "item 9 (accumulate)", LAYOUT)
    for r in (a, b):
        ST.zero_spans(r["grads"], offset, numel, ST.grad_mask(None))
    with pytest.raises(AssertionError, match=r"owned by b.weight\[8\]"):
        ST.assert_same_bits(a, b, "item 9 (accumulate)", LAYOUT)          # (an empty mask changes nothing)
    for r in (a, b):
        ST.zero_spans(r["grads"], offset, numel, frozenset({"b.weight"}))
    ST.assert_same_bits(a, b, "item 9 (accumulate)", LAYOUT)
    for index, owner in ((100, r"a.weight\[100\]"), (768, r"c.bias\[0\]"), (400, "padding between parameters")):
        c = dict(b, grads=_one_ulp(b["grads"], index))
        with pytest.raises(AssertionError, match="owned by " + owner):
            ST.assert_same_bits(a, c, "item 9 (accumulate)", LAYOUT)
    c = dict(b, grads=b["grads"].clone())
    c["grads"][768] = 3.0                                                # the first element behind the masked span
    ST.zero_spans(c["grads"], offset, numel, frozenset({"b.weight"}))
    with pytest.raises(AssertionError, match=r"c.bias\[0\]"):
        ST.assert_same_bits(a, c, "item 9 (accumulate)", LAYOUT)


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
