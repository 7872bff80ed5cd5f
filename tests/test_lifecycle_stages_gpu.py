"""A frozen step and an adapter step, launch by launch in float64 (tests/step_stages.py), with the arguments the MODEL passes: ``h[:rows]``
slices, ``dres=None`` at the layer where backward ends, ``accumulate=True`` onto what the optimizer left, the sparse top layer's mixed
few-row / all-row problem split, the grouped column sum of a bias-only layer.

One recorded step per test (the float64 recomputation is what takes the time), default (non-deterministic) mode, the batch and the two
small configurations of tests/test_step_stages_gpu.py (4 x 24 / 200 / 130; A: hidden 128, two layers; B: hidden 256, three), train mode with
all dropouts on, short cuts on, on a model that has already taken one optimizer step -- the adapters' B is non-zero and the lazily
zeroed gradients are dropped.  Every launch is inside its own family's bound (``SS.recompute_all``: tests/lora_ref.py's for the adapter
launches, tests/colsum_ref.py's for the column sums -- no bound is set here), the frozen form of the dataflow checks passes
(``SS.check_dataflow_frozen``; ``_wiring`` and ``check_grad_views`` assume a full backward and are not part of it), no launch writes a
frozen parameter's part of the gradient buffer, and the launch counts that the plan and the adapter record decide are exact.  The worst
ratios are reported as ``lifecycle_parity`` (tests/test_model_gpu.py::_report; a record, not a threshold; profiles/lifecycle_parity.json
is a copy).

Cases v - x put adapters on the dense seams (attention.output.dense, intermediate.dense, output.dense; tests/lora_dense_ref.py judges their
launches): v all six targets, r = 8, on a frozen base, at A and B -- the sparse top layer (gathered operands, ``h=None``, the split-K ``dy1``
updated in place), ``dres=None`` where backward ends, all three dense stages on every layer; vi the dense targets alone, r = 4, over a
trainable base with ``sparse_top_layer_backward = False`` -- ``h[:rows]`` slices on every layer, the W1 weight-gradient problem reading the
final ``du`` (``check_producers``); vii ``intermediate`` + ``ffn_output``, r = 16, on the top layer alone over a trainable base -- a layer with
dense adapters and no Q/K/V ones next to plain layers; viii the hidden dropout off -- ``thr16 == 0`` triples and LayerNorm' own output as the
adapter's ``dy``; ix two eval-mode forwards with labels under ``no_grad`` and no backward: the model's forward, which still keeps its
activations there, and ``predict_tokens``, which keeps nothing (``h_out=None``, ``aux=None`` in GELU mode); x the step behind ``merge_lora()``
of case v -- no adapter launch, the GELU epilogue back on every FFN-up GEMM.  Every case: ``SS.check_dataflow_frozen`` with
``SS.check_dense_adapter_wiring`` inside.  On every ``lora_qkv_bwd`` / ``lora_dense_bwd`` call of all ten cases the ``gA`` / ``gB`` found are
exactly zero: the recorded step is the first backward behind an optimizer step and the call accumulates."""
import pytest
import torch

from msa_amd import freeze as FZ
from tests import step_stages as SS
from tests.test_model_gpu import _report
from tests.test_step_stages_gpu import CFG, _batch, _model, _step

pytestmark = pytest.mark.gpu

_PARITY = {}
_QV = dict(r=4, alpha=8.0, targets=("query", "value"), freeze_base=True, seed=3)
_QKV = ("query", "key", "value")
_DENSE = ("attention_output", "intermediate", "ffn_output")


def _frozen_top(m, L):
    m.freeze(embeddings=True, layers=L - 1, layer_weights=True)


def _adapters_on_a_frozen_base(m, L):
    m.add_lora(**_QV)


def _adapters_on_the_top_layer(m, L):
    m.add_lora(r=16, alpha=16.0, targets=("key",), layers=[L - 1], freeze_base=False, seed=3)


def _all_linear_on_a_frozen_base(m, L):
    m.add_lora(r=8, alpha=16.0, targets="all-linear", freeze_base=True, seed=3)


def _dense_only_dense_top(m, L):
    m.sparse_top_layer_backward = False
    m.add_lora(r=4, alpha=8.0, targets=_DENSE, freeze_base=False, seed=3)


def _ffn_adapters_on_the_top_layer(m, L):
    m.add_lora(r=16, alpha=16.0, targets=("intermediate", "ffn_output"), layers=[L - 1], freeze_base=False, seed=3)


def _no_hidden_dropout(m, L):
    m.config.hidden_dropout_prob = 0.0
    m.add_lora(r=8, alpha=16.0, targets=("attention_output", "ffn_output"), freeze_base=True, seed=3)


# case -> (setup, what is called between the optimizer step and the recorded pass, the recorded pass: a training step or an eval forward)
CASES = {"i_bias_only_top_layer": (_frozen_top, None, "step"), "ii_adapters_on_a_frozen_base": (_adapters_on_a_frozen_base, None, "step"),
         "iii_adapters_on_the_top_layer": (_adapters_on_the_top_layer, None, "step"), "iv_behind_a_merge": (_adapters_on_a_frozen_base, "merge_lora", "step"),
         "v_all_linear_on_a_frozen_base": (_all_linear_on_a_frozen_base, None, "step"), "vi_dense_only_dense_top_layer": (_dense_only_dense_top, None, "step"),
         "vii_ffn_adapters_on_the_top_layer": (_ffn_adapters_on_the_top_layer, None, "step"), "viii_no_hidden_dropout": (_no_hidden_dropout, None, "step"),
         "ix_eval_forward_all_linear": (_all_linear_on_a_frozen_base, None, "eval"), "x_behind_a_merge_of_all_linear": (_all_linear_on_a_frozen_base, "merge_lora", "step")}
RUNS = [("i_bias_only_top_layer", "A"), ("i_bias_only_top_layer", "B"), ("ii_adapters_on_a_frozen_base", "A"), ("ii_adapters_on_a_frozen_base", "B"),
        ("iii_adapters_on_the_top_layer", "A"), ("iv_behind_a_merge", "A"), ("v_all_linear_on_a_frozen_base", "A"), ("v_all_linear_on_a_frozen_base", "B"),
        ("vi_dense_only_dense_top_layer", "A"), ("vii_ffn_adapters_on_the_top_layer", "A"), ("viii_no_hidden_dropout", "A"),
        ("ix_eval_forward_all_linear", "A"), ("x_behind_a_merge_of_all_linear", "A")]
NO_PLAN = ("iii_adapters_on_the_top_layer", "vi_dense_only_dense_top_layer", "vii_ffn_adapters_on_the_top_layer")       # (a trainable base)
NO_ADAPTERS = ("i_bias_only_top_layer", "iv_behind_a_merge", "x_behind_a_merge_of_all_linear")


def expected(plan, lora, L, backward=True, forwards=1, sparse_top=True):
    """The launch counts the plan (None: nothing frozen) and the adapter record (None: no adapters) decide, for one forward + backward
    (``backward`` False: ``forwards`` forward passes alone): one Q/K/V adapter launch per adapted layer (when a Q/K/V target is there), one dense adapter
    launch per dense target and adapted layer -- backward on the adapted layers at or above ``stop``.  The seam: one prologue per forward
    pass, one ``pack_i64`` per model forward, the heads' forward in two calls (levels 1 - 6 prelaunched on the side stream, level 7), with
    a backward ``heads_step_dmlm`` + ``heads_step_bwd`` and -- where the top layer runs its sparse backward -- one ``compact_rows``; the eval
    case's ``predict_tokens`` makes its own labelled-row list (``active_rows``)."""
    stop = 0 if plan is None else plan.stop
    emb = plan is None or plan.embedding_stage
    layers = () if lora is None else lora["layers"]
    qkv = 1 if lora is not None and any(t in _QKV for t in lora["targets"]) else 0
    dense = 0 if lora is None else sum(1 for t in _DENSE if t in lora["targets"])
    above = sum(1 for i in layers if i >= stop)
    colsum = 0
    if plan is not None:
        colsum += sum(1 for i in range(stop, L) if any(v == FZ.BIAS for v in plan.layers[i].values()))
        colsum += 1 if (not plan.word_table and "cls.predictions.bias" not in plan.frozen) else 0
    want = {"attn_fwd": forwards * L, "attn_bwd": max(0, L - stop), "lora_qkv_fwd": forwards * qkv * len(layers), "lora_qkv_bwd": qkv * above,
            "lora_dense_fwd": forwards * dense * len(layers), "lora_dense_bwd": dense * above,
            "colsum_grouped": colsum, "embed_scatter": 1 if emb else 0, "pair_proj_bwd": 2 if emb else 0,
            "prologue": forwards, "pack_i64": 1, "heads_step_fwd": 2, "heads_step_dmlm": 1, "heads_step_bwd": 1,
            "compact_rows": 1 if stop < L and sparse_top else 0, "active_rows": 0 if backward else 1}
    if not backward:
        want.update({k: 0 for k in ("attn_bwd", "lora_qkv_bwd", "lora_dense_bwd", "colsum_grouped", "embed_scatter", "pair_proj_bwd",
                                    "heads_step_dmlm", "heads_step_bwd", "compact_rows")})
    return want


def _zero(rec):
    return rec is None or not bool((rec.cpu() != 0).any())


@pytest.mark.parametrize("case,cfg", RUNS, ids=[f"{c}-{k}" for c, k in RUNS])
def test_every_launch_of_a_frozen_or_adapter_step_is_within_its_reference_bound(case, cfg):
    from msa_amd.optim import AdamW
    L = CFG[cfg]["layers"]
    setup, then, what = CASES[case]
    m = _model(cfg, True, True)
    setup(m, L)
    opt = AdamW(m.parameters(), lr=1e-2)
    _step(m, _batch(5))
    opt.step()
    if then is not None:
        getattr(m, then)()
    assert m.training and m.bert.jointEmbeddings.training
    backward = what == "step"
    if backward:
        with SS.record(m) as calls:
            _step(m, _batch(61))
    else:
        # two forward passes with labels in eval mode, no backward: the model's forward under no_grad -- which still keeps its activations
        # (model._TrunkFn: needs_input_grad stays set under no_grad), so h_out and aux are handed in -- and predict_tokens with the labels,
        # the dense inference path that keeps nothing: h_out = None, aux = None in GELU mode
        m.eval()
        b = _batch(61)
        with torch.no_grad(), SS.record(m) as calls:
            m(**b)
            m.predict_tokens(b["input_ids"], b["token_type_ids"], b["attention_mask"], masked_labels=b["masked_labels"], top_k=5)
    plan, lora = m.__dict__.get("_tplan"), m._lora
    assert (plan is None) == (case in NO_PLAN) and (lora is None) == (case in NO_ADAPTERS)
    if case == "i_bias_only_top_layer":
        assert plan.stop == L - 1 and not plan.embedding_stage and set(plan.layers[L - 1].values()) == {FZ.BIAS}
    elif case in ("ii_adapters_on_a_frozen_base", "v_all_linear_on_a_frozen_base", "viii_no_hidden_dropout", "ix_eval_forward_all_linear"):
        assert plan.stop == 0 and not plan.embedding_stage and all(set(plan.layers[i].values()) == {FZ.NONE} for i in range(L))
        assert all(bool((m._lw[i]["lora"]["B"][t] != 0).any()) for i in range(L) for t in lora["targets"] if t in _QKV), "B moved with the first step"
    elif case in ("iv_behind_a_merge", "x_behind_a_merge_of_all_linear"):
        assert plan.stop == L and not plan.embedding_stage and not plan.word_table
    if lora is not None:
        assert all(bool((m._lw[i]["lora_dense"]["B"][t] != 0).any()) for i in lora["layers"] for t in lora["targets"] if t in _DENSE), "B moved with the first step"
    per = SS.recompute_all(calls, m)
    print(case, cfg, {k: (n, round(w, 4)) for k, (n, w) in sorted(per.items())})
    _PARITY[f"{case} {cfg}"] = {k: dict(calls=n, worst_ratio=w) for k, (n, w) in sorted(per.items())}
    _report("lifecycle_parity", _PARITY)
    passes, sites, writes = SS.check_dataflow_frozen(calls, m, plan, lora, backward=backward)
    stop = 0 if plan is None else plan.stop
    forwards = 1 if backward else 2
    assert passes == {"fwd": forwards, "bwd": 1 if stop < L and backward else 0}, passes
    # (the hidden dropout feeds 2 L + 1 of the sites: the two residual seams of every layer and the embedding's)
    assert sites == (0 if not backward else L + 2 if case == "viii_no_hidden_dropout" else 3 * L + 1 + 2), sites
    assert (writes > 0) == backward
    folded = [id(x) for c in calls if c.op == "ln_bwd_reduce" for x in c.meta["calls"]]
    assert sorted(folded) == sorted(id(c) for c in calls if c.op == "ln_bwd"), "a LayerNorm' call folded twice or never"
    want = expected(plan, lora, L, backward, forwards, getattr(m, "sparse_top_layer_backward", True))
    got = {k: per.get(k, (0, 0.0))[0] for k in want}
    assert got == want, (case, cfg, got, want)
    # the arguments the model passes: no residual gradient where backward ends, accumulation onto what the optimizer left -- which is
    # exactly zero (the recorded step is the first backward behind an optimizer step: a launch that ignored ``accumulate`` would leave
    # the same bits, a twin cannot see it; a launch that found anything else there shows a stale gradient)
    for c in calls:
        if c.op == "lora_qkv_bwd":
            ends = plan is not None and not plan.embedding_stage and c.meta["layer"] == plan.stop
            assert (c.a["dres"] is None) == ends and (c.ret is None) == ends and c.a["accumulate"] is True and c.a["h"] is not None
            assert all(_zero(r) for k in ("gA", "gB") for r in (c.a[k] or {}).values()), f"call {c.index}: lora_qkv_bwd found a non-zero gradient"
        if c.op == "lora_dense_bwd":
            assert c.a["accumulate"] is True and c.a["dx"] is not None and _zero(c.a["gA"]) and _zero(c.a["gB"]), f"call {c.index}: lora_dense_bwd found a non-zero gradient"
        if c.op == "colsum_grouped":
            assert all(SS.colsum_flags(c))
    _case_specific(case, calls, m, lora, L)
    assert bool(torch.isfinite(m._flat.grads).all())


def _case_specific(case, calls, m, lora, L):
    """What each dense-adapter case is there for, asserted from the recorded arguments."""
    fwd = [c for c in calls if c.op == "lora_dense_fwd"]
    bwd = [c for c in calls if c.op == "lora_dense_bwd"]
    stage = lambda st, l: [c for c in calls if c.meta["stage"] == st and c.meta["layer"] == l]          # noqa: E731
    if case in ("v_all_linear_on_a_frozen_base", "vii_ffn_adapters_on_the_top_layer"):
        # the sparse top layer: gathered operands, h recomputed, the split-K dy1 updated in place; saved h slices below it
        top = [c for c in bwd if c.meta["layer"] == L - 1]
        assert top and all(c.a["h"] is None and c.a["dy"].shape[0] < stage("z2", L - 1)[0].ret.shape[0] for c in top)
        assert stage("dy1", L - 1)[0].op == "gemm_nt_splitk" and stage("lora_dy1", L - 1)[0].a["dx"].region() == stage("dy1", L - 1)[0].ret.region()
        assert all(c.a["h"] is not None for c in bwd if c.meta["layer"] < L - 1)
    if case == "v_all_linear_on_a_frozen_base":
        assert {(c.meta["stage"], c.meta["layer"]) for c in fwd} == {(s, l) for s in SS.DENSE_FWD_STAGE.values() for l in range(L)}
        assert {(c.meta["stage"], c.meta["layer"]) for c in bwd} == {(s, l) for s in SS.DENSE_BWD_STAGE.values() for l in range(L)}
        assert not stage("dx", 0) and [c.a["dres"] is None for c in calls if c.op == "lora_qkv_bwd"] == [False] * (L - 1) + [True]
    elif case == "vi_dense_only_dense_top_layer":
        # h[:rows] slices on every layer (a split layout: backward visits the leading rows only), no Q/K/V adapter anywhere
        assert len(bwd) == 3 * L and all(c.a["h"] is not None and c.a["h"].shape[0] == c.a["dy"].shape[0] for c in bwd)
        rows_f, rows_b = fwd[0].a["h_out"].shape[0], bwd[0].a["h"].shape[0]
        assert rows_b < rows_f, "backward on fewer rows than forward: h is a proper row slice"
        assert all(m._lw[i]["lora"] is None for i in range(L)) and not any(c.op.startswith("lora_qkv") for c in calls)
        assert not any(c.op in ("gemm_nt_splitk", "scatter_rows_zero") and c.meta["layer"] is not None for c in calls)
    elif case == "vii_ffn_adapters_on_the_top_layer":
        assert lora["layers"] == (L - 1,) and m._lw[L - 1]["lora"] is None and all(m._lw[i]["lora_dense"] is None for i in range(L - 1))
        assert [c.meta["stage"] for c in fwd] == ["lora_g", "lora_z2"] and [c.meta["stage"] for c in bwd] == ["lora_du", "lora_dy1"]
        assert all(stage("g", l)[0].a["gelu"] for l in range(L - 1)) and not stage("g", L - 1)[0].a["gelu"]
    elif case == "viii_no_hidden_dropout":
        # thr16 == 0 triples on the ADD seams; LayerNorm' hands out ONE gradient: the adapter's dy is the very buffer the residual path reads
        assert fwd and all(int(c.a["mode"]) == 0 and c.a["drop"] is not None and c.a["drop"][1] == 0 for c in fwd)
        for st, ln in (("lora_du", "ln2_bwd"), ("lora_dctx", "ln1_bwd")):
            for l in range(L):
                lb, ad = stage(ln, l)[0], stage(st, l)[0]
                assert lb.a["dx2"] is None and ad.a["dy"].region() == lb.ret.region(), f"layer {l} {st}: dy is not LayerNorm' own output"
        assert any(SS._on(c.a["drop"]) for c in calls if c.op == "attn_fwd")
    elif case == "ix_eval_forward_all_linear":
        assert len(fwd) == 2 * 3 * L and not bwd and not any(SS._on(c.a["drop"]) for c in fwd)
        kept, lean = fwd[:3 * L], fwd[3 * L:]                      # (the forward under no_grad | predict_tokens)
        assert all(c.a["h_out"] is not None and (c.a["aux"] is not None) == (int(c.a["mode"]) == 1) for c in kept)
        assert all(c.a["h_out"] is None and c.a["aux"] is None for c in lean) and [int(c.a["mode"]) for c in lean] == [0, 1, 0] * L
        assert [c.a["h_out"] is None for c in calls if c.op == "lora_qkv_fwd"] == [False] * L + [True] * L
    elif case == "x_behind_a_merge_of_all_linear":
        assert not fwd and not bwd and not any(c.op.startswith("lora_") for c in calls)
        ups = [c for c in calls if c.meta["stage"] == "g"]
        # (the GELU epilogue is back on every FFN-up GEMM; its aux is kept where a backward will read it: behind the merge of adapters
        # over a frozen base no encoder layer is trainable -- plan.stop == L --, so no layer keeps its pre-activation)
        stop = m.__dict__["_tplan"].stop
        assert len(ups) == L and all(c.a["gelu"] and not c.a["resid"] and (c.a["aux"] is not None) == (c.meta["layer"] >= stop) for c in ups), \
            "an FFN-up GEMM without its GELU epilogue behind the merge"
