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
is a copy)."""
import pytest
import torch

from msa_amd import freeze as FZ
from tests import step_stages as SS
from tests.test_model_gpu import _report
from tests.test_step_stages_gpu import CFG, _batch, _model, _step

pytestmark = pytest.mark.gpu

_PARITY = {}
_QV = dict(r=4, alpha=8.0, targets=("query", "value"), freeze_base=True, seed=3)


def _frozen_top(m, L):
    m.freeze(embeddings=True, layers=L - 1, layer_weights=True)


def _adapters_on_a_frozen_base(m, L):
    m.add_lora(**_QV)


def _adapters_on_the_top_layer(m, L):
    m.add_lora(r=16, alpha=16.0, targets=("key",), layers=[L - 1], freeze_base=False, seed=3)


CASES = {"i_bias_only_top_layer": (_frozen_top, None), "ii_adapters_on_a_frozen_base": (_adapters_on_a_frozen_base, None),
         "iii_adapters_on_the_top_layer": (_adapters_on_the_top_layer, None), "iv_behind_a_merge": (_adapters_on_a_frozen_base, "merge_lora")}
RUNS = [("i_bias_only_top_layer", "A"), ("i_bias_only_top_layer", "B"), ("ii_adapters_on_a_frozen_base", "A"), ("ii_adapters_on_a_frozen_base", "B"),
        ("iii_adapters_on_the_top_layer", "A"), ("iv_behind_a_merge", "A")]


def expected(plan, lora, L):
    """The launch counts the plan (None: nothing frozen) and the adapter record (None: no adapters) decide, for one forward + backward."""
    stop = 0 if plan is None else plan.stop
    emb = plan is None or plan.embedding_stage
    layers = () if lora is None else lora["layers"]
    colsum = 0
    if plan is not None:
        colsum += sum(1 for i in range(stop, L) if any(v == FZ.BIAS for v in plan.layers[i].values()))
        colsum += 1 if (not plan.word_table and "cls.predictions.bias" not in plan.frozen) else 0
    return {"attn_fwd": L, "attn_bwd": max(0, L - stop), "lora_qkv_fwd": len(layers), "lora_qkv_bwd": sum(1 for i in layers if i >= stop),
            "colsum_grouped": colsum, "embed_scatter": 1 if emb else 0, "pair_proj_bwd": 2 if emb else 0}


@pytest.mark.parametrize("case,cfg", RUNS, ids=[f"{c}-{k}" for c, k in RUNS])
def test_every_launch_of_a_frozen_or_adapter_step_is_within_its_reference_bound(case, cfg):
    from msa_amd.optim import AdamW
    L = CFG[cfg]["layers"]
    setup, then = CASES[case]
    m = _model(cfg, True, True)
    setup(m, L)
    opt = AdamW(m.parameters(), lr=1e-2)
    _step(m, _batch(5))
    opt.step()
    if then is not None:
        getattr(m, then)()
    assert m.training and m.bert.jointEmbeddings.training
    with SS.record(m) as calls:
        _step(m, _batch(61))
    plan, lora = m.__dict__.get("_tplan"), m._lora
    assert (plan is None) == (case == "iii_adapters_on_the_top_layer") and (lora is None) == (case in ("i_bias_only_top_layer", "iv_behind_a_merge"))
    if case == "i_bias_only_top_layer":
        assert plan.stop == L - 1 and not plan.embedding_stage and set(plan.layers[L - 1].values()) == {FZ.BIAS}
    elif case == "ii_adapters_on_a_frozen_base":
        assert plan.stop == 0 and not plan.embedding_stage and all(set(plan.layers[i].values()) == {FZ.NONE} for i in range(L))
        assert all(bool((m._lw[i]["lora"]["B"][t] != 0).any()) for i in range(L) for t in ("query", "value")), "B moved with the first step"
    elif case == "iv_behind_a_merge":
        assert plan.stop == L and not plan.embedding_stage and not plan.word_table
    per = SS.recompute_all(calls, m)
    print(case, cfg, {k: (n, round(w, 4)) for k, (n, w) in sorted(per.items())})
    _PARITY[f"{case} {cfg}"] = {k: dict(calls=n, worst_ratio=w) for k, (n, w) in sorted(per.items())}
    _report("lifecycle_parity", _PARITY)
    passes, sites, writes = SS.check_dataflow_frozen(calls, m, plan, lora)
    stop = 0 if plan is None else plan.stop
    assert passes == {"fwd": 1, "bwd": 1 if stop < L else 0}, passes
    assert sites == 3 * L + 1 + 2, sites
    assert writes > 0
    folded = [id(x) for c in calls if c.op == "ln_bwd_reduce" for x in c.meta["calls"]]
    assert sorted(folded) == sorted(id(c) for c in calls if c.op == "ln_bwd"), "a LayerNorm' call folded twice or never"
    want = expected(plan, lora, L)
    got = {k: per.get(k, (0, 0.0))[0] for k in want}
    assert got == want, (case, cfg, got, want)
    # the arguments the model passes: no residual gradient where backward ends, accumulation onto what the optimizer left
    for c in calls:
        if c.op == "lora_qkv_bwd":
            ends = plan is not None and not plan.embedding_stage and c.meta["layer"] == plan.stop
            assert (c.a["dres"] is None) == ends and (c.ret is None) == ends and c.a["accumulate"] is True and c.a["h"] is not None
        if c.op == "colsum_grouped":
            assert all(SS.colsum_flags(c))
    assert bool(torch.isfinite(m._flat.grads).all())
