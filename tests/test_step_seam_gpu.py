"""The seam between the last encoder LayerNorm of the forward pass and the first launch of the encoder's backward, in situ: the fused
heads (``heads_step_fwd`` / ``heads_step_dmlm`` / ``heads_step_bwd``), the step prologue and the row lists (``prologue``, ``compact_rows``,
``pack_i64``, ``active_rows``) of a real training step, recorded by tests/step_stages.py -- the heads through the tensors
model._HeadsStepFn hangs onto its argument record --, each recomputed from its own recorded operands by the reference the project already
has (tests/heads_ref.py, heads_cls_ref.py, heads_multilabel_ref.py, loss_options_ref.py by the record's fields; tests/layout_ref.py,
exact), and the hand-overs between them checked with exact comparisons (``step_stages.check_seam``; the [CLS] rows of the output gradient
through ``check_producers``).  No tolerance of its own.

The configurations and the batch are tests/test_step_stages_gpu.py's (A: hidden 128, B: hidden 256; 4 samples, 12 [CLS] rows).  Before
the step the 24 head parameters are loaded from ``make_case(4, H, seed, ...).params`` (as tests/test_heads_gpu.py::_load does): at the
initialisation scale several terms of the heads vanish.  The trunk's launches of these configurations are recomputed by
tests/test_step_stages_gpu.py; here they are recorded, counted and part of every dataflow check, and ``SEAM_OPS`` are recomputed.

Preconditions, not tolerances: the heads' references hold only where fp32 and float64 take the same side of relu (``kink_ratio``), of
the argmax (``gap_ratio``), of the thresholds (``decision_ratio``) and of the L1 / Huber kink (``loss_kink_ratio``) -- each >= 64 bounds.
In situ the [CLS] rows come out of the encoder and cannot be redrawn, so every case takes its model and batch seed from ``SEEDS``: the
first for which the conditions hold on the MI355X is written into ``SEED``; the adapter asserts them on the recorded operands (a
violation fails and says that it is one; no element or sample is left out) and the ratios reached go into the parity record
(``_report("step_seam_parity", ...)``, a copy in profiles/step_seam_parity.json; the suites that record whole steps keep theirs in
``step_stage_parity`` with the new op kinds in it).

No case under ``torch.cuda.graph``: no suite of the project captures a training step (tests/test_session_twin_gpu.py has no pattern for
it), and the recorder clones operands between the launches, which a capture would record as part of the graph."""
import pytest
import torch

from msa_amd.data import batch_to, synthetic_batch
from tests import heads_cls_ref as HCR
from tests import heads_multilabel_ref as HML
from tests import heads_ref as HR
from tests import loss_options_ref as LOR
from tests import step_stages as SS
from tests.test_model_gpu import _report, build
from tests.test_step_stages_gpu import CFG, expected_counts

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = (29, 31, 37, 41, 43, 47, 53, 59)
# case -> the first seed of SEEDS whose recorded [CLS] rows meet the references' preconditions (chosen on the MI355X; default SEEDS[0])
SEED = {"regression 1 eval side on": 31, "regression 1 eval side off": 31}       # (seed 29 there: kink_ratio 29.4)
HUBER_DELTA = 0.5
_PARITY = {}


def seed_of(case):
    return SEED.get(case, SEEDS[0])


def _batch(seed, head="reg"):
    C = {"cls": 3, "weights": 3, "multi": 6}.get(head)
    b = synthetic_batch(4, 24, 200, 130, dataset="mosei", vocab=4096, seed=seed, num_labels=C)
    if head == "multi":
        t = HML.targets_for(4, 6, torch.Generator().manual_seed(seed))
        t[1, 2] = -1.0                                              # one entry that is not annotated
        b["sentiment"] = t
    return b


def _model(cfg, seed, head="reg", num_labels=7, train=True, side=True):
    """tests/test_step_stages_gpu.py::_model (short cuts on) with the head under test and the 24 head parameters of the matching
    ``make_case``."""
    H = CFG[cfg]["hidden"]
    m = build(CFG[cfg], train=train)
    m.manual_seed(seed)
    m.composite_layers = False
    m.defer_wgrads = True
    m.heads_side_stream = side
    if head == "reg" or head == "huber":
        m.num_labels = num_labels
        params = HR.make_case(4, H, seed, num_labels=num_labels).params
    else:
        C = 6 if head == "multi" else 3
        m.set_num_labels(C, multi_label=head == "multi")
        params = HCR.make_case(4, H, seed, C).params
    if head == "huber":
        m.set_loss_options(regression="huber", huber_delta=HUBER_DELTA)
    elif head == "weights":
        m.set_loss_options(class_weights=LOR.class_weights_for(3, seed).tolist(), label_smoothing=0.1)
    own = dict(m.named_parameters())
    with torch.no_grad():
        for n, t in params.items():
            assert own[n].shape == t.shape, (n, tuple(own[n].shape), tuple(t.shape))
            own[n].copy_(t.to(DEV))
    m.parameters_changed()
    return m


def _step(m, batch):
    out, _logits = m(**batch)
    if torch.is_grad_enabled():
        out[0].mean().backward()
    return out


def seam_counts(L, steps=1, side=True, sparse_top=True, label_only=False):
    """``expected_counts`` (short cuts on) for the cases of this module: the dense hand-over has no ``compact_rows`` and none of the sparse
    top layer's helpers; a label-only step has no MLM-head op, no ``heads_step_dmlm``, no prelaunch (one forward call), no embedding of
    labels in ``pack_i64`` (still one call) -- and its top layer runs on the [CLS] rows alone."""
    c = expected_counts(L, True, 1, side)
    if not sparse_top:
        c["gemm_nt"] += 1
        c["gemm_nt_splitk"] -= 1
        c["gather_rows"] -= 1
        for k in ("scatter_rows_zero", "attn_q_limit", "compact_rows"):
            del c[k]
    if label_only:
        for k in ("ce_fwd", "ce_bwd", "gelu_bwd", "heads_step_dmlm"):
            c.pop(k, None)
        c["heads_step_fwd"] = 1
        c["gemm_nt_splitk"] -= 1                                    # (the vocabulary product's)
        c["gather_rows"] -= 1                                       # (the MLM head's gather of its labelled rows)
    return {k: v * steps for k, v in c.items()}


SEAM_KEYS = SS.SEAM_OPS + ("ce_fwd", "ce_bwd", "gelu_bwd", "gemm_nt_splitk", "gather_rows", "scatter_rows_zero", "attn_q_limit")


def _judge(calls, m, case, want, want_ran, frozen=None, keys=SEAM_KEYS):
    """Every seam op recomputed by its reference, the dataflow checks of the whole step, the counts of the seam's ops from the model's
    structure, the named checks of ``check_seam`` that must have run, the parity record."""
    per = SS.recompute_all(calls, m, only=SS.SEAM_OPS)
    print(case, {k: (n, round(w, 4)) for k, (n, w) in sorted(per.items()) if k in SS.SEAM_OPS})
    if frozen is None:
        SS.check_dataflow(calls, m)
    else:
        SS.check_dataflow_frozen(calls, m, *frozen)
    _expect, ran = SS.check_seam(calls, m)
    print(case, "checks", ran)
    got = {k: per.get(k, (0, 0.0))[0] for k in keys if per.get(k, (0, 0.0))[0] or want.get(k, 0)}
    assert got == {k: v for k, v in want.items() if k in keys and v}, (case, got, want)
    for k, n in want_ran.items():
        assert ran.get(k, 0) == n, (case, k, ran)
    pre = SS.preconditions(calls)                                 # asserted on the recorded operands: a violation fails and says so
    assert pre, "no heads call was judged"
    _PARITY[case] = {k: dict(calls=n, worst_ratio=w) for k, (n, w) in sorted(per.items()) if k in SS.SEAM_OPS}
    _PARITY[case]["preconditions"] = dict(seed=seed_of(case), **pre)
    _report("step_seam_parity", _PARITY)
    return per, ran


def _ran(steps=1, side=True, train=True, compact=True, label_only=False):
    r = {"prologue consumers": None, "heads y": steps * (2 if side and not label_only else 1), "heads first_rows": steps * (2 if side and not label_only else 1),
         "heads forward finals": steps if side and not label_only else 0, "mlm losses": 0 if label_only else steps,
         "dmlm twice": steps if side and not label_only else 0, "gscale": 0 if label_only else steps, "heads gradient views": steps,
         "compact row list": steps if compact else 0, "compact hand-over": steps if compact else 0, "dense hand-over": 0 if compact else steps,
         "label-only step": steps if label_only else 0}
    return {k: v for k, v in r.items() if v is not None}


def run_case(case, seed):
    """One case of the module at one seed (gpu_jobs' seed search calls it with the seeds of ``SEEDS`` in turn)."""
    kind, cfg, kw = CASES[case]
    L = CFG[cfg]["layers"]
    head = kw.get("head", "reg")
    m = _model(cfg, seed, head, kw.get("num_labels", 7), kw.get("train", True), kw.get("side", True))
    batch = batch_to(_batch(seed, head), DEV)
    side = kw.get("side", True)
    if kind == "step":
        with SS.record(m) as calls:
            _step(m, batch)
        return _judge(calls, m, case, seam_counts(L, 1, side), _ran(1, side))
    if kind == "label_only":
        with SS.record(m) as calls:
            _step(m, dict(batch, masked_labels=None))
        res = _judge(calls, m, case, seam_counts(L, 1, side, label_only=True), _ran(1, side, label_only=True))
        assert not any(str(c.meta.get("stage")).startswith("mlm_") for c in calls), "an MLM-head stage on a label-only step"
        return res
    if kind == "dense_top":
        m.sparse_top_layer_backward = False
        with SS.record(m) as calls:
            _step(m, batch)
        return _judge(calls, m, case, seam_counts(L, 1, side, sparse_top=False), _ran(1, side, compact=False))
    if kind == "freeze":
        m.freeze(embeddings=True, layers=1)
        with SS.record(m) as calls:
            _step(m, batch)
        plan = m.__dict__.get("_tplan")
        assert plan is not None and plan.stop == 1 and not plan.embedding_stage, (plan.stop, plan.embedding_stage)
        want = seam_counts(L, 1, side)
        return _judge(calls, m, case, want, _ran(1, side), frozen=(plan, None), keys=SS.SEAM_OPS + ("ce_fwd", "ce_bwd", "gelu_bwd"))
    if kind == "lora":
        m.add_lora(r=8, alpha=16.0, targets=("query", "value"), freeze_base=False, seed=3)
        with SS.record(m) as calls:
            _step(m, batch)
        return _judge(calls, m, case, seam_counts(L, 1, side), _ran(1, side), frozen=(m.__dict__.get("_tplan"), m._lora),
                      keys=SS.SEAM_OPS + ("ce_fwd", "ce_bwd", "gelu_bwd"))
    if kind == "two_micro_batches":
        from msa_amd.optim import AdamW
        opt = AdamW(m.parameters(), lr=1e-3)
        _step(m, batch_to(_batch(5), DEV))
        opt.step()
        with SS.record(m) as calls:
            _step(m, batch)
            _step(m, batch_to(_batch(seed + 1), DEV))
        per, ran = _judge(calls, m, case, seam_counts(L, 2, side), _ran(2, side))
        # the second backward's 22 gradient operands found what the first left (check_producers) -- and that is not zero
        bwd = [c for c in calls if c.op == "heads_step_bwd"]
        assert len(bwd) == 2 and all(SS._eq(bwd[0].post[g], bwd[1].a[g]) and bool((bwd[1].a[g].cpu() != 0).any()) for g in SS.HEAD_GRADS)
        return per, ran
    if kind == "async_prologue":
        with torch.cuda.stream(m.input_stream):                    # the batches are made on the input stream and complete before the first forward
            b1, b2 = batch_to(_batch(seed, head), DEV), batch_to(_batch(seed + 1, head), DEV)
        torch.cuda.synchronize()
        m.async_prologue = True
        with SS.record(m) as calls:
            _step(m, b1)
            _step(m, b2)
        pro = [c for c in calls if c.op == "prologue"]
        assert len(pro) == 2 and all(c.a["bufs"] is not None for c in pro) and all(c.meta["stream"] == m.input_stream.cuda_stream for c in pro)
        want_ran = dict(_ran(2, side), **{"alternating buffers": 1})
        return _judge(calls, m, case, seam_counts(L, 2, side), want_ran)
    raise KeyError(kind)


CASES = {}
for _n, _cfg in ((7, "A"), (1, "B")):
    for _train in (True, False):
        for _side in (True, False):
            CASES[f"regression {_n} {'train' if _train else 'eval'} side {'on' if _side else 'off'}"] = ("step", _cfg, dict(num_labels=_n, train=_train, side=_side))
CASES.update({"class head C=3": ("step", "A", dict(head="cls")), "multi-label C=6, one entry not annotated": ("step", "B", dict(head="multi")),
              "huber": ("step", "A", dict(head="huber")), "class weights + smoothing": ("step", "B", dict(head="weights")),
              "label-only": ("label_only", "A", {}), "dense hand-over": ("dense_top", "B", {}), "freeze embeddings + layer 0": ("freeze", "A", {}),
              "q + v adapters": ("lora", "B", {}), "two micro-batches": ("two_micro_batches", "A", {}),
              "async prologue, two steps": ("async_prologue", "B", {})})


@pytest.mark.parametrize("case", list(CASES))
def test_the_seam_of_a_recorded_step(case):
    run_case(case, seed_of(case))
