"""The level-launch heads with a MULTI-LABEL head (csrc/heads_coop.hip, ``mmbert_heads_multi``) against the float64 reference of
tests/heads_multilabel_ref.py through ``heads_ref.check``, in the mould of tests/test_heads_cls_gpu.py (whose helpers are imported): four
shapes x six variants through ``_HeadsStepFn`` in both operand forms (fp32 rows; bf16 encoder rows with a row stride != H through a
non-monotonic row list), a NaN-filled workspace, random words in the whole flat gradient buffer (every word outside the heads' views keeps
its bits), the loss level's counter words back at zero, ``pred`` [B, C] equal to the float64 decisions on EVERY entry (the cases keep every
logit 64 bounds off its threshold: tests/test_heads_multilabel_reference_cpu.py) and to ``returned logits > thr``.  Then the targeted
cases (nothing annotated, logits of +-100, logits exactly on the threshold, soft targets), the flag-clear path through the new-size record
against the entry points without options, bit for bit, and what the ABI refuses.  The largest ratios per output are printed at the end
(``-s``)."""
import ctypes
import functools

import pytest
import torch

from tests import heads_multilabel_ref as MLR
from tests import heads_ref as HR
from tests.test_heads_cls_gpu import _load, _NanWorkspace, _record, _scaled_head, _model as _cls_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
torch.set_num_threads(min(16, torch.get_num_threads()))
WORST = {}
_MODELS = {}
CANARY = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest ratios per output (elementwise, normwise; the case of each):")
        for k in sorted(WORST):
            w = WORST[k]
            print(f"  {k:28s} {w[0]:.3f} {w[1]:.3f}   {w[2]} | {w[3]}")


def _model(H, C):
    """An H-wide model with a C-label multi-label head."""
    key = (H, C)
    if key not in _MODELS:
        from tests.test_model_gpu import build
        m = build(dict(hidden=H, layers=1, heads=1, intermediate=4 * H, vocab=512, dataset="mosei"))
        m.set_num_labels(C, multi_label=True)
        m._ensure_ready(torch.device(DEV, 0))
        _MODELS[key] = m
    return _MODELS[key]


def _set_options(m, o):
    m.set_loss_options(pos_weight=o.pos_weight, multilabel_smoothing=o.eps)
    m.thresholds = None if o.thr is None else o.thr.clone().to(DEV)          # (the case's fp32 logit thresholds, bit for bit)


def _run(c, o, model_form=False):
    from msa_amd import model as MM, ops
    m = _model(c.H, c.C)
    _set_options(m, o)
    snap, outside = _load(m, c)
    B, H = c.B, c.H
    ap_v, ap_s, t = c.ap_v.to(DEV), c.ap_s.to(DEV), c.t.to(DEV).contiguous()
    mlm = c.mlm.to(DEV).requires_grad_(True) if c.nmlm else None
    with _NanWorkspace(ops):
        if model_form:
            ld = H + 48
            yy = torch.randn(5 * B + 7, ld, generator=torch.Generator().manual_seed(B)).to(torch.bfloat16).to(DEV)
            rows = torch.randperm(5 * B + 7, generator=torch.Generator().manual_seed(B + 1))[:3 * B].to(DEV)
            yy[rows, :H] = c.first.to(torch.bfloat16).to(DEV)
            yy = yy[:, :H]
            f = torch.empty(3 * B, H, device=DEV).requires_grad_(True)
            loss, aux, logits, t_rel, rel = MM._HeadsStepFn.apply(f, m, (ap_v, ap_s), t, mlm, (yy, rows))
        else:
            f = c.first.to(DEV).requires_grad_(True)
            loss, aux, logits, t_rel, rel = MM._HeadsStepFn.apply(f, m, torch.cat((ap_v, ap_s)), t, mlm)
        pred = loss.grad_fn.keep[-2]
        out5 = loss.grad_fn.keep[-1]
        loss.backward(torch.tensor(c.d, device=DEV))
        MM._join_heads(m)
        torch.cuda.synchronize()
    for q in ops._heads_sync.values():
        assert int(q.abs().sum()) == 0, "the loss level's counter words are not back at zero"
    g = m._flat.grads
    assert torch.equal(g[outside].view(torch.int32), snap[outside].view(torch.int32)), \
        f"{int((g[outside].view(torch.int32) != snap[outside].view(torch.int32)).sum())} words outside the heads' views changed"
    assert logits.shape == (B, c.C) and pred.shape == (B, c.C) and pred.dtype == torch.int64
    thr = torch.zeros(c.C, device=DEV) if o.thr is None else o.thr.to(DEV)
    assert torch.equal(pred, (logits > thr[None, :]).long()), "pred differs from (returned logits > thr)"
    params = dict(m.named_parameters())
    got = dict(loss=loss.detach(), aux=aux, out5=out5, logits=logits, t_rel=t_rel, rel=rel, dfirst=f.grad, pred=pred)
    if mlm is not None:
        got["dmlm"] = mlm.grad
    for n in HR.PARAMS:
        got[n] = params[n].grad.detach().clone()
    return got


@functools.lru_cache(maxsize=None)
def _expected(i):
    """The float64 reference of case i: computed once, shared by both operand forms, left unchanged."""
    return MLR.expected(*MLR.gpu_case(i))


@pytest.mark.parametrize("form", ["rows", "model"])
@pytest.mark.parametrize("i", range(len(MLR.SHAPES) * len(MLR.VARIANTS)))
def test_level_launch_multilabel_heads(i, form):
    c, o = MLR.gpu_case(i)
    what = f"multi-label {MLR.VARIANTS[i % len(MLR.VARIANTS)]} {form} B={c.B} H={c.H} C={c.C}"
    MLR.check_all(_run(c, o, model_form=form == "model"), _expected(i), what, WORST)


# ------------------------------------------------------------------------------------------------ targeted cases
def test_every_entry_masked():
    """N = 0: the label loss is exactly 0, classifier1_2's gradients keep their prior bits, and the alignment and CPC parts are those of
    the same inputs with annotated targets, bit for bit."""
    c, o = MLR.all_masked_case()
    got = _run(c, o)
    MLR.check_all(got, MLR.expected(c, o), "every entry masked", WORST)
    assert float(got["aux"][1]) == 0.0 and float(got["out5"][1]) == 0.0
    for k in ("classifier1_2.weight", "classifier1_2.bias"):
        assert torch.equal(got[k].cpu().view(torch.int32), c.prior[k].view(torch.int32)), k
    c.t = MLR.targets_for(c.B, c.C, torch.Generator().manual_seed(1))
    other = _run(c, o)
    assert float(other["aux"][1]) > 0.0
    for j in (0, 2):
        assert torch.equal(got["aux"][j].view(torch.int32), other["aux"][j].view(torch.int32)), j


def test_large_logits_stay_finite():
    c, o = MLR.large_logit_case()
    got = _run(c, o)
    assert bool((got["logits"].abs() == 100.0).all())
    assert all(bool(torch.isfinite(v).all()) for k, v in got.items() if k != "pred")
    MLR.check_all(got, MLR.expected(c, o), "logits of +-100", WORST)


def test_logit_on_the_threshold_decides_zero():
    c, o = MLR.on_threshold_case()
    got = _run(c, o)
    assert torch.equal(got["logits"].cpu(), o.thr.expand(c.B, c.C)) and int(got["pred"].sum()) == 0
    MLR.check_all(got, MLR.expected(c, o), "logits on the threshold", WORST)


@pytest.mark.parametrize("form", ["rows", "model"])
def test_soft_targets(form):
    c, o = MLR.soft_case()
    MLR.check_all(_run(c, o, model_form=form == "model"), MLR.expected(c, o), f"soft targets {form}", WORST)


# ------------------------------------------------------------------------------------------------ records built by hand
def _run_record(lib, stream, m, g0, B, seed, ncls, ml):
    """One forward + backward of a hand-built record from the gradient state ``g0``: through the _ml entry points with the flag CLEAR and
    ``multi_target`` on a NaN canary (``ml``), or through the entry points without options.  Returns (outputs, gradient buffer)."""
    m._flat.grads.copy_(g0)
    a, o, keep = _record(m, B, seed=seed, ncls=ncls, labels=ncls > 0)
    can = torch.full((B * 16 + 64,), float("nan"), device=DEV)
    if ml:
        assert a.multi_label == 0 and not a.pos_weight and not a.threshold
        a.multi_target = can[32:].data_ptr()
        assert lib.mmbert_heads_step_fwd_levels_ml(stream, ctypes.addressof(a), 1, 7) == 0
        assert lib.mmbert_heads_step_bwd_levels_ml(stream, ctypes.addressof(a), 1, 6) == 0
    else:
        assert lib.mmbert_heads_step_fwd_levels(stream, ctypes.addressof(a), 1, 7) == 0
        assert lib.mmbert_heads_step_bwd_levels(stream, ctypes.addressof(a), 1, 6) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(can).all()), "the canary behind multi_target was written"
    assert bool(torch.isfinite(o["loss"]).all()) and bool(torch.isfinite(o["dfirst"]).all())
    return {k: v.clone() for k, v in o.items()}, m._flat.grads.clone()


@pytest.mark.parametrize("B,H,C", [(17, 768, 6), (15, 768, 0)])
def test_flag_clear_through_the_new_size_record_is_todays_bits(B, H, C):
    """The class head and the regression head through mmbert_heads_step_{fwd,bwd}_levels_ml with multi_label = 0 give the bits of the entry
    points without options -- outputs, pred, dfirst and the whole gradient buffer -- with multi_target pointing at a NaN canary that is
    neither written nor (every result stays finite and equal) read.  pos_weight / threshold cannot be set with the flag clear: refused."""
    from msa_amd import ops, _lib
    m = _cls_model(H, C)
    _scaled_head(m, 7 + C)
    lib, stream = _lib.load(), ops._stream()
    g0 = torch.randn(m._flat.grads.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)
    old = _run_record(lib, stream, m, g0, B, 5, C, ml=False)
    new = _run_record(lib, stream, m, g0, B, 5, C, ml=True)
    for k in old[0]:
        assert torch.equal(old[0][k].view(torch.int32) if old[0][k].dtype == torch.float32 else old[0][k],
                           new[0][k].view(torch.int32) if new[0][k].dtype == torch.float32 else new[0][k]), k
    assert torch.equal(old[1].view(torch.int32), new[1].view(torch.int32)) and not torch.equal(old[1], g0)


def _multi_record(m, B, seed, C):
    """tests/test_heads_cls_gpu.py's record turned into a multi-label one: no sent_cls, targets [B, C], pred [B, C]."""
    a, o, keep = _record(m, B, seed=seed, ncls=C)
    t = MLR.targets_for(B, C, torch.Generator().manual_seed(seed), masked=True).to(DEV)
    o["pred"] = torch.full((B, C), -7, device=DEV, dtype=torch.int64)
    a.sent_cls, a.pred = None, o["pred"].data_ptr()
    a.multi_label, a.multi_target = 1, t.data_ptr()
    return a, o, keep + (t,)


def test_multilabel_abi_refusals_and_the_accepted_record():
    """Every refusal of the header returns -1 from forward, backward and predict before any launch: the outputs, pred, dfirst and the whole
    flat gradient buffer keep their canaries.  The same record without the fault is accepted by all three."""
    from msa_amd import ops, _lib
    C, B = 6, 5
    m = _model(64, C)
    _scaled_head(m, 3)
    reg = _cls_model(64, 0)
    lib, stream = _lib.load(), ops._stream()
    w = torch.ones(C, device=DEV)

    def entry_points(a, fwd_only=False):
        r = [lib.mmbert_heads_step_fwd_levels_ml(stream, ctypes.addressof(a), 1, 7)]
        if not fwd_only:
            r += [lib.mmbert_heads_step_bwd_levels_ml(stream, ctypes.addressof(a), 1, 6), lib.mmbert_heads_predict_opt(stream, ctypes.addressof(a))]
        return r

    faults = ("ncls0", "loss_kind", "cls_weight", "no_target", "pos_weight_without_flag", "threshold_without_flag", "flag2")
    for fault in faults:
        mm = reg if fault == "ncls0" else m
        if fault == "ncls0":
            a, o, keep = _record(mm, B, seed=11, ncls=0, labels=False)
            t = torch.zeros(B, C, device=DEV)
            a.multi_label, a.multi_target = 1, t.data_ptr()
        else:
            a, o, keep = _multi_record(mm, B, 11, C)
        if fault == "loss_kind":
            a.loss_kind = 1
        elif fault == "cls_weight":
            a.cls_weight = w.data_ptr()
        elif fault == "no_target":
            a.multi_target = None
        elif fault == "pos_weight_without_flag":
            a.multi_label, a.pos_weight = 0, w.data_ptr()
        elif fault == "threshold_without_flag":
            a.multi_label, a.threshold = 0, w.data_ptr()
        elif fault == "flag2":
            a.multi_label = 2
        snap = mm._flat.grads.clone()
        assert all(r == -1 for r in entry_points(a, fwd_only=fault == "no_target")), fault
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(v).all()) for k, v in o.items() if k != "pred") and bool((o["pred"] == -7).all()), fault
        assert torch.equal(mm._flat.grads.view(torch.int32), snap.view(torch.int32)), fault
    # the entry points without the record keep refusing a null sent_cls with ncls > 0
    a, o, keep = _multi_record(m, B, 11, C)
    assert lib.mmbert_heads_step_fwd_levels(stream, ctypes.addressof(a), 1, 7) == -1
    assert lib.mmbert_heads_step_bwd_levels(stream, ctypes.addressof(a), 1, 6) == -1
    assert lib.mmbert_heads_step_fwd_levels_opt(stream, ctypes.addressof(a), 1, 7) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for k, v in o.items() if k != "pred") and bool((o["pred"] == -7).all())
    # accepted: forward + backward, then predict (levels 1 - 5) with the same decisions and logits, bit for bit
    thr = MLR.thresholds_for(C, 5).to(DEV)
    a.threshold = thr.data_ptr()
    assert lib.mmbert_heads_step_fwd_levels_ml(stream, ctypes.addressof(a), 1, 7) == 0
    assert lib.mmbert_heads_step_bwd_levels_ml(stream, ctypes.addressof(a), 1, 6) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o["loss"]).all()) and bool(torch.isfinite(o["dfirst"]).all())
    assert torch.equal(o["pred"], (o["logits"] > thr[None, :]).long()) and 0 < int(o["pred"].sum()) < B * C
    b, ob, keepb = _multi_record(m, B, 11, C)
    b.threshold = thr.data_ptr()
    b.multi_target = b.ap = b.loss = b.aux = b.out5 = b.sync = b.dloss = b.dfirst = None
    assert lib.mmbert_heads_predict_opt(stream, ctypes.addressof(b)) == 0
    torch.cuda.synchronize()
    assert torch.equal(ob["pred"], o["pred"]) and torch.equal(ob["logits"].view(torch.int32), o["logits"].view(torch.int32))
