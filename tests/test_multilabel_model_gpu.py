"""The multi-label head through the module API on a 2-layer model, B = 3, C = 6, T = 8, pair length 12 -- at H = 128 with two attention
heads: the encoder's attention kernels take head dimension 64 only, so H = 80 (the heads kernels' odd width, covered by
tests/test_heads_multilabel_gpu.py) cannot carry a whole model.  ``forward`` + ``backward`` + ``AdamW.step`` against the eager form of the
same model (``coop_heads = False``) and against the float64 reference of tests/heads_multilabel_ref.py at the model's own [CLS] rows; the C
entry points of a step and of ``predict()`` against a class-head model's, name for name; ``predict()`` against ``forward``;
``return_probabilities``; ``eval_epoch`` / ``predict_epoch`` over a 7-item dataset."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from msa_amd.data import synthetic_batch, batch_to
from tests import heads_multilabel_ref as MLR
from tests import heads_ref as HR
from tests.test_classification_gpu import _Count
from tests.test_loss_options_model_gpu import _Recorder
from tests.test_model_gpu import build, rel

DEV = "cuda"
CFG = dict(hidden=128, layers=2, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)
B, C, T, P = 3, 6, 8, 12
OPTS = dict(pos_weight=[0.5, 1.0, 2.0, 4.0, 0.25, 1.5], thresholds=[0.5, 0.4, 0.6, 0.5, 0.3, 0.7], multilabel_smoothing=0.1)
# what the options-visible entry points are called on a class head: the same launches behind another name
SAME = {"mmbert_heads_step_fwd_levels_ml": "mmbert_heads_step_fwd_levels", "mmbert_heads_step_bwd_levels_ml": "mmbert_heads_step_bwd_levels",
        "mmbert_heads_predict_opt": "mmbert_heads_predict"}


def _model(multi=True, opts=OPTS):
    m = build(CFG)
    torch.manual_seed(1000)
    m.set_num_labels(C, multi_label=multi)
    with torch.no_grad():                                           # (the HF initialisation leaves the logits a few 1e-2 wide: spread them)
        m.classifier1_2.weight.mul_(40.0)
        m.classifier1_2.bias.copy_(torch.linspace(-0.3, 0.3, C))
    m.parameters_changed()
    m.set_alpha_beta(0.7, 1.3)
    if multi and opts:
        m.set_loss_options(**opts)
    return m


def _batch(multi=True, seed=9):
    b = synthetic_batch(B, T, P, P, seed=seed, vocab=CFG["vocab"], num_labels=C)
    if multi:
        t = MLR.targets_for(B, C, torch.Generator().manual_seed(seed))
        t[1, 2] = -1.0                                              # one entry that is not annotated
        b["sentiment"] = t
    return batch_to(b, DEV)


def _step(m, batch, coop):
    from msa_amd.optim import AdamW
    m.coop_heads = coop
    m._ensure_ready(torch.device(DEV, 0))
    opt = AdamW(m.parameters(), lr=1e-3)
    seen = {}
    orig = m._heads

    def heads(first, *a, **k):
        seen["first"] = first.detach().float().cpu().clone()
        return orig(first, *a, **k)
    m._heads = heads
    with _Count() as cnt, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, pred = m(**batch)
        out[0].mean().backward()
        grads = {n: q.grad.float().clone() for n, q in m.named_parameters()}
        before = m.classifier1_2.weight.detach().clone()
        opt.step()
        torch.cuda.synchronize()
    m._heads = orig
    assert (cnt.fwd >= 1 and cnt.bwd == 1) if coop else (cnt.fwd == 0 and cnt.bwd == 0), (coop, cnt.fwd, cnt.bwd)
    assert bool(torch.isfinite(m.classifier1_2.weight).all()) and not torch.equal(m.classifier1_2.weight, before)
    return out, pred, grads, seen.get("first")


def test_step_against_the_eager_form_and_float64():
    batch = _batch()
    (o1, p1, g1, _), (o2, p2, g2, first) = (_step(_model(), batch, coop) for coop in (True, False))
    assert p1.shape == (B, C) and p1.dtype == torch.int64 and p2.dtype == torch.int64 and torch.equal(p1, p2)
    assert 0 < int(p1.sum()) < B * C
    for i in (0, 4, 5, 6):                                          # (tests/test_model_gpu.py::test_fused_heads_equal_eager_heads' bound)
        assert bool(torch.isfinite(o1[i]).all()) and rel(o1[i], o2[i]) < 1e-5, (i, float(o1[i]), float(o2[i]))
    for n in g1:
        if "attention.self.key.bias" in n:                          # true gradient 0: both sides hold rounding noise
            continue
        scale = float(g2[n].abs().max()) + 1e-12
        err = float((g1[n] - g2[n]).abs().max())
        assert err <= 3e-4 * scale + 3e-7, f"{n}: err {err:.3e} scale {scale:.3e}"
    assert float(g2["classifier1_2.weight"].abs().max()) > 0
    # the heads' float64 reference at the [CLS] rows the eager form was handed (the bf16 rows the level-launch kernels read): the label
    # loss and the other heads' terms under the restatement's bound, the decisions exactly
    m = _model()
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    c = MLR.Case(B=B, H=CFG["hidden"], first=first, params={k: sd[k] for k in HR.PARAMS + list(HR.FWD_ONLY)}, ap_v=batch["ap_label"][0].cpu(),
                 ap_s=batch["ap_label"][1].cpu(), sent=None, num_labels=C, alpha=0.7, beta=1.3, mlm=None, d=1.0, prior={}, C=C,
                 y=None, t=batch["sentiment"].cpu())
    o = MLR.Opts(pos_weight=m.pos_weight.cpu(), eps=0.1, thr=m.thresholds.cpu())
    exp = MLR.expected(c, o)
    assert MLR.decision_ratio(c, o, exp) >= HR.KINK
    worst = {}
    HR.check_all(dict(aux=torch.stack([o1[4], o1[5], o1[6]]).detach().float().cpu()), exp, "model step", worst)
    print(f"\nheads' losses of the model step against float64: ratios {worst['aux'][0]:.3f} {worst['aux'][1]:.3f}")
    assert torch.equal(p1.cpu(), exp["pred"])


def _names(m, batch, what):
    with _Recorder() as rec:
        if what == "step":
            out, _ = m(**batch)
            out[0].mean().backward()
        else:
            m.predict(batch["input_ids"], batch["token_type_ids"], batch["attention_mask"])
        torch.cuda.synchronize()
    return rec.names


@pytest.mark.parametrize("what", ["step", "predict"])
def test_entry_points_are_a_class_heads_name_for_name(what):
    """A multi-label step / predict() calls what a class-head step / predict() calls, in the same order: the same launches (the
    options-visible entry points issue the launches of the plain ones: ``SAME``).  And a class-head model calls none of the new names."""
    for warm in (True, False):                                      # (the first call of a process also resolves once-only names: struct sizes)
        multi = _names(_model(), _batch(), what)
        cls = _names(_model(multi=False), _batch(multi=False), what)
    assert not [n for n in cls if n in SAME], cls
    assert [n for n in multi if n in SAME], "the multi-label entry points did not run"
    assert [SAME.get(n, n) for n in multi] == cls
    plain = _names(build(CFG), batch_to(synthetic_batch(B, T, P, P, seed=9, vocab=CFG["vocab"]), DEV), what)
    assert not [n for n in plain if n in SAME or n.endswith("_opt")], plain


def test_predict_equals_forward_and_returns_probabilities():
    m = _model()
    batch = _batch()
    m.eval()
    with torch.no_grad():
        out, pred = m(**batch)
    args3 = (batch["input_ids"], batch["token_type_ids"], batch["attention_mask"])
    p = m.predict(*args3)
    assert p.dtype == torch.int64 and p.shape == (B, C) and torch.equal(p, pred)
    p2, extra = m.predict(*args3, return_pooled=True)
    assert torch.equal(p2, p) and extra["class_logits"].shape == (B, C) and extra["class_logits"].dtype == torch.float32
    assert torch.equal(p, (extra["class_logits"] > m.thresholds[None, :]).long())
    p3, prob = m.predict(*args3, return_probabilities=True)
    assert torch.equal(p3, p) and prob.dtype == torch.float32 and torch.equal(prob, torch.sigmoid(extra["class_logits"]))
    p4, prob4, extra4 = m.predict(*args3, return_pooled=True, return_probabilities=True)
    assert torch.equal(p4, p) and torch.equal(prob4, prob) and torch.equal(extra4["class_logits"], extra["class_logits"])
    with pytest.raises(ValueError):
        _model(multi=False).predict(*args3, return_probabilities=True)
    with pytest.raises(TypeError):
        m(**dict(batch, sentiment=batch["sentiment"].long()))
    with pytest.raises(ValueError):
        m(**dict(batch, sentiment=batch["sentiment"][:, :5]))


def test_epochs_over_a_dataset_collect_decisions():
    import random
    from tests.golden.dataset_features import synthetic_features
    from msa_amd.dataset import MMBertDataset
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    from msa_amd import trainer as Tr
    ds = MMBertDataset(None, synthetic_features(n_items=7, L=16, seed=4, dataset="mosei"), "mosei", "emotions", C)
    torch.manual_seed(5)
    m = MMBertForPretraining(MMBertConfig(vocab_size=2048, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512),
                             num_labels=C, multi_label=True)
    m.bert.set_joint_embeddings("mosei")
    m = m.to(DEV)
    random.seed(9)
    torch.manual_seed(100)
    args = Tr.default_args(train_batch_size=3, val_batch_size=3, num_labels=C, pos_weight="balanced")
    assert Tr.apply_loss_options(m, args, ds) is True and m.pos_weight.shape == (C,) and m.pos_weight.is_cuda
    with _Count() as cnt:
        te = Tr.eval_epoch(args, m, ds, device=DEV)
    assert cnt.fwd >= 3
    assert np.isfinite(te[5]) and te[6].dtype == np.int64 and te[6].shape == (7, C) and te[7].shape == (7, C) and te[7].dtype == np.float32
    assert set(np.unique(te[6])) <= {0, 1}
    r = Tr.test_multilabel_score_model(te[6], te[7])
    assert 0.0 <= r["weighted_accuracy"] <= 1.0 and len(r["per_label"]["f1"]) == C
    p = Tr.predict_epoch(args, m, ds, device=DEV)
    assert p.dtype == np.int64 and p.shape == (7, C) and set(np.unique(p)) <= {0, 1}
    assert Tr.predict_epoch(args, m, None, device=DEV, batches=[]).shape == (0, C)
