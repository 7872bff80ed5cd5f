"""CPU-only: the float64 reference of the multi-label head (tests/heads_multilabel_ref.py) against torch's own
``binary_cross_entropy_with_logits``, its emulation against its bound on every case the GPU test uses, the mutations the bound must catch,
the decision safety of those cases, the ABI's new record and entry points, and the host logic around the head (``set_loss_options`` /
``set_num_labels``, the dataset rule, vector labels through ``collate`` / ``DeviceBatchBuilder``, ``balanced_pos_weight``,
``test_multilabel_score_model``).

Every mutation below fails its check (a condition of acceptance); the smallest margin of each, as the worst ratio error / bound over every
case where the mutation changes anything, is printed by ``pytest -s`` (``inf``: a non-finite value, or a decision that differs)."""
import copy
import ctypes
import math
import os
import pickle
import random

import pytest
import torch
import torch.nn.functional as F

from tests import heads_multilabel_ref as MLR
from tests import heads_ref as HR

torch.set_num_threads(min(16, torch.get_num_threads()))
MARGINS = {}
WORST = {}
NCASES = len(MLR.SHAPES) * len(MLR.VARIANTS)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest ratios of the emulation per output (elementwise, normwise):")
        for k in sorted(WORST):
            print(f"  {k:28s} {WORST[k][0]:.3f} {WORST[k][1]:.3f}")
    if MARGINS:
        print("\nsmallest margin of each mutation (worst ratio; > 1 fails):")
        for k in sorted(MARGINS):
            print(f"  {k:60s} {MARGINS[k]:.3g}")


# ------------------------------------------------------------------------------------------------ the reference against torch
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True])
def test_label_term_is_torchs_bce_with_logits(weighted, eps, masked):
    """The issue's closed forms against F.binary_cross_entropy_with_logits(x[valid], t'[valid], pos_weight=) and its autograd gradient of
    the logits, in float64 -- hard and soft targets."""
    B, C = 9, 6
    g = torch.Generator().manual_seed(3)
    for soft in (False, True):
        x = (3.0 * torch.randn(B, C, generator=g, dtype=torch.float64)).requires_grad_(True)
        t = MLR.targets_for(B, C, g, masked=masked, soft=soft).double()
        o = MLR.Opts(pos_weight=MLR.pos_weight_for(C, 1) if weighted else None, eps=eps)
        valid = t >= 0
        e = MLR.eps32(eps)
        tp = t * (1 - e) + e / 2
        pw = None if not weighted else o.pos_weight.double()[None, :].expand(B, C)[valid]
        loss = F.binary_cross_entropy_with_logits(x[valid], tp[valid], pos_weight=pw)
        loss.backward()
        mine, dlo, N = MLR.label_term(x.detach(), t, o)
        assert N == int(valid.sum()) and (N < B * C) == masked
        assert abs(float(mine - loss.detach())) <= 1e-14 and float((dlo - x.grad).abs().max()) <= 1e-15
        assert float(dlo[~valid].abs().max() if masked else 0.0) == 0.0


def test_label_term_without_annotated_entries_is_exactly_zero():
    x = torch.randn(4, 3, dtype=torch.float64)
    loss, dlo, N = MLR.label_term(x, torch.full((4, 3), -1.0), MLR.Opts(pos_weight=MLR.pos_weight_for(3, 2), eps=0.1))
    assert N == 0 and float(loss) == 0.0 and float(dlo.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ emulation, decision safety
@pytest.mark.parametrize("i", range(NCASES))
def test_emulation_passes_restates_the_reference_and_decisions_are_safe(i):
    c, o = MLR.gpu_case(i)
    exp = MLR.expected(c, o)
    assert MLR.decision_ratio(c, o, exp) >= HR.KINK and HR.kink_ratio(c) >= HR.KINK
    var = MLR.VARIANTS[i % len(MLR.VARIANTS)]
    nmask = int((c.t < 0).sum())
    if var in ("masked", "all") and c.B * c.C >= 4:
        assert 0 < nmask < c.B * c.C
    else:
        assert nmask == 0 or var in ("masked", "all")
    MLR.check_all(MLR.emulated(c, o), exp, f"case {i}", WORST)
    r = MLR.restate(c, o)
    for k in ("aux", "loss", "dfirst", "classifier1_2.weight", "classifier1_2.bias"):
        assert float((r[k].v - exp[k].val).abs().max()) <= 1e-9 * max(1.0, float(exp[k].val.abs().max())), k
    assert torch.equal(r["pred"], exp["pred"]) and tuple(exp["pred"].shape) == (c.B, c.C)


@pytest.mark.parametrize("make", [MLR.soft_case, MLR.all_masked_case, MLR.large_logit_case, MLR.on_threshold_case], ids=lambda f: f.__name__)
def test_targeted_cases_emulate_within_bound(make):
    c, o = make()
    exp = MLR.expected(c, o)
    MLR.check_all(MLR.emulated(c, o), exp, make.__name__, WORST)
    if make is MLR.all_masked_case:
        r = MLR.emulated(c, o)
        assert float(exp["aux"].val[1]) == 0.0 and float(r["aux"][1]) == 0.0
        for k in ("classifier1_2.weight", "classifier1_2.bias"):
            assert torch.equal(r[k], c.prior[k].double().reshape(r[k].shape)), k            # the prior bits: a zero seed adds nothing
    if make is MLR.large_logit_case:
        assert float(exp["logits"].val.abs().min()) == 100.0 and bool(torch.isfinite(exp["aux"].val).all())
        assert MLR.decision_ratio(c, o, exp) >= HR.KINK
    if make is MLR.on_threshold_case:
        assert torch.equal(exp["logits"].val, o.thr.double().expand(c.B, c.C)) and int(exp["pred"].sum()) == 0
    if make is MLR.soft_case:
        assert sorted(set(c.t.reshape(-1).tolist())) == [0.25, 0.75] and MLR.decision_ratio(c, o, exp) >= HR.KINK


# ------------------------------------------------------------------------------------------------ mutations
def _worst(got, exp):
    w = 0.0
    for k, t in got.items():
        if k == "pred":
            if tuple(t.shape) != tuple(exp["pred"].shape) or not torch.equal(t, exp["pred"]):
                w = math.inf
            continue
        r = HR.ratios(t.reshape(exp[k].val.shape), exp[k])
        w = max(w, r.elem, r.norm)
    return w


def _changes(c, o, mut):
    a, b = MLR.emulated(c, o), MLR.emulated(c, o, mut)
    return b, any(not torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("mut", [MLR.N_taken_as_BC, MLR.pos_weight_on_the_negative_term, MLR.seed_on_masked_entries,
                                 MLR.smoothing_without_half_eps, MLR.pred_transposed], ids=lambda f: f.__name__)
def test_mutations_fail_on_every_gpu_case_they_change(mut):
    hit = 0
    for i in range(NCASES):
        if MLR.SHAPES[i // len(MLR.VARIANTS)][0] > 17 and i % len(MLR.VARIANTS) not in (3, 5):
            continue                                                     # (the 128-sample shape: its masked and "all" variants)
        c, o = MLR.gpu_case(i)
        got, changed = _changes(c, o, mut())
        if not changed:
            continue
        hit += 1
        w = _worst(got, MLR.expected(c, o))
        MARGINS[mut().name] = min(MARGINS.get(mut().name, math.inf), w)
        assert w > 1.0, f"{mut().name} passes on case {i}: ratio {w:.3g}"
    assert hit >= 2, f"{mut().name} changed {hit} cases"


def test_naive_softplus_is_not_finite_beyond_fp32_exp():
    c, o = MLR.large_logit_case()
    got = MLR.emulated(c, o, MLR.naive_softplus())
    assert not bool(torch.isfinite(got["aux"][1])) and not bool(torch.isfinite(got["loss"]).all())
    w = _worst(got, MLR.expected(c, o))
    MARGINS[MLR.naive_softplus().name] = w
    assert w > 1.0


def test_threshold_compared_with_ge_fails_on_the_threshold():
    c, o = MLR.on_threshold_case()
    got = MLR.emulated(c, o, MLR.threshold_not_strict())
    assert int(got["pred"].sum()) == c.B * c.C
    w = _worst(got, MLR.expected(c, o))
    MARGINS[MLR.threshold_not_strict().name] = w
    assert w > 1.0


# ------------------------------------------------------------------------------------------------ the ABI
def test_record_sizes_header_exports_and_bindings_agree():
    from msa_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mmbert_hip.h")).read()
    lib = _lib.load()
    assert lib.mmbert_heads_step_struct_size() == ctypes.sizeof(ops._HeadsStep)
    assert lib.mmbert_heads_step_opt_struct_size() == ctypes.sizeof(ops._HeadsStepOpt)
    assert lib.mmbert_heads_step_ml_struct_size() == ctypes.sizeof(ops._HeadsStepMl) == ctypes.sizeof(ops._HeadsStepOpt) + ctypes.sizeof(ops._HeadsMulti)
    assert [f[0] for f in ops._HeadsMulti._fields_] == ["multi_label", "multi_target", "pos_weight", "threshold"]
    assert issubclass(ops._HeadsStepMl, ops._HeadsStepOpt) and ops._HeadsStepMl.ml.offset == ctypes.sizeof(ops._HeadsStepOpt)
    assert ops._HeadsStepMl.step.offset == 0 and ops._HeadsStepMl.opt.offset == ctypes.sizeof(ops._HeadsStep)
    for n in ("mmbert_heads_step_ml_struct_size", "mmbert_heads_step_fwd_levels_ml", "mmbert_heads_step_bwd_levels_ml", "mmbert_heads_predict_opt"):
        assert f"int {n}(" in header and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert _lib.SIGNATURES["mmbert_heads_step_fwd_levels_ml"] == _lib.SIGNATURES["mmbert_heads_step_fwd_levels"]
    assert _lib.SIGNATURES["mmbert_heads_step_bwd_levels_ml"] == _lib.SIGNATURES["mmbert_heads_step_bwd_levels"]
    assert _lib.SIGNATURES["mmbert_heads_predict_opt"] == _lib.SIGNATURES["mmbert_heads_predict"]
    a = ops.heads_step_struct()
    assert isinstance(a, ops._HeadsStepMl) and ctypes.addressof(a) == ctypes.addressof(a.step)
    assert (a.multi_label, a.multi_target, a.pos_weight, a.threshold, a.loss_kind, a.ncls) == (0, None, None, None, 0, 0)
    assert not ops._heads_multi_on(a)
    a.multi_label = 1
    assert ops._heads_multi_on(a) and a.ml.multi_label == 1


# ------------------------------------------------------------------------------------------------ host logic without a GPU
def _tiny(num_labels=None, **kw):
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    return MMBertForPretraining(MMBertConfig(vocab_size=128, hidden_size=32, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64),
                                num_labels=num_labels, **kw)


def test_construction_rules():
    from msa_amd.model import _class_head, _multi_head
    m = _tiny(6, multi_label=True)
    assert m.multi_label is True and _multi_head(m) == 6 == _class_head(m) and m.classifier1_2.out_features == 6
    assert list(m.state_dict().keys()) == list(_tiny(6).state_dict().keys())
    assert _multi_head(_tiny(6)) == 0 and _multi_head(_tiny()) == 0
    for n in (1, 7):
        with pytest.raises(ValueError):
            _tiny(n, multi_label=True)
    with pytest.raises(ValueError):
        _tiny(None, multi_label=True)                                    # (the reference's model: num_labels 7)
    with pytest.raises(ValueError):
        _tiny(17, multi_label=True)
    with pytest.raises(ValueError):
        _tiny(6, multi_label=1)
    r = _tiny()
    for n in (1, 7):
        with pytest.raises(ValueError):
            r.set_num_labels(n, multi_label=True)
    assert r.classifier1_2.out_features == 1 and not r.multi_label
    r.set_num_labels(4, multi_label=True)
    assert r.multi_label and r.classifier1_2.out_features == 4 and _multi_head(r) == 4
    r.set_num_labels(4)
    assert not r.multi_label and _class_head(r) == 4


def test_set_loss_options_rules_and_refusals_store_nothing():
    m = _tiny(3, multi_label=True)
    m.set_loss_options(pos_weight=[1, 2, 3], thresholds=[0.5, 0.25, 0.9], multilabel_smoothing=0.1, mlm_label_smoothing=0.2)
    want = torch.log(torch.tensor([0.5, 0.25, 0.9], dtype=torch.float64) / (1 - torch.tensor([0.5, 0.25, 0.9], dtype=torch.float64))).float()
    assert torch.equal(m.thresholds, want) and float(m.thresholds[0]) == 0.0 and m.thresholds.dtype == torch.float32
    assert m.pos_weight.tolist() == [1.0, 2.0, 3.0] and m.pos_weight.dtype == torch.float32 and m.multilabel_smoothing == 0.1
    state = (m.multilabel_smoothing, m.mlm_label_smoothing, m.pos_weight.clone(), m.thresholds.clone())
    bad = [dict(pos_weight=[1, 2]), dict(pos_weight=[1, 2, 0]), dict(pos_weight=[1, 2, -1]), dict(pos_weight=[1, 2, float("nan")]),
           dict(pos_weight=[1, 2, float("inf")]), dict(thresholds=[0.5, 0.5]), dict(thresholds=[0.5, 0.5, 0.0]), dict(thresholds=[0.5, 0.5, 1.0]),
           dict(thresholds=[0.5, 0.5, float("nan")]), dict(multilabel_smoothing=1.0), dict(multilabel_smoothing=-0.1),
           dict(multilabel_smoothing=float("nan")), dict(class_weights=[1, 2, 3]), dict(label_smoothing=0.1), dict(regression="l1"),
           dict(regression="huber")]
    for kw in bad:
        with pytest.raises(ValueError):
            m.set_loss_options(**kw)
        assert (m.multilabel_smoothing, m.mlm_label_smoothing) == state[:2] and torch.equal(m.pos_weight, state[2]) and torch.equal(m.thresholds, state[3]), kw
    keys = list(_tiny(3).state_dict().keys())
    assert list(m.state_dict().keys()) == keys and {"pos_weight", "thresholds"} <= set(dict(m.named_buffers()))
    for q in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert torch.equal(q.pos_weight, m.pos_weight) and torch.equal(q.thresholds, m.thresholds) and q.multi_label and q.multilabel_smoothing == 0.1
    m.double()
    assert m.pos_weight.dtype == torch.float32 and m.thresholds.dtype == torch.float32 and m.classifier1_2.weight.dtype == torch.float64
    m.float()
    with pytest.raises(ValueError):
        m.set_num_labels(4, multi_label=True)                            # buffers of another length: clear them first
    with pytest.raises(ValueError):
        m.set_num_labels(3)                                              # ... or of a head that is no longer multi-label
    m.set_loss_options()                                                 # every call sets all options
    assert m.pos_weight is None and m.thresholds is None and m.multilabel_smoothing == 0.0 and m.mlm_label_smoothing == 0.0
    m.set_num_labels(4, multi_label=True)
    # each of the three raises on a head that is not multi-label
    for r in (_tiny(3), _tiny()):
        for kw in (dict(pos_weight=[1, 2, 3]), dict(thresholds=[0.5, 0.5, 0.5]), dict(multilabel_smoothing=0.1)):
            with pytest.raises(ValueError):
                r.set_loss_options(**kw)
    c = _tiny(3)
    c.set_loss_options(class_weights=[1, 2, 3])
    with pytest.raises(ValueError):
        c.set_num_labels(3, multi_label=True)


def test_forward_refuses_bad_targets_before_anything_runs():
    m = _tiny(3, multi_label=True)
    for bad, err in ((torch.zeros(4, 3, dtype=torch.int64), TypeError), (torch.zeros(4, 3, dtype=torch.bool), TypeError),
                     (torch.zeros(4), ValueError), (torch.zeros(4, 2), ValueError), (torch.zeros(3, 4), ValueError)):
        with pytest.raises(err):
            m._check_class_labels(bad)
    assert m._check_class_labels(torch.zeros(4, 3)) == 3 and m._check_class_labels(torch.zeros(4, 3, dtype=torch.float64)) == 3


def test_eager_heads_are_the_reference():
    """model._heads (the eager form) against the float64 reference at one case, in double: loss and decisions."""
    c, o = MLR.gpu_case(11)                                              # (2, 80, 6), every option on
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    m = MMBertForPretraining(MMBertConfig(vocab_size=128, hidden_size=c.H, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64),
                             num_labels=c.C, multi_label=True).double()
    m.set_alpha_beta(c.alpha, c.beta)
    m.set_loss_options(pos_weight=o.pos_weight, thresholds=torch.sigmoid(o.thr.double()), multilabel_smoothing=o.eps)
    m.thresholds = o.thr.clone()                                         # (the exact fp32 logits of the case)
    params = dict(m.named_parameters())
    with torch.no_grad():
        for n, t in c.params.items():
            params[n].copy_(t.double())
    out = m._heads(c.first.double(), c.ap_v, c.ap_s, c.t)
    ref = MLR.reference(c, o)
    # (the model holds the smoothing as the python float 0.1, the reference as the fp32 value the kernel receives: 1.5e-9 apart)
    assert abs(float(out[2].detach()) - float(ref["aux"][1])) <= 1e-8 * max(1.0, abs(float(ref["aux"][1])))
    assert torch.equal(out[4], ref["pred"]) and out[4].dtype == torch.int64
    none = m._heads(c.first.double(), c.ap_v, c.ap_s, torch.full((c.B, c.C), -1.0))
    assert float(none[2]) == 0.0


def test_balanced_pos_weight_and_score_model_by_hand():
    from msa_amd import trainer as T
    y = torch.tensor([[1, 0, 1], [0, 0, 1], [1, 1, 0], [0, 1, -1], [1, 0, 0], [0, 0, 1]], dtype=torch.float32)
    p = torch.tensor([[1, 0, 1], [1, 0, 1], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], dtype=torch.int64)
    w = T.balanced_pos_weight(y)
    assert w.dtype == torch.float32 and torch.allclose(w, torch.tensor([3 / 3, 4 / 2, 2 / 3]))
    assert T.balanced_pos_weight(torch.tensor([[0.0], [0.0], [-1.0]])).tolist() == [2.0]          # no positive: counted once
    with pytest.raises(ValueError):
        T.balanced_pos_weight([1.0, 0.0])
    r = T.test_multilabel_score_model(p.numpy(), y.numpy())
    acc, wacc, f1 = [4 / 6, 4 / 6, 4 / 5], [2 / 3, 5 / 8, 3 / 4], [2 / 3, 1 / 2, 6 / 7]
    for k, want in (("accuracy", acc), ("weighted_accuracy", wacc), ("f1", f1)):
        assert r["per_label"][k] == pytest.approx(want, abs=1e-12), k
        assert r[k] == pytest.approx(sum(want) / 3, abs=1e-12), k
    assert r["mae"] == pytest.approx(5 / 17, abs=1e-12)
    with pytest.raises(ValueError):
        T.test_multilabel_score_model(p.numpy()[:, :2], y.numpy())


def test_apply_loss_options_reads_the_multilabel_arguments():
    from msa_amd import trainer as T
    m = _tiny(3, multi_label=True)
    data = [(None, None, None, torch.tensor(v, dtype=torch.float32)) for v in ([1, 0, 1], [0, 0, 1], [1, 1, 0], [0, 1, 0])]
    assert T.apply_loss_options(m, T.default_args()) is False
    assert T.apply_loss_options(m, T.default_args(pos_weight="balanced", thresholds=(0.5, 0.4, 0.6), multilabel_smoothing=0.05), data) is True
    assert torch.allclose(m.pos_weight, torch.tensor([1.0, 1.0, 1.0])) and m.multilabel_smoothing == 0.05 and float(m.thresholds[0]) == 0.0
    T.apply_loss_options(m, T.default_args(pos_weight=(1.0, 2.0, 3.0)))
    assert m.pos_weight.tolist() == [1.0, 2.0, 3.0] and m.thresholds is None and m.multilabel_smoothing == 0.0
    with pytest.raises(ValueError):
        T.apply_loss_options(m, T.default_args(pos_weight="balanced"))
    with pytest.raises(ValueError):
        T.apply_loss_options(m, T.default_args(pos_weight="uniform"), data)
    with pytest.raises(ValueError):
        T.apply_loss_options(_tiny(3), T.default_args(pos_weight=(1.0, 2.0, 3.0)))


def test_dataset_rule_and_vector_labels_through_the_batch_builders():
    from tests.golden.dataset_features import synthetic_features
    from msa_amd.dataset import MMBertDataset, DeviceBatchBuilder
    from msa_amd import trainer as T
    feats = synthetic_features(n_items=7, L=10, seed=3, dataset="mosei")
    ds = MMBertDataset(None, feats, "mosei", "emotions", 6)
    for i in range(len(ds)):
        raw = torch.tensor(feats[i][1][0])
        v = ds.sentiment_selection(feats[i][1][0], "6")
        assert v.dtype == torch.float32 and v.shape == (6,) and torch.equal(v, (raw[1:] != 0).float())
    assert ds.sentiment_selection(feats[0][1][0], "2") is None and ds.sentiment_selection(feats[0][1][0], "7") is None
    # the existing rules keep their outputs; another dataset with that task has no rule
    old = MMBertDataset(None, feats, "mosei", "sad", 6)
    assert torch.equal(old.sentiment_selection(feats[0][1][0], "6"), torch.argmax(torch.tensor(feats[0][1][0][1:])))
    assert MMBertDataset(None, synthetic_features(n_items=3, L=10, seed=3, dataset="mosi"), "mosi", "emotions", 6).sentiment_selection(0.5, "6") is None
    idx = (0, 3, 4, 2)
    random.seed(9)
    batch = T.collate([ds[i] for i in idx])
    random.seed(9)
    dbatch = DeviceBatchBuilder(ds, "cpu").batch(idx)
    want = torch.stack([(torch.tensor(feats[i][1][0][1:]) != 0).float() for i in idx])
    for b in (batch, dbatch):
        for part in b[:3]:
            assert part[-1].dtype == torch.float32 and torch.equal(part[-1], want)
    args = T.default_args(mlm=False)
    kw = T.pack_step_inputs(dbatch, args, "cpu")
    assert kw["sentiment"].shape == (4, 6) and kw["sentiment"].dtype == torch.float32 and torch.equal(kw["sentiment"], want)
    # scalar labels: the tensors they were before -- one python number per item, float32 or int64 [B]
    for task, nl, dt in (("sentiment", 7, torch.float32), ("sad", 6, torch.int64), ("sad", 2, torch.int64)):
        sc = MMBertDataset(None, feats, "mosei", task, nl)
        random.seed(9)
        b1 = T.collate([sc[i] for i in idx])
        random.seed(9)
        b2 = DeviceBatchBuilder(sc, "cpu").batch(idx)
        sel = [sc.sentiment_selection(feats[i][1][0], str(nl)) for i in idx]
        flat = torch.tensor([float(torch.as_tensor(s).reshape(-1)[0]) if dt == torch.float32 else int(torch.as_tensor(s).reshape(-1)[0]) for s in sel], dtype=dt)
        for b in (b1, b2):
            for part in b[:3]:
                assert part[-1].dtype == dt and part[-1].shape == (4,) and torch.equal(part[-1], flat), (task, nl)
