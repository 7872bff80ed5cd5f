"""CPU-only: the float64 references of the loss options (tests/loss_options_ref.py) against torch's own losses, their emulations
against their bounds on every case the GPU tests use, the mutations the bounds must catch, and the host logic of
``set_loss_options`` / ``trainer.apply_loss_options``.

Every mutation below fails its check (a condition of acceptance).  The smallest margin, as the worst ratio error / bound (> 1 fails;
``inf`` = an element that must be exact is not), measured here:

    cross-entropy   (1 - eps) missing on the label term 1.1e5   eps/V dropped in the backward 2.5e3   eps/V subtracted on the pad
                    columns inf   sum of x over ldv instead of V 561   the smoothing term on an unlabelled row inf
    class head      (1 - eps) missing 2.5e4   weights not normalised by W 7.5e3   W taken as B 3.7e3   sum_c w_c replaced by C 3.1e3
    regression      L1 seed without tanh' 2.2e3   Huber using delta^2 2.4e5   sign(0) = 1 7.5e6

(printed by ``pytest -s``; each is the smallest over every case where the mutation changes anything: the cross-entropy's over the
bf16, three-segment cases of every shape and eps, the heads' over every GPU case of the head they touch).
"""
import copy
import math
import pickle
import types

import pytest
import torch
import torch.nn.functional as F

from tests import heads_cls_ref as HCR
from tests import heads_ref as HR
from tests import loss_options_ref as LR
from tests import rowwise_ref as R

torch.set_num_threads(min(16, torch.get_num_threads()))
MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MARGINS:
        print("\nsmallest margin of each mutation (worst ratio; > 1 fails):")
        for k in sorted(MARGINS):
            print(f"  {k:60s} {MARGINS[k]:.3g}")


def _margin(name, ratio):
    MARGINS[name] = min(MARGINS.get(name, math.inf), ratio)


# ------------------------------------------------------------------------------------------------ cross-entropy: the reference against torch
def _torch_ce(X, lab, V, bounds, nseg, gs, eps):
    """F.cross_entropy(label_smoothing=eps, ignore_index=-100) per segment in float64: (losses [nseg], d(sum_s gs_s loss_s)/dX [M, V])."""
    Xb = X.to(torch.bfloat16).to(torch.float64)[:, :V].clone().requires_grad_(True)
    seg = R.seg_of_rows(lab.numel(), bounds, nseg)
    labt = torch.where((lab >= 0) & (lab < V), lab, torch.full_like(lab, -100))
    losses, tot = [], 0.0
    for s in range(nseg):
        m = seg == s
        if int((labt[m] >= 0).sum()) == 0:
            losses.append(torch.zeros((), dtype=torch.float64))             # (torch's mean over no rows is NaN; the kernel's documented 0)
            continue
        l = F.cross_entropy(Xb[m], labt[m], label_smoothing=LR.eps32(eps), ignore_index=-100)
        losses.append(l.detach())
        tot = tot + gs[s].double() * l
    tot.backward()
    return torch.stack(losses), Xb.grad


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("shape", [(1000, 1000), (13, 16)])
@pytest.mark.parametrize("nseg,empty", [(1, None), (3, None), (4, 2)])
def test_ce_reference_is_torchs_cross_entropy(eps, shape, nseg, empty):
    V, ldv = shape
    X, lab, bounds = LR.ce_inputs(V, ldv, nseg, empty, 5, torch.float32)
    assert int((lab == -100).sum()) > 0 and int(lab[0]) == V and int(lab[2]) == -1          # ignored rows of every kind
    gs = torch.tensor(LR.CE_GS)[:nseg]
    want_loss, want_grad = _torch_ce(X, lab, V, bounds, nseg, gs, eps)
    ref = LR.ce_fwd(X, lab, V, bounds, nseg, eps)
    assert float((ref["loss"].val - want_loss).abs().max()) <= 1e-13
    if empty is not None:
        assert float(ref["loss"].val[empty]) == 0.0 and float(ref["loss"].exact[empty]) == 0.0
    lse32 = ref["lse64"].float()
    seen = torch.zeros(lab.numel(), dtype=torch.bool)
    for j, rf in LR.ce_bwd(X, lab, V, bounds, nseg, gs, lse32, eps):
        # (the reference differentiates at the fp32 row_lse the kernel reads: 2^-24 of |lse| off the float64 value)
        assert float((rf.val[:, :V] - want_grad[j]).abs().max()) <= 2e-6
        assert float(rf.val[:, V:].abs().max() if ldv > V else 0.0) == 0.0
        seen[j] = True
    assert float(want_grad[~seen].abs().max()) == 0.0                                       # unlabelled rows: exactly zero in torch too


# ------------------------------------------------------------------------------------------------ cross-entropy: emulation and mutations
def _ce_emulate_and_check(case, mutation=None):
    """The emulation of one GPU case through the GPU test's checks; returns the worst ratio (inf: an exact value missed)."""
    V, ldv, eps, dtype, nseg, empty, seed = case
    X, lab, bounds = LR.ce_inputs(V, ldv, nseg, empty, seed, dtype)
    gs = torch.tensor(LR.CE_GS)[:nseg]
    ref = LR.ce_fwd(X, lab, V, bounds, nseg, eps)
    emu = LR.ce_fwd(X, lab, V, bounds, nseg, eps, emu=True, mutation=mutation)
    worst = 0.0
    for k in ("loss", "row_lse"):
        r = R.ratios(emu[k], ref[k])
        worst = max(worst, r.worst)
    lse32 = LR.ce_fwd(X, lab, V, bounds, nseg, eps, emu=True)["row_lse"].float()
    for rows in (None, LR.ce_compact_rows(lab, V)):
        out = LR.ce_bwd_emu(X, lab, V, bounds, nseg, gs, lse32, eps, rows=rows, mutation=mutation)
        try:
            el, nm = LR.ce_check_bwd(out, X, lab, V, bounds, nseg, gs, lse32, eps, rows=rows, count=ref["count"])
            worst = max(worst, el, nm)
        except AssertionError as e:
            if "exact" in str(e):
                worst = math.inf
            else:
                src = torch.arange(lab.numel()) if rows is None else rows.long()
                for j, rf in LR.ce_bwd(X, lab, V, bounds, nseg, gs, lse32, eps, rows=rows, count=ref["count"]):
                    worst = max(worst, R.ratios(out[j][:, :ldv], rf, gathered=True).worst)
    return worst


@pytest.mark.parametrize("i", range(len(LR.ce_cases())))
def test_ce_emulation_passes_its_own_bounds_on_every_gpu_case(i):
    case = LR.ce_cases()[i]
    X, lab, _ = LR.ce_inputs(case[0], case[1], case[4], case[5], case[6], case[3])
    assert int(((lab >= 0) & (lab < case[0])).sum()) >= 10 and int((lab == -100).sum()) >= 5
    assert _ce_emulate_and_check(case) <= 1.0


@pytest.mark.parametrize("mut", LR.CE_MUTATIONS, ids=lambda f: f.__name__)
def test_ce_mutations_fail(mut):
    """Each mutation fails the check on EVERY case where it changes anything (bf16 logits, three segments, every shape and eps)."""
    for case in LR.ce_cases():
        V, ldv, eps, dtype, nseg, empty, seed = case
        if dtype != torch.bfloat16 or nseg != 3:
            continue
        if mut in (LR.bwd_eps_over_v_on_pad, LR.rowsum_over_ldv) and ldv == V:
            continue                                                     # (no pad columns: the mutation is the identity)
        w = _ce_emulate_and_check(case, mut())
        _margin(f"ce: {mut().name}", w)
        assert w > 1.0, f"{mut().name} passes at V = {V}, eps = {eps}: ratio {w:.3g}"


# ------------------------------------------------------------------------------------------------ heads: the references against torch and each other
def test_default_options_are_the_existing_references():
    o = LR.Opts()
    for c, ref, rst in ((HCR.make_case(17, 80, 5, 6), HCR.reference, HCR.restate), (HR.make_case(15, 80, 5, num_labels=1), HR.reference, HR.restate)):
        a, b = ref(c), LR.reference(c, o)
        for k in a:
            if a[k] is not None:
                assert float((a[k].reshape(-1).double() - b[k].reshape(-1).double()).abs().max()) <= 1e-12, k
        ra, rb = rst(c), LR.restate(c, o)
        for k in HR.OUTPUTS:
            if ra[k] is not None:
                assert torch.equal(ra[k].v, rb[k].v) and torch.equal(ra[k].e, rb[k].e), k


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("weighted", [False, True])
def test_class_head_label_term_is_torchs_cross_entropy(eps, weighted):
    """The issue's closed forms (the restatement's float64 value) against F.cross_entropy(weight=, label_smoothing=) and its autograd
    gradient of the logits, in float64."""
    B, C = 9, 6
    g = torch.Generator().manual_seed(3)
    lo = torch.randn(B, C, generator=g, dtype=torch.float64).requires_grad_(True)
    y = torch.randint(0, C, (B,), generator=g)
    w = LR.class_weights_for(C, 1).double() if weighted else None
    loss = F.cross_entropy(lo, y, weight=w, label_smoothing=eps)
    loss.backward()
    wv = torch.ones(C, dtype=torch.float64) if w is None else w
    W, SW = wv[y].sum(), wv.sum()
    lse = torch.logsumexp(lo.detach(), 1)
    p = torch.exp(lo.detach() - lse[:, None])
    oh = F.one_hot(y, C).double()
    mine = (1 - eps) * (wv[y] * (lse - lo.detach().gather(1, y[:, None])[:, 0])).sum() / W + eps / (C * W) * (wv[None, :] * (lse[:, None] - lo.detach())).sum()
    dlo = (1 - eps) * wv[y][:, None] * (p - oh) / W + eps / (C * W) * (SW * p - wv[None, :])
    assert abs(float(mine - loss.detach())) <= 1e-14 and float((dlo - lo.grad).abs().max()) <= 1e-15


@pytest.mark.parametrize("i", range(len(LR.CLS_SHAPES) * 3))
def test_class_head_emulation_passes_and_restates_the_reference(i):
    c, o = LR.cls_case(i)
    exp = LR.expected(c, o)
    assert HCR.gap_ratio(c) >= HR.KINK
    LR.check_all(LR.emulated(c, o), exp, f"cls case {i}")
    r = LR.restate(c, o)
    for k in ("aux", "loss", "dfirst", "classifier1_2.weight", "classifier1_2.bias"):
        assert float((r[k].v - exp[k].val).abs().max()) <= 1e-9 * max(1.0, float(exp[k].val.abs().max())), k


@pytest.mark.parametrize("i", range(len(LR.reg_cases())))
def test_regression_emulation_passes_and_keeps_off_the_kinks(i):
    c, o = LR.reg_case(i)
    exp = LR.expected(c, o)
    assert LR.loss_kink_ratio(c, o, exp) >= HR.KINK and HR.kink_ratio(c) >= HR.KINK
    LR.check_all(LR.emulated(c, o), exp, f"regression case {i}")
    r = LR.restate(c, o)
    for k in ("aux", "loss", "dfirst", "classifier1_2.weight", "classifier1_2.bias"):
        assert float((r[k].v - exp[k].val).abs().max()) <= 1e-9 * max(1.0, float(exp[k].val.abs().max())), k
    if o.kind == "huber" and c.B >= 15:
        dv = (exp["logits"].val.reshape(-1) - c.sent.double()).abs()
        assert bool((dv <= o.delta).any()) and bool((dv > o.delta).any()), "both Huber branches"


def test_exact_zero_case():
    c, o = LR.exact_zero_case()
    exp = LR.expected(c, o)
    dv = exp["logits"].val.reshape(-1) - c.sent.double()
    assert int((dv == 0).sum()) == c.B // 2
    LR.check_all(LR.emulated(c, o), exp, "exact zero")


def _worst(got, exp):
    w = 0.0
    for k, t in got.items():
        if k == "pred":
            continue
        r = HR.ratios(t.reshape(exp[k].val.shape), exp[k])
        w = max(w, r.elem, r.norm)
    return w


CLS_MUTS = (LR.weights_not_normalised, LR.W_taken_as_B, LR.sum_w_replaced_by_C, LR.heads_one_minus_eps_missing)


@pytest.mark.parametrize("mut", CLS_MUTS, ids=lambda f: f.__name__)
def test_class_head_mutations_fail(mut):
    for i in range(len(LR.CLS_SHAPES) * 3):
        var = LR.CLS_VARIANTS[i % 3]
        if mut in (LR.sum_w_replaced_by_C, LR.heads_one_minus_eps_missing) and var == "weights":
            continue                                                     # (eps = 0: the term is not there)
        if mut in (LR.weights_not_normalised, LR.W_taken_as_B, LR.sum_w_replaced_by_C) and var == "smoothing":
            continue                                                     # (no weights: W = B and sum_c w_c = C)
        c, o = LR.cls_case(i)
        w = _worst(LR.emulated(c, o, mut()), LR.expected(c, o))
        _margin(f"class head: {mut().name}", w)
        assert w > 1.0, f"{mut().name} passes on class case {i}: ratio {w:.3g}"


def test_regression_mutations_fail():
    for i, (B, H, t, k) in enumerate(LR.reg_cases()):
        c, o = LR.reg_case(i)
        exp = LR.expected(c, o)
        if t and k == "l1":
            w = _worst(LR.emulated(c, o, LR.l1_seed_without_tanh()), exp)
            _margin("regression: L1 seed without tanh'", w)
            assert w > 1.0, (i, w)
        if k == "huber":
            dv = (exp["logits"].val.reshape(-1) - c.sent.double()).abs()
            if bool((dv > o.delta).any()):
                w = _worst(LR.emulated(c, o, LR.huber_delta_squared()), exp)
                _margin("regression: Huber using delta^2", w)
                assert w > 1.0, (i, w)
    c, o = LR.exact_zero_case()
    w = _worst(LR.emulated(c, o, LR.sign_zero_is_one()), LR.expected(c, o))
    _margin("regression: sign(0) = 1", w)
    assert w > 1.0


# ------------------------------------------------------------------------------------------------ host logic without a GPU
def _tiny(num_labels=None):
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    return MMBertForPretraining(MMBertConfig(vocab_size=128, hidden_size=32, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64),
                                num_labels=num_labels)


def test_set_loss_options_refusals_store_nothing():
    m = _tiny(6)
    m.set_loss_options(class_weights=[1, 2, 3, 4, 5, 6], label_smoothing=0.1, mlm_label_smoothing=0.2)
    state = (m.label_loss_kind, m.huber_delta, m.label_smoothing, m.mlm_label_smoothing, m.class_weights.clone())
    bad = [dict(regression="mae"), dict(regression="l1"), dict(regression="huber"), dict(class_weights=[1, 2]), dict(class_weights=[1, 2, 3, 4, 5, 0]),
           dict(class_weights=[1, 2, 3, 4, 5, -1]), dict(class_weights=[1, 2, 3, 4, 5, float("nan")]), dict(class_weights=[1, 2, 3, 4, 5, float("inf")]),
           dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan")), dict(mlm_label_smoothing=1.0),
           dict(mlm_label_smoothing=-1e-9), dict(huber_delta=0.0), dict(huber_delta=-1.0), dict(huber_delta=float("inf")), dict(huber_delta=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            m.set_loss_options(**kw)
        assert (m.label_loss_kind, m.huber_delta, m.label_smoothing, m.mlm_label_smoothing) == state[:4] and torch.equal(m.class_weights, state[4]), kw
    with pytest.raises(TypeError):
        m.set_loss_options("l1")                                         # keywords only
    r = _tiny()
    for kw in (dict(class_weights=[1.0]), dict(class_weights=[1.0] * 7), dict(label_smoothing=0.1)):
        with pytest.raises(ValueError):
            r.set_loss_options(**kw)
    r.set_loss_options(regression="huber", huber_delta=0.5, mlm_label_smoothing=0.1)
    assert (r.label_loss_kind, r.huber_delta, r.mlm_label_smoothing, r.class_weights) == ("huber", 0.5, 0.1, None)
    r.set_loss_options()                                                 # every call sets all five
    assert (r.label_loss_kind, r.huber_delta, r.label_smoothing, r.mlm_label_smoothing, r.class_weights) == ("mse", 1.0, 0.0, 0.0, None)


def test_options_are_no_state_dict_keys_and_follow_copies():
    m = _tiny(6)
    keys = list(m.state_dict().keys())
    m.set_loss_options(class_weights=[1, 2, 3, 4, 5, 6], label_smoothing=0.1, mlm_label_smoothing=0.2)
    assert list(m.state_dict().keys()) == keys
    assert m.class_weights.dtype == torch.float32 and "class_weights" in dict(m.named_buffers())
    for q in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert torch.equal(q.class_weights, m.class_weights) and q.class_weights.data_ptr() != m.class_weights.data_ptr()
        assert (q.label_smoothing, q.mlm_label_smoothing, q.label_loss_kind) == (0.1, 0.2, "mse")
        assert list(q.state_dict().keys()) == keys
    m.double()                                                           # (a buffer follows .to(); its dtype stays the kernels' fp32)
    assert m.class_weights.dtype == torch.float32 and m.classifier1_2.weight.dtype == torch.float64
    first = torch.randn(12, 32, dtype=torch.float64)
    out = m._heads(first, torch.zeros(4, dtype=torch.long), torch.ones(4, dtype=torch.long), torch.tensor([0, 5, 2, 2]))
    assert bool(torch.isfinite(out[2])) and out[4].shape == (4,) and out[4].dtype == torch.int64      # eager heads: the classes, not logits
    m.float()
    assert m.class_weights.dtype == torch.float32 and m.half().class_weights.dtype == torch.float32
    m.float()
    with pytest.raises(ValueError):
        m.set_num_labels(3)                                              # weights of another length: clear them first
    m.set_num_labels(6)
    m.set_loss_options()
    m.set_num_labels(3)
    assert m.classifier1_2.out_features == 3


def test_balanced_class_weights_and_apply_loss_options():
    from msa_amd import trainer
    w = trainer.balanced_class_weights([0, 0, 0, 1, 2, 2], 4)
    assert w.dtype == torch.float32 and torch.allclose(w, torch.tensor([6 / 12, 6 / 4, 6 / 8, 6 / 4]))
    with pytest.raises(ValueError):
        trainer.balanced_class_weights([0, 4], 4)
    args = trainer.default_args()
    assert not any(hasattr(args, n) for n in ("label_loss", "huber_delta", "class_weights", "label_smoothing", "mlm_label_smoothing"))
    r = _tiny()
    r.set_loss_options(regression="l1")
    assert trainer.apply_loss_options(r, args) is False and r.label_loss_kind == "l1"       # nothing asked: the model is left alone
    assert trainer.apply_loss_options(r, trainer.default_args(label_loss="huber", huber_delta=0.25, mlm_label_smoothing=0.05)) is True
    assert (r.label_loss_kind, r.huber_delta, r.mlm_label_smoothing) == ("huber", 0.25, 0.05)
    m = _tiny(3)
    data = [(None, None, None, y) for y in (0, 0, 1, 2, 2, 2)]
    trainer.apply_loss_options(m, trainer.default_args(class_weights="balanced", label_smoothing=0.1), data)
    assert torch.allclose(m.class_weights, torch.tensor([1.0, 2.0, 2 / 3])) and m.label_smoothing == 0.1
    trainer.apply_loss_options(m, trainer.default_args(class_weights=(1.0, 2.0, 3.0)))
    assert m.class_weights.tolist() == [1.0, 2.0, 3.0] and m.label_smoothing == 0.0
    with pytest.raises(ValueError):
        trainer.apply_loss_options(m, trainer.default_args(class_weights="balanced"))       # no labels to balance
    with pytest.raises(ValueError):
        trainer.apply_loss_options(m, trainer.default_args(class_weights="uniform"), data)


def test_new_symbols_and_struct_mirror():
    import ctypes
    import os
    from msa_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mmbert_hip.h")).read()
    lib = _lib.load()
    for n, extra in (("mmbert_ce_fwd_smooth", "mmbert_ce_fwd"), ("mmbert_ce_bwd_smooth", "mmbert_ce_bwd")):
        assert f"int {n}(" in header and hasattr(lib, n)
        res, args = _lib.SIGNATURES[n]
        assert res is _lib.I and args == _lib.SIGNATURES[extra][1] + [_lib.F]                # the old arguments plus ``float smoothing``
    # the record keeps its size and fields; the options sit in a struct of their own behind it (mmbert_heads_step_opt)
    assert lib.mmbert_heads_step_struct_size() == ctypes.sizeof(ops._HeadsStep)
    assert lib.mmbert_heads_step_opt_struct_size() == ctypes.sizeof(ops._HeadsStepOpt) == ctypes.sizeof(ops._HeadsStep) + ctypes.sizeof(ops._HeadsLoss)
    assert [f[0] for f in ops._HeadsStep._fields_][-3:] == ["sync", "sent_cls", "pred"]
    assert [f[0] for f in ops._HeadsLoss._fields_] == ["loss_kind", "huber_delta", "label_smoothing", "cls_weight"]
    assert ops._HeadsStepOpt.step.offset == 0 and ops._HeadsStepOpt.opt.offset == ctypes.sizeof(ops._HeadsStep)
    for n in ("mmbert_heads_step_opt_struct_size", "mmbert_heads_step_fwd_levels_opt", "mmbert_heads_step_bwd_levels_opt"):
        assert f"int {n}(" in header and hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.SIGNATURES["mmbert_heads_step_fwd_levels_opt"] == _lib.SIGNATURES["mmbert_heads_step_fwd_levels"]
    a = ops.heads_step_struct()
    assert isinstance(a, ops._HeadsStepOpt) and ctypes.addressof(a) == ctypes.addressof(a.step)
    assert (a.loss_kind, a.huber_delta, a.label_smoothing, a.cls_weight, a.ncls) == (0, 0.0, 0.0, None, 0)
    for bad in (-0.5, 1.0, float("nan")):
        with pytest.raises(ValueError):
            ops._ce_smoothing(bad)
    t = types.SimpleNamespace(mlm_label_smoothing=0.0)
    assert ops._ce_smoothing(t.mlm_label_smoothing) == 0.0
