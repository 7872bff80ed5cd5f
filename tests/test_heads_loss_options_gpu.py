"""The label loss's options in the level-launch heads (csrc/heads_coop.hip, forward level 7: ``mmbert_heads_step_opt``'s ``loss_kind`` /
``huber_delta`` / ``label_smoothing`` / ``cls_weight``) against the float64 reference of tests/loss_options_ref.py, through ``_HeadsStepFn`` in both
operand forms as tests/test_heads_cls_gpu.py runs it (NaN-filled workspace, a random-filled gradient buffer whose words outside the
heads' views must keep their bits, the counter words back at zero): the class head at (B, H, C) = (1, 16, 2), (2, 80, 6),
(17, 768, 6), (128, 256, 16) with weights, with smoothing 0.1, and with both; the regression head at B = 1, 15, 33, 128 x H = 16, 768,
with and without tanh, under L1 and Huber(0.5); the exact-zero case (every logit exactly the target on half the samples: the L1 seed
there is exactly 0); all-default fields = the plain losses, reading none of the new fields; ``pred`` untouched by any option; and
what the ABI refuses.  The largest ratios per output are printed at the end (``-s``)."""
import ctypes

import pytest
import torch

from tests import heads_cls_ref as HCR
from tests import heads_ref as HR
from tests import loss_options_ref as LR
from tests import test_heads_cls_gpu as TC
from tests import test_heads_gpu as TR

pytestmark = pytest.mark.gpu

DEV = "cuda"
torch.set_num_threads(min(16, torch.get_num_threads()))
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest ratios per output (elementwise, normwise; the case of each):")
        for k in sorted(WORST):
            w = WORST[k]
            print(f"  {k:28s} {w[0]:.3f} {w[1]:.3f}   {w[2]} | {w[3]}")


class _options:
    """The options on the shared test model of a (H, head) for the length of one run: other modules' tests find it as they left it."""

    def __init__(self, m, o: LR.Opts):
        self.m, self.o = m, o

    def __enter__(self):
        o = self.o
        self.m.set_loss_options(regression=o.kind, huber_delta=o.delta, label_smoothing=o.eps, class_weights=o.weight)
        return self.m

    def __exit__(self, *exc):
        self.m.set_loss_options()


def _run_cls(c, o, model_form=False):
    with _options(TC._model(c.H, c.C), o):
        return TC._run(c, model_form=model_form)


def _run_reg(c, o, model_form=False):
    with _options(TR._model(c.H, c.num_labels), o):
        return TR._run(c, model_form=model_form)


@pytest.mark.parametrize("i", range(len(LR.CLS_SHAPES) * 3))
def test_class_head_with_weights_and_smoothing(i):
    c, o = LR.cls_case(i)
    exp = LR.expected(c, o)
    what = f"cls B={c.B} H={c.H} C={c.C} {LR.CLS_VARIANTS[i % 3]}"
    for form in (False, True):
        got = _run_cls(c, o, model_form=form)
        LR.check_all(got, exp, what + (" model form" if form else ""), WORST)
    plain = _run_cls(c, LR.Opts())                                     # ``pred`` does not depend on the options: the bits of the plain head
    assert torch.equal(plain["pred"], got["pred"]) and torch.equal(plain["logits"], got["logits"])


@pytest.mark.parametrize("i", range(len(LR.reg_cases())))
def test_regression_head_with_l1_and_huber(i):
    c, o = LR.reg_case(i)
    exp = LR.expected(c, o)
    what = f"reg B={c.B} H={c.H} tanh={int(c.num_labels == 1)} {o.kind}"
    for form in (False, True):
        LR.check_all(_run_reg(c, o, model_form=form), exp, what + (" model form" if form else ""), WORST)


def test_exact_zero_differences_give_an_exactly_zero_l1_seed():
    """classifier1_2.weight = 0, bias b, targets b on the even samples: d is exactly 0 there.  With sign(0) = 0 the seeds of the other
    samples (+1/B and -1/B, as many of each) cancel exactly: the bias gradient keeps its prior's bits and the weight gradient is the
    reference's; a seed of 1/B on the zero samples would move the bias gradient by d / 2."""
    c, o = LR.exact_zero_case()
    exp = LR.expected(c, o)
    got = _run_reg(c, o)
    LR.check_all(got, exp, "exact zero", WORST)
    assert torch.equal(got["logits"].reshape(-1).cpu(), torch.full((c.B,), float(c.params["classifier1_2.bias"])))
    assert torch.equal(got["classifier1_2.bias"].cpu(), c.prior["classifier1_2.bias"]), "sum of the L1 seeds is not exactly 0"
    assert float(got["aux"][1]) == 0.5                               # mean |d|: half the samples at 0, half at 1, exactly


def _outputs(o, m):
    return {k: v.clone() for k, v in o.items()}, m._flat.grads.clone()


@pytest.mark.parametrize("ncls", [0, 6])
def test_default_fields_are_the_plain_losses_and_read_nothing_new(ncls):
    """All four option fields zero / NULL (what ``heads_step_struct()`` hands out) through the ``_opt`` entry points against the same record
    through the entry points without options, bit for bit: the plain label loss -- the float64 value of the MSE /
    the unweighted cross-entropy from the returned logits -- with the same bits on repeat, and with the fields the plain loss must not
    read set to junk (a ``huber_delta`` that ``loss_kind`` 0 never reads): outputs and the whole gradient buffer bit for bit."""
    from msa_amd import ops, _lib
    m = TC._model(64, ncls)
    TC._scaled_head(m, 7)
    lib, stream = _lib.load(), ops._stream()
    B = 17
    g0 = torch.randn(m._flat.grads.numel(), generator=torch.Generator().manual_seed(2)).to(DEV)
    res = []
    for junk in (False, False, True):
        m._flat.grads.copy_(g0)
        a, o, keep = TC._record(m, B, seed=5, ncls=ncls, labels=ncls > 0)
        assert (a.loss_kind, a.huber_delta, a.label_smoothing, a.cls_weight) == (0, 0.0, 0.0, None)
        if junk:
            a.huber_delta = -3.0
        # (the first run through the entry points that know no options, the others through the _opt ones)
        fwd, bwd = ((lib.mmbert_heads_step_fwd_levels_opt, lib.mmbert_heads_step_bwd_levels_opt) if res else
                    (lib.mmbert_heads_step_fwd_levels, lib.mmbert_heads_step_bwd_levels))
        assert fwd(stream, ctypes.addressof(a), 1, 7) == 0
        assert bwd(stream, ctypes.addressof(a), 1, 6) == 0
        torch.cuda.synchronize()
        res.append(_outputs(o, m))
        lg = o["logits"].double().cpu()
        if ncls:
            want = torch.nn.functional.cross_entropy(lg, keep[3].cpu())
        else:
            want = torch.nn.functional.mse_loss(lg.reshape(-1), keep[2].double().cpu())
        assert abs(float(o["aux"][1]) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    for other in res[1:]:
        for k in res[0][0]:
            x, y = res[0][0][k], other[0][k]
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y), k
        assert torch.equal(res[0][1].view(torch.int32), other[1].view(torch.int32))
    assert not torch.equal(res[0][1], g0)


def test_option_refusals_launch_nothing():
    """Every combination the header refuses: -1 from the forward and the backward entry points, outputs, dfirst and the whole flat
    gradient buffer keep their bits; the accepted neighbours of each run."""
    from msa_amd import ops, _lib
    lib, stream = _lib.load(), ops._stream()
    B = 4
    w6 = torch.ones(6, device=DEV)
    nan, inf = float("nan"), float("inf")
    reg_bad = [dict(loss_kind=3), dict(loss_kind=-1), dict(loss_kind=2, huber_delta=0.0), dict(loss_kind=2, huber_delta=-1.0), dict(loss_kind=2, huber_delta=nan),
               dict(loss_kind=2, huber_delta=inf), dict(label_smoothing=0.1), dict(cls_weight=w6.data_ptr()), dict(label_smoothing=nan)]
    cls_bad = [dict(loss_kind=1), dict(loss_kind=2, huber_delta=1.0), dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=nan),
               dict(label_smoothing=inf), dict(loss_kind=3)]
    for ncls, bads in ((0, reg_bad), (6, cls_bad)):
        m = TC._model(64, ncls)
        for kw in bads:
            a, o, keep = TC._record(m, B, seed=11, ncls=ncls, labels=ncls > 0)
            for k, v in kw.items():
                setattr(a, k, v)
            snap = m._flat.grads.clone()
            assert lib.mmbert_heads_step_fwd_levels_opt(stream, ctypes.addressof(a), 1, 7) == -1, (ncls, kw)
            assert lib.mmbert_heads_step_fwd_levels_opt(stream, ctypes.addressof(a), 7, 7) == -1, (ncls, kw)
            assert lib.mmbert_heads_step_bwd_levels_opt(stream, ctypes.addressof(a), 1, 6) == -1, (ncls, kw)
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(t).all()) for k, t in o.items() if k != "pred") and bool((o["pred"] == -7).all()), (ncls, kw)
            assert torch.equal(m._flat.grads.view(torch.int32), snap.view(torch.int32)), (ncls, kw)
    good = [(0, dict(loss_kind=1)), (0, dict(loss_kind=2, huber_delta=0.5)), (0, dict(loss_kind=1, huber_delta=-1.0)),
            (6, dict(label_smoothing=0.5)), (6, dict(cls_weight=w6.data_ptr())), (6, dict(cls_weight=w6.data_ptr(), label_smoothing=0.1))]
    for ncls, kw in good:
        m = TC._model(64, ncls)
        a, o, keep = TC._record(m, B, seed=11, ncls=ncls, labels=ncls > 0)
        for k, v in kw.items():
            setattr(a, k, v)
        assert lib.mmbert_heads_step_fwd_levels_opt(stream, ctypes.addressof(a), 1, 7) == 0, (ncls, kw)
        assert lib.mmbert_heads_step_bwd_levels_opt(stream, ctypes.addressof(a), 1, 6) == 0, (ncls, kw)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o["loss"]).all()) and bool(torch.isfinite(o["dfirst"]).all()), (ncls, kw)
