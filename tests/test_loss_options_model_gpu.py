"""``model.set_loss_options`` through the module API on the tiny model of tests/test_classification_gpu.py (B = 4, T = 50, 64 / 64
pair positions): the level-launch heads under every option set against the eager heads (``fused_heads = False``) at the bounds of
tests/test_model_gpu.py::test_fused_heads_equal_eager_heads, with the call counter showing that the level-launch path really ran;
the MLM smoothing's effect on the joint loss against its float64 value from the returned fp32 scores; all-default options = never
calling the setter, bit for bit, without a call of either ``_smooth`` symbol; and one ``trainer.train`` epoch on class labels with
balanced class weights and label smoothing from ``args``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from msa_amd.data import synthetic_batch, batch_to
from tests import loss_options_ref as LR
from tests import rowwise_ref as R
from tests.test_classification_gpu import _Count, _class_model
from tests.test_model_gpu import CFG1, build, rel

DEV = "cuda"

REG_OPTIONS = [dict(regression="l1"), dict(regression="huber", huber_delta=0.5), dict(regression="huber", huber_delta=0.5, mlm_label_smoothing=0.1)]
CLS_OPTIONS = [dict(class_weights=[0.5, 1.0, 2.0, 4.0, 0.25, 1.5]), dict(label_smoothing=0.1),
               dict(class_weights=[0.5, 1.0, 2.0, 4.0, 0.25, 1.5], label_smoothing=0.1, mlm_label_smoothing=0.1)]


def _step(m, batch, opts, fused):
    m.fused_heads = fused
    m.set_alpha_beta(0.7, 1.3)
    if opts is not None:
        m.set_loss_options(**opts)
    with _Count() as cnt:
        out, pred = m(**batch)
        out[0].mean().backward()
        torch.cuda.synchronize()
    assert (cnt.fwd >= 1 and cnt.bwd == 1) if fused else (cnt.fwd == 0 and cnt.bwd == 0), (fused, cnt.fwd, cnt.bwd)
    return out, pred, {n: q.grad.float().clone() for n, q in m.named_parameters()}


def _compare(make, batch, opts):
    (o1, p1, g1), (o2, p2, g2) = (_step(make(), batch, opts, fused) for fused in (True, False))
    for i in (0, 4, 5, 6):
        assert bool(torch.isfinite(o1[i]).all()) and rel(o1[i], o2[i]) < 1e-5, (i, float(o1[i]), float(o2[i]))
    for n in g1:
        if "attention.self.key.bias" in n:                  # true gradient 0: both sides hold rounding noise
            continue
        scale = float(g2[n].abs().max()) + 1e-12
        err = float((g1[n] - g2[n]).abs().max())
        assert err <= 3e-4 * scale + 3e-7, f"{n}: err {err:.3e} scale {scale:.3e}"
    assert float(g2["classifier1_2.weight"].abs().max()) > 0
    # forward's second value: the same kind of tensor from both paths (a class head: the int64 [B] predicted classes, equal on every
    # sample -- the eager raw logits' two largest are far more than a logit bound apart on this batch, as in test_classification_gpu)
    assert p1.shape == p2.shape and p1.dtype == p2.dtype
    if p1.dtype == torch.int64:
        assert p1.dim() == 1 and torch.equal(p1, p2)
    return o1, o2


@pytest.mark.parametrize("opts", REG_OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("num_labels", [7, 1])
def test_regression_options_fused_against_eager(opts, num_labels):
    batch = batch_to(synthetic_batch(4, 50, 64, 64, seed=9), DEV)

    def make():
        m = build(CFG1)
        m.num_labels = num_labels
        return m
    o1, o2 = _compare(make, batch, opts)
    plain = _step(make(), batch, None, True)[0]
    assert abs(float(plain[5]) - float(o1[5])) > 1e-4 * abs(float(plain[5]))      # (the option is seen: not the MSE)


@pytest.mark.parametrize("opts", CLS_OPTIONS, ids=["weights", "smoothing", "both+mlm"])
def test_class_options_fused_against_eager(opts):
    batch = batch_to(synthetic_batch(4, 50, 64, 64, seed=9, num_labels=6), DEV)
    o1, o2 = _compare(lambda: _class_model(6), batch, opts)
    # outputs[5] is the loss as configured in eval mode too (torch's loss modules do not look at the mode)
    m = _class_model(6)
    m.set_loss_options(**opts)
    m.set_alpha_beta(0.7, 1.3)
    m.eval()
    with torch.no_grad():
        oe, _ = m(**batch)
    assert rel(oe[5], o2[5]) < 1e-5


def test_mlm_smoothing_moves_the_joint_loss_by_its_float64_value():
    """scores_dtype = float32: joint(eps) - joint(0) = alpha / 3 sum_pass mean_rows eps (x_y - mean_c x), the right-hand side in float64
    from the returned scores (as the kernel reads them: rounded to bf16).  Bound: the reference's loss bound of those rows (both losses')."""
    eps = 0.1
    batch = batch_to(synthetic_batch(4, 50, 64, 64, seed=9), DEV)
    alpha = 0.7
    outs = []
    for e in (0.0, eps):
        m = build(CFG1)
        m.scores_dtype = torch.float32
        m.set_alpha_beta(alpha, 1.3)
        m.set_loss_options(mlm_label_smoothing=e)
        m.eval()
        with torch.no_grad():
            out, _ = m(**batch)
        outs.append(out)
    V = CFG1["vocab"]
    e32 = LR.eps32(eps)
    want, bound = 0.0, 0.0
    for p, si in enumerate((7, 9, 11)):
        scores = outs[1][si]
        assert scores.dtype == torch.float32 and torch.equal(scores, outs[0][si])
        lab = batch["masked_labels"][p].reshape(-1).cpu()
        X = scores.reshape(-1, scores.shape[-1]).cpu()
        assert X.shape[1] == V and X.shape[0] == lab.numel()
        ok = (lab >= 0) & (lab < V)
        assert int(ok.sum()) > 0
        Xb = X.to(torch.bfloat16).double()
        xy = Xb[ok].gather(1, lab[ok][:, None])[:, 0]
        want += float((e32 * (xy - Xb[ok].mean(1))).mean())
        bnd = torch.tensor([0, lab.numel()], dtype=torch.int32)
        Xp = torch.nn.functional.pad(X, (0, (-V) % 8))
        for e in (0.0, eps):
            ref = LR.ce_fwd(Xp, lab, V, bnd, 1, e)["loss"]
            bound += float(R.C_OUT * R.U_F32 * ref.val.abs() + R.C_ACC * R.EPS24 * ref.acc)
    want *= alpha / 3.0
    got = float(outs[1][0].double() - outs[0][0].double())
    # (the joint loss itself is an fp32 sum of the heads' terms: its own rounding, 2^-23 of each joint loss, joins the bound)
    bound = alpha / 3.0 * bound + 2.0 ** -23 * (abs(float(outs[0][0])) + abs(float(outs[1][0])))
    print(f"\njoint(eps) - joint(0) = {got:.9f}, float64 {want:.9f}, bound {bound:.3e}")
    assert want != 0.0 and abs(got - want) <= bound, (got, want, bound)


class _Recorder:
    """Records the names of the C entry points called on the library object (ops resolves ``lib.<name>`` at every call)."""

    def __init__(self):
        from msa_amd import _lib
        self._lib, self.names = _lib, []

    def __enter__(self):
        real, names = self._lib.load(), self.names

        class Proxy:
            def __getattr__(self, n):
                names.append(n)
                return getattr(real, n)
        self.real = real
        self._lib._lib = Proxy()
        return self

    def __exit__(self, *exc):
        self._lib._lib = self.real


@pytest.mark.parametrize("C", [0, 6])
def test_all_default_options_are_never_calling_the_setter(C):
    """set_loss_options() with every default: loss and every gradient bit for bit those of a model the setter never touched (deterministic
    mode: the atomic sums' bits depend on the arrival order), and neither ``_smooth`` symbol nor an ``_opt`` entry point is called."""
    batch = batch_to(synthetic_batch(4, 50, 64, 64, seed=9, **({"num_labels": C} if C else {})), DEV)
    res = []
    for call in (False, True):
        m = _class_model(C) if C else build(CFG1)
        m.deterministic = True
        try:
            m.manual_seed(3)
            with _Recorder() as rec:
                out, pred, g = _step(m, batch, {} if call else None, True)
        finally:
            m.deterministic = False
        assert "mmbert_ce_fwd" in rec.names and "mmbert_ce_bwd" in rec.names
        new = [n for n in rec.names if n.endswith("_smooth") or n.endswith("_opt")]
        assert not new, new
        res.append((out, g))
    for i in (0, 4, 5, 6):
        assert torch.equal(res[0][0][i], res[1][0][i]), i
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n
    # ... and with the smoothing on, the _smooth symbols ARE what runs
    m = _class_model(C) if C else build(CFG1)
    with _Recorder() as rec:
        _step(m, batch, dict(mlm_label_smoothing=0.1), True)
    assert "mmbert_ce_fwd_smooth" in rec.names and "mmbert_ce_bwd_smooth" in rec.names and "mmbert_ce_fwd" not in rec.names


def test_trainer_epoch_with_balanced_weights_and_smoothing(tmp_path):
    """One trainer.train epoch on synthetic six-class data with args.class_weights = "balanced" and args.label_smoothing = 0.1: the model
    carries the balanced weights of the training labels, every step goes through the level-launch heads, the losses are finite, and the
    saved checkpoint has exactly the keys of a model that never saw an option (the reference's format)."""
    from tests.golden.dataset_features import synthetic_features
    from msa_amd.dataset import MMBertDataset
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    from msa_amd import trainer as T
    C = 6
    ds = MMBertDataset(None, synthetic_features(n_items=24, L=16, seed=4, dataset="mosei"), "mosei", "sad", C)
    torch.manual_seed(5)
    m = MMBertForPretraining(MMBertConfig(vocab_size=2048, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512), num_labels=C)
    m.bert.set_joint_embeddings("mosei")
    m = m.to(DEV)
    keys = list(m.state_dict().keys())
    m.manual_seed(3)
    args = T.default_args(train_batch_size=8, val_batch_size=8, learning_rate=1e-3, n_epochs=1, num_labels=C, class_weights="balanced",
                          label_smoothing=0.1, mlm_label_smoothing=0.05)
    opt, sched = T.build_optimizer(m, args, num_train_optimization_steps=3)
    with _Count() as cnt:
        best = T.train(args, m, ds, ds, ds, opt, sched, device=DEV, save_root=str(tmp_path / "model_save"), numpy_root=str(tmp_path / "numpy_save"))
    labels = [int(ds[i][3]) for i in range(len(ds))]
    assert torch.equal(m.class_weights.cpu(), T.balanced_class_weights(labels, C)) and m.class_weights.is_cuda
    assert (m.label_smoothing, m.mlm_label_smoothing) == (0.1, 0.05)
    assert cnt.fwd >= 3 * 3 and cnt.bwd == 3
    h = best["history"]
    assert len(h) == 1 and np.isfinite(h[0]["train_loss"]) and np.isfinite(h[0]["valid_loss"])
    import glob
    import os
    # train() saves when the test accuracy rises above 0: on these 24 items the epoch's predictions hit some labels
    assert best["acc"] > 0.0 and best["path"] is not None
    files = glob.glob(os.path.join(best["save_dir"], "model_*.pt"))
    assert files == [best["path"]] and best["path"].endswith("model_1.pt")
    sd = torch.load(files[0], map_location="cpu")
    assert list(sd.keys()) == keys and "class_weights" not in sd
