"""The C-class label head through the module API: ``MMBertForPretraining(config, num_labels=C)`` / ``set_num_labels`` with the
level-launch heads (csrc/heads_coop.hip, ``ncls`` = C) against the eager heads of the same model, ``predict()`` against ``forward``,
``forward_fused``, and the trainer end to end on class labels (UR-FUNNY's binary task, MOSEI's six emotions)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from msa_amd.data import synthetic_batch, batch_to, to_fused
from tests.test_model_gpu import CFG1, build, rel

DEV = "cuda"
LOGIT_TOL = 2e-2            # tests/test_predict_gpu.py's logit_tol: predict() and forward differ by the top layer's rounding points
SEED = {2: 9, 6: 9}         # batch seeds at which every sample's two largest eager logits are more than 2e-5 apart (asserted)
PREDICT_SCALE = 64.0        # classifier1_2.weight x 64 in the predict test: HF-initialised logits are a few 1e-2 wide
PREDICT_SEED = {2: 5, 6: 5}


def _class_model(C, seed=0, cfg=CFG1, train=False):
    """build(cfg) with a C-class head: classifier1_2 re-created by set_num_labels under a fixed torch seed."""
    m = build(cfg, train=train)
    torch.manual_seed(1000 + seed)
    m.set_num_labels(C)
    assert m.classifier1_2.weight.shape == (C, cfg["hidden"]) and m.classifier1_2.weight.is_cuda
    return m


class _Count:
    """Counts the calls of ops.heads_step_fwd / heads_step_bwd (the level-launch heads' two C entry points)."""

    def __enter__(self):
        from msa_amd import ops
        self.ops, self.fwd, self.bwd = ops, 0, 0
        self.of, self.ob = ops.heads_step_fwd, ops.heads_step_bwd

        def f(*a, **k):
            self.fwd += 1
            return self.of(*a, **k)

        def b(*a, **k):
            self.bwd += 1
            return self.ob(*a, **k)
        ops.heads_step_fwd, ops.heads_step_bwd = f, b
        return self

    def __exit__(self, *exc):
        self.ops.heads_step_fwd, self.ops.heads_step_bwd = self.of, self.ob


def _hook_logits(m, store):
    return m.classifier1_2.register_forward_hook(lambda mod, inp, out: store.append(out.detach().float().clone()))


def _gap(raw):
    top = raw.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def _fused_against_eager(C, batch, forward="forward"):
    res = []
    for fused in (True, False):
        m = _class_model(C)
        m.fused_heads = fused
        m.set_alpha_beta(0.7, 1.3)
        raw = []
        h = _hook_logits(m, raw)
        with _Count() as cnt:
            out, pred = getattr(m, forward)(**batch)
            out[0].mean().backward()
            torch.cuda.synchronize()
        h.remove()
        # the level-launch path really ran in the fused model (forward in one or two calls: levels 1-6 may be queued ahead), and not in the eager one
        assert (cnt.fwd >= 1 and cnt.bwd == 1 and not raw) if fused else (cnt.fwd == 0 and cnt.bwd == 0 and len(raw) == 1), (fused, cnt.fwd, cnt.bwd, len(raw))
        res.append((out, pred, {n: q.grad.float().clone() for n, q in m.named_parameters()}, raw[0] if raw else None))
    (o1, p1, g1, _), (o2, p2, g2, raw) = res
    B = raw.shape[0]
    assert raw.shape == (B, C) and p1.shape == (B,) and p1.dtype == torch.int64 and p2.dtype == torch.int64
    for i in (0, 4, 5, 6):
        assert bool(torch.isfinite(o1[i]).all()) and rel(o1[i], o2[i]) < 1e-5, (i, float(o1[i]), float(o2[i]))
    for i in ((8, 10, 12) if forward == "forward" else (8,)):
        assert float((o1[i] - o2[i]).abs().max()) < 1e-5
    gap = _gap(raw)
    print(f"\nC={C} {forward}: label loss fused {float(o1[5]):.6f} eager {float(o2[5]):.6f}; smallest gap of the two largest eager logits {float(gap.min()):.3e}")
    keep = gap > 2e-5                                        # twice the logit bound
    assert bool(keep.all()), f"samples under the gap: {(~keep).nonzero().flatten().tolist()} -- pick another batch seed"
    assert torch.equal(p1, p2) and torch.equal(p1, raw.argmax(1))
    for n in g1:
        if "attention.self.key.bias" in n:                  # true gradient 0: both sides hold rounding noise
            continue
        scale = float(g2[n].abs().max()) + 1e-12
        err = float((g1[n] - g2[n]).abs().max())
        assert err <= 3e-4 * scale + 3e-7, f"{n}: err {err:.3e} scale {scale:.3e}"
    assert float(g2["classifier1_2.weight"].abs().max()) > 0


@pytest.mark.parametrize("C", [2, 6])
def test_fused_class_heads_equal_eager_heads(C):
    """tests/test_model_gpu.py::test_fused_heads_equal_eager_heads restated for a C-wide head (its bounds, for the reasons its
    docstring gives): losses 1e-5 relative, relationship scores 1e-5, every parameter gradient 3e-4 max|g| + 3e-7; the predicted
    classes equal on every sample (none is left out: the eager raw logits' two largest are more than 2e-5 apart on all of them)."""
    batch = batch_to(synthetic_batch(4, 50, 64, 64, seed=SEED[C], num_labels=C), DEV)
    _fused_against_eager(C, batch)


def test_forward_fused_with_a_class_head():
    batch = batch_to(to_fused(synthetic_batch(4, 50, 64, 64, seed=SEED[2], num_labels=2)), DEV)
    _fused_against_eager(2, batch, forward="forward_fused")


def test_class_head_refuses_float_labels_before_any_launch():
    m = _class_model(3)
    batch = batch_to(synthetic_batch(2, 50, 64, 64, seed=1), DEV)
    with _Count() as cnt, pytest.raises(TypeError, match="integer class labels"):
        m(**batch)
    assert cnt.fwd == 0


def _args3(b):
    return b["input_ids"], b["token_type_ids"], b["attention_mask"]


@pytest.mark.parametrize("C", [2, 6])
def test_predict_returns_the_classes_of_forward(C):
    """predict() against forward (eager heads, eval mode, no_grad) on the same unmasked batch: ``class_logits`` [B, C] within LOGIT_TOL
    of the eager raw logits, classes equal on every sample whose two largest eager logits are more than 2 LOGIT_TOL apart -- with
    classifier1_2.weight x PREDICT_SCALE that is every sample (asserted).  The model stays in train mode, no autograd graph; B = 300
    in chunks equals its chunks."""
    m = _class_model(C, train=True)
    with torch.no_grad():
        m.classifier1_2.weight.mul_(PREDICT_SCALE)
    batch = batch_to(synthetic_batch(4, 50, 64, 64, seed=PREDICT_SEED[C], mlm_probability=0.0, num_labels=C), DEV)
    pred, extra = m.predict(*_args3(batch), return_pooled=True)
    assert m.training and pred.shape == (4,) and pred.dtype == torch.int64 and not pred.requires_grad
    cl = extra["class_logits"]
    assert cl.shape == (4, C) and cl.dtype == torch.float32 and not cl.requires_grad and torch.equal(pred, cl.argmax(1))
    assert torch.equal(m.predict(*_args3(batch)), pred)
    raw = []
    h = _hook_logits(m, raw)
    m.eval()
    m.fused_heads = False
    with torch.no_grad():
        _, fpred = m(**batch)
    h.remove()
    m.fused_heads = True
    m.train()
    raw = raw[0]
    gap = _gap(raw)
    print(f"\nC={C}: |class_logits - eager| max {float((cl - raw).abs().max()):.3e}; eager logits in [{float(raw.min()):.3f}, {float(raw.max()):.3f}], "
          f"smallest gap {float(gap.min()):.3e}")
    assert float((cl - raw).abs().max()) <= LOGIT_TOL
    assert bool((gap > 2 * LOGIT_TOL).all()), f"samples under the gap: {(gap <= 2 * LOGIT_TOL).nonzero().flatten().tolist()}"
    assert torch.equal(pred, raw.argmax(1)) and torch.equal(pred, fpred)
    # B = 300: chunks of 128 in the heads = the three chunks on their own
    big = batch_to(synthetic_batch(300, 12, 16, 16, seed=3, mlm_probability=0.0, num_labels=C), DEV)
    pw, ew = m.predict(*_args3(big), return_pooled=True)
    assert pw.shape == (300,) and ew["class_logits"].shape == (300, C)
    for b0 in range(0, 300, 128):
        sl = slice(b0, min(b0 + 128, 300))
        part = _slice_batch(big, sl)
        pp, ep = m.predict(*_args3(part), return_pooled=True)
        assert torch.equal(pw[sl], pp) and torch.equal(ew["class_logits"][sl], ep["class_logits"]), b0


def _slice_batch(b, sl):
    def cut(x):
        if torch.is_tensor(x):
            return x[sl]
        if isinstance(x, (tuple, list)):
            return tuple(cut(y) for y in x)
        return x
    return {k: cut(v) for k, v in b.items()}


@pytest.mark.parametrize("dataset,task,C", [("ur_funny", "sentiment", 2), ("mosei", "sad", 6)])
def test_trainer_end_to_end_on_class_labels(tmp_path, dataset, task, C):
    """MMBertDataset -> collate -> trainer.train for 2 epochs at a small width: finite label loss, int64 test predictions in [0, C),
    the test_CE_score_model triple in range, and the saved model_<epoch>.pt reloads into a model built with the same num_labels and
    reproduces predict_epoch bit for bit."""
    import random
    from tests.golden.dataset_features import synthetic_features
    from msa_amd.dataset import MMBertDataset
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    from msa_amd import trainer as T
    ds = MMBertDataset(None, synthetic_features(n_items=24, L=16, seed=4, dataset=dataset), dataset, task, C)

    def model():
        torch.manual_seed(5)
        m = MMBertForPretraining(MMBertConfig(vocab_size=2048, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512),
                                 num_labels=C)
        m.bert.set_joint_embeddings(dataset)
        return m.to(DEV)
    m = model()
    m.manual_seed(3)
    random.seed(9)
    torch.manual_seed(100)
    args = T.default_args(train_batch_size=8, val_batch_size=8, learning_rate=1e-3, n_epochs=2, num_labels=C)
    b0 = T.collate([ds[i] for i in range(8)])
    assert b0[0][-1].dtype == torch.int64 and b0[0][-1].shape == (8,) and int(b0[0][-1].min()) >= 0 and int(b0[0][-1].max()) < C
    opt, sched = T.build_optimizer(m, args, num_train_optimization_steps=6)
    label_losses = []
    orig = m.forward

    def rec(*a, **k):
        out = orig(*a, **k)
        label_losses.append(out[0][5].detach())
        return out
    m.forward = rec
    with _Count() as cnt:
        best = T.train(args, m, ds, ds, ds, opt, sched, device=DEV, save_root=str(tmp_path / "model_save"), numpy_root=str(tmp_path / "numpy_save"))
    m.forward = orig
    assert cnt.fwd >= 2 * 3 * 3 and cnt.bwd == 2 * 3                        # every step of every epoch through the level-launch heads
    assert len(best["history"]) == 2 and all(np.isfinite(h["train_loss"]) and np.isfinite(h["valid_loss"]) for h in best["history"])
    assert bool(torch.isfinite(torch.stack(label_losses)).all())
    te = T.eval_epoch(args, m, ds, device=DEV)
    assert np.isfinite(te[5]) and te[6].dtype == np.int64 and te[6].shape == (24,) and te[6].min() >= 0 and te[6].max() < C and te[7].shape == (24,)
    acc, mae, f1 = T.test_CE_score_model(te[6], te[7])
    assert 0.0 <= acc <= 1.0 and 0.0 <= mae <= C - 1 and 0.0 <= f1 <= 1.0
    assert 0.0 <= best["acc"] <= 1.0 and best["path"] is not None, best
    saved_epoch = best["epoch"] + 1
    assert best["path"].endswith(f"model_{saved_epoch}.pt")
    sd = torch.load(best["path"], map_location="cpu")
    assert sd["classifier1_2.weight"].shape == (C, 128)
    if saved_epoch == 2:                                                    # the model in hand IS the saved one: bit for bit
        p1 = T.predict_epoch(args, m, ds, device=DEV)
        m2 = model()
        m2.load_state_dict(sd)
        p2 = T.predict_epoch(args, m2, ds, device=DEV)
        assert p1.dtype == np.int64 and p1.shape == (24,) and np.array_equal(p1, p2)
    m3, m4 = model(), model()
    m3.load_state_dict(sd)
    m4.load_state_dict(torch.load(best["path"], map_location="cpu"))
    p3, p4 = T.predict_epoch(args, m3, ds, device=DEV), T.predict_epoch(args, m4, ds, device=DEV)
    assert p3.dtype == np.int64 and p3.shape == (24,) and p3.min() >= 0 and p3.max() < C and np.array_equal(p3, p4)


def test_train_epoch_fused_against_eager_class_heads():
    """trainer.train_epoch over 4 micro-batches with C = 2, once with the fused heads and once with fused_heads = False, under
    model.deterministic = True and one manual_seed: the FIRST step's joint and label losses agree at the fused-against-eager bound
    (1e-5 relative); the later steps must be finite and are printed side by side (-s), not asserted -- how fast two trajectories drift
    apart has no derived bound."""
    from msa_amd import ops, trainer as T
    was = ops.deterministic()
    runs = []
    try:
        for fused in (True, False):
            m = _class_model(2, train=True)
            m.deterministic = True
            m.fused_heads = fused
            m.manual_seed(3)
            torch.manual_seed(100)
            args = T.default_args(train_batch_size=4, learning_rate=1e-3, mlm=True)
            opt, sched = T.build_optimizer(m, args, 4)
            batches = [batch_to(synthetic_batch(4, 50, 64, 64, seed=40 + i, num_labels=2), DEV) for i in range(4)]
            steps = []
            orig = m.forward

            def rec(*a, _o=orig, _s=steps, **k):
                out = _o(*a, **k)
                _s.append((out[0][0].detach().float().clone(), out[0][5].detach().float().clone()))
                return out
            m.forward = rec
            with _Count() as cnt:
                ret = T.train_epoch(args, m, None, opt, sched, device=DEV, quirk_step=False, batches=batches)
            torch.cuda.synchronize()
            assert (cnt.bwd == 4) if fused else (cnt.fwd == 0 and cnt.bwd == 0)
            assert len(steps) == 4 and all(np.isfinite(x) for x in ret)
            runs.append([(float(a), float(b)) for a, b in steps])
    finally:
        ops.set_deterministic(was)
    print("\nstep: joint fused / eager, label fused / eager")
    for i, ((jf, lf), (je, le)) in enumerate(zip(*runs)):
        print(f"  {i}: {jf:.6f} / {je:.6f}   {lf:.6f} / {le:.6f}")
        assert np.isfinite(jf) and np.isfinite(je) and np.isfinite(lf) and np.isfinite(le)
    (jf, lf), (je, le) = runs[0][0], runs[1][0]
    assert abs(jf - je) <= 1e-5 * abs(je) and abs(lf - le) <= 1e-5 * abs(le), (runs[0][0], runs[1][0])
