"""``MMBertForPretraining.predict`` / ``trainer.predict_epoch``: the label-free prediction path with its [CLS]-only top layer.

* against the fp32 CPU oracle (pinned to the real reference by tests/test_oracle_golden.py) on the shapes tests/test_model_gpu.py uses
  for ``forward``, at that file's bounds for exactly these quantities: regression logits and relationship scores ``logit_tol = 2e-2``
  absolute at two layers, ``3e-2`` at twelve; the pooler outputs and the classifier1_1 output are held to the same bound (tanh outputs
  and an O(1) linear map of them: the same scale as the logits).  The oracle needs labels; the logits do not depend on them.
* against ``forward`` in eval mode (``logit_tol``; the two differ by the top layer's rounding points only);
* every measured deviation goes to the suite's report directory as predict_parity.json (test_model_gpu._report), next to ``forward``'s own deviation on the same inputs;
* the short cut really runs (launch spies), the [tokens, vocab] buffer is never allocated, any batch size, no side effects on a
  train step, ``predict_epoch`` in dataset order."""
import json
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmbert_oracle as O
from msa_amd.data import synthetic_batch, batch_to

import tests.test_model_gpu as TM

DEV = "cuda"
CFG1 = TM.CFG1
CFG12 = dict(hidden=768, layers=12, heads=12, intermediate=3072, vocab=30522, dataset="mosei", alpha=1.0, beta=1.0)
_PARITY = {}


def _record(name, payload):
    _PARITY[name] = payload
    TM._report("predict_parity", _PARITY)                    # (the whole record so far: one file for the module)


def _args3(batch):
    return batch["input_ids"], batch["token_type_ids"], batch["attention_mask"]


def _maxabs(a, b):
    return float((a.detach().float().cpu() - b.detach().float().cpu()).abs().max())


def _oracle(cfg, batch, with_pooled):
    """The oracle's logits and relationship scores from its pinned full forward; pooler outputs and the classifier1_1 output from the
    same functions (mmbert_model per pass, the gate / classifier1_1 expressions of fusion_objective)."""
    p = O.seeded_params(cfg)
    ocfg = dict(cfg, hidden_dropout=0.0, attn_dropout=0.0, joint_dropout=0.0)
    with torch.no_grad():
        oout, ologits = O.pretraining_forward(p, ocfg, **batch)
        res = dict(logits=ologits, t_rel=oout[8], v_rel=oout[10], s_rel=oout[12])
        if with_pooled:
            text_ids, visual, speech, twv, tws = batch["input_ids"]
            tt = batch["token_type_ids"]
            am_t, am_v, am_s = batch["attention_mask"]
            pooled = [O.mmbert_model(p, ocfg, text_ids, am_t, tt[0], False)[1], O.mmbert_model(p, ocfg, (twv, visual), am_v, tt[1], True)[1],
                      O.mmbert_model(p, ocfg, (tws, speech), am_s, tt[2], True)[1]]
            gate = lambda x, v: O._linear(torch.relu(O._linear(torch.cat((x, x), dim=1), p, "attn")), p, v)
            cat = torch.cat([x * gate(x, v) for x, v in zip(pooled, ("vt", "vv", "vs"))], dim=1)
            res.update(pooled=torch.stack(pooled), fused=O._linear(cat, p, "classifier1_1"))
    return res


def _check_against_oracle(name, cfg, shape, seed, tol, num_labels=7, with_pooled=True, m=None):
    B, T, Pv, Pa = shape
    batch = synthetic_batch(B, T, Pv, Pa, dataset=cfg["dataset"], vocab=cfg["vocab"], seed=seed)
    ocfg = dict(cfg, num_labels=num_labels)
    ref = _oracle(ocfg, batch, with_pooled)
    m = m if m is not None else TM.build(cfg)
    m.num_labels = num_labels
    dbatch = batch_to(batch, DEV)
    logits, extra = m.predict(*_args3(dbatch), return_pooled=True)
    with torch.no_grad():
        fout, flogits = m(**dbatch)
    torch.cuda.synchronize()
    H = cfg["hidden"]
    assert logits.shape == (B, 1) and logits.dtype == torch.float32
    assert extra["pooled"].shape == (3, B, H) and extra["fused"].shape == (B, H) and all(extra[k].shape == (B, 2) for k in ("t_rel", "v_rel", "s_rel"))
    rep = dict(shape=list(shape), layers=cfg["layers"], hidden=H, num_labels=num_labels, bound=tol,
               predict_vs_oracle=dict(logits=_maxabs(logits, ref["logits"]), **{k: _maxabs(extra[k], ref[k]) for k in ("t_rel", "v_rel", "s_rel")}),
               forward_vs_oracle=dict(logits=_maxabs(flogits, ref["logits"]), t_rel=_maxabs(fout[8], ref["t_rel"]), v_rel=_maxabs(fout[10], ref["v_rel"]),
                                      s_rel=_maxabs(fout[12], ref["s_rel"])),
               predict_vs_forward=dict(logits=_maxabs(logits, flogits), t_rel=_maxabs(extra["t_rel"], fout[8]), v_rel=_maxabs(extra["v_rel"], fout[10]),
                                       s_rel=_maxabs(extra["s_rel"], fout[12])))
    if with_pooled:
        rep["predict_vs_oracle"].update(pooled=_maxabs(extra["pooled"], ref["pooled"]), fused=_maxabs(extra["fused"], ref["fused"]))
    _record(name, rep)
    print(name, json.dumps(rep))
    for k, v in rep["predict_vs_oracle"].items():
        assert v < tol, (name, "oracle", k, v)
    for k, v in rep["predict_vs_forward"].items():
        assert v < tol, (name, "forward", k, v)
    return m


@pytest.mark.parametrize("num_labels", [7, 1])
def test_cfg1_matches_oracle(num_labels):
    _check_against_oracle(f"cfg1_nl{num_labels}", CFG1, (2, 50, 64, 64), 1, 2e-2, num_labels=num_labels)


def test_bert_base_width_two_layers_matches_oracle():
    cfg = dict(hidden=768, layers=2, heads=12, intermediate=3072, vocab=30522, dataset="mosei", alpha=1.0, beta=1.0)
    _check_against_oracle("bert_base_L2", cfg, (2, 50, 500, 500), 5, 2e-2)


def test_bert_large_width_matches_oracle():
    cfg = dict(hidden=1024, layers=2, heads=16, intermediate=4096, vocab=8192, dataset="mosei", alpha=1.0, beta=1.0)
    _check_against_oracle("bert_large_width_L2", cfg, (2, 50, 96, 80), 8, 2e-2)


def test_mosi_dims_and_unequal_pair_lengths():
    cfg = dict(CFG1, dataset="mosi", vocab=4096, alpha=0.5, beta=0.25)
    _check_against_oracle("mosi_unequal", cfg, (3, 24, 70, 33), 6, 2e-2)


def test_ur_funny_dims_single_layer():
    """One layer: the top layer is the only one (layers 0 .. L - 2 are none)."""
    cfg = dict(hidden=256, layers=1, heads=4, intermediate=1024, vocab=2048, dataset="ur_funny", alpha=1.0, beta=1.0)
    _check_against_oracle("ur_funny_L1", cfg, (2, 50, 1375, 1375), 9, 2e-2)


@pytest.fixture(scope="module")
def model12():
    return TM.build(CFG12)


def test_bert_base_12_layers_matches_oracle(model12):
    _check_against_oracle("bert_base_L12_B2", CFG12, (2, 50, 500, 500), 12, 3e-2, with_pooled=False, m=model12)


def test_peak_memory_stays_below_the_vocabulary_logits(model12):
    """Headline shape (B = 16, T = 50, A = V = 500: 18 400 rows): ``predict`` never allocates as much as the [rows, vocab] bf16 logits
    alone (1.12 GB) above the level before the call; ``forward`` in eval mode does."""
    m = model12
    dbatch = batch_to(synthetic_batch(16, 50, 500, 500, dataset="mosei", vocab=CFG12["vocab"], seed=3), DEV)
    rows = 16 * (50 + 550 + 550)
    peaks = {}
    for tag in ("predict", "forward", "predict"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        if tag == "predict":
            out = m.predict(*_args3(dbatch))
        else:
            with torch.no_grad():
                out = m(**dbatch)
        torch.cuda.synchronize()
        peaks[tag] = torch.cuda.max_memory_allocated() - base
        del out
    cap = rows * m._flat.vpad * 2                                # [rows, ceil(V)] bf16
    assert cap > 1.1e9
    _record("peak_memory_headline", dict(cap_bytes=cap, **peaks))
    print("peak bytes above the level before the call:", peaks, "cap", cap)
    assert peaks["predict"] < cap < peaks["forward"], (peaks, cap)


def test_the_short_cut_really_runs(monkeypatch):
    from msa_amd import ops
    cfg = dict(hidden=128, layers=3, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)
    B = 4
    m = TM.build(cfg)
    dbatch = batch_to(synthetic_batch(B, 24, 60, 40, dataset="mosei", vocab=cfg["vocab"], seed=2), DEV)
    calls = []

    def spy(name):
        orig = getattr(ops, name)

        def f(*a, **k):
            calls.append((name, tuple(a[0].shape) if torch.is_tensor(a[0]) else None, tuple(a[1].shape) if len(a) > 1 and torch.is_tensor(a[1]) else None))
            return orig(*a, **k)
        monkeypatch.setattr(ops, name, f)
    for n in ("gemm_nt", "attn_fwd", "attn_fwd_first", "attn_bwd", "ce_fwd", "ce_bwd", "gemm_nt_splitk", "heads_step_fwd", "heads_predict"):
        spy(n)
    assert not ops.launches_unwrapped()
    logits = m.predict(*_args3(dbatch))
    torch.cuda.synchronize()
    names = [c[0] for c in calls]
    assert names.count("attn_fwd") == cfg["layers"] - 1 and names.count("attn_fwd_first") == 1 and names.count("heads_predict") == 1
    assert not any(n in names for n in ("ce_fwd", "ce_bwd", "attn_bwd", "heads_step_fwd", "gemm_nt_splitk"))
    gemms = [c for c in calls if c[0] == "gemm_nt"]
    assert all(c[2][0] < cfg["vocab"] for c in gemms), "a vocabulary-sized GEMM ran"
    behind = [c for c in calls[names.index("attn_fwd_first") + 1:] if c[0] == "gemm_nt"]
    assert len(behind) == 3 and all(c[1][0] == 3 * B for c in behind), behind
    monkeypatch.undo()
    assert ops.launches_unwrapped()
    assert torch.equal(logits, m.predict(*_args3(dbatch)))     # the composite per-layer path below the top layer: the same bits


def _slice(x, sl):
    if torch.is_tensor(x):
        return x[sl]
    return type(x)(_slice(y, sl) for y in x)


def test_any_batch_size_runs_in_chunks_without_a_warning():
    """B = 160 (beyond the 128 samples of one heads launch): equal to ``predict`` on its first 128 and last 32 samples -- the heads'
    chunks are independent, and a sample's encoder rows do not depend on its neighbours."""
    cfg = dict(CFG1, vocab=4096)
    B = 160
    m = TM.build(cfg)
    dbatch = batch_to(synthetic_batch(B, 24, 40, 30, dataset="mosei", vocab=cfg["vocab"], seed=4), DEV)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        whole, ex = m.predict(*_args3(dbatch), return_pooled=True)
    assert not w, [str(x.message) for x in w]
    parts = [m.predict(*(_slice(a, sl) for a in _args3(dbatch)), return_pooled=True) for sl in (slice(0, 128), slice(128, 160))]
    torch.cuda.synchronize()
    assert whole.shape == (B, 1) and ex["pooled"].shape == (3, B, cfg["hidden"]) and ex["fused"].shape == (B, cfg["hidden"])
    both = torch.cat([p[0] for p in parts])
    print("B = 160 against 128 + 32: largest difference", _maxabs(whole, both))
    assert torch.equal(whole, both)
    assert torch.equal(ex["pooled"], torch.cat([p[1]["pooled"] for p in parts], dim=1))
    for k in ("fused", "t_rel", "v_rel", "s_rel"):
        assert torch.equal(ex[k], torch.cat([p[1][k] for p in parts])), k


def test_dedupe_on_off_and_repeatability():
    cfg = dict(hidden=256, layers=2, heads=4, intermediate=1024, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)
    dbatch = batch_to(synthetic_batch(4, 24, 200, 130, dataset="mosei", vocab=cfg["vocab"], seed=35), DEV)
    m = TM.build(cfg)
    outs = {}
    for dd in (True, False):
        m.dedupe_masked_rows = dd
        seen = []
        orig = m._split_layout
        m._split_layout = lambda *a, _o=orig, _s=seen: (_s.append(_o(*a)), _s[-1])[1]
        outs[dd] = m.predict(*_args3(dbatch))
        again = m.predict(*_args3(dbatch))
        m._split_layout = orig
        assert (seen[0] is not None) == dd
        assert torch.equal(outs[dd], again)
    assert torch.allclose(outs[True], outs[False], rtol=1e-5, atol=1e-7), _maxabs(outs[True], outs[False])


@pytest.mark.parametrize("async_prologue", [False, True])
def test_predict_between_two_train_steps_changes_nothing(async_prologue):
    """Deterministic mode, train mode with dropout: step, predict, step == step, step -- losses, gradients and parameters bit for bit
    (no seed drawn, the prologue's alternating buffer sets untouched, no leftovers); the module's mode is not flipped."""
    from msa_amd import ops
    from msa_amd import trainer as T
    import tests.test_train_gpu as TT
    cfg = dict(hidden=128, layers=2, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)
    shape = (4, 24, 60, 40)
    pool = [batch_to(synthetic_batch(*shape, dataset="mosei", vocab=cfg["vocab"], seed=90 + i), DEV) for i in range(3)]
    torch.cuda.synchronize()

    def run(with_predict):
        m = TT.build(cfg, dropout=0.1)
        m.train()
        m.manual_seed(17)
        m.async_prologue = async_prologue
        opt, sched = T.build_optimizer(m, T.default_args(train_batch_size=shape[0], learning_rate=1e-3), 10, mode="hf")
        sched.step()
        losses, grads = [], []
        for i in range(3):
            out, _ = m(**pool[i])
            out[0].mean().backward()
            losses.append(out[0].detach().clone())
            grads.append(m._flat.grads.clone())
            opt.step(); sched.step(); opt.zero_grad()
            if with_predict:
                p = m.predict(*_args3(pool[(i + 1) % 3]))
                assert m.training and bool(torch.isfinite(p).all())
                assert not any(k in m.__dict__ for k in ("_heads_src", "_heads_pre")) and m.__dict__.get("_last_trunk") is None
                assert not m.__dict__.get("_late_wgrads")
        torch.cuda.synchronize()
        return losses, grads, m._flat.params.clone()
    was = ops.deterministic()
    try:
        ops.set_deterministic(True)
        a, b = run(False), run(True)
    finally:
        ops.set_deterministic(was)
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), (i, float(x), float(y))
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), f"gradients of step {i} differ"
    assert torch.equal(a[2], b[2])


def test_predict_works_inside_and_outside_no_grad_and_builds_no_graph():
    m = TM.build(dict(CFG1, vocab=4096), train=True)
    dbatch = batch_to(synthetic_batch(2, 16, 30, 20, dataset="mosei", vocab=4096, seed=8), DEV)
    a = m.predict(*_args3(dbatch))
    with torch.no_grad():
        b = m.predict(*_args3(dbatch))
    assert m.training and not a.requires_grad and a.grad_fn is None and torch.equal(a, b)        # train mode: still no dropout
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.predict(*_args3(synthetic_batch(2, 16, 30, 20, dataset="mosei", vocab=4096, seed=8)))
    m.num_labels = 3
    with pytest.raises(NotImplementedError, match="num_labels"):
        m.predict(*_args3(dbatch))


def test_predict_epoch_in_dataset_order():
    from torch.utils.data import Dataset, RandomSampler
    from tests.golden.dataset_features import synthetic_features
    from msa_amd import trainer as T
    from msa_amd.dataset import MMBertDataset
    import random
    random.seed(5)
    ds0 = MMBertDataset(None, synthetic_features(n_items=10, L=10, seed=3), "mosei", "sentiment", 1)
    items = [ds0[i] for i in range(len(ds0))]                   # (the dataset draws its negative pairs from `random` at every access)

    class Frozen(Dataset):
        def __len__(self):
            return len(items)

        def __getitem__(self, i):
            return items[i]
    ds = Frozen()
    cfg = dict(CFG1, vocab=30522)
    m = TM.build(cfg, train=True)
    args = T.default_args(val_batch_size=4, test_batch_size=3, mlm=False)
    preds = T.predict_epoch(args, m, ds, device=DEV)
    assert m.training and preds.shape == (10, 1) and preds.dtype == np.float32
    for i0 in range(0, 10, 3):                                   # row order = dataset order; equals per-batch predict
        kw = T.pack_predict_inputs(T.collate([ds[i] for i in range(i0, min(i0 + 3, 10))]), DEV)
        one = m.predict(kw["input_ids"], kw["token_type_ids"], kw["attention_mask"]).cpu().numpy()
        assert np.array_equal(preds[i0:i0 + 3], one), i0
    # batches of model kwargs (labels and other extra keys are ignored)
    loader = torch.utils.data.DataLoader(ds, batch_size=3, collate_fn=T.collate)
    again = T.predict_epoch(args, m, None, device=DEV, batches=(T.pack_step_inputs(b, args, DEV) for b in loader))
    assert np.array_equal(preds, again)
    # eval_epoch without MLM masking predicts the same utterances, in its sampler's order
    del args.test_batch_size                                     # (falls back to val_batch_size)
    assert np.array_equal(T.predict_epoch(args, m, ds, device=DEV).shape, (10, 1))
    class Index(Dataset):
        def __len__(self):
            return len(items)

        def __getitem__(self, i):
            return i
    torch.manual_seed(123)                                      # eval_epoch's own loader, replayed over the indices: the same draws
    order = [int(i) for b in torch.utils.data.DataLoader(Index(), sampler=RandomSampler(Index()), batch_size=args.val_batch_size) for i in b]
    torch.manual_seed(123)
    ev = T.eval_epoch(args, m, ds, device=DEV)
    m.train()
    assert sorted(order) == list(range(10)) and np.allclose(ev[7].reshape(-1), [float(items[i][3]) for i in order])
    d = float(np.abs(ev[6] - preds[order]).max())
    print("eval_epoch preds against predict_epoch: largest difference", d)
    assert d < 2e-2
