"""``MMBertForPretraining.predict(return_attention=...)`` / ``trainer.predict_epoch(return_attention=...)``: the [CLS] attention maps.

* against the fp32 CPU oracle: attention row 0 of every layer, rebuilt from the oracle's collected hidden states with its own
  ``_linear`` / ``_r`` / ``extended_attention_mask`` and a float64 softmax.  Bound per layer and pass: the L1 distance of every (sample,
  head) row <= 3 x the largest L1 distance that ``oracle.bf16_storage_emulation()`` ALONE produces for that layer and pass against the
  fp32 oracle (computed here on the CPU, from the reference side only; the factor 3 is the one ``check_against_oracle`` grants bf16
  storage: two independent roundings of the same size, plus margin).  A key the oracle gives exactly 0 must be exactly 0.  The
  measured distances go to the suite's report directory as predict_attention_parity.json.
* in situ: every ``ops.attn_probs_first`` call of a ``predict`` is captured and recomputed with ``reference_probs``; the maps the model
  returns must pass ``check_probs`` against that -- layer order, pass order and key order, independently of the oracle bound; dedupe
  on equals dedupe off at the existing predict test's rtol 1e-5 / atol 1e-7.
* behaviour: 0 / 1 / L launches, the prediction and the pooled outputs keep their bits (regression and 3-class head), B = 160 equals
  128 + 32, the modality masses, ``predict_epoch`` in dataset order, no side effect on a train step."""
import contextlib
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmbert_oracle as O
from msa_amd.data import synthetic_batch, batch_to

import tests.test_model_gpu as TM
from tests import attention_probs_ref as P

DEV = "cuda"
CFG3 = dict(TM.CFG1, layers=3)
CFG_BASE2 = dict(hidden=768, layers=2, heads=12, intermediate=3072, vocab=30522, dataset="mosei", alpha=1.0, beta=1.0)
SMALL = dict(hidden=128, layers=3, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)
NAMES = ("text", "visual", "speech")
_PARITY = {}


def _args3(batch):
    return batch["input_ids"], batch["token_type_ids"], batch["attention_mask"]


def _oracle_attention(cfg, batch, emulate):
    """{"text" | "visual" | "speech": float64 [L, B, heads, S]}: attention row 0 of every layer of the fp32 oracle (``emulate``: with its
    bf16 storage emulation on), from the hidden states it collects."""
    p = O.seeded_params(cfg)
    ocfg = dict(cfg, hidden_dropout=0.0, attn_dropout=0.0, joint_dropout=0.0)
    text_ids, visual, speech, twv, tws = batch["input_ids"]
    tt = batch["token_type_ids"]
    am_t, am_v, am_s = batch["attention_mask"]
    heads, dh = cfg["heads"], cfg["hidden"] // cfg["heads"]
    out = {}
    with torch.no_grad(), (O.bf16_storage_emulation() if emulate else contextlib.nullcontext()):
        for name, ids, mask, tts, joint in (("text", text_ids, am_t, tt[0], False), ("visual", (twv, visual), am_v, tt[1], True),
                                            ("speech", (tws, speech), am_s, tt[2], True)):
            col = {}
            O.mmbert_model(p, ocfg, ids, mask, tts, joint, collect=col)
            xs = [col["jemb"] if joint else col["emb"]] + list(col["hidden"][:-1])
            if joint:
                ext = torch.cat((O.extended_attention_mask(mask[0], True), O.extended_attention_mask(mask[1], True)), dim=-1)
            else:
                ext = O.extended_attention_mask(mask, False)
            rows = []
            for i, x in enumerate(xs):
                pre = f"bert.encoder.layer.{i}."
                B, S, _ = x.shape
                q = O._r(O._linear(x[:, :1], p, pre + "attention.self.query", True)).view(B, 1, heads, dh).transpose(1, 2)
                k = O._r(O._linear(x, p, pre + "attention.self.key", True)).view(B, S, heads, dh).transpose(1, 2)
                w = torch.matmul(q.double(), k.double().transpose(2, 3)) * (dh ** -0.5) + ext.double()
                rows.append(torch.softmax(w, dim=-1)[:, :, 0])                   # [B, heads, S]
            out[name] = torch.stack(rows)
    return out


def _l1(a, b):
    """[L]: the largest L1 distance of a (sample, head) row, per layer."""
    return (a.double().cpu() - b.double().cpu()).abs().sum(-1).amax((1, 2))


@pytest.mark.parametrize("tag,cfg,shape,seed", [("cfg1_L3", CFG3, (2, 50, 64, 64), 1), ("bert_base_L2", CFG_BASE2, (2, 50, 500, 500), 5)],
                         ids=["cfg1_L3", "bert_base_L2"])
def test_attention_maps_match_the_oracle(tag, cfg, shape, seed):
    """Measured (L1 of the product against 3 x the calibrator, per layer): see DESIGN.md 3.8 and predict_attention_parity.json."""
    B, T, Pv, Pa = shape
    batch = synthetic_batch(B, T, Pv, Pa, dataset=cfg["dataset"], vocab=cfg["vocab"], seed=seed)
    ref, emu = _oracle_attention(cfg, batch, False), _oracle_attention(cfg, batch, True)
    m = TM.build(cfg)
    _, ex = m.predict(*_args3(batch_to(batch, DEV)), return_attention="all")
    torch.cuda.synchronize()
    assert ex["attention_layers"] == list(range(cfg["layers"]))
    rep = {}
    for name, S in zip(NAMES, (T, T + Pv, T + Pa)):
        got = ex["attention"][name]
        assert got.shape == (cfg["layers"], B, cfg["heads"], S) and got.dtype == torch.float32 and got.is_cuda
        cal, dist = _l1(emu[name], ref[name]), _l1(got, ref[name])
        rep[name] = dict(product_l1=dist.tolist(), calibrator_l1=cal.tolist(), ratio=(dist / (3.0 * cal)).tolist())
    _PARITY[tag] = rep
    TM._report("predict_attention_parity", _PARITY)
    print(tag, json.dumps(rep))
    for name in NAMES:
        got = ex["attention"][name].cpu()
        assert bool(torch.isfinite(got).all())
        assert bool((got[ref[name] == 0] == 0).all()), (tag, name, "a key the oracle gives exactly 0 has weight")
        for i, r in enumerate(rep[name]["ratio"]):
            assert r <= 1.0, (tag, name, "layer", i, rep[name])


def _predict(m, dbatch, **kw):
    return m.predict(*_args3(dbatch), **kw)


@pytest.fixture(scope="module")
def small():
    m = TM.build(SMALL)
    dbatch = batch_to(synthetic_batch(3, 24, 60, 40, dataset="mosei", vocab=SMALL["vocab"], seed=2), DEV)
    return m, dbatch


def test_returned_maps_are_the_captured_launches_recomputed(small, monkeypatch):
    from msa_amd import ops
    m, dbatch = small
    B, lens3 = 3, (24, 24 + 60, 24 + 40)
    calls = []
    orig = ops.attn_probs_first

    def spy(qkv, key_bias, layout, H, q_rows, **kw):
        calls.append((qkv.clone(), key_bias.clone(), layout, q_rows.clone()))
        return orig(qkv, key_bias, layout, H, q_rows, **kw)
    monkeypatch.setattr(ops, "attn_probs_first", spy)
    m.dedupe_masked_rows = False
    try:
        _, ex = _predict(m, dbatch, return_attention="all")
    finally:
        m.dedupe_masked_rows = True
    monkeypatch.undo()
    torch.cuda.synchronize()
    L, heads = SMALL["layers"], SMALL["heads"]
    assert len(calls) == L and ex["attention_layers"] == list(range(L))
    for i, (qkv, kb, layout, q_rows) in enumerate(calls):
        lens = list(layout.lens)
        assert lens == [n for n in lens3 for _ in range(B)] and not getattr(layout, "split", False)
        assert torch.equal(q_rows.cpu(), layout.seq_start.cpu().to(torch.int32))        # the [CLS] rows: position 0 of every sequence
        bias = kb[layout.bias_index].cpu()
        rp, rs = P.reference_probs(qkv.cpu(), bias, lens, heads)
        got = torch.zeros(3 * B, heads, max(lens))
        for k, name in enumerate(NAMES):
            got[k * B:(k + 1) * B, :, :lens3[k]] = ex["attention"][name][i].cpu()
        l1, el = P.check_probs(got, rp, rs, f"layer {i}")
        print("layer", i, "L1 %.3f u, elementwise %.3f u max p" % (l1, el))
    _, dd = _predict(m, dbatch, return_attention="all")                                   # the inference packing
    for name in NAMES:
        assert torch.allclose(dd["attention"][name], ex["attention"][name], rtol=1e-5, atol=1e-7), name


def test_launch_counts_and_unchanged_outputs(small, monkeypatch):
    from msa_amd import ops
    m, dbatch = small
    L = SMALL["layers"]
    plain, pooled = _predict(m, dbatch, return_pooled=True)
    count = []
    orig = ops.attn_probs_first
    monkeypatch.setattr(ops, "attn_probs_first", lambda *a, **k: (count.append(1), orig(*a, **k))[1])
    assert not ops.launches_unwrapped()
    spied = {}
    for mode, n in ((None, 0), (False, 0), ("top", 1), ("all", L)):
        del count[:]
        spied[mode] = _predict(m, dbatch, return_attention=mode)
        assert len(count) == n, (mode, len(count))
    monkeypatch.undo()
    assert ops.launches_unwrapped()
    assert torch.is_tensor(spied[None]) and torch.equal(spied[None], plain)
    top, ex_top = _predict(m, dbatch, return_attention="top")                             # the composite per-layer path
    full, ex = _predict(m, dbatch, return_attention="all", return_pooled=True)
    torch.cuda.synchronize()
    assert torch.equal(top, plain) and torch.equal(full, plain) and torch.equal(spied["all"][0], plain)
    for k in ("pooled", "fused", "t_rel", "v_rel", "s_rel"):
        assert torch.equal(ex[k], pooled[k]), k
    assert set(ex_top) == {"attention", "attention_layers", "attention_mass"} and set(ex) == set(ex_top) | set(pooled)
    assert ex_top["attention_layers"] == [L - 1] and ex["attention_layers"] == list(range(L))
    for name in NAMES:
        assert torch.equal(ex_top["attention"][name][0], ex["attention"][name][-1]), name
        assert torch.equal(spied["all"][1]["attention"][name], ex["attention"][name]), name     # per-launch path: the same bits
        rows = ex["attention"][name].sum(-1)
        assert bool((rows - 1.0).abs().max() < 1e-5), name
    from msa_amd.model import attention_modality_mass
    for name in NAMES[1:]:
        mass = ex["attention_mass"][name]
        assert mass.shape == (L, 3, SMALL["heads"], 2)
        assert torch.equal(mass, attention_modality_mass(ex["attention"][name], 24))
        assert torch.allclose(mass.sum(-1), ex["attention"][name].sum(-1), rtol=0, atol=1e-6)
        assert torch.equal(ex_top["attention_mass"][name][0], mass[-1])
    assert "text" not in ex["attention_mass"]


def test_class_head_model_keeps_its_bits():
    from tests.test_classification_gpu import _class_model
    m = _class_model(3)
    dbatch = batch_to(synthetic_batch(4, 50, 64, 64, seed=5, mlm_probability=0.0, num_labels=3), DEV)
    cls, pooled = _predict(m, dbatch, return_pooled=True)
    cls2, ex = _predict(m, dbatch, return_pooled=True, return_attention="all")
    cls3, ex3 = _predict(m, dbatch, return_attention="top")
    torch.cuda.synchronize()
    assert cls.dtype == torch.int64 and torch.equal(cls, cls2) and torch.equal(cls, cls3)
    for k in ("pooled", "fused", "t_rel", "v_rel", "s_rel", "class_logits"):
        assert torch.equal(ex[k], pooled[k]), k
    assert "class_logits" not in ex3 and ex3["attention"]["visual"].shape == (1, 4, TM.CFG1["heads"], 114)


def _slice(x, sl):
    if torch.is_tensor(x):
        return x[sl]
    return type(x)(_slice(y, sl) for y in x)


def test_a_batch_of_160_equals_its_parts():
    cfg = dict(TM.CFG1, vocab=4096)
    m = TM.build(cfg)
    dbatch = batch_to(synthetic_batch(160, 24, 40, 30, dataset="mosei", vocab=cfg["vocab"], seed=4), DEV)
    whole, ex = _predict(m, dbatch, return_attention="all")
    parts = [m.predict(*(_slice(a, sl) for a in _args3(dbatch)), return_attention="all") for sl in (slice(0, 128), slice(128, 160))]
    torch.cuda.synchronize()
    assert torch.equal(whole, torch.cat([p[0] for p in parts]))
    for name in NAMES:
        assert torch.equal(ex["attention"][name], torch.cat([p[1]["attention"][name] for p in parts], dim=1)), name
    for name in NAMES[1:]:
        assert torch.equal(ex["attention_mass"][name], torch.cat([p[1]["attention_mass"][name] for p in parts], dim=1)), name


def test_predict_epoch_returns_the_maps_in_dataset_order():
    from torch.utils.data import Dataset
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
    m = TM.build(dict(TM.CFG1, vocab=30522), train=True)
    args = T.default_args(val_batch_size=4, test_batch_size=3, mlm=False)
    preds, ex = T.predict_epoch(args, m, ds, device=DEV, return_attention="all")
    assert m.training and preds.shape == (10, 1) and ex["attention_layers"] == [0, 1]
    assert np.array_equal(preds, T.predict_epoch(args, m, ds, device=DEV))
    for name in NAMES:
        assert isinstance(ex["attention"][name], np.ndarray) and ex["attention"][name].shape[:3] == (2, 10, TM.CFG1["heads"])
    for i0 in range(0, 10, 3):
        kw = T.pack_predict_inputs(T.collate([ds[i] for i in range(i0, min(i0 + 3, 10))]), DEV)
        one, e1 = m.predict(kw["input_ids"], kw["token_type_ids"], kw["attention_mask"], return_attention="all")
        assert np.array_equal(preds[i0:i0 + 3], one.cpu().numpy()), i0
        for name in NAMES:
            assert np.array_equal(ex["attention"][name][:, i0:i0 + 3], e1["attention"][name].cpu().numpy()), (name, i0)
        for name in NAMES[1:]:
            assert np.array_equal(ex["attention_mass"][name][:, i0:i0 + 3], e1["attention_mass"][name].cpu().numpy()), (name, i0)
    top = T.predict_epoch(args, m, ds, device=DEV, return_attention="top")[1]
    assert top["attention_layers"] == [1] and np.array_equal(top["attention"]["speech"][0], ex["attention"]["speech"][1])
    # two batches of different key widths cannot be concatenated
    loader = torch.utils.data.DataLoader(ds, batch_size=5, collate_fn=T.collate)
    kws = [T.pack_predict_inputs(b, DEV) for b in loader]
    ids, tts, masks = kws[1]["input_ids"], kws[1]["token_type_ids"], kws[1]["attention_mask"]
    cut = ids[1].shape[1] - 1                                   # one visual position fewer in the second batch
    kws[1] = dict(input_ids=(ids[0], ids[1][:, :cut].contiguous(), ids[2], ids[3], ids[4]), token_type_ids=tts,      # (joint token types are not read)
                  attention_mask=(masks[0], (masks[1][0], masks[1][1][:, :cut].contiguous()), masks[2]))
    with pytest.raises(ValueError, match="key width"):
        T.predict_epoch(args, m, None, device=DEV, batches=kws, return_attention="top")


def test_predict_with_attention_between_two_train_steps_changes_nothing():
    """The construction of test_predict_gpu.test_predict_between_two_train_steps_changes_nothing (synchronous prologue)."""
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
        m.async_prologue = False
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
                p, ex = m.predict(*_args3(pool[(i + 1) % 3]), return_attention="all")
                assert m.training and bool(torch.isfinite(p).all()) and bool(torch.isfinite(ex["attention"]["visual"]).all())
                assert not any(k in m.__dict__ for k in ("_heads_src", "_heads_pre")) and m.__dict__.get("_last_trunk") is None
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
