"""Low-rank adapters in the model (model.add_lora), on the config and batch of tests/test_freeze_gpu.py: hidden 128, 4 layers,
2 heads, synthetic_batch(2, 16, 40, 24), deterministic mode, single-layer weight-gradient launches.

Yardsticks: a twin without adapters (B = 0 changes no bit), the weight gradient the existing TN kernel wrote in the same backward
(the gradient identity, bound from tests/lora_ref.py), the CPU oracle on the merged weights, launch spies, and the eval-mode forward."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmbert_oracle as O
from tests import lora_ref as LR
import tests.test_freeze_gpu as TF

DEV = "cuda"
CFG, L = TF.CFG, TF.L
H = CFG["hidden"]
build, batch, settings, fb, result = TF.build, TF.batch, TF.settings, TF.fb, TF.result
_deterministic = TF._deterministic                  # (the autouse fixture of that module, here as well)
TARGETS = ("query", "value")


def lora_names(m):
    return [n for n, _ in m.named_parameters() if ".lora_" in n]


def randomize(m, seed=3, a_std=0.02, b_std=0.02):
    """A and B ~ N(0, std) from a CPU generator, through the documented route for out-of-band writes."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_A"):
                p.copy_((torch.randn(p.shape, generator=g) * a_std).to(DEV))
            elif n.endswith("lora_B"):
                p.copy_((torch.randn(p.shape, generator=g) * b_std).to(DEV))
    m.parameters_changed()
    return m


class LoraSpy(TF.Spy):
    NAMES = TF.Spy.NAMES + ("lora_qkv_fwd", "lora_qkv_bwd", "layer_fwd", "attn_fwd")


# ---- 1. fresh adapters change nothing ----------------------------------------------------------------------------------------------
def test_zero_b_twin():
    m = settings(build())
    m.add_lora(r=8, alpha=16.0, targets=TARGETS, freeze_base=False, seed=1)
    res = result(m, *fb(m))
    tw = TF.twin()
    for x, y in zip(res["losses"], tw["losses"]):
        assert torch.equal(x, y)
    assert torch.equal(res["logits"], tw["logits"])
    ad = set(lora_names(m))
    assert len(ad) == 2 * 2 * L
    for n, g in tw["grads"].items():
        if g is None:
            assert res["grads"][n] is None, n
        else:
            assert torch.equal(res["grads"][n], g), n
    for n in ad:
        g = res["grads"][n]
        assert g is not None, n
        if n.endswith("lora_A"):
            assert not bool(g.any()), n                                # dA = s g^T x with g = dqkv B = 0: exactly zero
        else:
            assert float(g.abs().max()) > 0.0, n


# ---- 2. the gradient identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse_top", [True, False])
def test_gradient_identity_against_the_tn_kernel(sparse_top):
    """dB_t = s dW_t A_t^T and dA_t = s B_t^T dW_t in float64, dW_t = the rows t H .. (t + 1) H of g_Wqkv that the existing weight-gradient
    kernel wrote in the same backward from the same dqkv and x.  Bound: lora_ref.identity (C_OUT = 2 on 2^-23, C_ACC = 0.75, C_MID = 4),
    calibrated on the CPU like the kernels' own (tests/test_lora_reference_cpu.py::test_identity_bound_on_the_cpu: the emulation reaches
    0.18 of it on realistic inputs, 0.43 on the 2^+-20-scaled ones; at most 0.5).  Dense top layer and the row-sparse one."""
    m = settings(build())
    if not sparse_top:
        m.sparse_top_layer_backward = False
    m.add_lora(r=8, alpha=16.0, targets=TARGETS, freeze_base=False, seed=1)
    randomize(m)
    with LoraSpy() as spy:
        fb(m)
        calls = [(a[0].detach().clone(), a[1].detach().clone(), a[2].detach().clone()) for a, k in spy.calls["lora_qkv_bwd"]]
    assert len(calls) == L
    s = 16.0 / 8
    worst = 0.0
    for (dqkv, x, h), i in zip(calls, reversed(range(L))):
        lw = m._lw[i]
        dW = lw["g_Wqkv"].detach().double().cpu()
        for ti, t in enumerate(TARGETS):
            k = LR.TARGETS.index(t)
            ref = LR.identity(dW[k * H:(k + 1) * H], lw["lora"]["A"][t].cpu(), lw["lora"]["B"][t].cpu(), dqkv[:, k * H:(k + 1) * H].cpu(), x.cpu(),
                              h[:, ti * 8:(ti + 1) * 8].cpu(), s)
            named = dict(m.named_parameters())
            p = f"bert.encoder.layer.{i}.attention.self.{t}."
            qa = LR.check(named[p + "lora_A"].grad, ref["dA"], f"layer {i} {t} dA")
            qb = LR.check(named[p + "lora_B"].grad, ref["dB"], f"layer {i} {t} dB")
            assert float(named[p + "lora_A"].grad.abs().max()) > 0 and float(named[p + "lora_B"].grad.abs().max()) > 0
            worst = max(worst, qa, qb)
    print("gradient identity, sparse top layer", sparse_top, "largest error / bound", worst)


# ---- 3. merged twin against the oracle ---------------------------------------------------------------------------------------------------
def _pooled_oracle(sd, b):
    p = {k: v.detach().float().cpu() for k, v in sd.items()}
    ocfg = dict(CFG, hidden_dropout=0.0, attn_dropout=0.0, joint_dropout=0.0)
    text_ids, visual, speech, twv, tws = b["input_ids"]
    tt = b["token_type_ids"]
    am_t, am_v, am_s = b["attention_mask"]
    with torch.no_grad():
        return torch.stack([O.mmbert_model(p, ocfg, text_ids, am_t, tt[0], False)[1], O.mmbert_model(p, ocfg, (twv, visual), am_v, tt[1], True)[1],
                            O.mmbert_model(p, ocfg, (tws, speech), am_s, tt[2], True)[1]]).double()


def test_merged_twin_against_the_oracle():
    """M1 = adapters (A ~ N(0, 0.02), B ~ N(0, 0.05)) on q and v of every layer, M2 = its merge_lora()d copy, O = the CPU oracle on M2's
    state dict: ||pooled(M1) - O|| <= 2 ||pooled(M2) - O||  (M1 rounds q and v to bf16 once more than M2: that cannot double the error of
    a layer that already rounds seven tensors).  OBSERVED on MI355X: |M1 - O| 4.06e-2, |M2 - O| 4.24e-2, ratio 0.96.  B's scale (0.05: s B A
    is then about a quarter of W's own scale 0.02; at 0.02 this small model's pooled vectors hardly move) is chosen so that the same run
    with alpha doubled on M1 breaks the bound (observed: 1.11e-1, ratio 2.6)."""
    from msa_amd.data import synthetic_batch, batch_to
    cb = synthetic_batch(2, 16, 40, 24, vocab=CFG["vocab"], seed=5)
    db = batch_to(cb, DEV)
    args = (db["input_ids"], db["token_type_ids"], db["attention_mask"])
    m1 = build()
    m1.add_lora(r=8, alpha=16.0, targets=TARGETS, seed=1)
    randomize(m1, b_std=0.05)
    m2 = copy.deepcopy(m1).merge_lora()
    assert not lora_names(m2) and set(m2.state_dict()) == set(build().state_dict())
    ref = _pooled_oracle(m2.state_dict(), cb)
    p1 = m1.predict(*args, return_pooled=True)[1]["pooled"].double().cpu()
    p2 = m2.predict(*args, return_pooled=True)[1]["pooled"].double().cpu()
    e1, e2 = float((p1 - ref).norm()), float((p2 - ref).norm())
    m3 = build()
    m3.add_lora(r=8, alpha=32.0, targets=TARGETS)
    m3.load_state_dict(m1.state_dict())
    p3 = m3.predict(*args, return_pooled=True)[1]["pooled"].double().cpu()
    e3 = float((p3 - ref).norm())
    print(f"merged twin: |M1 - O| {e1:.4e} |M2 - O| {e2:.4e} ratio {e1 / e2:.3f}; alpha doubled {e3:.4e} ratio {e3 / e2:.3f}")
    assert e2 > 0 and e1 <= 2.0 * e2, (e1, e2)
    assert e3 > 2.0 * e2, (e3, e2)


# ---- 4. frozen base ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers,first", [(None, 0), ([2, 3], 2)])
def test_frozen_base_plan_and_launches(layers, first):
    m = settings(build())
    m.add_lora(r=8, targets=TARGETS, layers=layers, seed=1)
    randomize(m)
    plan = m.trainable_plan()
    assert plan.first_layer == first and plan.stop == first and not plan.embedding_stage
    assert all(v == "none" for i in plan.layers for v in plan.layers[i].values())
    with LoraSpy() as spy:
        fb(m)
    dense = {m._lw[i]["g_" + k].data_ptr() for i in range(L) for k in ("Wqkv", "Wo", "W1", "W2")}
    assert not (set(TF._tn_targets(spy)) & dense), "a weight-gradient tile ran for the frozen encoder"
    assert len(spy.calls["attn_bwd"]) == L - first and len(spy.calls["lora_qkv_bwd"]) == L - first
    assert len(spy.calls["lora_qkv_fwd"]) == L - first                     # (the three passes share one token matrix: one call per adapted layer)
    bound = m._lw[first]["WqkvT"].data_ptr()
    assert not any(a[1].data_ptr() == bound for a, k in spy.calls["gemm_nt"]), "the layer where backward ends computed an input gradient"
    named = dict(m.named_parameters())
    for n in lora_names(m):
        assert named[n].grad is not None and float(named[n].grad.abs().max()) > 0, n
    assert named["bert.encoder.layer.3.attention.self.query.weight"].grad is None


@pytest.mark.parametrize("variant", ["plain", "clip+ema"])
def test_optimizer_moves_the_adapters_only(variant):
    from msa_amd.optim import AdamW
    m = settings(build())
    m.add_lora(r=8, targets=TARGETS, seed=1)
    randomize(m)
    opt = AdamW(list(m.parameters()), lr=1e-3, weight_decay=0.01)
    if variant != "plain":
        opt.ema(0.99)
    m._ensure_ready(next(m.parameters()).device)
    fz = {n for n in TF.frozen_names(m) if n.startswith(("bert.embeddings.", "bert.jointEmbeddings.", "bert.encoder."))}
    assert fz and not any(".lora_" in n for n in fz)
    before, beforeT = TF._snap(m, fz)
    ad0 = {n: p.detach().clone() for n, p in m.named_parameters() if ".lora_" in n}
    fb(m)
    if variant != "plain":
        opt.clip_grad_norm_(1.0)
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    after, afterT = TF._snap(m, fz)
    for n in fz:
        assert torch.equal(after[n][0], before[n][0]) and torch.equal(after[n][1], before[n][1]), n
    TF._frozen_transposes_equal(m, beforeT, afterT)
    named = dict(m.named_parameters())
    for n, v in ad0.items():
        assert not torch.equal(named[n].detach(), v), (n, "did not move")


def test_thirty_adapter_steps_lower_the_label_loss():
    """Only the adapters train; the objective is the alignment + label loss (alpha = beta = 0 take the MLM and CPC terms out of the joint
    loss, whose gradients at this size drown the label loss's: this 4-layer model's logits move by 1e-5 under an adapter of scale 0.05).
    OBSERVED on MI355X (deterministic mode): 3.59950 -> 3.59928, not monotone along the way."""
    from msa_amd.optim import AdamW
    m = settings(build(dropout=0.0))
    m.set_alpha_beta(0.0, 0.0)
    m.add_lora(r=8, targets=TARGETS, seed=1)
    for n, p in m.named_parameters():                                    # only the adapters train
        if ".lora_" not in n:
            p.requires_grad_(False)
    opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=2e-2, weight_decay=0.0)
    losses = []
    for _ in range(30):
        out, _ = m(**batch())
        losses.append(float(out[5]))
        out[0].mean().backward()
        opt.step()
        opt.zero_grad()
    print("label loss over 30 adapter-only steps:", losses[0], "->", losses[-1], losses[::5])
    assert losses[-1] < losses[0]


# ---- 5. other paths and round trips -------------------------------------------------------------------------------------------------------
def _adapted(seed=1):
    m = build()
    m.add_lora(r=8, targets=TARGETS, seed=seed)
    return randomize(m, b_std=0.05)


def test_predict_paths_apply_the_adapters():
    """predict, predict(return_attention="all") and predict_tokens against the eval-mode forward at the existing predict tests' standards:
    logits and relationship scores 2e-2 absolute (tests/test_predict_gpu.py), the MLM losses 3e-3 relative
    (tests/test_predict_tokens_gpu.py: test_model_gpu's loss_tol), attention rows summing to 1 within 1e-5
    (tests/test_predict_attention_gpu.py); and the adapters matter: the same calls on the adapter-free base differ by more."""
    m = _adapted()
    b = batch()
    args = (b["input_ids"], b["token_type_ids"], b["attention_mask"])
    m.eval()
    with torch.no_grad():
        fout, flogits = m(**b)
    logits, extra = m.predict(*args, return_pooled=True)
    la, ea = m.predict(*args, return_attention="all")
    tok = m.predict_tokens(*args, masked_labels=b["masked_labels"])
    base = build()
    base.eval()
    blogits = base.predict(*args)
    blogits = blogits[0] if isinstance(blogits, tuple) else blogits
    d = lambda x, y: float((x.detach().float() - y.detach().float()).abs().max())
    print("predict vs forward", d(logits, flogits), "attention call", d(la, flogits), "vs base", d(logits, blogits))
    assert d(logits, flogits) < 2e-2 and d(la, flogits) < 2e-2
    for k, j in (("t_rel", 8), ("v_rel", 10), ("s_rel", 12)):
        assert d(extra[k], fout[j]) < 2e-2, k
    assert d(logits, blogits) > d(logits, flogits)
    batt = base.predict(*args, return_attention="all")[1]["attention"]
    for name, att in ea["attention"].items():
        rows = att.float().sum(-1)
        assert bool((rows - 1.0).abs().max() < 1e-5), name
        assert not torch.equal(att, batt[name]), name                      # the probe sees the adapted q: the maps are not the base model's
    # forward drops the three per-pass MLM losses; their mean is what its joint loss holds: joint = mean(mlm) + ap + label - nce (alpha = beta = 1)
    want = float(fout[0]) - float(fout[4]) - float(fout[5]) + float(fout[6])
    got = float(tok["loss"].double().mean())
    print("predict_tokens mean MLM loss", got, "forward's", want)
    assert abs(got - want) <= 3e-3 * max(1.0, abs(want)), (got, want)


def test_adapter_file_round_trip_and_merge():
    m = _adapted()
    b = batch()
    args = (b["input_ids"], b["token_type_ids"], b["attention_mask"])
    sd = m.lora_state_dict()
    assert sd["r"] == 8 and sd["alpha"] == 16.0 and sd["targets"] == TARGETS and sd["layers"] == tuple(range(L))
    assert sorted(k for k in sd if k not in ("r", "alpha", "targets", "layers")) == sorted(lora_names(m))
    full = m.state_dict()
    assert all(k in full for k in lora_names(m))
    want = m.predict(*args)
    want = want[0] if isinstance(want, tuple) else want
    fresh = build()
    fresh.load_lora_state_dict(sd)
    got = fresh.predict(*args)
    got = got[0] if isinstance(got, tuple) else got
    assert torch.equal(got, want)
    other = build()
    other.add_lora(r=4, targets=TARGETS)
    with pytest.raises(ValueError, match="differ"):
        other.load_lora_state_dict(sd)
    twin2 = build()
    twin2.add_lora(r=8, targets=TARGETS)
    twin2.load_state_dict(full)                                            # the whole state dict carries the adapter keys
    got2 = twin2.predict(*args)
    got2 = got2[0] if isinstance(got2, tuple) else got2
    assert torch.equal(got2, want)
    ref_keys = set(build().state_dict())
    m.merge_lora()
    assert set(m.state_dict()) == ref_keys and m._lora is None
    m.add_lora(r=4, targets=("key",))                                      # ... and a new set may follow a merge
    m.remove_lora()
    assert set(m.state_dict()) == ref_keys


# ---- 6. nothing changes without adapters --------------------------------------------------------------------------------------------------
def test_without_adapters_nothing_changes():
    from msa_amd import ops
    m = settings(build())
    calls = {"lora": 0, "layer_fwd": 0}
    of, ob, ol = ops.lora_qkv_fwd, ops.lora_qkv_bwd, ops.layer_fwd
    # (layer_fwd is not one of the wrappers launches_unwrapped() watches: the composite path stays on)
    ops.layer_fwd = lambda *a, _o=ol: (calls.__setitem__("layer_fwd", calls["layer_fwd"] + 1), _o(*a))[1]
    try:
        assert ops.launches_unwrapped()
        fb(m)
    finally:
        ops.layer_fwd = ol
    assert calls["layer_fwd"] == L
    with LoraSpy() as spy:
        assert not ops.launches_unwrapped()                                # the adapter launches are among the watched wrappers
        fb(m)
    assert not spy.calls["lora_qkv_fwd"] and not spy.calls["lora_qkv_bwd"]
    f = m._flat
    assert not any(".lora_" in n for n in f.order)
    a = build()
    a.add_lora(r=8, targets=TARGETS, freeze_base=False)
    a._ensure_ready(next(a.parameters()).device)
    fa = a._flat
    assert [n for n in fa.order if ".lora_" not in n] == f.order           # the same order with the adapter names taken out ...
    q = "bert.encoder.layer.3.attention.self.query."
    assert fa.order.index(q + "lora_A") == fa.order.index("bert.encoder.layer.3.attention.self.value.bias") + 1   # ... right behind the q/k/v biases
    b2 = build()
    b2._ensure_ready(next(b2.parameters()).device)
    assert b2._flat.offset == f.offset and b2._flat.total == f.total


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from msa_amd import parallel
    from msa_amd.data import to_fused
    m = build()
    for kw in (dict(r=3), dict(r=32), dict(r=True), dict(targets=()), dict(targets=("query", "output")), dict(targets=("query", "query")),
               dict(layers=[]), dict(layers=[L]), dict(layers=[-1]), dict(layers=[1, 1]), dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            m.add_lora(**kw)
        assert not lora_names(m) and m._lora is None, kw
    m.add_lora(r=8, targets=TARGETS)
    with pytest.raises(ValueError, match="already has adapters"):
        m.add_lora(r=8, targets=TARGETS)
    with pytest.raises(NotImplementedError, match="adapters"):
        m.forward_fused(**to_fused(batch()))
    with pytest.raises(NotImplementedError, match="adapters"):
        parallel.DataParallel(m)
    alone = copy.deepcopy(m.bert)
    b = batch()
    with pytest.raises(NotImplementedError, match="stand-alone"):
        alone(b["input_ids"][0], attention_mask=b["attention_mask"][0], token_type_ids=b["token_type_ids"][0])
    for fn in (build().merge_lora, build().lora_state_dict):
        with pytest.raises(ValueError, match="no adapters"):
            fn()
