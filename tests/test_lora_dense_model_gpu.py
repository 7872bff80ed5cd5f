"""Adapters on attention.output.dense / intermediate.dense / output.dense in the model (model.add_lora's dense targets), on the
config and batch of tests/test_lora_model_gpu.py: hidden 128, 4 layers, 2 heads, intermediate 512, synthetic_batch(2, 16, 40, 24),
deterministic mode, single-layer weight-gradient launches.

Yardsticks: a twin without adapters (B = 0 on the two dropout + residual seams changes no bit), the weight gradients the existing TN kernel
wrote in the same backward (the gradient identity, bound from tests/lora_ref.py), the CPU oracle on the merged weights, the merged twin in
train mode under the same dropout seed (the dropout seam), launch spies, fresh twins along the adapters' life."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lora_dense_ref as DR
import tests.test_freeze_gpu as TF
import tests.test_lora_model_gpu as TL

DEV = "cuda"
CFG, L = TF.CFG, TF.L
H, I = CFG["hidden"], CFG["intermediate"]
build, batch, settings, fb, result = TF.build, TF.batch, TF.settings, TF.fb, TF.result
_deterministic = TF._deterministic                  # (the autouse fixture of that module, here as well)
randomize, lora_names = TL.randomize, TL.lora_names
DENSE = ("attention_output", "intermediate", "ffn_output")
ADD2 = ("attention_output", "ffn_output")
ALL = ("query", "key", "value") + DENSE
PATH = {"attention_output": "attention.output.dense", "intermediate": "intermediate.dense", "ffn_output": "output.dense"}
GW = {"attention_output": "g_Wo", "intermediate": "g_W1", "ffn_output": "g_W2"}


class DenseSpy(TL.LoraSpy):
    NAMES = TL.LoraSpy.NAMES + ("lora_dense_fwd", "lora_dense_bwd")


def _args(b=None):
    b = batch() if b is None else b
    return (b["input_ids"], b["token_type_ids"], b["attention_mask"])


def _target_of(lw, A):
    """Which dense target of the layer views ``lw`` the adapter matrix A belongs to (None: another layer's)."""
    dl = lw["lora_dense"]
    for t in dl["targets"]:
        if dl["A"][t].data_ptr() == A.data_ptr():
            return t
    return None


# ---- 1. fresh adapters on the dropout + residual seams change nothing -------------------------------------------------------------------
def test_zero_b_twin_on_the_add_seams():
    """Train mode, dropout 0.1, the twin's seed: with B = 0 the update fma(s c, 0, float(z)) leaves every element of z1 / z2 as the GEMM
    wrote it, and g = dY . B = 0 leaves every input gradient: losses, logits and every other gradient are the twin's bits, dA is exactly
    zero, dB is not.  (intermediate is not part of it: its seam rounds the pre-activation to bf16 once more than the fused epilogue.)"""
    m = settings(build())
    m.add_lora(r=8, alpha=16.0, targets=ADD2, freeze_base=False, seed=1)
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
            assert not bool(g.any()), n
        else:
            assert float(g.abs().max()) > 0.0, n


# ---- 2. the gradient identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse_top", [True, False])
def test_gradient_identity_against_the_tn_kernel(sparse_top):
    """dB = s dW A^T and dA = s B^T dW in float64, dW = g_Wo / g_W1 / g_W2 as the existing weight-gradient kernel wrote them in the same
    backward from the same dY and x (the final du for W1: the ffn_output term included).  Bound: lora_ref.identity through
    lora_dense_ref.identity (K != N), calibrated on the CPU (tests/test_lora_dense_reference_cpu.py::test_identity_bound_on_the_cpu: at
    most 0.42 of it).  Dense top layer and the row-sparse one (gathered operands, h recomputed)."""
    m = settings(build())
    if not sparse_top:
        m.sparse_top_layer_backward = False
    m.add_lora(r=8, alpha=16.0, targets=DENSE, freeze_base=False, seed=1)
    randomize(m)
    with DenseSpy() as spy:
        fb(m)
        calls = [(a[0].detach().clone(), a[1].detach().clone(), None if a[2] is None else a[2].detach().clone(), a[3], a[4], k)
                 for a, k in spy.calls["lora_dense_bwd"]]
    assert len(calls) == 3 * L
    assert any(c[2] is None for c in calls) == sparse_top                  # the sparse top layer recomputes h from the gathered rows
    s, worst, seen = 16.0 / 8, 0.0, set()
    named = dict(m.named_parameters())
    for dy, x, h, A, B, kw in calls:
        (i, t), = [(i, _target_of(m._lw[i], A)) for i in range(L) if _target_of(m._lw[i], A) is not None]
        seen.add((i, t))
        K, N = x.shape[1], dy.shape[1]
        assert (K, N) == {"attention_output": (H, H), "intermediate": (H, I), "ffn_output": (I, H)}[t]
        assert (kw.get("gelu_u") is not None) == (t == "ffn_output") and kw.get("dx") is not None
        if h is None:
            h = (x.float() @ A.float().t()).to(torch.bfloat16)              # (only the bound's magnitudes read it)
        dW = m._lw[i][GW[t]].detach().double().cpu()
        ref = DR.identity(dW, A.cpu(), B.cpu(), dy.cpu(), x.cpu(), h.cpu(), s)
        p = f"bert.encoder.layer.{i}.{PATH[t]}."
        ga, gb = named[p + "lora_A"].grad, named[p + "lora_B"].grad
        qa = DR.check(ga, ref["dA"], f"layer {i} {t} dA")
        qb = DR.check(gb, ref["dB"], f"layer {i} {t} dB")
        assert float(ga.abs().max()) > 0 and float(gb.abs().max()) > 0
        worst = max(worst, qa, qb)
    assert seen == {(i, t) for i in range(L) for t in DENSE}
    print("dense gradient identity, sparse top layer", sparse_top, "largest error / bound", worst)


# ---- 3. merged twin against the oracle --------------------------------------------------------------------------------------------------
def test_merged_twin_against_the_oracle():
    """M1 = adapters (A ~ N(0, 0.02), B ~ N(0, 0.05)) on all six projections of every layer, M2 = its merge_lora()d copy, O = the CPU oracle
    on M2's state dict: ||pooled(M1) - O|| <= 2 ||pooled(M2) - O||, the criterion of tests/test_lora_model_gpu.py."""
    from msa_amd.data import synthetic_batch, batch_to
    cb = synthetic_batch(2, 16, 40, 24, vocab=CFG["vocab"], seed=5)
    args = _args(batch_to(cb, DEV))
    m1 = build()
    m1.add_lora(r=8, alpha=16.0, targets="all-linear", seed=1)
    assert m1._lora["targets"] == ALL
    randomize(m1, b_std=0.05)
    m2 = copy.deepcopy(m1).merge_lora()
    assert not lora_names(m2) and set(m2.state_dict()) == set(build().state_dict())
    ref = TL._pooled_oracle(m2.state_dict(), cb)
    p1 = m1.predict(*args, return_pooled=True)[1]["pooled"].double().cpu()
    p2 = m2.predict(*args, return_pooled=True)[1]["pooled"].double().cpu()
    p0 = build().predict(*args, return_pooled=True)[1]["pooled"].double().cpu()
    e1, e2, e0 = float((p1 - ref).norm()), float((p2 - ref).norm()), float((p0 - ref).norm())
    print(f"merged twin, six targets: |M1 - O| {e1:.4e} |M2 - O| {e2:.4e} ratio {e1 / e2:.3f}; the base model without adapters {e0:.4e}")
    assert e2 > 0 and e1 <= 2.0 * e2, (e1, e2)
    assert e0 > 2.0 * e2, (e0, e2)                                          # the adapters matter at this scale: leaving them out breaks the bound


# ---- 4. the dropout seam at model level -------------------------------------------------------------------------------------------------
K_SEAM = 2.0
B_SEAM = 0.2          # B ~ N(0, 0.2): s B A is then about W's own size, so a delta under the wrong mask stands out of the bf16 roundings


def _seam_hidden(train, no_drop=False):
    """(largest, mean |difference|, largest |value|) of the top layer's hidden states, live adapters against the merged twin on the same batch
    and dropout seed; ``no_drop``: the adapter launches get NO_DROP in place of their dropout triple, through a spy."""
    from msa_amd import ops
    m1 = settings(build())
    m1.add_lora(r=8, alpha=16.0, targets=ADD2, seed=1)
    randomize(m1, b_std=B_SEAM)
    m2 = copy.deepcopy(m1).merge_lora()
    for m in (m1, m2):
        m.train(train)
        m.manual_seed(17)
    orig = ops.lora_dense_fwd
    if no_drop:
        ops.lora_dense_fwd = lambda *a, **k: orig(*a, **dict(k, drop=ops.NO_DROP))
    m1.debug_hidden, m2.debug_hidden = {}, {}
    try:
        with torch.no_grad():
            m1(**batch())
    finally:
        ops.lora_dense_fwd = orig
    with torch.no_grad():
        m2(**batch())
    h1, h2 = m1.debug_hidden["layers"][-1].float(), m2.debug_hidden["layers"][-1].float()
    return float((h1 - h2).abs().max()), float((h1 - h2).abs().mean()), float(h2.abs().max())


def test_the_dropout_seam_matches_the_merged_twin_in_train_mode():
    """Live adapters on the two dropout + residual seams against the merged twin, train mode (dropout 0.1), the same seed: the delta must
    carry the GEMM's own mask and scale, dropout(v + d) + R = (dropout(v) + R) + c d.  Observable: the mean |difference| of the top layer's
    hidden states (the logits of this small model hardly move under any adapter).  In eval mode the two differ by bf16 roundings only; in
    train mode the difference may be at most K_SEAM = 2 times that.  MEASURED on MI355X before K_SEAM was fixed: eval 5.61e-3, train 4.89e-3
    (0.87 x), and 2.72e-2 (4.85 x) with the adapter launches' triple replaced by NO_DROP -- an unmasked, unscaled delta -- which must break
    the bound; 2 sits a factor 2.3 from either.  (With B ~ N(0, 0.05) the wrong mask stayed within 1.6 x of the rounding floor: B_SEAM.)"""
    (_, d_eval, mag), (_, d_train, _), (_, d_wrong, _) = _seam_hidden(False), _seam_hidden(True), _seam_hidden(True, no_drop=True)
    print(f"dropout seam: live vs merged, mean |difference| of the top layer's hidden states: eval {d_eval:.4e} train {d_train:.4e} "
          f"train with NO_DROP on the adapter launches {d_wrong:.4e} (largest |hidden| {mag:.3f})")
    assert d_eval > 0
    assert d_train <= K_SEAM * d_eval, (d_train, d_eval)
    assert d_wrong > K_SEAM * d_eval, (d_wrong, d_eval)


# ---- 5. prediction paths ----------------------------------------------------------------------------------------------------------------
def _adapted(targets="all-linear", seed=1):
    m = build()
    m.add_lora(r=8, targets=targets, seed=seed)
    return randomize(m, b_std=0.05)


def test_predict_paths_apply_the_adapters():
    """predict (the [CLS]-row top layer: all three seams on the gathered rows), predict(return_attention="all") and predict_tokens (the full
    encoder) on live adapters against the merged twin, at the standards of tests/test_lora_model_gpu.py::test_predict_paths_apply_the_adapters:
    logits and relationship scores 2e-2 absolute, the MLM losses 3e-3 relative; and the adapters matter: the adapter-free base differs by more."""
    m = _adapted()
    mm = copy.deepcopy(m).merge_lora()
    base = build()
    for x in (m, mm, base):
        x.eval()
    b = batch()
    args = _args(b)
    d = lambda x, y: float((x.detach().float() - y.detach().float()).abs().max())
    lg, ex = m.predict(*args, return_pooled=True)
    lgm, exm = mm.predict(*args, return_pooled=True)
    lgb = base.predict(*args)
    lgb = lgb[0] if isinstance(lgb, tuple) else lgb
    la, ea = m.predict(*args, return_attention="all")
    lam, eam = mm.predict(*args, return_attention="all")
    print("predict live vs merged", d(lg, lgm), "attention call", d(la, lam), "live vs base", d(lg, lgb))
    assert d(lg, lgm) < 2e-2 and d(la, lam) < 2e-2
    for k in ("t_rel", "v_rel", "s_rel"):
        assert d(ex[k], exm[k]) < 2e-2, k
    assert d(lg, lgb) > d(lg, lgm)
    batt = base.predict(*args, return_attention="all")[1]["attention"]
    for name, att in ea["attention"].items():
        assert bool((att.float().sum(-1) - 1.0).abs().max() < 1e-5), name
        assert float((att.float() - eam["attention"][name].float()).abs().max()) < 2e-2, name
    assert any(not torch.equal(att, batt[name]) for name, att in ea["attention"].items())
    tok = m.predict_tokens(*args, masked_labels=b["masked_labels"])
    tokm = mm.predict_tokens(*args, masked_labels=b["masked_labels"])
    tokb = base.predict_tokens(*args, masked_labels=b["masked_labels"])
    got, want, off = (float(t["loss"].double().mean()) for t in (tok, tokm, tokb))
    print("predict_tokens mean MLM loss: live", got, "merged", want, "base", off)
    assert abs(got - want) <= 3e-3 * max(1.0, abs(want)), (got, want)
    # a model with dense adapters only on the top layer: the gathered-row path alone carries them
    top = build()
    top.add_lora(r=8, targets=DENSE, layers=[L - 1], seed=2)
    randomize(top, b_std=0.05)
    topm = copy.deepcopy(top).merge_lora()
    top.eval(); topm.eval()
    lt, ltm = top.predict(*args), topm.predict(*args)
    lt, ltm = (v[0] if isinstance(v, tuple) else v for v in (lt, ltm))
    assert d(lt, ltm) < 2e-2 and d(lt, lgb) > d(lt, ltm)


# ---- 6. launches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers,first", [(None, 0), ([2, 3], 2)])
def test_launches_per_adapted_layer_and_the_frozen_base_plan(layers, first):
    m = settings(build())
    m.add_lora(r=8, targets="all-linear", layers=layers, seed=1)
    randomize(m)
    plan = m.trainable_plan()
    assert plan.first_layer == first and plan.stop == first and not plan.embedding_stage
    assert all(v == "none" for i in plan.layers for v in plan.layers[i].values())
    with DenseSpy() as spy:
        fb(m)
    n = L - first
    # one forward and one backward launch group per dense target and adapted layer (the three passes share one token matrix)
    assert len(spy.calls["lora_dense_fwd"]) == 3 * n and len(spy.calls["lora_dense_bwd"]) == 3 * n
    assert len(spy.calls["lora_qkv_fwd"]) == n and len(spy.calls["lora_qkv_bwd"]) == n
    modes = [k.get("mode", 0) for a, k in spy.calls["lora_dense_fwd"]]
    assert modes == [0, 1, 0] * n                                          # attention_output (ADD), intermediate (GELU), ffn_output (ADD)
    drops = [k.get("drop") for a, k in spy.calls["lora_dense_fwd"] if k.get("mode", 0) == 0]
    assert all(dr is not None and dr[1] > 0 for dr in drops) and len({dr[0] for dr in drops}) == 2 * n      # the GEMMs' own triples, one stream per site
    order = [_target_of(m._lw[i], a[3]) for i in reversed(range(first, L)) for a, k in spy.calls["lora_dense_bwd"] if _target_of(m._lw[i], a[3])]
    assert order == ["ffn_output", "intermediate", "attention_output"] * n  # the order the data fixes
    dense = {m._lw[i]["g_" + k].data_ptr() for i in range(L) for k in ("Wqkv", "Wo", "W1", "W2")}
    assert not (set(TF._tn_targets(spy)) & dense), "a weight-gradient tile ran for the frozen encoder"
    assert len(spy.calls["attn_bwd"]) == n                                  # backward ends at the lowest adapted layer
    bound = m._lw[first]["WqkvT"].data_ptr()
    assert not any(a[1].data_ptr() == bound for a, k in spy.calls["gemm_nt"]), "the layer where backward ends computed an input gradient"
    # forward of an adapted layer: the FFN-up GEMM runs without its GELU epilogue and without aux (the adapter launch applies both)
    for i in range(L):
        up = [k for a, k in spy.calls["gemm_nt"] if a[1].data_ptr() == m._lw[i]["W1"].data_ptr()]
        assert len(up) == 1 and bool(up[0].get("gelu")) == (i < first), i
    named = dict(m.named_parameters())
    for nme in lora_names(m):
        assert named[nme].grad is not None and float(named[nme].grad.abs().max()) > 0, nme
    assert named["bert.encoder.layer.3.output.dense.weight"].grad is None


def test_qkv_only_and_adapter_free_models_make_no_dense_adapter_call():
    from msa_amd import ops
    for targets in (None, ("query", "value")):
        m = settings(build())
        if targets:
            m.add_lora(r=8, targets=targets, seed=1)
            randomize(m)
        with DenseSpy() as spy:
            assert not ops.launches_unwrapped()                            # the dense adapter launches are among the watched wrappers
            fb(m)
        assert not spy.calls["lora_dense_fwd"] and not spy.calls["lora_dense_bwd"]
        assert all(lw["lora_dense"] is None for lw in m._lw)
        assert len(spy.calls["lora_qkv_fwd"]) == (L if targets else 0)
    # the flat layout without dense adapters is the one it was; with them the names sit behind the layer's Q / K / V adapters
    plain = build()
    plain._ensure_ready(next(plain.parameters()).device)
    a = build()
    a.add_lora(r=8, targets="all-linear", freeze_base=False)
    a._ensure_ready(next(a.parameters()).device)
    fa, f = a._flat, plain._flat
    assert [n for n in fa.order if ".lora_" not in n] == f.order
    p = "bert.encoder.layer.3."
    assert fa.order.index(p + "attention.output.dense.lora_A") == fa.order.index(p + "attention.self.value.lora_B") + 1
    assert all(fa.offset[n] % 8 == 0 for n in fa.order if ".lora_" in n)
    # a layer with dense adapters only leaves the composite path, the others stay on it
    c = settings(build())
    c.add_lora(r=8, targets=("ffn_output",), layers=[1], freeze_base=False, seed=1)
    calls = {"layer_fwd": 0}
    ol = ops.layer_fwd
    ops.layer_fwd = lambda *x, _o=ol: (calls.__setitem__("layer_fwd", calls["layer_fwd"] + 1), _o(*x))[1]
    try:
        assert ops.launches_unwrapped()
        fb(c)
    finally:
        ops.layer_fwd = ol
    assert calls["layer_fwd"] == L - 1


# ---- 7. optimizer and training ----------------------------------------------------------------------------------------------------------
def test_optimizer_moves_the_adapters_only():
    """AdamW under clipping and the EMA: the adapters move; the frozen masters, their bf16 copies and the transposed copies keep their bits."""
    from msa_amd.optim import AdamW
    m = settings(build())
    m.add_lora(r=8, targets=DENSE, seed=1)
    randomize(m)
    opt = AdamW(list(m.parameters()), lr=1e-3, weight_decay=0.01)
    opt.ema(0.99)
    m._ensure_ready(next(m.parameters()).device)
    fz = {n for n in TF.frozen_names(m) if n.startswith(("bert.embeddings.", "bert.jointEmbeddings.", "bert.encoder."))}
    assert fz and not any(".lora_" in n for n in fz)
    before, beforeT = TF._snap(m, fz)
    ad0 = {n: p.detach().clone() for n, p in m.named_parameters() if ".lora_" in n}
    assert len(ad0) == 2 * 3 * L
    fb(m)
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
    """Only the dense adapters train; the objective is the alignment + label loss, as in tests/test_lora_model_gpu.py."""
    from msa_amd.optim import AdamW
    m = settings(build(dropout=0.0))
    m.set_alpha_beta(0.0, 0.0)
    m.add_lora(r=8, targets=DENSE, seed=1)
    for n, p in m.named_parameters():
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
    print("label loss over 30 dense-adapter-only steps:", losses[0], "->", losses[-1], losses[::5])
    assert losses[-1] < losses[0]


# ---- 8. lifecycle -----------------------------------------------------------------------------------------------------------------------
def test_lifecycle_states_equal_fresh_twins():
    """add -> save -> remove -> load -> merge on ONE model; after each step predict() is torch.equal to a model built fresh in that state."""
    args = _args()
    pred = lambda x: (lambda v: v[0] if isinstance(v, tuple) else v)(x.predict(*args))
    base = pred(build())
    m = _adapted(targets=("value",) + DENSE)
    sd, full = m.lora_state_dict(), m.state_dict()
    assert sd["targets"] == ("value",) + DENSE and sorted(k for k in sd if k not in ("r", "alpha", "targets", "layers")) == sorted(lora_names(m))
    live = pred(m)
    assert not torch.equal(live, base)
    fresh = build()
    fresh.load_lora_state_dict(sd)                                          # a fresh model from the adapter file
    assert torch.equal(pred(fresh), live)
    twin2 = build()
    twin2.add_lora(r=8, targets=("value",) + DENSE)
    twin2.load_state_dict(full)                                             # ... and from the whole state dict
    assert torch.equal(pred(twin2), live)
    m.remove_lora()
    assert not lora_names(m) and torch.equal(pred(m), base)                # removed: the base model's bits
    m.load_lora_state_dict(sd)
    assert torch.equal(pred(m), live)                                      # loaded again: the live bits
    other = build()
    other.add_lora(r=8, targets=DENSE)
    with pytest.raises(ValueError, match="differ"):
        other.load_lora_state_dict(sd)
    ref_keys = set(build().state_dict())
    merged_sd = copy.deepcopy(m).merge_lora().state_dict()
    m.merge_lora()
    assert set(m.state_dict()) == ref_keys and m._lora is None
    fresh_merged = build()
    fresh_merged.load_state_dict(merged_sd)
    assert torch.equal(pred(m), pred(fresh_merged))                         # merged: a fresh model with the merged state dict
    m.add_lora(r=4, targets=("intermediate",))                              # ... and a new set may follow a merge
    m.remove_lora()
    assert set(m.state_dict()) == ref_keys


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from msa_amd import parallel
    from msa_amd.data import to_fused
    m = build()
    for kw in (dict(targets=("output",)), dict(targets=("attention_output", "attention_output")), dict(targets=("ffn",)),
               dict(targets=DENSE, r=32), dict(targets=DENSE, layers=[L])):
        with pytest.raises(ValueError):
            m.add_lora(**kw)
        assert not lora_names(m) and m._lora is None, kw
    m.add_lora(r=8, targets=DENSE)
    with pytest.raises(ValueError, match="already has adapters"):
        m.add_lora(r=8, targets=DENSE)
    with pytest.raises(NotImplementedError, match="adapters"):
        m.forward_fused(**to_fused(batch()))
    with pytest.raises(NotImplementedError, match="adapters"):
        parallel.DataParallel(m)
    alone = copy.deepcopy(m.bert)
    b = batch()
    with pytest.raises(NotImplementedError, match="stand-alone"):
        alone(b["input_ids"][0], attention_mask=b["attention_mask"][0], token_type_ids=b["token_type_ids"][0])
