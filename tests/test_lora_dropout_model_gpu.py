"""The adapters' input dropout in the model (model.add_lora(dropout=...) / set_lora_dropout), on the config and batch of
tests/test_lora_model_gpu.py: hidden 128, 4 layers, 2 heads, synthetic_batch(2, 16, 40, 24), deterministic mode, single-layer
weight-gradient launches.

Yardsticks: a twin with dropout 0 after the same manual_seed (B = 0: the low-rank branch adds nothing, so every bit outside the adapters'
own gradients is the twin's); every adapter launch of a real step against tests/lora_dropout_ref.py with the mask rebuilt by
tests/rng_ref.py from (the step's seed, the site) -- never from the triple the launch got; steps run separately; the launch list."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lora_dropout_ref as XR
from tests import lora_ref as LR
import tests.test_freeze_gpu as TF
import tests.test_lora_model_gpu as TL

DEV = "cuda"
CFG, L = TF.CFG, TF.L
build, batch, settings = TF.build, TF.batch, TF.settings
_deterministic = TF._deterministic                  # (the autouse fixture of that module, here as well)
ALL = ("query", "key", "value", "attention_output", "intermediate", "ffn_output")
OPS = ("lora_qkv_fwd", "lora_qkv_bwd", "lora_dense_fwd", "lora_dense_bwd")
P = 0.3


def adapted(dropout, targets=ALL, b_std=None, freeze_base=False, bd=0.1):
    m = settings(build(dropout=bd))
    m.add_lora(r=8, alpha=16.0, targets=targets, freeze_base=freeze_base, seed=1, dropout=dropout)
    if b_std is not None:
        TL.randomize(m, b_std=b_std)
    return m


def step(m, b=None):
    out, logits = m(**(b if b is not None else batch()))
    out[0].mean().backward()
    torch.cuda.synchronize()
    return dict(losses=[out[i].detach().clone() for i in (0, 4, 5, 6)], logits=logits.detach().clone(),
                grads={n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()})


def same_result(a, b, names=None, what=""):
    for x, y in zip(a["losses"], b["losses"]):
        assert torch.equal(x, y), (what, float(x), float(y))
    assert torch.equal(a["logits"], b["logits"]), what
    for n in (a["grads"] if names is None else names):
        g, w = a["grads"][n], b["grads"][n]
        assert (g is None) == (w is None) and (g is None or torch.equal(g, w)), (what, n)


def label_only(b):
    return dict(b, masked_labels=None)


# ---- 1. fresh adapters: only the adapters' own gradients see the mask ------------------------------------------------------------
def test_zero_b_twin_over_two_steps():
    m, tw = adapted(P), adapted(0.0)
    assert m.lora_dropout == P and tw.lora_dropout == 0.0
    ad = [n for n in TL.lora_names(m)]
    assert len(ad) == 2 * 6 * L
    others = [n for n, _ in m.named_parameters() if ".lora_" not in n]
    differs = 0
    for k in range(2):
        a, b = step(m), step(tw)
        same_result(a, b, others, f"step {k}")
        for n in ad:
            g, w = a["grads"][n], b["grads"][n]
            assert g is not None and w is not None, n
            if n.endswith("lora_A"):
                assert not bool(g.any()), n                            # dA = s g^T (Kp . x) with g = c dy B = 0
            else:
                assert float(g.abs().max()) > 0.0, n
                differs += int(not torch.equal(g, w))                  # dB = s dy^T h, h = c (Kp . x) A^T
        m.zero_grad(); tw.zero_grad()
    assert differs == 2 * 6 * L, differs


# ---- 2. every launch of a real step against the reference, the mask from (seed, site) -------------------------------------------
class Spy:
    """Wraps the four ops.lora_* wrappers: operands as the call found them, what it left, its keywords."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        from msa_amd import ops
        self.ops, self.orig = ops, {k: getattr(ops, k) for k in OPS}
        for k in OPS:
            setattr(ops, k, self._wrap(k, self.orig[k]))
        return self

    def __exit__(self, *exc):
        for k, f in self.orig.items():
            setattr(self.ops, k, f)

    def _wrap(self, name, fn):
        def snap(v):
            if torch.is_tensor(v):
                return v.detach().clone()
            if isinstance(v, dict):
                return {k: snap(x) for k, x in v.items()}
            return v

        def f(*a, **kw):
            pre = ([snap(v) for v in a], {k: snap(v) for k, v in kw.items()})
            ret = fn(*a, **kw)
            self.calls.append(dict(op=name, a=a, kw=kw, pre=pre, post=([snap(v) for v in a], {k: snap(v) for k, v in kw.items()}), ret=snap(ret)))
            return ret
        return f


def _site(m, c):
    """(layer, seam, target or None) of a spied call, from the address of its A operand."""
    A = c["a"][2] if c["op"].endswith("_fwd") else c["a"][3]         # (x, y, A, B, ...) forward, (dy, x, h, A, B, ...) backward
    for i in range(L):
        lw = m._lw[i]
        if c["op"].startswith("lora_qkv"):
            if lw["lora"] is not None and all(A[t].data_ptr() == lw["lora"]["A"][t].data_ptr() for t in A):
                return i, "qkv", None
        elif lw.get("lora_dense") is not None:
            for t, v in lw["lora_dense"]["A"].items():
                if v.data_ptr() == A.data_ptr():
                    return i, t, t
    raise AssertionError("an adapter launch on no layer's adapter")


def _cpu(v):
    if torch.is_tensor(v):
        return v.cpu()
    if isinstance(v, dict):
        return {k: _cpu(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_cpu(x) for x in v]
    return v


def check_calls(m, calls, seed, p, expect_rows):
    """Every spied launch against lora_dropout_ref under the mask of (seed, 8 * layer + offset); returns the ops seen and how many
    backward launches got a row list."""
    seen, with_rows, worst = set(), 0, 0.0
    for c in calls:
        i, seam, _ = _site(m, c)
        want = XR.in_drop(p, seed, 8 * i + XR.SITES[seam])
        got = c["kw"].get("in_drop")
        assert got is not None and (got[0], got[1]) == (want[0], want[1]) and abs(got[2] - want[2]) < 1e-12, (c["op"], i, seam, got, want)
        a, kw, pa, pk = c["a"], c["kw"], _cpu(c["pre"][0]), _cpu(c["pre"][1])
        qa, qk = _cpu(c["post"][0]), _cpu(c["post"][1])
        seen.add(c["op"])
        q = []
        if c["op"] == "lora_qkv_fwd":
            x, qkv0, A, B, targets, s = pa[:6]
            ref = XR.qkv_fwd(x, qkv0, A, B, targets, s, want)
            q.append(XR.check(qa[1], ref["qkv"], "qkv"))
            if qk.get("h_out") is not None:
                q.append(XR.check(qk["h_out"], ref["h"], "h"))
        elif c["op"] == "lora_qkv_bwd":
            dqkv, x, h, A, B, gA0, gB0, targets, s = pa[:9]
            names = LR._names(targets)
            z = lambda g, shape: {t: (g[t] if (g is not None and t in g) else torch.zeros(shape)) for t in names}
            r, H = A[names[0]].shape
            ref = XR.qkv_bwd(dqkv, x, h, A, B, targets, s, want, dres=pk.get("dres"), gA0=z(gA0, (r, H)), gB0=z(gB0, (H, r)), accumulate=pk.get("accumulate", True))
            for key, g in (("dA", qa[5]), ("dB", qa[6])):
                for t in (g or {}):
                    q.append(XR.check(g[t], ref[key][t], f"{key}[{t}]"))
            if pk.get("dres") is not None:
                q.append(XR.check(_cpu(c["ret"]), ref["dres"], "dres"))
        elif c["op"] == "lora_dense_fwd":
            x, y0, A, B, s = pa[:5]
            mode = pk.get("mode", XR.ADD)
            ref = XR.dense_fwd(x, y0, A, B, s, mode, drop=pk.get("drop"), in_drop=want)
            q.append(XR.check(qa[1], ref["y"], "y"))
            if qk.get("aux") is not None:
                q.append(XR.check(qk["aux"], ref["aux"], "aux"))
            if qk.get("h_out") is not None:
                q.append(XR.check(qk["h_out"], ref["h"], "h"))
        else:
            dy, x, h, A, B, gA0, gB0, s = pa[:8]
            rows = pk.get("rows")
            with_rows += int(rows is not None)
            ref = XR.dense_bwd(dy, x, h, A, B, s, in_drop=want, rows=None if rows is None else rows.tolist(), dx=pk.get("dx"), gelu_u=pk.get("gelu_u"),
                               gA0=gA0, gB0=gB0, accumulate=pk.get("accumulate", True))
            if qa[5] is not None:
                q.append(XR.check(qa[5], ref["dA"], "dA"))
            if qa[6] is not None:
                q.append(XR.check(qa[6], ref["dB"], "dB"))
            if pk.get("dx") is not None:
                q.append(XR.check(qk["dx"], ref["dx"], "dx"))
                assert bool(ref["dx"].exact.any())                 # the mask dropped something and those elements kept their bits
        worst = max([worst] + q)
    print(f"{len(calls)} adapter launches, {with_rows} with a row list, largest error / bound {worst:.3f}")
    if expect_rows:
        assert with_rows > 0, "no backward launch ran on gathered rows"
    return seen


@pytest.mark.parametrize("form", ["standard", "label-only", "frozen-prefix"])
def test_every_launch_against_the_reference_in_situ(form):
    m = adapted(P, b_std=0.05)
    if form == "frozen-prefix":
        m.freeze(layers=2)
    b = label_only(batch()) if form == "label-only" else batch()
    m._ensure_ready(next(m.parameters()).device)
    with Spy() as spy:
        step(m, b)
    seed = m._seed * 1000003 + m._calls
    assert m._calls == 1
    seen = check_calls(m, spy.calls, seed, P, expect_rows=form != "frozen-prefix")
    assert seen == set(OPS)
    n_fwd = sum(c["op"] in ("lora_qkv_fwd", "lora_dense_fwd") for c in spy.calls)
    n_bwd = len(spy.calls) - n_fwd
    assert n_fwd == 4 * L and n_bwd == 4 * L, (n_fwd, n_bwd)
    if form == "frozen-prefix":
        # the embeddings still train, so backward passes through the frozen layers: their adapters' launches run for the masked input
        # gradient alone -- no gradient of a frozen adapter is asked for
        low = [c for c in spy.calls if c["op"].endswith("_bwd") and _site(m, c)[0] < 2]
        assert len(low) == 8
        for c in low:
            gA, gB = c["a"][5], c["a"][6]
            assert not gA and not gB, c["op"]
            assert (c["kw"].get("dres") if c["op"] == "lora_qkv_bwd" else c["kw"].get("dx")) is not None


# ---- 3. the triples travel in the saved record ------------------------------------------------------------------------------------
def test_two_forwards_then_their_backwards_in_reverse_order():
    b1, b2 = batch(5), batch(6)
    ref = []
    for k, b in enumerate((b1, b2)):                       # each step alone, from the seed state the joint run has at that forward
        m = adapted(P, b_std=0.05)
        m._calls = k
        ref.append(step(m, b)["grads"])
    m = adapted(P, b_std=0.05)
    o1, _ = m(**b1)
    o2, _ = m(**b2)
    named = dict(m.named_parameters())
    ad = TL.lora_names(m)
    o2[0].mean().backward()
    torch.cuda.synchronize()
    g2 = {n: named[n].grad.detach().clone() for n in ad}
    m.zero_grad()
    o1[0].mean().backward()
    torch.cuda.synchronize()
    g1 = {n: named[n].grad.detach().clone() for n in ad}
    for n in ad:
        assert torch.equal(g1[n], ref[0][n]), (n, "first forward's backward")
        assert torch.equal(g2[n], ref[1][n]), (n, "second forward's backward")
    assert any(not torch.equal(g1[n], g2[n]) for n in ad)


# ---- 4. eval and predict never drop ---------------------------------------------------------------------------------------------------
def test_eval_and_predict_are_untouched():
    m, tw = adapted(P, b_std=0.05), adapted(0.0, b_std=0.05)
    b = batch()
    args = (b["input_ids"], b["token_type_ids"], b["attention_mask"])
    first = lambda v: v[0] if isinstance(v, tuple) else v

    def passes(x):
        with Spy() as spy:
            x.eval()
            with torch.no_grad():
                out, logits = x(**b)
            res = [out[0].detach().clone(), logits.detach().clone(), first(x.predict(*args)).clone()]
            res += [t.clone() for t in tensors(x.predict(*args, return_attention="all"))]
            res += [t.clone() for t in tensors(x.predict_tokens(*args, masked_labels=b["masked_labels"]))]
            x.train()
        return res, [(c["op"], sorted(c["kw"])) for c in spy.calls]

    def tensors(v):
        if torch.is_tensor(v):
            return [v]
        if isinstance(v, dict):
            return [t for k in sorted(v) for t in tensors(v[k])]
        if isinstance(v, (tuple, list)):
            return [t for x in v for t in tensors(x)]
        return []

    ra, la = passes(m)
    rb, lb = passes(tw)
    assert la == lb and la and not any("in_drop" in kw or "rows" in kw for _, kw in la)
    assert len(ra) == len(rb) and all(torch.equal(x, y) for x, y in zip(ra, rb))
    # an evaluation pass between two train steps leaves the second step's bits unchanged
    m1, m2 = adapted(P, b_std=0.05), adapted(P, b_std=0.05)
    step(m1); step(m2)
    m1.zero_grad(); m2.zero_grad()
    m1.eval()
    with torch.no_grad():
        m1(**b)
    m1.predict(*args)
    m1.train()
    same_result(step(m1), step(m2), what="second step after an evaluation pass")
    # train mode under no_grad drops, as the other sites do
    m3 = adapted(P, b_std=0.05)
    with Spy() as spy, torch.no_grad():
        m3(**b)
    assert spy.calls and all(c["kw"].get("in_drop") is not None for c in spy.calls)


# ---- 5. set_lora_dropout(0) ---------------------------------------------------------------------------------------------------------------
def test_dropout_switched_off_equals_a_model_that_never_dropped():
    m = adapted(P, b_std=0.05)
    step(m); m.zero_grad()
    step(m); m.zero_grad()
    flat = m._flat
    m.set_lora_dropout(0.0)
    tw = adapted(0.0, b_std=0.05)
    tw.load_state_dict(m.state_dict())
    tw.parameters_changed()
    tw._calls = m._calls                                     # the same seed state
    with Spy() as spy:
        a = step(m)
    assert m._flat is flat                                   # no rebuild of the flat storage
    assert spy.calls and not any("in_drop" in c["kw"] or "rows" in c["kw"] for c in spy.calls)      # exactly today's calls
    same_result(a, step(tw), what="after set_lora_dropout(0)")


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------------
def test_deterministic_and_default_mode_give_the_same_adapter_gradients():
    from msa_amd import ops
    ad = None
    res = []
    for det in (True, False, False):
        ops.set_deterministic(det)
        m = adapted(P, b_std=0.05, freeze_base=True)
        ad = TL.lora_names(m)
        res.append(step(m))
    ops.set_deterministic(True)
    same_result(res[1], res[2], ad, "two runs from one seed")
    for n in ad:
        assert torch.equal(res[0]["grads"][n], res[1]["grads"][n]), n


# ---- 7. / 8. training -------------------------------------------------------------------------------------------------------------------
def test_thirty_adapter_steps_lower_the_label_loss():
    """tests/test_lora_model_gpu.py's test of the same name with dropout = 0.1 on the adapters' input (the base model's own dropout off,
    alpha = beta = 0: the objective is the alignment + label loss; only the adapters train)."""
    from msa_amd.optim import AdamW
    m = settings(build(dropout=0.0))
    m.set_alpha_beta(0.0, 0.0)
    m.add_lora(r=8, targets=TL.TARGETS, seed=1, dropout=0.1)
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
    print("label loss over 30 adapter-only steps at dropout 0.1:", losses[0], "->", losses[-1], losses[::5])
    assert losses[-1] < losses[0]


def test_optimizer_with_clipping_and_ema_moves_the_adapters_only():
    from msa_amd.optim import AdamW
    m = settings(build())
    m.add_lora(r=8, targets=ALL, seed=1, dropout=P)
    TL.randomize(m)
    opt = AdamW(list(m.parameters()), lr=1e-3, weight_decay=0.01)
    opt.ema(0.99)
    m._ensure_ready(next(m.parameters()).device)
    fz = {n for n in TF.frozen_names(m) if n.startswith(("bert.embeddings.", "bert.jointEmbeddings.", "bert.encoder."))}
    assert fz and not any(".lora_" in n for n in fz)
    before, beforeT = TF._snap(m, fz)
    ad0 = {n: p.detach().clone() for n, p in m.named_parameters() if ".lora_" in n}
    TF.fb(m)
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
