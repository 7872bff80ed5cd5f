"""The label-only step of ``MMBertForPretraining.forward`` (``masked_labels=None``): no MLM head, the heads' [CLS]-row gradient handed
to the encoder's backward in compact form with an empty labelled-row list.

Bounds: against the CPU oracle the ones of tests/test_model_gpu.py (``check_against_oracle`` / ``compare_gradients``: losses 3e-3
relative, gradients 4.5 % or 3x the bf16-storage calibrator); against the standard step at ``alpha = 0`` on the same inputs
``same_grads`` -- the bound ``test_sparse_backward_of_the_top_layer_equals_dense`` uses for two row sets of one gradient (the standard
step's top layer also visits its labelled rows, whose gradient is exactly zero at ``alpha = 0``); eval-mode outputs and everything
stated as "keeps its bits" bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from msa_amd.data import synthetic_batch, batch_to
from msa_amd.model import _MLM_ONLY
from tests.test_model_gpu import build, oracle_run, compare_gradients, same_grads, rel, DEV
from tests import session_twin as TW
from tests import step_stages as SS

CFG = dict(hidden=128, layers=2, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)
SHAPE = (3, 12, 40, 30)                               # B, T, visual, speech: unequal pair lengths


def one_label_per_pass(batch):
    """The batch with MLM labels on ONE token per pass (sample 0, position 1; never a [CLS] row): the oracle's per-pass cross-entropy stays
    finite, and at alpha = 0 it adds nothing to the loss or to any gradient."""
    labs = []
    for l in batch["masked_labels"]:
        l = torch.full_like(l, -100)
        l[0, 1] = 7
        labs.append(l)
    return dict(batch, masked_labels=tuple(labs))


def cpu_batch(seed=3, num_labels=None, shape=SHAPE):
    return one_label_per_pass(synthetic_batch(*shape, dataset="mosei", vocab=CFG["vocab"], seed=seed, num_labels=num_labels))


def label_only(batch):
    return dict(batch, masked_labels=None)


def no_dropout(m):
    m.config.hidden_dropout_prob = 0.0
    m.config.attention_probs_dropout_prob = 0.0
    m.bert.jointEmbeddings.dropout_prob = 0.0
    return m


def grads_of(m):
    return {n: (None if q.grad is None else q.grad.detach().float().clone()) for n, q in m.named_parameters()}


class _Reached:
    """The model's parameters for compare_gradients without the ones a label-only backward leaves at ``.grad is None``."""

    def __init__(self, m):
        self.m = m

    def named_parameters(self):
        return [(n, q) for n, q in self.m.named_parameters() if n not in _MLM_ONLY]


def assert_mlm_only_none(m):
    named = dict(m.named_parameters())
    for n in _MLM_ONLY:
        assert named[n].grad is None, n
    word = named["bert.embeddings.word_embeddings.weight"]
    assert word.grad is not None or not word.requires_grad       # (still reached, through the embeddings)


def test_eval_outputs_equal_the_standard_eval_forward():
    b = batch_to(cpu_batch(), DEV)
    m = build(CFG, train=False)
    with torch.no_grad():
        so, sl = m(**b)
        lo, ll = m(**label_only(b))
    for k in (4, 5, 6, 8, 10, 12):
        assert torch.equal(so[k], lo[k]), k
    assert torch.equal(sl, ll)
    for k in (1, 2, 3, 7, 9, 11):
        assert lo[k] is None, k
    want = lo[4].double() + lo[5].double() - CFG["beta"] * lo[6].double()
    assert abs(float(lo[0]) - float(want)) <= 1e-6 * abs(float(want))
    # eval mode WITH autograd, and train mode without: the same route
    # (with a backward to save for, the forward leaves out the rows nothing reads instead of sharing one: other tiles, fp32 sums in another order)
    lo2, _ = m(**label_only(b))
    assert abs(float(lo2[0]) - float(lo[0])) <= 1e-5 * abs(float(lo[0])) and lo2[0].requires_grad
    m.train()
    with torch.no_grad():
        lo3, _ = m(**label_only(b))
    assert torch.isfinite(lo3[0]) and not lo3[0].requires_grad


def test_train_mode_without_dropout_matches_the_oracle_at_alpha_zero():
    cb = cpu_batch()
    cfg0 = dict(CFG, alpha=0.0)
    p, oout, ologits = oracle_run(cfg0, cb)
    pe, eout, _ = oracle_run(cfg0, cb, emulate_bf16=True)
    m = no_dropout(build(CFG, train=True))
    out, logits = m(**label_only(batch_to(cb, DEV)))
    for i, name in ((0, "joint"), (4, "ap"), (5, "label"), (6, "nce")):
        tol = max(3e-3, 3.0 * rel(eout[i].detach(), oout[i].detach()))
        print(name, float(out[i].detach()), float(oout[i].detach()), tol)
        assert rel(out[i].detach(), oout[i].detach()) < tol, name
    assert float((logits.detach().float().cpu() - ologits.detach()).abs().max()) < 2e-2
    out[0].mean().backward()
    torch.cuda.synchronize()
    assert_mlm_only_none(m)
    compare_gradients(_Reached(m), p, pe)
    assert TW.leftovers(m) == []


def _configure(m, case):
    if case == "freeze":
        m.freeze(embeddings=True, layers=1)
    elif case == "lora_qv":
        m.add_lora(r=4, targets=("query", "value"), seed=5)
    elif case == "lora_all":
        m.add_lora(r=4, targets="all-linear", seed=5)
    return m


def _build_case(case, train=True):
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    if case in ("class3", "multi6"):
        C = 3 if case == "class3" else 6
        ref = build(CFG, train=train)
        c = ref.config
        m = MMBertForPretraining(c, num_labels=C, multi_label=(case == "multi6"))
        m.bert.set_joint_embeddings(CFG["dataset"])
        m.set_alpha_beta(0.0, CFG["beta"])
        sd = {k: v for k, v in ref.state_dict().items() if not k.startswith("classifier1_2.")}
        torch.manual_seed(11)
        m.load_state_dict(sd, strict=False)
        m = m.to(DEV)
        m.train(train)
        return m
    m = build(dict(CFG, alpha=0.0), train=train)
    return _configure(m, case)


def _case_batch(case):
    if case == "class3":
        return batch_to(cpu_batch(num_labels=3), DEV)
    b = cpu_batch()
    if case == "multi6":
        g = torch.Generator().manual_seed(4)
        t = (torch.rand((SHAPE[0], 6), generator=g) > 0.5).float()
        t[0, 2] = -1.0
        b = dict(b, sentiment=t)
    return batch_to(b, DEV)


@pytest.mark.parametrize("case", ["plain", "class3", "multi6", "freeze", "lora_qv", "lora_all"])
def test_label_only_equals_the_standard_step_at_alpha_zero(case):
    b = _case_batch(case)
    res = {}
    for lo in (False, True):
        torch.manual_seed(11)
        m = no_dropout(_build_case(case))
        out, _ = m(**(label_only(b) if lo else b))
        out[0].mean().backward()
        torch.cuda.synchronize()
        if lo:
            assert_mlm_only_none(m)
        res[lo] = (out, grads_of(m))
    for k in (0, 4, 5, 6):
        a, s = float(res[True][0][k].detach()), float(res[False][0][k].detach())
        print(case, k, a, s)
        assert abs(a - s) <= 1e-6 * abs(s) + 1e-7, (k, a, s)
    moved = 0
    for n, g in res[True][1].items():
        s = res[False][1][n]
        if n in _MLM_ONLY:
            assert g is None and (s is None or float(s.abs().max()) == 0.0), n       # (alpha = 0: the standard step's are exact zeros)
            continue
        assert (g is None) == (s is None), n
        if g is None or "attention.self.key.bias" in n:
            continue
        same_grads(g, s, n)
        moved += int(float(g.abs().max()) > 0)
    assert moved > 10


def _optimizer(m, route):
    from msa_amd.optim import AdamW
    if route == "grouped":
        named = list(m.named_parameters())
        head = [q for n, q in named if not n.startswith("bert.")]
        body = [q for n, q in named if n.startswith("bert.")]
        return AdamW([dict(params=body, lr=1e-3, weight_decay=0.01), dict(params=head, lr=2e-3, weight_decay=0.0)], lr=1e-3)
    opt = AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    if route == "ema":
        opt.ema(0.9)
    return opt


@pytest.mark.parametrize("route", ["plain", "devscale", "grouped", "ema"])
def test_optimizer_leaves_the_unreached_parameters_alone(route):
    b = batch_to(cpu_batch(), DEV)
    m = no_dropout(build(CFG, train=True))
    opt = _optimizer(m, route)
    named = dict(m.named_parameters())

    def step(batch):
        out, _ = m(**batch)
        out[0].mean().backward()
        if route == "devscale":
            opt.clip_grad_norm_(0.5)
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()

    step(b)                                            # a standard step first: m, v of every parameter are non-zero
    f = m._flat

    def state():
        sd = opt.state_dict()
        keep = {k: v.detach().clone() for k, v in sd.items() if torch.is_tensor(v) and v.numel() == f.total}
        keep.update(params=f.params.clone(), half=f.half.clone(), halfT=f.halfT.clone())
        return keep

    def span(t, n):
        return t[f.offset[n]:f.offset[n] + f.numel[n]]

    s0 = state()
    assert any(k for k in s0 if k not in ("params", "half", "halfT")), "the optimizer's flat m / v are in its state dict"
    step(label_only(b))
    s1 = state()
    for n in _MLM_ONLY:
        for k in s0:
            if k == "halfT":
                continue
            assert torch.equal(span(s0[k], n), span(s1[k], n)), (n, k)
    o, rows, ld = f.t_off["transform"]
    assert torch.equal(s0["halfT"][o:o + rows * ld], s1["halfT"][o:o + rows * ld])
    for n, q in named.items():
        if n in _MLM_ONLY or any(n.startswith(x) for x in ("bert.jointEmbeddings.W_c", "cls.seq_relationship.")):
            continue
        assert not torch.equal(span(s0["params"], n), span(s1["params"], n)), n
    step(b)                                            # a standard step afterwards updates them again
    s2 = state()
    for n in _MLM_ONLY:
        assert not torch.equal(span(s1["params"], n), span(s2["params"], n)), n


def _three_steps(seed, batches):
    m = build(CFG, train=True)
    m.deterministic = True
    m.manual_seed(seed)
    res = []
    for b in batches:
        out, _ = m(**label_only(b))
        out[0].mean().backward()
        torch.cuda.synchronize()
        res.append((out[0].detach().clone(), grads_of(m)))
        m._flat.grads.zero_()
    m.deterministic = False
    return res


def test_train_mode_with_dropout_is_deterministic_and_seeded():
    batches = [batch_to(cpu_batch(seed=20 + i), DEV) for i in range(3)]
    from msa_amd import ops
    try:
        a, b2, c = _three_steps(5, batches), _three_steps(5, batches), _three_steps(6, batches)
    finally:
        ops.set_deterministic(False)
    for (la, ga), (lb, gb) in zip(a, b2):
        assert torch.equal(la, lb)
        for n in ga:
            assert (ga[n] is None and gb[n] is None) or torch.equal(ga[n], gb[n]), n
    assert not torch.equal(a[0][0], c[0][0])


def test_long_lived_model_equals_fresh_twins():
    """[standard, label-only, predict, label-only, standard] on one model against a fresh twin built from its state_dict at each point."""
    from msa_amd.optim import AdamW
    bs = [batch_to(cpu_batch(seed=40 + i), DEV) for i in range(5)]
    kinds = ["standard", "label_only", "predict", "label_only", "standard"]
    m = build(CFG, train=True)
    m.deterministic = True
    m.manual_seed(9)
    opt = AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)

    def run(model, kind, b):
        if kind == "predict":
            return dict(pred=model.predict(b["input_ids"], b["token_type_ids"], b["attention_mask"]).detach().clone())
        out, logits = model(**(label_only(b) if kind == "label_only" else b))
        out[0].mean().backward()
        torch.cuda.synchronize()
        r = dict(loss=out[0].detach().clone(), logits=logits.detach().clone())
        r.update({"g." + n: g for n, g in grads_of(model).items() if g is not None})
        r["none"] = sorted(n for n, g in grads_of(model).items() if g is None)
        return r

    try:
        for kind, b in zip(kinds, bs):
            sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
            seed = (m._seed, m._calls)
            t = build(CFG, train=True)
            t.load_state_dict(sd)
            t._seed, t._calls = seed
            got, want = run(m, kind, b), run(t, kind, b)
            assert got.keys() == want.keys(), kind
            for k in got:
                assert (got[k] == want[k]) if k == "none" else torch.equal(got[k], want[k]), (kind, k)
            if kind != "predict":
                opt.step()
                opt.zero_grad()
            assert TW.leftovers(m) == [], kind
            del t
    finally:
        m.deterministic = False


def test_the_launch_list_of_a_label_only_step_holds_no_mlm_head():
    b = batch_to(cpu_batch(), DEV)
    m = build(CFG, train=True)
    out, _ = m(**b)
    out[0].mean().backward()
    m._flat.grads.zero_()
    vpad = m._flat.vpad
    lists = {}
    for lo in (False, True):
        with SS.record(m) as calls:
            out, _ = m(**(label_only(b) if lo else b))
            out[0].mean().backward()
        lists[lo] = calls
        m._flat.grads.zero_()
    wide = lambda c: any(vpad in r.shape for r in SS._recs(list(c.a.values())))
    ops_std = [c.op for c in lists[False]]
    assert "ce_fwd" in ops_std and "ce_bwd" in ops_std and any(wide(c) and c.op.startswith("gemm") for c in lists[False])
    for c in lists[True]:
        assert c.op not in ("ce_fwd", "ce_bwd", "gelu_bwd", "active_rows"), c.op
        assert not (wide(c) and c.op.startswith("gemm")), c.op
    mlm_w = {m._w[k].data_ptr() for k in ("Wt", "WtT", "word_h", "wordT", "mlm_ln_g")}
    for c in lists[True]:
        for r in SS._recs(list(c.a.values())):
            assert r.ptr not in mlm_w or c.op in ("embed_gather", "embed_scatter"), c.op
    assert len(lists[True]) < len(lists[False])


def test_a_backward_that_raises_leaves_nothing_pending():
    from msa_amd import ops
    b = batch_to(cpu_batch(), DEV)
    ref = no_dropout(build(CFG, train=True))
    out, _ = ref(**label_only(b))
    out[0].mean().backward()
    torch.cuda.synchronize()
    want = grads_of(ref)
    m = no_dropout(build(CFG, train=True))
    out, _ = m(**label_only(b))
    orig = ops.attn_bwd

    def boom(*a, **k):
        raise RuntimeError("injected")

    ops.attn_bwd = boom
    try:
        with pytest.raises(RuntimeError, match="injected"):
            out[0].mean().backward()
    finally:
        ops.attn_bwd = orig
    m._flat.join_side_writers()
    torch.cuda.synchronize()
    m._flat.grads.zero_()
    out, _ = m(**label_only(b))
    out[0].mean().backward()
    torch.cuda.synchronize()
    assert TW.leftovers(m) == []
    got = grads_of(m)
    for n, g in want.items():
        assert (g is None) == (got[n] is None), n
        if g is not None and "attention.self.key.bias" not in n:
            same_grads(got[n], g, n)                 # (two runs of one step: fp32 atomics in arrival order)


def test_unsupported_options_raise():
    b = batch_to(cpu_batch(), DEV)
    m = build(CFG, train=True)
    with pytest.raises(NotImplementedError, match="forward_fused"):
        m.forward_fused(b["input_ids"][:3], b["token_type_ids"][0], b["attention_mask"][0], None, b["ap_label"], b["sentiment"])
    m.fused_heads = False
    with pytest.raises(NotImplementedError, match="fused_heads"):
        m(**label_only(b))
    m.fused_heads = True
    m.grad_hook = lambda i: None
    with pytest.raises(NotImplementedError, match="DataParallel"):
        m(**label_only(b))


def test_two_label_only_backwards_accumulate_and_the_async_prologue_gives_the_same_step():
    b1, b2 = batch_to(cpu_batch(seed=61), DEV), batch_to(cpu_batch(seed=62), DEV)
    single = []
    for b in (b1, b2):
        m = no_dropout(build(CFG, train=True))
        out, _ = m(**label_only(b))
        out[0].mean().backward()
        torch.cuda.synchronize()
        single.append((float(out[0]), grads_of(m)))
    m = no_dropout(build(CFG, train=True))
    for b in (b1, b2):
        out, _ = m(**label_only(b))
        out[0].mean().backward()
    torch.cuda.synchronize()
    assert_mlm_only_none(m)
    for n, g in grads_of(m).items():
        if g is None or "attention.self.key.bias" in n:
            continue
        same_grads(g, single[0][1][n] + single[1][1][n], n)
    # the prologue on the input stream (the caller states its inputs are complete): the same step
    m = no_dropout(build(CFG, train=True))
    m.async_prologue = True
    torch.cuda.synchronize()
    out, _ = m(**label_only(b1))
    out[0].mean().backward()
    torch.cuda.synchronize()
    assert abs(float(out[0]) - single[0][0]) <= 1e-6 * abs(single[0][0])
    for n, g in grads_of(m).items():
        if g is None or "attention.self.key.bias" in n:
            continue
        same_grads(g, single[0][1][n], n)
    assert TW.leftovers(m) == []
