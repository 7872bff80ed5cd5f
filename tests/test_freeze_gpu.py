"""GPU tests of frozen parameters (``requires_grad == False``): model.freeze / unfreeze, the shorter backward, bias-only gradients, the
optimizer.

THE YARDSTICK IS A TWIN, not a tolerance: an unfrozen model with the same state dict, dropout seed and batch computes the gradients of the
trainable names with code this feature does not alter.  With ``pair_wgrads = False`` and ``defer_wgrads = False`` on both, every running
layer's weight-gradient launch holds the same problems over the same rows, so losses, logits and each trainable ``p.grad`` are
``torch.equal`` (train mode, dropout 0.1, deterministic mode).  At the default settings the pairing of layers shifts; the yardstick per
parameter is then the difference between the twin's own two forms (default and single-layer), times 4, and exact where that is zero.
OBSERVED on MI355X at this shape: see ``test_twin_default_settings``' docstring.

Two kinds of gradient cannot be bit-equal to the twin's, because another kernel sums them (ops.colsum_grouped instead of a rider on a
weight-gradient launch that no longer runs): the biases of frozen weights (``layer_weights=True``) and -- whenever the word-embedding table
is frozen, sets a, b, c, f, h -- ``cls.predictions.bias``, whose gradient rode on the tied decoder's weight-gradient launch.  Both are held to
the float64 column sum of the very matrix the kernel read, within ``M * 2^-24 * sum|x| + 2^-23 * |ref|`` (any fp32 summation order of M terms
plus the output rounding), and to the twin within twice that (``test_bias_only_gradients``).  Because of them an unfrozen twin's
trajectory leaves the frozen model's after the first optimizer step; the optimizer tests therefore hold ``AdamW`` exactly against a twin
frozen the same way, and use the unfrozen twin for the first step only."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmbert_oracle as O
from msa_amd.data import synthetic_batch, batch_to, to_fused

DEV = "cuda"
CFG = dict(hidden=128, layers=4, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)
L = CFG["layers"]
PRED_BIAS = "cls.predictions.bias"
WORD = "bert.embeddings.word_embeddings.weight"
W1 = "bert.encoder.layer.1.intermediate.dense."
NEVER = ("bert.jointEmbeddings.W_cv.", "bert.jointEmbeddings.W_cs.", "cls.seq_relationship.")
_CACHE = {}


def build(cfg=CFG, dropout=0.1):
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    c = MMBertConfig(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                     intermediate_size=cfg["intermediate"], hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout)
    m = MMBertForPretraining(c)
    m.bert.set_joint_embeddings(cfg["dataset"])
    key = ("sd", cfg["hidden"])
    if key not in _CACHE:
        _CACHE[key] = O.seeded_params(cfg)                                # (computed once; load_state_dict copies out of it)
    m.load_state_dict(_CACHE[key], strict=False)
    m = m.to(DEV)
    m.train()
    m.manual_seed(17)
    return m


def batch(seed=5, cfg=CFG):
    key = ("batch", seed, cfg["hidden"])
    if key not in _CACHE:
        _CACHE[key] = batch_to(synthetic_batch(2, 16, 40, 24, vocab=cfg["vocab"], seed=seed), DEV)
    return _CACHE[key]


def _set(names):
    def f(m):
        named = dict(m.named_parameters())
        for n in names:
            named[n].requires_grad_(False)
    return f


def _freeze_unfreeze(m):
    m.freeze(embeddings=True, layers=2)
    m.unfreeze()


SETS = {
    "a": lambda m: m.freeze(embeddings=True, layers=2),
    "b": lambda m: m.freeze(embeddings=True, layers=3),
    "c": lambda m: m.freeze(embeddings=True, layers=4),
    "d": lambda m: m.freeze(layers=2),
    "e": lambda m: m.freeze(layer_weights=True),
    "f": lambda m: m.freeze(embeddings=True, layers=2, layer_weights=True),
    "g": _set([W1 + "weight", W1 + "bias"]),
    "h": _set([WORD]),
    "i": _freeze_unfreeze,
}
FIRST = {"a": 2, "b": 3, "c": 4}


@pytest.fixture(autouse=True)
def _deterministic():
    from msa_amd import ops
    was = ops.deterministic()
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(was)


def settings(m, single=True, shortcuts=True):
    if single:
        m.pair_wgrads = False
        m.defer_wgrads = False
    if not shortcuts:
        m.sparse_top_layer_backward = False
        m.skip_padded_backward = False
    return m


def fb(m, b=None):
    out, logits = m(**(b if b is not None else batch()))
    out[0].mean().backward()
    torch.cuda.synchronize()
    return out, logits


def result(m, out, logits):
    return dict(losses=[out[i].detach().clone() for i in (0, 4, 5, 6)], logits=logits.detach().clone(),
                grads={n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()},
                flat=m._flat.grads.clone(), offset=dict(m._flat.offset))


def twin(single=True, shortcuts=True):
    """The unfrozen twin's result, computed once per form and never changed."""
    key = ("twin", single, shortcuts)
    if key not in _CACHE:
        m = settings(build(), single, shortcuts)
        _CACHE[key] = result(m, *fb(m))
    return _CACHE[key]


def frozen_names(m):
    return {n for n, p in m.named_parameters() if not p.requires_grad}


def colsum_fed(m):
    """The names whose gradient the grouped column sum produces (not bit-equal to the twin's by construction)."""
    plan = m.trainable_plan()
    if plan is None:
        return set()
    from msa_amd import freeze as F
    names = set()
    for i, modes in plan.layers.items():
        for key, mode in modes.items():
            if mode == "bias":
                names.update(f"bert.encoder.layer.{i}." + b for b in F.PROBLEMS[key][1])
    if not plan.word_table and PRED_BIAS not in plan.frozen:
        names.add(PRED_BIAS)
    return names


def check_against_twin(m, res, tw, yard=None, what=""):
    """Losses and logits bit-equal; every frozen parameter without a gradient; every trainable, differentiated one bit-equal to the twin's
    (``yard``: name -> allowed absolute difference instead); the column-sum-fed ones are test_bias_only_gradients' business."""
    for x, y in zip(res["losses"], tw["losses"]):
        assert torch.equal(x, y), (what, float(x), float(y))
    assert torch.equal(res["logits"], tw["logits"]), what
    frozen, loose, checked = frozen_names(m), colsum_fed(m), 0
    for n, g in res["grads"].items():
        if n in frozen:
            assert g is None, (what, n, "a frozen parameter has a gradient")
            continue
        assert g is not None, (what, n, "a trainable parameter has no gradient")
        if n in loose or n.startswith(NEVER):
            continue
        w = tw["grads"][n]
        d = float((g.double() - w.double()).abs().max())
        tol = 0.0 if yard is None else yard[n]
        if tol == 0.0:
            assert torch.equal(g, w), (what, n, d, float(w.double().abs().max()))
        else:
            assert d <= tol, (what, n, d, tol)
        checked += 1
    assert checked
    return checked


# ---- 1. twin equality ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETS))
def test_twin_single_layer_launches(name):
    m = settings(build())
    SETS[name](m)
    res = result(m, *fb(m))
    check_against_twin(m, res, twin(), what=name)
    if name == "i":
        assert m.trainable_plan() is None and torch.equal(res["flat"], twin()["flat"])


def test_twin_without_the_short_cuts():
    m = settings(build(), shortcuts=False)
    SETS["a"](m)
    check_against_twin(m, result(m, *fb(m)), twin(shortcuts=False), what="a, dense top layer, no padded-row skipping")


@pytest.mark.parametrize("name", ["a", "d", "e"])
def test_twin_default_settings(name):
    """At the default settings the layers pair up differently once a prefix is frozen.  The yardstick per parameter is the largest absolute
    difference between the unfrozen twin's own default and single-layer forms; the frozen model (default settings) may differ from the
    single-layer twin by 4 x that, and must match exactly where it is zero.  OBSERVED on MI355X at this shape (177 rows in backward: no launch splits
    its token axis, every weight-gradient tile sums its rows in one order): the twin's two forms are bit-identical for every parameter, so
    the yardstick is zero everywhere and this test is exact."""
    t_def, t_one = twin(single=False), twin()
    yard = {n: 4.0 * float((g.double() - t_one["grads"][n].double()).abs().max()) for n, g in t_def["grads"].items() if g is not None}
    print(name, "yardstick: largest", max(yard.values()), "non-zero for", sum(1 for v in yard.values() if v > 0), "of", len(yard))
    m = settings(build(), single=False)
    SETS[name](m)
    check_against_twin(m, result(m, *fb(m)), t_one, yard=yard, what=name + " (default settings)")


# ---- 2. bias-only gradients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["e", "f", "a", "b", "c", "h"])
def test_bias_only_gradients(name):
    from msa_amd import ops
    m = settings(build())
    SETS[name](m)
    rec, orig = [], ops.colsum_grouped

    def spy(problems, **kw):
        assert kw.get("accumulate", True) is True and kw.get("alpha", 1.0) == 1.0 and kw.get("alpha_dev") is None
        rec.extend((x.detach().clone(), out.data_ptr(), out.numel()) for x, out in problems)
        return orig(problems, **kw)
    ops.colsum_grouped = spy
    try:
        res = result(m, *fb(m))
    finally:
        ops.colsum_grouped = orig
    flat, tw = m._flat, twin()
    want = colsum_fed(m)
    seen = set()
    assert rec
    for x, ptr, n in rec:
        o = (ptr - flat.grads.data_ptr()) // 4
        got, ref_t = res["flat"][o:o + n].double(), tw["flat"][o:o + n].double()
        x64 = x.double()
        ref = x64.sum(0)
        bound = x.shape[0] * 2.0 ** -24 * x64.abs().sum(0) + 2.0 ** -23 * ref.abs()
        e64, et = (got - ref).abs(), (got - ref_t).abs()
        print(name, flat.name_at(o), "rows", x.shape[0], "err vs float64", float(e64.max()), "vs twin", float(et.max()), "bound", float(bound.max()))
        assert bool((e64 <= bound).all()), (name, flat.name_at(o), float((e64 - bound).max()))
        assert bool((et <= 2 * bound).all()), (name, flat.name_at(o), float((et - 2 * bound).max()))
        assert float(ref.abs().max()) > 0.0
        seen.update(k for k in want if o <= flat.offset[k] < o + n)
    assert seen == want, (sorted(want - seen), "no column sum produced these")


# ---- 3. elision is real -------------------------------------------------------------------------------------------------------------------
class Spy:
    """Records the calls of the per-launch wrappers (which also takes the model off the composite path, as the other spying tests do)."""
    NAMES = ("gemm_nt", "attn_bwd", "ln_bwd", "pair_proj_bwd", "embed_scatter", "gemm_tn_grouped", "gemm_tn", "colsum_grouped")

    def __enter__(self):
        from msa_amd import ops
        self.ops, self.calls, self.orig = ops, {n: [] for n in self.NAMES}, {n: getattr(ops, n) for n in self.NAMES}
        for n in self.NAMES:
            setattr(ops, n, (lambda *a, _n=n, **k: (self.calls[_n].append((a, k)), self.orig[_n](*a, **k))[1]))
        return self

    def __exit__(self, *exc):
        for n in self.NAMES:
            setattr(self.ops, n, self.orig[n])


def _tn_targets(spy):
    t = [p[2].data_ptr() for a, k in spy.calls["gemm_tn_grouped"] for p in a[0]]
    return t + [a[2].data_ptr() for a, k in spy.calls["gemm_tn"]]


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_backward_stops_at_the_lowest_trainable_layer(name):
    m = settings(build())
    SETS[name](m)
    b = FIRST[name]
    with Spy() as spy:
        res = result(m, *fb(m))
    check_against_twin(m, res, twin(), what=name)
    plan = m.trainable_plan()
    assert plan.first_layer == b and plan.stop == b and not plan.embedding_stage
    assert len(spy.calls["attn_bwd"]) == L - b, (len(spy.calls["attn_bwd"]), L - b)
    w = m._w
    if b < L:
        bound = m._lw[b]["WqkvT"].data_ptr()
        assert not any(a[1].data_ptr() == bound for a, k in spy.calls["gemm_nt"]), "the boundary layer computed an input gradient"
    for i in range(L):
        used = [a for a, k in spy.calls["gemm_nt"] if a[1].data_ptr() == m._lw[i]["WqkvT"].data_ptr()]
        assert len(used) == (1 if i > b else 0), (i, len(used))
    assert not spy.calls["pair_proj_bwd"] and not spy.calls["embed_scatter"]
    emb_gammas = {w["emb_ln_g"].data_ptr(), w["joint_ln_g"].data_ptr()}
    assert not any(a[4].data_ptr() in emb_gammas for a, k in spy.calls["ln_bwd"])
    assert len(spy.calls["ln_bwd"]) == 2 * (L - b) + 1                      # two per running layer + the MLM transform's
    frozen_w = {m._lw[i]["g_" + k].data_ptr() for i in range(b) for k in ("Wqkv", "Wo", "W1", "W2")} | {w["g_word_pad"].data_ptr()}
    targets = _tn_targets(spy)
    assert targets and not (set(targets) & frozen_w)
    for i in range(L):                                                       # forward keeps nothing below the boundary
        up = [k for a, k in spy.calls["gemm_nt"] if a[1].data_ptr() == m._lw[i]["W1"].data_ptr()]
        assert len(up) == 1 and (up[0].get("aux") is None) == (i < b), (i, up[0].get("aux") is None)
    for i in range(b):                                                       # the frozen prefix's gradient region stays zero
        for n, o in m._flat.offset.items():
            if n.startswith(f"bert.encoder.layer.{i}."):
                assert float(res["flat"][o:o + m._flat.numel[n]].abs().sum()) == 0.0, n


def test_frozen_word_table_and_single_problem():
    m = settings(build())
    SETS["h"](m)
    with Spy() as spy:
        res = result(m, *fb(m))
    check_against_twin(m, res, twin(), what="h")
    assert m._w["g_word_pad"].data_ptr() not in set(_tn_targets(spy))
    assert len(spy.calls["embed_scatter"]) == 1 and spy.calls["embed_scatter"][0][0][4] is None       # no word rows
    assert len(spy.calls["pair_proj_bwd"]) == 2
    m = settings(build())
    SETS["g"](m)
    with Spy() as spy:
        res = result(m, *fb(m))
    check_against_twin(m, res, twin(), what="g")
    assert m._lw[1]["g_W1"].data_ptr() not in set(_tn_targets(spy)) and m._lw[0]["g_W1"].data_ptr() in set(_tn_targets(spy))
    assert not spy.calls["colsum_grouped"]


def test_bias_only_layers_launch_no_weight_gradient_tile():
    m = settings(build())
    SETS["e"](m)
    with Spy() as spy:
        fb(m)
    dense = {m._lw[i]["g_" + k].data_ptr() for i in range(L) for k in ("Wqkv", "Wo", "W1", "W2")}
    assert not (set(_tn_targets(spy)) & dense)
    assert len(spy.calls["colsum_grouped"]) == L and all(len(a[0]) == 4 for a, k in spy.calls["colsum_grouped"])     # one launch per layer


@pytest.mark.parametrize("name", ["a", "e"])
def test_composite_path_is_bit_identical(name):
    from msa_amd import ops
    res = {}
    for comp in (True, False):
        m = settings(build())
        SETS[name](m)
        m.composite_layers = comp
        calls, ob = [], ops.layer_bwd
        ops.layer_bwd = lambda *a, _o=ob: (calls.append(1), _o(*a))[1]
        try:
            res[comp] = result(m, *fb(m))
        finally:
            ops.layer_bwd = ob
        running = L - m.trainable_plan().stop                               # (less one when the top layer takes the row-sparse path)
        assert len(calls) in ((running - 1, running) if comp else (0,)), (comp, len(calls))
    for x, y in zip(res[True]["losses"], res[False]["losses"]):
        assert torch.equal(x, y)
    assert torch.equal(res[True]["logits"], res[False]["logits"]) and torch.equal(res[True]["flat"], res[False]["flat"])


# ---- 4. the optimizer leaves frozen weights alone -------------------------------------------------------------------------------------------
LR, WD = 1e-3, 0.01


def _snap(m, names):
    f = m._flat
    out = {n: (f.params[f.offset[n]:f.offset[n] + f.numel[n]].clone(), f.half[f.offset[n]:f.offset[n] + f.numel[n]].clone()) for n in names}
    return out, f.halfT.clone()


def _frozen_transposes_equal(m, before, after):
    """The transposed copies of the GEMM weights that are frozen."""
    f, fz, n = m._flat, frozen_names(m), 0
    for i in range(L):
        p = f"bert.encoder.layer.{i}."
        for key, ws in (("qkv", [p + f"attention.self.{x}.weight" for x in ("query", "key", "value")]), ("o", [p + "attention.output.dense.weight"]),
                        ("w1", [p + "intermediate.dense.weight"]), ("w2", [p + "output.dense.weight"])):
            if all(w in fz for w in ws):
                o, rows, ld = f.t_off[p + key]
                assert torch.equal(before[o:o + rows * ld], after[o:o + rows * ld]), (p + key)
                n += 1
    if WORD in fz:
        o, rows, ld = f.t_off["word"]
        assert torch.equal(before[o:o + rows * ld], after[o:o + rows * ld])
        n += 1
    assert n


@pytest.mark.parametrize("name", ["a", "e"])
@pytest.mark.parametrize("variant", ["plain", "clip", "ema"])
def test_optimizer_leaves_frozen_parameters_alone(name, variant):
    """Two steps of ``AdamW(list(m.parameters()), lr=1e-3, weight_decay=0.01)`` -- frozen parameters listed, weight decay on -- against
    ``AdamW(trainable parameters only)``, the existing "not owned" path, on a twin frozen THE SAME WAY: both models then compute
    bit-identical gradients, so the optimizer's property is held exactly -- every parameter, the whole of m and v, the clipping norm and
    the EMA ``torch.equal`` after both steps in all three variants.  Frozen: fp32 master, bf16 copy and transposed copy keep their bits.
    The UNFROZEN twin (optimizer over the same trainable parameters) is compared after the first step, where it is exact: every
    trainable parameter but those fed by the grouped column sum, whose gradient differs from that twin's in its last bits (module
    docstring) -- from there on its trajectory is another one, and under clipping those bits reach every parameter through the norm."""
    from msa_amd.optim import AdamW
    m, t, u = settings(build()), settings(build()), settings(build())
    SETS[name](m)
    SETS[name](t)
    fz = frozen_names(m)
    named_m, named_t, named_u = dict(m.named_parameters()), dict(t.named_parameters()), dict(u.named_parameters())
    om = AdamW(list(m.parameters()), lr=LR, weight_decay=WD)
    ot = AdamW([p for n, p in named_t.items() if n not in fz], lr=LR, weight_decay=WD)
    ou = AdamW([p for n, p in named_u.items() if n not in fz], lr=LR, weight_decay=WD)
    if variant == "ema":
        for o in (om, ot, ou):
            o.ema(0.99)
    m._ensure_ready(next(m.parameters()).device)
    before, beforeT = _snap(m, fz)
    loose = colsum_fed(m)
    for step in (1, 2):
        pairs = ((m, om), (t, ot)) + (((u, ou),) if step == 1 else ())
        for mod, opt in pairs:
            fb(mod, batch(seed=5 + step))
        if variant == "clip":
            norms = [opt.clip_grad_norm_(1.0) for _, opt in pairs]
            print(name, "step", step, "norms", [float(x) for x in norms])
            assert torch.equal(norms[0], norms[1]), (float(norms[0]), float(norms[1]))
        for _, opt in pairs:
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        after, afterT = _snap(m, fz)
        for n in fz:
            assert torch.equal(after[n][0], before[n][0]) and torch.equal(after[n][1], before[n][1]), (name, variant, step, n, "a frozen parameter moved")
            assert named_m[n].grad is None
        _frozen_transposes_equal(m, beforeT, afterT)
        for n, p in named_m.items():
            assert torch.equal(p.detach(), named_t[n].detach()), (name, variant, step, n, float((p.detach() - named_t[n].detach()).abs().max()))
            if step == 1 and variant != "clip" and n not in fz and n not in loose and not n.startswith(NEVER):
                assert torch.equal(p.detach(), named_u[n].detach()), (name, variant, n, "against the unfrozen twin")
        assert torch.equal(m._flat.half, t._flat.half) and torch.equal(m._flat.halfT, t._flat.halfT)
        assert torch.equal(om._m, ot._m) and torch.equal(om._v, ot._v) and om._steps == ot._steps == step
        if variant == "ema":
            assert torch.equal(om._ema, ot._ema)
    assert float(om._m.abs().sum()) > 0.0
    if variant == "ema":
        esd, sd = om.ema_state_dict(), m.state_dict()
        for n in fz:
            assert torch.equal(esd[n], sd[n]), n
        om.swap_ema()
        om.swap_ema()
        for n, v in m.state_dict().items():
            assert torch.equal(v, sd[n]), n


def test_today_s_failure_frozen_weights_move_without_the_feature():
    """What the parent commit does (this test fails there): ``requires_grad_(False)`` + ``AdamW(model.parameters(), weight_decay > 0)``
    updated the "frozen" weights.  One step; the frozen table must keep its bits and have no gradient."""
    from msa_amd.optim import AdamW
    m = settings(build())
    for n, p in m.named_parameters():                                        # (plain torch: set a without model.freeze)
        if n.startswith(("bert.embeddings.", "bert.jointEmbeddings.", "bert.encoder.layer.0.", "bert.encoder.layer.1.")):
            p.requires_grad_(False)
    opt = AdamW(list(m.parameters()), lr=LR, weight_decay=WD)
    m._ensure_ready(next(m.parameters()).device)
    w0 = dict(m.named_parameters())[WORD].detach().clone()
    fb(m)
    opt.step()
    torch.cuda.synchronize()
    p = dict(m.named_parameters())[WORD]
    assert p.grad is None and torch.equal(p.detach(), w0)


# ---- 5. changing the set ------------------------------------------------------------------------------------------------------------------
def test_freezing_more_after_a_step_and_unfreezing_raises():
    """Freeze layer 2 as well after one step: the optimizer (every parameter listed) rebuilds its maps, keeps layer 2's m and v and the
    one step count, and the next step equals -- every parameter, m and v bit for bit -- that of a twin frozen the same way whose SECOND
    optimizer is built anew over the then trainable parameters and loaded with the first one's state.  Then: a parameter that becomes
    trainable again after steps were taken makes step() raise; a fresh optimizer works."""
    from msa_amd.optim import AdamW
    m, t = settings(build()), settings(build())
    for mod in (m, t):
        mod.freeze(embeddings=True, layers=2)
    fz1 = frozen_names(m)
    named_m, named_t = dict(m.named_parameters()), dict(t.named_parameters())
    om = AdamW(list(m.parameters()), lr=LR, weight_decay=WD)
    ot = AdamW([p for n, p in named_t.items() if n not in fz1], lr=LR, weight_decay=WD)
    for mod, opt in ((m, om), (t, ot)):
        fb(mod, batch(6))
        opt.step()
        opt.zero_grad()
    for mod in (m, t):
        mod.freeze(layers=[2])
    fz2 = frozen_names(m)
    l2 = fz2 - fz1
    assert l2 and all(n.startswith("bert.encoder.layer.2.") for n in l2)
    f = m._flat
    span = lambda buf, n: buf[f.offset[n]:f.offset[n] + f.numel[n]]
    keep = {n: (named_m[n].detach().clone(), span(om._m, n).clone(), span(om._v, n).clone()) for n in l2}
    assert any(float(k[1].abs().sum()) > 0.0 for k in keep.values())        # (layer 2 was stepped: its moments are not the zeros they began as)
    ot2 = AdamW([p for n, p in named_t.items() if n not in fz2], lr=LR, weight_decay=WD)
    ot2.load_state_dict(ot.state_dict())
    for mod, opt in ((m, om), (t, ot2)):
        fb(mod, batch(7))
        opt.step()
        opt.zero_grad()
    torch.cuda.synchronize()
    for n, p in named_m.items():
        assert torch.equal(p.detach(), named_t[n].detach()), (n, float((p.detach() - named_t[n].detach()).abs().max()))
    for n in l2:
        assert named_m[n].grad is None and torch.equal(named_m[n].detach(), keep[n][0]), n
        assert torch.equal(span(om._m, n), keep[n][1]) and torch.equal(span(om._v, n), keep[n][2]), (n, "m / v of a newly frozen parameter changed")
    assert torch.equal(om._m, ot2._m) and torch.equal(om._v, ot2._v) and om._steps == ot2._steps == 2
    top = "bert.encoder.layer.3.output.dense.weight"
    assert not torch.equal(named_m[top].detach(), _CACHE[("sd", CFG["hidden"])][top].to(DEV))
    # unfreezing a parameter this optimizer has stepped past: refused, with the reason; a fresh optimizer works
    for n, p in m.named_parameters():
        if n.startswith("bert.encoder.layer.0."):
            p.requires_grad_(True)
    fb(m, batch(8))
    with pytest.raises(NotImplementedError, match="step count.*bias correction.*new optimizer"):
        om.step()
    fresh = AdamW(list(m.parameters()), lr=LR, weight_decay=WD)
    w = dict(m.named_parameters())["bert.encoder.layer.0.output.dense.weight"]
    w0 = w.detach().clone()
    fresh.step()
    torch.cuda.synchronize()
    assert not torch.equal(w.detach(), w0)


def test_unfreezing_before_the_first_step_is_fine():
    from msa_amd.optim import AdamW
    m = settings(build())
    m.freeze(embeddings=True, layers=2)
    opt = AdamW(list(m.parameters()), lr=LR, weight_decay=WD)
    m.unfreeze()
    res = result(m, *fb(m))
    assert torch.equal(res["flat"], twin()["flat"])
    w = dict(m.named_parameters())["bert.encoder.layer.0.output.dense.weight"]
    w0 = w.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(w.detach(), w0)


def test_backward_follows_the_set_its_forward_saw():
    m = settings(build())
    m.freeze(embeddings=True, layers=2)
    out, logits = m(**batch())
    m.unfreeze()                                                             # between forward and backward: this backward does not see it
    out[0].mean().backward()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    assert named["bert.encoder.layer.0.output.dense.weight"].grad is None and named[WORD].grad is None
    tw = twin()
    for n in ("bert.encoder.layer.2.output.dense.weight", "bert.encoder.layer.3.attention.self.query.weight", "bert.pooler.dense.weight"):
        assert torch.equal(named[n].grad, tw["grads"][n]), n
    # and the other way round: frozen after the forward, the backward still computes what its forward kept
    m = settings(build())
    out, logits = m(**batch())
    m.freeze(embeddings=True, layers=2)
    out[0].mean().backward()
    torch.cuda.synchronize()
    assert torch.equal(m._flat.grads, tw["flat"])


# ---- 6. packed neighbours -----------------------------------------------------------------------------------------------------------------
def test_packed_neighbours_are_refused():
    q = "bert.encoder.layer.0.attention.self.query.bias"
    m = settings(build())
    _set([q])(m)
    with pytest.raises(NotImplementedError) as e:
        m(**batch())
    assert q in str(e.value) and "bert.encoder.layer.0.attention.self.key.bias" in str(e.value)
    m.unfreeze()
    ln = "bert.encoder.layer.1.attention.output.LayerNorm.weight"
    _set([ln])(m)
    with pytest.raises(NotImplementedError) as e:
        m(**batch())
    assert ln in str(e.value) and ln[:-6] + "bias" in str(e.value)
    cfg = dict(CFG, hidden=256, heads=4, layers=2, intermediate=1024)
    m = build(cfg)
    _set([q])(m)
    fb(m, batch(cfg=cfg))
    named = dict(m.named_parameters())
    assert named[q].grad is None and named[q.replace("query", "key")].grad is not None


# ---- 7. hook order ------------------------------------------------------------------------------------------------------------------------
def test_hooks_fire_for_every_layer_in_order():
    m = settings(build(), single=False)
    m.freeze(embeddings=True, layers=2)
    m._ensure_ready(next(m.parameters()).device)
    flat = m._flat
    bounds = [0]
    for i in reversed(range(L)):                                             # the slices parallel.DataParallel builds
        last = f"bert.encoder.layer.{i}.attention.self.value.bias"
        bounds.append(flat.offset[last] + flat.numel[last])
    snaps, order, heads = {}, [], []

    def hook(i):
        k = L - 1 - i
        order.append(i)
        snaps[i] = (bounds[k], bounds[k + 1], flat.grads[bounds[k]:bounds[k + 1]].clone())
    m.grad_hook = hook
    m.head_grad_hook = lambda: heads.append(len(order))
    fb(m)
    assert order == [3, 2, 1, 0] and heads == [0]
    for i, (lo, hi, snap) in snaps.items():
        assert torch.equal(snap, flat.grads[lo:hi]), i
        if i >= 2:
            assert float(snap.abs().sum()) > 0.0, i
        else:
            assert float(snap.abs().sum()) == 0.0, i


# ---- 8. unaffected paths and refusals -----------------------------------------------------------------------------------------------------
def test_unaffected_paths_and_refusals():
    from msa_amd.model import MMBertModel
    m, t = settings(build()), settings(build())
    m.freeze(embeddings=True, layers=2)
    b = batch()
    args3 = (b["input_ids"], b["token_type_ids"], b["attention_mask"])
    m.eval()
    t.eval()
    with torch.no_grad():
        om, lm = m(**b)
        ot, lt = t(**b)
    assert torch.equal(lm, lt) and all(torch.equal(om[i], ot[i]) for i in (0, 4, 5, 6, 7, 9, 11))
    assert torch.equal(m.predict(*args3), t.predict(*args3))
    pm, pt = m.predict_tokens(*args3, masked_labels=b["masked_labels"]), t.predict_tokens(*args3, masked_labels=b["masked_labels"])
    assert torch.equal(pm["loss"], pt["loss"])
    for k in ("text", "visual", "speech"):
        assert sorted(pm[k]) == sorted(pt[k]) and all(torch.equal(pm[k][q], pt[k][q]) for q in pm[k]), k
    assert all(torch.equal(v, t.state_dict()[k]) for k, v in m.state_dict().items())
    m.train()
    with pytest.raises(NotImplementedError, match="frozen"):
        m.forward_fused(**to_fused(b))
    with pytest.raises(NotImplementedError, match="frozen"):
        m.bert(input_ids=b["input_ids"][0], attention_mask=b["attention_mask"][0])
    n = settings(build())                                                    # only parameters that are never differentiated carry the flag:
    for k, p in n.named_parameters():                                        # nothing is refused, and nothing changed when a call is refused
        if k.startswith(NEVER):
            p.requires_grad_(False)
    out_f, _ = n.forward_fused(**to_fused(b))
    assert torch.isfinite(out_f[0]).all()
    assert dict(m.named_parameters())[WORD].grad is None
    r = settings(build())
    r._ensure_ready(next(r.parameters()).device)
    r.freeze(embeddings=True)
    with pytest.raises(NotImplementedError, match="frozen"):
        r.forward_fused(**to_fused(b))
    assert dict(r.named_parameters())[WORD].grad is not None and not r._flat.frozen      # (the refused call left the storage as it was)
    c = copy.deepcopy(m)
    assert frozen_names(c) == frozen_names(m)
    settings(c)
    c.manual_seed(17)
    check_against_twin(c, result(c, *fb(c)), twin(), what="deepcopy of a")


# ---- 9. trainer ---------------------------------------------------------------------------------------------------------------------------
def test_trainer_freezes_and_trains():
    from msa_amd import trainer
    args = trainer.default_args(learning_rate=1e-3, freeze_embeddings=True, freeze_layers=2)
    batches = [batch(21), batch(22), batch(23)]
    m, h = settings(build()), settings(build())
    names = trainer.apply_freeze(m, args)
    assert set(names) == frozen_names(m) and names
    opt, sched = trainer.build_optimizer(m, args, 3)
    m._ensure_ready(next(m.parameters()).device)
    before, beforeT = _snap(m, set(names))
    trainer.train_epoch(args, m, None, opt, sched, batches=batches, quirk_step=False)       # (an optimizer step per batch)
    # the hand-written loop over the same batches
    trainer.apply_freeze(h, args)
    oh, sh = trainer.build_optimizer(h, args, 3)
    h.train()
    for b in batches:
        out, _ = h(**b)
        out[0].mean().backward()
        oh.step()
        sh.step()
        oh.zero_grad()
    torch.cuda.synchronize()
    after, afterT = _snap(m, set(names))
    for n in names:
        assert torch.equal(after[n][0], before[n][0]) and torch.equal(after[n][1], before[n][1]), n
    _frozen_transposes_equal(m, beforeT, afterT)
    for (n, p), (_, q) in zip(m.named_parameters(), h.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    top = "bert.encoder.layer.3.output.dense.weight"
    assert not torch.equal(dict(m.named_parameters())[top].detach(), _CACHE[("sd", CFG["hidden"])][top].to(DEV))       # (it trained)
