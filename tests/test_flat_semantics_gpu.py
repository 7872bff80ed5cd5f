"""GPU tests of the flat parameter storage (msa_amd/flat.py) as a torch module sees it: ``.data`` / ``.grad`` of every parameter are
views into the flat buffers, and the model, ``msa_amd.optim.AdamW`` and foreign torch code must agree on what they hold.

One oracle, no tolerance -- STATE-DICT EQUIVALENCE (``assert_equals_fresh``): in deterministic mode and eval mode (dropout 0), after any
sequence of supported operations the model gives the same BITS as a freshly built model loaded from ``copy.deepcopy(model.state_dict())``:
the losses ``out[0, 4, 5, 6]``, the logits and every ``p.grad`` after ``out[0].mean().backward()`` on the same batch.  (Two freshly built
models are bit-identical: tests/test_train_gpu.py::test_deterministic_mode_gives_bit_identical_steps; after a fused AdamW step the bf16
working copy is ``p.bfloat16()``: tests/test_adamw_groups_gpu.py::test_grouped_kernel_against_float64 -- a fresh model casts to the same
working weights.)

A. parameter edits torch reports (version counters): seen without a call;  B. ``p.data`` writes and re-pointing: seen after
``model.parameters_changed()``;  C. a ``.grad`` set to None is a dropped gradient, whichever subset;  D. a storage replaced under a bound
optimizer raises at the next optimizer call;  E. ``copy.deepcopy`` / ``torch.save`` of the module give an independent, equal model."""
import copy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

from oracle import mmbert_oracle as O
from msa_amd.data import synthetic_batch, batch_to

DEV = "cuda"
CFG = dict(hidden=128, layers=2, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)

DENSE = "bert.encoder.layer.1.intermediate.dense.weight"                  # has a transposed bf16 copy
LN_W = "bert.encoder.layer.0.attention.output.LayerNorm.weight"           # packed next to its bias
WORD = "bert.embeddings.word_embeddings.weight"                           # the tied decoder
CLS2 = "classifier1_2.weight"
EDITED = [DENSE, LN_W, WORD, CLS2]
TIED = {WORD: "cls.predictions.decoder.weight"}                           # the second state-dict key of the same tensor
HEAD = ("classifier1_1.", "classifier1_2.", "attn.", "vt.", "vv.", "vs.")

_SEEDED = {}


def build(cfg=CFG):
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    c = MMBertConfig(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                     intermediate_size=cfg["intermediate"], hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = MMBertForPretraining(c)
    m.bert.set_joint_embeddings(cfg["dataset"])
    m.bert.jointEmbeddings.dropout_prob = 0.0
    if "sd" not in _SEEDED:
        _SEEDED["sd"] = O.seeded_params(cfg)                              # (computed once; load_state_dict copies out of it)
    m.load_state_dict(_SEEDED["sd"], strict=False)
    m = m.to(DEV)
    m.eval()
    return m


def _batch(seed, cfg=CFG):
    return batch_to(synthetic_batch(2, 16, 40, 24, vocab=cfg["vocab"], seed=seed), DEV)


def _fb(m, b):
    out, logits = m(**b)
    out[0].mean().backward()
    return out, logits


def p0_device(m):
    return next(m.parameters()).device


def _args3(b):
    return b["input_ids"], b["token_type_ids"], b["attention_mask"]


@pytest.fixture(autouse=True)
def _deterministic():
    from msa_amd import ops
    was = ops.deterministic()
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(was)


def _opt(m, **kw):
    from msa_amd.optim import AdamW
    return AdamW(list(m.parameters()), lr=1e-3, weight_decay=0.01, **kw)


def _grads(m):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}


def _same_grads(got, want, names=None, what=""):
    checked = 0
    for n in (got if names is None else names):
        g, w = got[n], want[n]
        assert g is not None and w is not None, (what, n, "grad is None", g is None, w is None)
        assert torch.equal(g, w), (what, n, float((g.double() - w.double()).abs().max()), float(w.double().abs().max()))
        checked += 1
    assert checked
    return checked


def fresh_from(model):
    sd = copy.deepcopy(model.state_dict())
    f = build()
    f.load_state_dict(sd)
    return f


def assert_equals_fresh(model, batch, clear=True):
    """State-dict equivalence (module docstring).  ``clear``: the gradients the model still holds are zeroed through their ``.grad``
    views first (``clear=False``: the caller has dropped them, and that drop is part of what is tested).  Leaves this batch's gradients
    in ``model``."""
    fresh = fresh_from(model)
    if clear:
        for p in model.parameters():
            if p.grad is not None:
                p.grad.zero_()
    out, logits = _fb(model, batch)
    fout, flogits = _fb(fresh, batch)
    torch.cuda.synchronize()
    for i in (0, 4, 5, 6):
        assert torch.equal(out[i].detach(), fout[i].detach()), (i, float(out[i]), float(fout[i]))
    assert torch.equal(logits.detach(), flogits.detach()), float((logits.detach() - flogits.detach()).abs().max())
    assert bool(torch.isfinite(out[0].detach()).all())
    from msa_amd.flat import FROZEN
    got, want = _grads(model), _grads(fresh)
    assert all(g is not None for k, g in got.items() if not k.startswith(FROZEN))      # every differentiated parameter takes part
    _same_grads(got, want, [k for k, g in got.items() if g is not None], "fresh")
    return fresh


# ---------------------------------------------------------------------------------------------------------------------------------
# A. edits that bump the parameter's version counter: the model sees them by itself
# ---------------------------------------------------------------------------------------------------------------------------------
def _edit_load_state_dict(m, name):
    sd = copy.deepcopy(m.state_dict())
    w = sd[name] * 1.25 + 0.01
    sd[name] = w
    if name in TIED:
        sd[TIED[name]] = w
    m.load_state_dict(sd)


def _edit_mul(m, name):
    p = dict(m.named_parameters())[name]
    with torch.no_grad():
        p.mul_(1.5)


def _edit_init(m, name):
    torch.manual_seed(1234)
    nn.init.normal_(dict(m.named_parameters())[name], std=0.05)


def _edit_detach_add(m, name):
    dict(m.named_parameters())[name].detach().add_(0.1)


EDITS = {"load_state_dict": _edit_load_state_dict, "no_grad_mul_": _edit_mul, "nn_init_normal_": _edit_init, "detach_add_": _edit_detach_add}


def _changed(m, name, before):
    assert not torch.equal(dict(m.named_parameters())[name].detach(), before), "the edit did not change the parameter"


@pytest.mark.parametrize("name", EDITED)
@pytest.mark.parametrize("edit", list(EDITS))
@pytest.mark.parametrize("when", ["forward", "step_predict", "step_step"])
def test_versioned_edits_are_seen(when, edit, name):
    """forward: the edit after a bare forward + backward;  step_predict: after a fused AdamW step, then predict();  step_step: after a
    step, then a second step() with no forward in between (the side-stream transposed copy may still be in flight)."""
    m = build()
    _fb(m, _batch(1))
    opt = None
    if when != "forward":
        opt = _opt(m)
        opt.step()
    before = dict(m.named_parameters())[name].detach().clone()
    EDITS[edit](m, name)
    _changed(m, name, before)
    if when == "step_predict":
        b = _batch(2)
        got = m.predict(*_args3(b))
        want = fresh_from(m).predict(*_args3(b))
        assert torch.equal(got, want), float((got - want).abs().max())
    elif when == "step_step":
        edited = dict(m.named_parameters())[name].detach().clone()
        opt.step()
        _changed(m, name, edited)                                         # (momentum and weight decay: the second step moved it again)
    assert_equals_fresh(m, _batch(3))


# ---------------------------------------------------------------------------------------------------------------------------------
# B. edits torch cannot report: parameters_changed()
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EDITED)
@pytest.mark.parametrize("after_step", [False, True])
def test_data_copy_then_parameters_changed(name, after_step):
    m = build()
    _fb(m, _batch(1))
    if after_step:
        _opt(m).step()
    p = dict(m.named_parameters())[name]
    w = p.detach().clone() * 1.5 + 0.02
    p.data.copy_(w)                                                       # (no version bump: torch cannot report it)
    m.parameters_changed()
    assert torch.equal(p.detach(), w)
    assert_equals_fresh(m, _batch(3))
    assert p.data_ptr() == m._flat.params.data_ptr() + 4 * p._mmb_flat[1] and p._mmb_flat[0] is m._flat     # refreshed in place: still the view


@pytest.mark.parametrize("name", EDITED)
def test_repointed_data_then_parameters_changed(name):
    m = build()
    _fb(m, _batch(1))
    m._ensure_ready(p0_device(m))                                         # (a second use: the storage has picked its sentinels)
    old = m._flat
    assert name not in old._sentinels
    p = dict(m.named_parameters())[name]
    w = p.detach().clone() * 1.5 + 0.02
    p.data = w                                                            # re-pointed: no longer a view of the storage
    m.parameters_changed()
    assert_equals_fresh(m, _batch(3))
    assert m._flat is not old and torch.equal(p.detach(), w)              # rebuilt from the parameters as they are
    assert p.data_ptr() == m._flat.params.data_ptr() + 4 * p._mmb_flat[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# C. a .grad set to None is a dropped gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def _drop_module(m, opt):
    m.zero_grad()


def _drop_sgd(m, opt):
    torch.optim.SGD(m.parameters(), lr=0.0).zero_grad()


def _drop_loop(m, opt):
    for p in m.parameters():
        p.grad = None


def _drop_own(m, opt):
    opt.zero_grad()


DROPS = {"module_zero_grad": _drop_module, "sgd_zero_grad": _drop_sgd, "loop_grad_none": _drop_loop, "own_zero_grad": _drop_own}


def _assert_views(m):
    """Every parameter backward differentiates has the view into flat.grads as its .grad."""
    from msa_amd.flat import FROZEN
    f = m._flat
    for n, p in m.named_parameters():
        if n.startswith(FROZEN):
            continue
        assert p.grad is not None, n
        assert p.grad.data_ptr() == f.grads.data_ptr() + 4 * f.offset[n] and p.grad.shape == p.shape, n


@pytest.mark.parametrize("drop", list(DROPS))
@pytest.mark.parametrize("stepped", [False, True])
def test_dropped_gradients_stay_dropped(drop, stepped):
    """A: fb(batch1), the drop, fb(batch2); fresh B: fb(batch2) only.  ``stepped``: a fused AdamW step and its own zero_grad() come first,
    so the lazily zeroed blocks are stale and their .grad detached when the (first) foreign drop arrives."""
    a = build()
    opt = _opt(a)
    if stepped:
        _fb(a, _batch(10))
        opt.step()
        opt.zero_grad()
        assert a._flat.stale and a._flat.lazy_detached
        DROPS[drop](a, opt)
    _fb(a, _batch(11))
    DROPS[drop](a, opt)
    b = fresh_from(a)
    _fb(a, _batch(12))
    _fb(b, _batch(12))
    torch.cuda.synchronize()
    _assert_views(a)
    got, want = _grads(a), _grads(b)
    _same_grads(got, want, what=drop)
    assert float(want[DENSE].abs().max()) > 0 and float(want[CLS2].abs().max()) > 0 and float(want[WORD].abs().max()) > 0


@pytest.mark.parametrize("drop", ["module_zero_grad", "sgd_zero_grad", "loop_grad_none"])
def test_a_drop_between_forward_and_backward(drop):
    """``out = model(batch2); optimizer.zero_grad(); out[0].backward()``: the gradients are batch2's alone."""
    a = build()
    _fb(a, _batch(11))
    out, _ = a(**_batch(12))
    DROPS[drop](a, None)
    b = fresh_from(a)
    out[0].mean().backward()
    _fb(b, _batch(12))
    torch.cuda.synchronize()
    _assert_views(a)
    _same_grads(_grads(a), _grads(b), what=drop)


@pytest.mark.parametrize("drop", ["module_zero_grad", "loop_grad_none"])
def test_dropped_gradients_count_as_zero_for_the_optimizer(drop):
    """fb, the drop, then step() / clip_grad_norm_() with no forward in between: the step sees zero gradients -- the same parameters as a
    model that zeroed them through the optimizer's own zero_grad()."""
    res = []
    for how in (drop, "own_zero_grad"):
        m = build()
        opt = _opt(m)
        _fb(m, _batch(11))
        opt.step()
        _fb(m, _batch(12))
        DROPS[how](m, opt)
        norm = opt.clip_grad_norm_(1.0)
        opt.step()
        torch.cuda.synchronize()
        res.append((float(norm), copy.deepcopy(m.state_dict())))
    assert res[0][0] == 0.0 and res[1][0] == 0.0
    for k, v in res[0][1].items():
        assert torch.equal(v, res[1][1][k]), k


def test_a_dropped_subset_is_reattached_and_the_rest_accumulates():
    """Only the fusion head's gradients are set to None (none of them is one of the storage's sentinels): after fb(batch2) they equal a
    fresh model's fb(batch2); every other gradient equals that of a model that ran fb(batch1), fb(batch2) with no drop."""
    a, c = build(), build()
    for m in (a, c):
        _fb(m, _batch(11))
    head = [n for n, _ in a.named_parameters() if n.startswith(HEAD)]
    a._ensure_ready(p0_device(a))                                         # (a second use: the storage has picked its sentinels)
    assert len(head) == 12 and not set(head) & set(a._flat._sentinels)
    named = dict(a.named_parameters())
    for n in head:
        named[n].grad = None
    b = fresh_from(a)
    for m in (a, b, c):
        _fb(m, _batch(12))
    torch.cuda.synchronize()
    _assert_views(a)
    ga, gb, gc = _grads(a), _grads(b), _grads(c)
    _same_grads(ga, gb, head, "dropped head")
    _same_grads(ga, gc, [n for n in ga if n not in head], "kept")
    assert not torch.equal(gb[DENSE], gc[DENSE])                          # (the kept gradients did accumulate)


def test_head_only_foreign_optimizer_trains_the_head():
    """torch.optim.SGD over the fusion head alone, default zero_grad(): at every step the head's gradients are that step's alone (those of
    a fresh model on the same batch), and the step moves the head exactly as the same SGD moves the fresh model's."""
    m = build()
    head = {n: p for n, p in m.named_parameters() if n.startswith(HEAD)}
    sgd = torch.optim.SGD(list(head.values()), lr=1e-2)
    for k in range(3):
        sgd.zero_grad()
        _fb(m, _batch(20 + k))
        fresh = fresh_from(m)
        _fb(fresh, _batch(20 + k))
        fhead = {n: p for n, p in fresh.named_parameters() if n.startswith(HEAD)}
        before = head[CLS2].detach().clone()
        for n, p in head.items():
            assert p.grad is not None, (k, n)
            assert torch.equal(p.grad, fhead[n].grad), (k, n)
        sgd.step()
        torch.optim.SGD(list(fhead.values()), lr=1e-2).step()
        for n, p in head.items():
            assert torch.equal(p.detach(), fhead[n].detach()), (k, n)
        assert not torch.equal(head[CLS2].detach(), before)


def test_foreign_optimizer_trajectory():
    """Three steps of torch.optim.SGD with its default zero_grad(): after each, the model equals a fresh one loaded from its state dict --
    the weights the model computes with are current, and the gradient of step k is step k's alone."""
    from msa_amd.flat import FROZEN
    m = build()
    sgd = torch.optim.SGD([p for n, p in m.named_parameters() if not n.startswith(FROZEN)], lr=1e-2)
    for k in range(3):
        sgd.zero_grad()
        _fb(m, _batch(30 + k))
        before = dict(m.named_parameters())[DENSE].detach().clone()
        sgd.step()
        assert not torch.equal(dict(m.named_parameters())[DENSE].detach(), before)
        sgd.zero_grad()
        assert_equals_fresh(m, _batch(40), clear=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# D. the storage replaced under a bound optimizer: the optimizer raises, before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
def _replace_to(m):
    m.to("cuda")
    return _batch(3)


def _replace_float(m):
    m.float()
    return _batch(3)


def _replace_num_labels(m):
    m.set_num_labels(3)
    return batch_to(synthetic_batch(2, 16, 40, 24, vocab=CFG["vocab"], seed=3, num_labels=3), DEV)


@pytest.mark.parametrize("replace", [_replace_to, _replace_float, _replace_num_labels], ids=["to_cuda", "float", "set_num_labels"])
@pytest.mark.parametrize("call", ["step", "clip_grad_norm_"])
def test_replaced_storage_under_a_bound_optimizer_raises(replace, call):
    m = build()
    opt = _opt(m)
    _fb(m, _batch(1))
    opt.step()
    opt.zero_grad()
    old = m._flat
    b = replace(m)
    _fb(m, b)
    assert m._flat is not old                                             # the next use built a new storage
    torch.cuda.synchronize()
    snap = (old.params.clone(), m._flat.params.clone(), opt._m.clone(), opt._steps)
    with pytest.raises(RuntimeError, match="re-materialised"):
        opt.step() if call == "step" else opt.clip_grad_norm_(1.0)
    torch.cuda.synchronize()
    assert torch.equal(old.params, snap[0]) and torch.equal(m._flat.params, snap[1]) and torch.equal(opt._m, snap[2]) and opt._steps == snap[3]
    opt2 = _opt(m)                                                        # a rebuilt optimizer drives the new storage
    opt2.step()
    torch.cuda.synchronize()
    assert not torch.equal(m._flat.params, snap[1])
    if replace is not _replace_num_labels:
        assert_equals_fresh(m, _batch(4))


# ---------------------------------------------------------------------------------------------------------------------------------
# E. deepcopy / torch.save of the whole module
# ---------------------------------------------------------------------------------------------------------------------------------
def _sd_equal(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _two_steps(m):
    opt = _opt(m)
    for k in range(2):
        _fb(m, _batch(50 + k))
        opt.step()
        opt.zero_grad()
    torch.cuda.synchronize()


@pytest.mark.parametrize("state", ["forward", "step", "step_async_prologue"])
def test_deepcopy_is_equal_and_independent(state):
    m = build()
    if state == "step_async_prologue":
        m.async_prologue = True
    _fb(m, _batch(1))
    if state != "forward":
        opt = _opt(m)
        opt.step()                                                        # (the side-stream transposed copy is in flight)
    c = copy.deepcopy(m)
    assert c._flat is None and c.bert._owner() is c and c.cls._owner() is c and c.bert.jointEmbeddings._owner() is c
    assert c.cls.predictions.decoder.weight is c.bert.embeddings.word_embeddings.weight
    assert all(getattr(p, "_mmb_flat", None) is None for p in c.parameters())
    _sd_equal(copy.deepcopy(m.state_dict()), c.state_dict())
    assert_equals_fresh(c, _batch(3))
    assert_equals_fresh(m, _batch(3))
    sd_m, sd_c = copy.deepcopy(m.state_dict()), copy.deepcopy(c.state_dict())
    _two_steps(c)
    _sd_equal(sd_m, m.state_dict())
    assert not torch.equal(sd_c[DENSE], c.state_dict()[DENSE])
    sd_c = copy.deepcopy(c.state_dict())
    _two_steps(m)
    _sd_equal(sd_c, c.state_dict())
    assert not torch.equal(sd_m[DENSE], m.state_dict()[DENSE])


def test_torch_save_of_the_module_round_trips(tmp_path):
    m = build()
    _fb(m, _batch(1))
    _opt(m).step()
    path = tmp_path / "model.pt"
    torch.save(m, path)
    c = torch.load(path, weights_only=False)
    assert c._flat is None and c.bert._owner() is c and c.cls._owner() is c
    _sd_equal(copy.deepcopy(m.state_dict()), c.state_dict())
    assert_equals_fresh(c, _batch(3))
    sd_m = copy.deepcopy(m.state_dict())
    _two_steps(c)
    _sd_equal(sd_m, m.state_dict())
