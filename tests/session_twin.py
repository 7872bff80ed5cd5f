"""A long-lived model held to fresh twins, bit for bit.

Not a test module (pytest does not collect it): ``from tests import session_twin as ST``.  Importing it needs no GPU.

Every other GPU test builds a fresh model, runs a step or two at one shape and throws the model away.  A model in use lives for
thousands of steps whose batch shape changes with the data, with evaluation, ``predict``, ``predict_tokens`` and the EMA swap in
between -- and keeps state from step to step: the plan cache, the prologue's buffer sets, the stamped row inverse, the deferred
LayerNorm' collector, the side-stream joins, the dropout seed counter on the model; slabs, workspaces, sync words, tile queues and
side streams per process (msa_amd/ops.py); the lazy-zero flags, the clip coefficient, the EMA and the bf16 / transposed working
copies in the flat storage and the optimizer.  Each is right only while an invariant holds ACROSS steps.  Deterministic mode makes
"the same" mean ``torch.equal``, so the check is exact:

* a **script** is a list of items ``(kind, shape, seed, options)``; ``shape = (B, T, Pv, Pa[, full_length])`` of
  ``msa_amd.data.synthetic_batch``; ``kind`` one of ``KINDS``;
* a ``Session`` (model + AdamW with EMA and clipping + warm-up schedule) plays a script item by item; ``result`` of an item = clones of
  every tensor the call returned, behind a backward the WHOLE flat gradient buffer (a lazily-zeroed block nobody overwrote shows
  there, not in the ``.grad`` views), behind an optimizer step the fp32 parameters, the bf16 working copy, m, v, the EMA and layer
  0's transposed copies;
* ``snapshot`` at an optimizer-step boundary holds everything that DEFINES the state (parameters, optimizer state, schedule position,
  dropout seed counter, switches) and nothing of what merely caches it; ``twin`` builds a fresh session holding exactly that;
* ``check_against_twins`` replays, per boundary, the items since on a twin and compares with ``assert_same_bits``; a training item's
  twin never runs the inference items in between."""
from __future__ import annotations

import contextlib
import copy

import torch

KINDS = ("accumulate", "train", "eval", "predict", "predict_attention", "predict_tokens", "ema_eval")
TRAINING = ("accumulate", "train")

# the main script's shapes, taken from what the suite already runs (tests/test_train_gpu.py, tests/test_step_stages_gpu.py); the last one is
# #6's (T, Pv, Pa) at ANOTHER batch size: the plan cache must not answer it with #6's plan
MAIN_SHAPES = ((3, 20, 60, 40), (5, 24, 200, 170), (2, 12, 30, 30), (5, 24, 200, 170), (6, 30, 260, 90), (4, 24, 200, 130), (1, 8, 8, 8),
               (5, 24, 170, 200), (3, 20, 60, 40), (3, 24, 200, 130, True))


def main_script(n=None, seed0=900):
    """Items alternate ``accumulate`` / ``train``: two micro-batches of DIFFERENT shape per optimizer step."""
    shapes = MAIN_SHAPES[:n]
    return [("accumulate" if i % 2 == 0 else "train", s, seed0 + i, {}) for i, s in enumerate(shapes)]


MODES_SCRIPT = [("train", (3, 20, 60, 40), 950, {}), ("predict", (5, 24, 200, 170), 951, {}), ("train", (2, 12, 30, 30), 952, {}),
                ("predict_tokens", (4, 24, 200, 130), 953, {}), ("eval", (6, 30, 260, 90), 954, {}), ("ema_eval", (1, 8, 8, 8), 955, {}),
                ("predict_attention", (5, 24, 170, 200), 956, {}), ("train", (4, 24, 200, 130, True), 957, {})]


# ------------------------------------------------------------------------------------------------ what the shapes alone say
def shape_facts(shape):
    """(packed rows B (3T + Pv + Pa), longest sequence, the prologue's (floats, ints), (T, Pv, Pa), B, full_length) of a script shape."""
    from msa_amd import ops
    B, T, Pv, Pa = shape[:4]
    full = bool(shape[4]) if len(shape) > 4 else False
    lens = [T, T + Pv, T + Pa]
    return dict(rows=B * (3 * T + Pv + Pa), longest=max(lens), prologue=ops.prologue_sizes(lens, B), lens=tuple(lens), tpp=(T, Pv, Pa), B=B,
                full_length=full)


def transitions(script):
    """Which of the cache transitions a script is there for it really contains, from its shapes alone: name -> item indices (0-based)
    at which the transition happens (empty = missing)."""
    f = [shape_facts(it[1]) for it in script]
    out = {k: [] for k in ("grows_past_everything", "shrinks_right_after_the_largest", "exact_repeat", "same_lens_other_batch",
                           "pair_lengths_exchanged", "longer_than_256", "one_sample_labels_on_pair_rows", "full_length")}
    largest = max(range(len(f)), key=lambda i: f[i]["rows"])
    for i, x in enumerate(f):
        before = f[:i]
        if before and all(x["rows"] > y["rows"] and x["prologue"][0] > y["prologue"][0] and x["prologue"][1] > y["prologue"][1] for y in before):
            out["grows_past_everything"].append(i)
        if i == largest + 1 and x["rows"] < f[largest]["rows"] and all(a < b for a, b in zip(x["prologue"], f[largest]["prologue"])):
            out["shrinks_right_after_the_largest"].append(i)
        if any(script[j][1] == script[i][1] for j in range(i)):
            out["exact_repeat"].append(i)
        if any(y["tpp"] == x["tpp"] and y["B"] != x["B"] for y in before):
            out["same_lens_other_batch"].append(i)
        if any(y["B"] == x["B"] and y["tpp"][0] == x["tpp"][0] and y["tpp"][1:] == x["tpp"][:0:-1] and y["tpp"][1] != y["tpp"][2] for y in before):
            out["pair_lengths_exchanged"].append(i)
        if x["longest"] > 256:
            out["longer_than_256"].append(i)
        if x["B"] == 1 and x["tpp"][0] == x["tpp"][1] == x["tpp"][2]:
            out["one_sample_labels_on_pair_rows"].append(i)
        if x["full_length"]:
            out["full_length"].append(i)
    return out


# ------------------------------------------------------------------------------------------------ comparing
def _owner_of(layout, index):
    """The parameter (name, element within it) that owns element ``index`` of a flat buffer; ``layout`` = [(offset, numel, name)]."""
    for o, k, n in layout or ():
        if o <= index < o + k:
            return f"{n}[{index - o}]"
    return "padding between parameters"


FLAT_KEYS = ("grads", "params", "half", "m", "v", "ema")


def assert_same_bits(a: dict, b: dict, where: str, layout=None):
    """``a`` and ``b``: results (dicts of tensors).  Equal key sets, and ``torch.equal`` on every entry -- same shape, same dtype, same
    bits up to the sign of zero.  ``where`` names the item (index and kind); a failure adds the entry, the first differing element and,
    for the flat buffers (``FLAT_KEYS``, with ``layout`` = [(offset, numel, parameter name)]), the parameter that owns it."""
    assert set(a) == set(b), f"{where}: entries differ: only in the first {sorted(set(a) - set(b))}, only in the second {sorted(set(b) - set(a))}"
    for k in sorted(a):
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, f"{where}: entry {k!r}: {tuple(x.shape)} {x.dtype} against {tuple(y.shape)} {y.dtype}"
        if torch.equal(x, y):
            continue
        ne = (x != y).reshape(-1)
        if x.is_floating_point():
            ne |= (torch.isnan(x) | torch.isnan(y)).reshape(-1)
        idx = int(ne.nonzero()[0]) if bool(ne.any()) else 0
        xv, yv = x.reshape(-1)[idx].item(), y.reshape(-1)[idx].item()
        own = f", owned by {_owner_of(layout, idx)}" if k in FLAT_KEYS else ""
        raise AssertionError(f"{where}: entry {k!r} differs in {int(ne.sum())} of {x.numel()} elements, first at flat index {idx}{own}: {xv!r} against {yv!r}")


def where(index, item):
    return f"item {index} ({item[0]} {tuple(item[1])})"


# ------------------------------------------------------------------------------------------------ the session
SWITCHES = ("async_prologue", "composite_layers", "defer_wgrads", "fused_heads", "coop_heads", "late_wgrads", "wgrad_side_stream",
            "heads_side_stream", "pairs_side_stream", "return_scores", "scores_dtype", "dedupe_masked_rows", "device_split_layout",
            "fused_rowset_packing", "token_chunk_rows", "alpha", "beta", "num_labels", "multi_label",
            "label_loss_kind", "huber_delta", "label_smoothing", "mlm_label_smoothing", "multilabel_smoothing")
SWITCH_PREFIXES = ("skip_", "sparse_")
SWITCH_BUFFERS = ("class_weights", "pos_weight", "thresholds")

_batches = {}


def batch(shape, seed, cfg, device="cuda"):
    """The item's batch on the device, built once per (shape, seed, vocabulary) and never written to."""
    from msa_amd.data import batch_to, synthetic_batch
    key = (tuple(shape), seed, cfg["vocab"], cfg["dataset"], str(device))
    b = _batches.get(key)
    if b is None:
        B, T, Pv, Pa = shape[:4]
        full = bool(shape[4]) if len(shape) > 4 else False
        b = _batches[key] = batch_to(synthetic_batch(B, T, Pv, Pa, dataset=cfg["dataset"], vocab=cfg["vocab"], seed=seed, full_length=full), device)
    return b


def _args3(b):
    return b["input_ids"], b["token_type_ids"], b["attention_mask"]


def _switches(model):
    out = {k: getattr(model, k) for k in SWITCHES if hasattr(model, k)}          # (a switch nobody set is absent on the twin as well)
    out.update({k: v for k, v in model.__dict__.items() if k.startswith(SWITCH_PREFIXES) and not torch.is_tensor(v)})
    for k in SWITCH_BUFFERS:
        v = getattr(model, k, None)
        out[k] = None if v is None else v.detach().clone()
    return out


def snapshot(model, opt, sched):
    """What defines the session at an optimizer-step boundary, as deep copies: ``model.state_dict()``, ``opt.state_dict()`` (steps, m, v,
    the EMA and its decay state, the groups' learning rates), the schedule's position, the dropout seed counter, the model's switches
    (mode, deterministic mode, launch paths, short cuts, loss options).  Nothing of what the session merely caches."""
    from msa_amd import ops
    osd = opt.state_dict()
    return dict(model={k: v.detach().clone() for k, v in model.state_dict().items()},
                opt={k: (v.detach().clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in osd.items()},
                groups=[{k: copy.deepcopy(v) for k, v in g.items() if k != "params"} for g in opt.param_groups],
                opt_kw=dict(mode={0: "hf", 1: "torch"}[opt.mode], lazy_zero=opt.lazy_zero, grad_scale=opt.grad_scale),
                sched=dict(warmup=sched.warmup, total=sched.total, last_step=sched.last_step),
                seed=(model._seed, model._calls), training=model.training, je_training=model.bert.jointEmbeddings.training,
                deterministic=ops.deterministic(), switches=_switches(model), max_norm=None)


class Session:
    """One model, one optimizer (EMA on, clipping), one warm-up schedule.  ``build``: tests.test_model_gpu.build."""

    def __init__(self, cfg, build, *, seed=29, lr=2e-3, weight_decay=0.01, ema_decay=0.9, warmup=4, total=40, max_norm=1.0, train=True,
                 setup=None, _snapshot=None):
        from msa_amd.optim import AdamW, LinearWarmupSchedule
        self.cfg, self.build, self.max_norm, self.setup = cfg, build, max_norm, setup
        snap = _snapshot
        m = self.model = build(cfg, train=train)
        if snap is None:
            m.manual_seed(seed)
            if setup is not None:
                setup(m)
            self.opt = AdamW(m.parameters(), lr=lr, weight_decay=weight_decay).ema(ema_decay, warmup=True)
            self.sched = LinearWarmupSchedule(self.opt, warmup, total)
            self.sched.step()                    # (position 0 of a warm-up is lr = 0: the first step would change nothing)
        else:
            from msa_amd import ops
            assert ops.deterministic() == snap["deterministic"], "the twin runs in the snapshot's mode"
            m.load_state_dict(snap["model"])
            for k, v in snap["switches"].items():
                if k in SWITCH_BUFFERS:
                    if v is not None or getattr(m, k, None) is not None:
                        setattr(m, k, None if v is None else v.clone())
                elif k not in ("num_labels", "multi_label") or getattr(m, k) != v:
                    setattr(m, k, v)
            m.train(snap["training"])
            m.bert.jointEmbeddings.train(snap["je_training"])
            m._seed, m._calls = snap["seed"]
            m._ensure_ready(next(m.parameters()).device)              # (the optimizer binds to the flat storage)
            self.opt = AdamW(m.parameters(), lr=lr, weight_decay=weight_decay, mode=snap["opt_kw"]["mode"])
            for g, s in zip(self.opt.param_groups, snap["groups"]):
                g.update(copy.deepcopy(s))
            self.opt.lazy_zero, self.opt.grad_scale = snap["opt_kw"]["lazy_zero"], snap["opt_kw"]["grad_scale"]
            self.opt.load_state_dict(snap["opt"])
            s = snap["sched"]
            self.sched = LinearWarmupSchedule(self.opt, s["warmup"], s["total"])
            self.sched.last_step = s["last_step"]
            self.sched._apply()
            assert [g["lr"] for g in self.opt.param_groups] == snap["opt"]["lrs"], "schedule position and learning rates of the snapshot disagree"

    def snapshot(self):
        return snapshot(self.model, self.opt, self.sched)

    def layout(self):
        f = self.model._flat
        return sorted((f.offset[n], f.numel[n], n) for n in f.order)

    # ---- one item
    def _forward(self, b, res, tag=""):
        out, logits = self.model(**b)
        for i, t in enumerate(out):
            if torch.is_tensor(t):
                res[f"{tag}out{i}"] = t.detach().clone()
        res[f"{tag}logits"] = logits.detach().clone()
        return out

    def _after_step(self, res):
        f, o = self.model._flat, self.opt
        ev = f.__dict__.get("_t_event")
        if ev is not None:
            ev.synchronize()          # the HOST waits for the transposed copies; the event stays for backward to wait on, as without a reader
        res.update(params=f.params.clone(), half=f.half.clone(), m=o._m.clone(), v=o._v.clone(), ema=o._ema.clone())
        for k in ("WqkvT", "WoT", "W1T", "W2T"):
            res["layer0." + k] = self.model._lw[0][k].clone()

    def begin(self, item, tag=""):
        """The forward pass of a training item: (outputs, result so far)."""
        res = {}
        return self._forward(batch(item[1], item[2], self.cfg), res, tag), res

    def finish(self, item, res):
        """Behind the backward pass of a training item: the whole gradient buffer, and for ``train`` the optimizer step."""
        res["grads"] = self.model._flat.grads.clone()
        if item[0] == "train":
            res["norm"] = self.opt.clip_grad_norm_(self.max_norm).detach().clone()
            self.opt.step()
            self.sched.step()
            self.opt.zero_grad()
            self._after_step(res)
        return res

    def run(self, item, around_step=None, after_backward=None):
        """Plays one item; returns its result.  ``around_step``: a context manager factory entered around forward + backward of a
        training item (tests.step_stages.record), ``after_backward(what it yielded)``: called between that and the optimizer."""
        kind, shape, seed, options = item
        assert kind in KINDS, kind
        m, b, res = self.model, batch(shape, seed, self.cfg), {}
        if kind in TRAINING:
            with (around_step(m) if around_step is not None else contextlib.nullcontext()) as rec:
                out, res = self.begin(item)
                out[0].mean().backward()
            if after_backward is not None:
                after_backward(rec)
            self.finish(item, res)
        elif kind == "eval":
            was = m.training
            m.eval()
            try:
                with torch.no_grad():
                    self._forward(b, res)
            finally:
                m.train(was)
        elif kind == "predict":
            logits, extra = m.predict(*_args3(b), return_pooled=True)
            res.update(_tensors(dict(logits=logits, **extra)))
        elif kind == "predict_attention":
            logits, extra = m.predict(*_args3(b), return_attention=options.get("return_attention", "all"))
            res.update(_tensors(dict(logits=logits, **extra)))
        elif kind == "predict_tokens":
            res.update(_tensors(m.predict_tokens(*_args3(b), masked_labels=b["masked_labels"], top_k=options.get("top_k", 5))))
        elif kind == "ema_eval":
            self.opt.swap_ema()
            was = m.training
            m.eval()
            try:
                with torch.no_grad():
                    self._forward(b, res, "eval.")
                logits, extra = m.predict(*_args3(b), return_pooled=True)
                res.update(_tensors(dict(logits=logits, **extra), "predict."))
            finally:
                m.train(was)
                self.opt.swap_ema()
        return res


def _tensors(d, prefix=""):
    """Every tensor of a nested dict / list result as clones under dotted names."""
    out = {}
    for k, v in d.items():
        if torch.is_tensor(v):
            out[prefix + str(k)] = v.detach().clone()
        elif isinstance(v, dict):
            out.update(_tensors(v, prefix + str(k) + "."))
        elif isinstance(v, (list, tuple)) and v and all(isinstance(x, int) for x in v):
            out[prefix + str(k)] = torch.tensor(list(v))
    return out


def twin(snap, cfg, build):
    """A fresh Session -- new model, new flat storage, new optimizer and schedule -- that holds exactly the snapshot's state."""
    return Session(cfg, build, _snapshot=snap, max_norm=snap["max_norm"])


def play(sess, script, enter=None, around=None, snapshots=True):
    """The long-lived run: every item in turn on ``sess``.  Returns (results, snapshots): snapshots[i] = the state in front of item i
    where item i is the first behind an optimizer-step boundary (item 0, and every item behind a ``train``).
    ``enter(i)``: a context manager for item i (a stream); ``around[i]``: (``around_step``, ``after_backward``) of item i."""
    results, snaps = [], {}
    for i, item in enumerate(script):
        with (enter(i) if enter is not None else contextlib.nullcontext()):
            if snapshots and (i == 0 or script[i - 1][0] == "train"):
                snaps[i] = sess.snapshot()
                snaps[i]["max_norm"] = sess.max_norm
            results.append(sess.run(item, *(around or {}).get(i, ())))
    return results, snaps


def check_against_twins(results, snaps, script, cfg, build):
    """Every item of the long-lived run against a fresh twin of the last boundary in front of it.  The TRAINING items since that boundary
    are replayed on one twin that runs nothing else (an ``accumulate`` item together with the ``train`` item that consumes it, never the
    inference items in between); every inference item gets a twin of its own that replays the ``accumulate`` items in front of it (they
    move the dropout seed counter and the gradients, which an inference call must not read) and then the item.  Returns the number of
    items compared: the caller asserts it is the script's length."""
    compared, lay = 0, None
    starts = sorted(snaps)
    for n, s0 in enumerate(starts):
        s1 = starts[n + 1] if n + 1 < len(starts) else len(script)
        t = twin(snaps[s0], cfg, build)
        lay = t.layout()
        acc = []
        for i in range(s0, s1):
            item = script[i]
            if item[0] in TRAINING:
                assert_same_bits(results[i], t.run(item), where(i, item) + " against its fresh twin", lay)
                acc.append(item)
            else:
                t2 = twin(snaps[s0], cfg, build)
                for a in acc:
                    t2.run(a)
                assert_same_bits(results[i], t2.run(item), where(i, item) + " against its fresh twin", lay)
                del t2
            compared += 1
        del t
    return compared


# ------------------------------------------------------------------------------------------------ what must be left behind: nothing
LEFTOVERS = ("_late_wgrads", "_wgrad_join", "_heads_join", "_heads_src", "_deferred_embed_rows")


def leftovers(model):
    """What a finished step may not leave behind, as a list of findings (empty = clean): the model's hand-overs of a backward pass,
    items in its LayerNorm' collector, a non-zero heads sync word or tile-queue counter of ANY stream of the process."""
    from msa_amd import ops
    torch.cuda.synchronize()
    found = [k for k in LEFTOVERS if model.__dict__.get(k)]
    lnd = model.__dict__.get("_lnd")
    if lnd is not None and lnd.items:
        found.append(f"_lnd holds {len(lnd.items)} items")
    for name, cache in (("heads sync words", ops._heads_sync), ("tile queue", ops._tile_queues)):
        for key, t in cache.items():
            if bool((t != 0).any()):
                found.append(f"{name} of stream {key[1]:#x}: {t.tolist()}")
    return found
