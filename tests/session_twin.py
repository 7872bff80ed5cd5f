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
  twin never runs the inference items in between.

The fine-tuning lifecycle.  Besides the items above a script may hold **mutations** (``MUTATIONS``): ``freeze`` /
``unfreeze`` / ``add_lora`` / ``merge_lora`` / ``remove_lora`` / ``reload_lora``.  They take no batch (shape ``None``), their arguments are
the item's ``options``, and they stand only at an optimizer-step boundary -- no micro-batch pending: at item 0, or where the last
training item in front is a ``train`` (inference items and other mutations, which leave the optimizer alone, may stand in between;
``misplaced_mutations``).  THE OPTIMIZER RULE that makes the twin well defined: ``freeze`` keeps the optimizer (it follows through
``AdamW._follow_frozen`` and keeps m, v and the step count); every other mutation replaces it by a fresh ``AdamW`` -- same lr, weight
decay, mode, ``lazy_zero``, ``grad_scale``, the EMA restarted with the same decay and warm-up, step count 0, zero moments -- and re-binds
the warm-up schedule to it at the position it had (msa_amd/optim.py: "build a new optimizer" behind an unfreeze that follows a step and
behind a dropped storage).  ``snapshot`` also records ``{name: requires_grad}`` and the adapter record; a snapshot behind such a rebuild
holds an UNBOUND optimizer (m / v / ema None), which the twin reproduces.  ``play`` snapshots in front of the first batch item behind a
boundary, so a twin never runs a mutation.

The gradient buffer under freezing: msa_amd/flat.py leaves the ``grads`` span of a frozen parameter unspecified while it is frozen (a
lazily dropped weight gradient that is then frozen is never zero-filled).  ``Session.finish`` therefore zero-fills, on its CLONE only, the
spans of exactly ``grad_mask(plan)`` = the plan's frozen names (asserted equal to ``model._flat.frozen``) -- a condition derived from the
names alone, empty wherever nothing is frozen, not a tolerance: trainable spans, the padding between parameters and the whole of params,
half, m, v and ema stay compared bit for bit, and the first training item behind an ``unfreeze`` compares those spans again
(``set_frozen`` must have zero-filled them)."""
from __future__ import annotations

import contextlib
import copy

import torch

KINDS = ("accumulate", "train", "eval", "predict", "predict_attention", "predict_tokens", "ema_eval")
TRAINING = ("accumulate", "train")
MUTATIONS = ("freeze", "unfreeze", "add_lora", "merge_lora", "remove_lora", "reload_lora")

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


def _mut(kind, **options):
    return (kind, None, None, options)


# the one-sample batch runs the DENSE top-layer backward only when enough of its 40 rows carry a label (``top_layer_is_dense``): seeds at
# which they do (906: the main script's item 7)
DENSE_TOP_SEEDS = (906, 1003)


def _seeded(items, seed0):
    """(kind, shape) -> seed0 + index; (kind, shape, seed) and whole items as they are."""
    return [it if len(it) == 4 else (it[0], it[1], it[2] if len(it) == 3 else seed0 + i, {}) for i, it in enumerate(items)]


def freeze_script(L, seed0=1000):
    """Freezing over a model's life (L encoder layers): a frozen prefix that grows until backward is the top layer alone and ends there
    without an input gradient, a bias-only top layer, everything trainable again behind steps, a frozen layer between trainable ones, a
    freeze that is taken back before any optimizer step --
    with two micro-batches per step, the largest batch, the small one right behind it, the one-sample batch (dense top-layer backward)
    and the inference paths in between."""
    a, b, c, d, e, f, g, h = (MAIN_SHAPES[k] for k in (0, 1, 2, 4, 5, 6, 7, 9))
    items = [("train", a), _mut("freeze", embeddings=True, layers=1), ("accumulate", b), ("train", c), ("predict", e),
             _mut("freeze", layers=L - 1), ("train", d), ("ema_eval", c), _mut("freeze", layer_weights=True), ("accumulate", a), ("train", f, DENSE_TOP_SEEDS[0]),
             ("predict_tokens", e), _mut("unfreeze"), ("train", g), _mut("freeze", layers=[1]), ("train", h), ("eval", b),
             # a freeze taken back before any optimizer step: layer 0's lazily dropped weight gradients are still in the buffer when an
             # eval forward reads the flags (they leave the stale set) and when the next forward finds them trainable again -- only
             # set_frozen's zero fill stands between them and the first weight-gradient launch, which accumulates.  (Behind a step the
             # optimizer's fused zero_grad has zero-filled every frozen block already: the unfreeze above cannot show it.)
             _mut("freeze", layers=1), ("eval", c), _mut("unfreeze"), ("train", a)]
    return _seeded(items, seed0)


def lora_script(L, seed0=1100):
    """Adapters over a model's life: rank 4 on query + value of every layer over a frozen base, saved / removed / loaded again, merged
    (after which NO encoder layer is trainable: backward is the heads and the MLM head's few rows), everything trainable again, rank 16
    on the key projection of the top layer alone over a trainable base, removed."""
    a, b, c, d, e, f, g, h = (MAIN_SHAPES[k] for k in (0, 1, 2, 4, 5, 6, 7, 9))
    items = [("train", a), _mut("add_lora", r=4, alpha=8.0, targets=("query", "value"), freeze_base=True, seed=77), ("accumulate", b), ("train", f, DENSE_TOP_SEEDS[1]),
             ("predict_tokens", e), ("train", d), ("predict_attention", c), _mut("reload_lora"), ("train", e), ("ema_eval", a), _mut("merge_lora"),
             ("train", g), ("predict", c), _mut("unfreeze"), _mut("add_lora", r=16, alpha=16.0, targets=("key",), layers=[L - 1], freeze_base=False, seed=78),
             ("train", h), ("eval", b), _mut("remove_lora"), ("train", c)]
    return _seeded(items, seed0)


def dense_lora_script(L, seed0=1300):
    """Adapters on the dense seams over a model's life (attention.output.dense, intermediate.dense, output.dense: DESIGN 3.15): rank 8 on all
    six targets of every layer over a frozen base behind a step -- two micro-batches onto the adapter gradients, the one-sample batch (dense
    top-layer backward, saved h slices), the largest batch, ``predict`` / ``predict_tokens`` / ``predict_attention`` / ``eval`` / the EMA swap
    while they are live --, saved / removed / loaded again, merged (the FFN-up GEMM gets its GELU epilogue back; no encoder layer is
    trainable), everything trainable again; rank 4 on the key projection of layer 0 alone (no dense target), removed; rank 16 on
    intermediate + ffn_output of the top layer alone over a trainable base (a layer with dense adapters and no Q/K/V ones, next to layers
    on the composite path), ``predict`` through the [CLS]-only top layer on its gathered rows, removed."""
    a, b, c, d, e, f, g, h = (MAIN_SHAPES[k] for k in (0, 1, 2, 4, 5, 6, 7, 9))
    items = [("train", a), _mut("add_lora", r=8, alpha=16.0, targets="all-linear", freeze_base=True, seed=81), ("accumulate", b), ("train", f, DENSE_TOP_SEEDS[0]),
             ("predict", e), ("predict_tokens", c), ("train", d), ("predict_attention", c), _mut("reload_lora"), ("train", e), ("ema_eval", a), ("eval", b),
             _mut("merge_lora"), ("train", g), _mut("unfreeze"), _mut("add_lora", r=4, alpha=8.0, targets=("key",), layers=[0], freeze_base=False, seed=82),
             ("train", h), _mut("remove_lora"),
             _mut("add_lora", r=16, alpha=16.0, targets=("intermediate", "ffn_output"), layers=[L - 1], freeze_base=False, seed=83), ("train", a), ("predict", c),
             _mut("remove_lora"), ("train", c)]
    return _seeded(items, seed0)


# ------------------------------------------------------------------------------------------------ what the names alone say
LORA_BASE = ("bert.embeddings.", "bert.jointEmbeddings.", "bert.encoder.")          # what add_lora(freeze_base=True) freezes
LIFECYCLE = ("stop_rises", "stop_is_top_layer_without_input_gradient", "bias_only_layer", "frozen_layer_between_trainable_ones",
             "unfreeze_behind_steps", "unfreeze_without_a_step_since_the_freeze", "no_encoder_layer_trainable", "adapters_on_frozen_base", "adapters_on_trainable_base",
             "adapters_on_a_subset_of_layers", "rank_changes", "targets_change", "merge", "remove", "reload",
             # the dense seams: a training item with a dense target adapted / with ``intermediate`` adapted (the FFN-up GEMM loses its GELU
             # epilogue to the adapter launch) / with adapted layers that have no Q/K/V adapters
             "dense_targets", "ffn_up_adapter", "dense_only_layer")
LORA_QKV = ("query", "key", "value")
LORA_DENSE_PATHS = {"attention_output": "attention.output.dense", "intermediate": "intermediate.dense", "ffn_output": "output.dense"}


def misplaced_mutations(script):
    """The indices of the mutations that do NOT stand at an optimizer-step boundary (a micro-batch is pending: the last training item in
    front is an ``accumulate``), and of those that carry a shape or, for ``add_lora``, no seed."""
    bad, pending = [], False
    for i, (kind, shape, _seed, options) in enumerate(script):
        if kind in MUTATIONS:
            if pending or shape is not None or (kind == "add_lora" and "seed" not in options):
                bad.append(i)
        elif kind in TRAINING:
            pending = kind == "accumulate"
    return bad


def base_frozen(flags):
    """Whether every base parameter (``LORA_BASE``, the adapters left out) has ``requires_grad == False``: ``reload_lora``'s ``freeze_base``."""
    return not any(t for n, t in flags.items() if n.startswith(LORA_BASE) and ".lora_" not in n)


def _lora_record(options, L):
    """model._lora behind ``add_lora(**options)``: the targets (any of the six names, or "all-linear") in ops.lora_split_targets' canonical
    order, Q/K/V first."""
    from msa_amd import ops
    layers = options.get("layers")
    qkv, dense = ops.lora_split_targets(options.get("targets", ("query", "value")))
    assert qkv == tuple(t for t in LORA_QKV if t in qkv) and dense == tuple(t for t in LORA_DENSE_PATHS if t in dense)
    return dict(r=options.get("r", 8), alpha=float(options.get("alpha", 16.0)), targets=qkv + dense,
                layers=tuple(range(L)) if layers is None else tuple(sorted(layers)))


def lora_module_path(target):
    """The module below an encoder layer that carries a target's ``lora_A`` / ``lora_B``."""
    return "attention.self." + target if target in LORA_QKV else LORA_DENSE_PATHS[target]


def _with_adapters(flags, rec, freeze_base):
    out = dict(flags)
    for i in rec["layers"]:
        for t in rec["targets"]:
            for m in ("lora_A", "lora_B"):
                out[f"bert.encoder.layer.{i}.{lora_module_path(t)}.{m}"] = True
    if freeze_base:
        for n in out:
            if n.startswith(LORA_BASE) and ".lora_" not in n:
                out[n] = False
    return out


def lifecycle_states(script, names, L):
    """Per item of ``script``: (``{name: requires_grad}`` in force, the adapter record or None, the freeze.TrainablePlan of a training item
    -- None for other items and while everything is trainable).  Pure: ``names`` = the parameter names of a model WITHOUT adapters (a
    CPU-built MMBertForPretraining), the flags behind each mutation from freeze.resolve_freeze and add_lora's rule, the plan from
    freeze.trainable_plan(flags, L, {}, {})."""
    from msa_amd import freeze as FZ
    flags, lora, out = {n: True for n in names}, None, []
    for kind, _shape, _seed, options in script:
        if kind == "freeze":
            flags = dict(flags)
            for n in FZ.resolve_freeze(list(flags), L, **options):
                flags[n] = False
        elif kind == "unfreeze":
            flags = {n: True for n in flags}
        elif kind == "add_lora":
            assert lora is None, "add_lora on a model that has adapters"
            lora = _lora_record(options, L)
            flags = _with_adapters(flags, lora, options.get("freeze_base", True))
        elif kind in ("merge_lora", "remove_lora"):
            assert lora is not None, kind + " without adapters"
            lora, flags = None, {n: t for n, t in flags.items() if ".lora_" not in n}
        elif kind == "reload_lora":
            assert lora is not None, "reload_lora without adapters"
            fb = base_frozen(flags)
            flags = _with_adapters({n: t for n, t in flags.items() if ".lora_" not in n}, lora, fb)
        out.append((flags, lora, FZ.trainable_plan(flags, L, {}, {}) if kind in TRAINING else None))
    return out


def grad_mask(plan):
    """The names whose span of the gradient buffer ``Session.finish`` zero-fills on its clone: the plan's frozen names; nothing without a plan."""
    return frozenset() if plan is None else frozenset(plan.frozen)


def zero_spans(g, offset, numel, names):
    """Zero-fills, in the flat buffer ``g`` (a clone), the spans of ``names`` and nothing else -- not the padding behind them."""
    for n in names:
        g[offset[n]:offset[n] + numel[n]] = 0
    return g


def lifecycle_facts(script, names, L):
    """Which of the lifecycle transitions (``LIFECYCLE``) a script really contains, from the names alone: name -> item indices (0-based,
    counting every item of the script) at which it happens; the states of a training item are judged at that item, what a mutation does
    at the mutation."""
    from msa_amd import freeze as FZ
    out = {k: [] for k in LIFECYCLE}
    states = lifecycle_states(script, names, L)
    prev_stop, steps, last_lora = 0, 0, None
    since_freeze = None                                            # the kinds of the batch items since the last ``freeze`` (None: none yet)
    for i, (item, (flags, lora, plan)) in enumerate(zip(script, states)):
        kind = item[0]
        if kind in TRAINING:
            stop = 0 if plan is None else plan.stop
            if stop > prev_stop:
                out["stop_rises"].append(i)
            prev_stop = stop
            if plan is not None:
                if plan.stop == L - 1 and not plan.embedding_stage:
                    out["stop_is_top_layer_without_input_gradient"].append(i)
                if any(m == FZ.BIAS for modes in plan.layers.values() for m in modes.values()):
                    out["bias_only_layer"].append(i)
                dead = lambda j: all(m == FZ.NONE for m in plan.layers[j].values())           # noqa: E731
                if any(dead(j) and not dead(plan.stop) and any(not dead(k) for k in range(j + 1, L)) for j in range(plan.stop + 1, L)):
                    out["frozen_layer_between_trainable_ones"].append(i)
                if plan.stop >= L and any(t for n, t in flags.items() if not FZ.never_trainable(n)):
                    out["no_encoder_layer_trainable"].append(i)
            if lora is not None:
                out["adapters_on_frozen_base" if base_frozen(flags) else "adapters_on_trainable_base"].append(i)
                if lora["layers"] != tuple(range(L)):
                    out["adapters_on_a_subset_of_layers"].append(i)
                dense = [t for t in lora["targets"] if t in LORA_DENSE_PATHS]
                if dense:
                    out["dense_targets"].append(i)
                    if "intermediate" in dense:
                        out["ffn_up_adapter"].append(i)
                    if not any(t in LORA_QKV for t in lora["targets"]):
                        out["dense_only_layer"].append(i)
            steps += kind == "train"
        elif kind == "unfreeze" and steps:
            out["unfreeze_behind_steps"].append(i)
            if since_freeze is not None and "train" not in since_freeze and (set(since_freeze) & {"eval", "accumulate"}):
                out["unfreeze_without_a_step_since_the_freeze"].append(i)      # (a forward read the frozen flags, no step zero-filled the spans)
        elif kind == "add_lora":
            if last_lora is not None and lora["r"] != last_lora["r"]:
                out["rank_changes"].append(i)
            if last_lora is not None and lora["targets"] != last_lora["targets"]:
                out["targets_change"].append(i)
        elif kind in ("merge_lora", "remove_lora", "reload_lora"):
            out[kind.split("_")[0]].append(i)
        if lora is not None:
            last_lora = lora
        if kind == "freeze":
            since_freeze = []
        elif kind == "unfreeze":
            since_freeze = None
        elif since_freeze is not None and kind not in MUTATIONS:
            since_freeze.append(kind)
    return out


def top_layer_is_dense(item, cfg, device="cpu"):
    """Whether a training item's top encoder layer runs the DENSE backward, from the batch alone (model._EncoderFn._sparse_rows: the
    sparse path needs 4 (n + 3 B) <= ra; n = MLM-labelled rows, ra = the rows backward visits -- tests/test_session_twin_gpu.py::_counts)."""
    b = batch(item[1], item[2], cfg, device)
    B = b["input_ids"][0].shape[0]
    am = b["attention_mask"]
    masks = [am[0] != 0] + [torch.cat((m[0] != 0, m[1][:, :, 0] != 0), 1) for m in am[1:]]
    n = ra = 0
    for mask, lab in zip(masks, b["masked_labels"]):
        pos = torch.arange(1, mask.shape[1] + 1, device=mask.device)
        on = (lab >= 0) & (lab < cfg["vocab"])
        n += int(on.sum())
        ra += int(torch.maximum((mask * pos).amax(1), (on * pos).amax(1)).sum())
    return 4 * (n + 3 * B) > ra


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
    at which the transition happens (empty = missing).  Mutations have no shape: the indices count the batch items of the script."""
    script = [it for it in script if it[0] not in MUTATIONS]
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
    (mode, deterministic mode, launch paths, short cuts, loss options), ``{name: requires_grad}`` and the adapter record (``model._lora``
    or None; the adapter tensors are in the state dict).  Nothing of what the session merely caches.  An optimizer that has not been
    bound yet (fresh behind a mutation) gives m / v / ema None."""
    from msa_amd import ops
    osd = opt.state_dict()
    return dict(model={k: v.detach().clone() for k, v in model.state_dict().items()},
                opt={k: (v.detach().clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in osd.items()},
                groups=[{k: copy.deepcopy(v) for k, v in g.items() if k != "params"} for g in opt.param_groups],
                opt_kw=dict(mode={0: "hf", 1: "torch"}[opt.mode], lazy_zero=opt.lazy_zero, grad_scale=opt.grad_scale),
                sched=dict(warmup=sched.warmup, total=sched.total, last_step=sched.last_step),
                seed=(model._seed, model._calls), training=model.training, je_training=model.bert.jointEmbeddings.training,
                deterministic=ops.deterministic(), switches=_switches(model), max_norm=None,
                flags={n: bool(p.requires_grad) for n, p in model.named_parameters()}, lora=copy.deepcopy(getattr(model, "_lora", None)))


class Session:
    """One model, one optimizer (EMA on, clipping), one warm-up schedule.  ``build``: tests.test_model_gpu.build."""

    def __init__(self, cfg, build, *, seed=29, lr=2e-3, weight_decay=0.01, ema_decay=0.9, warmup=4, total=40, max_norm=1.0, train=True,
                 setup=None, _snapshot=None, _overrides=None):
        from msa_amd.optim import AdamW, LinearWarmupSchedule
        self.cfg, self.build, self.max_norm, self.setup = cfg, build, max_norm, setup
        self.lr, self.weight_decay = lr, weight_decay
        self.moves = None                        # a list: finish() appends (trainable names a step moved, frozen names it moved)
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
            if snap.get("lora"):
                m.add_lora(**snap["lora"], freeze_base=False)
            m.load_state_dict(snap["model"])
            named = dict(m.named_parameters())
            assert set(named) == set(snap.get("flags", named)), "the twin's parameter names are not the snapshot's"
            for n, t in snap.get("flags", {}).items():
                named[n].requires_grad_(t)
            for k, v in snap["switches"].items():
                if k in SWITCH_BUFFERS:
                    if v is not None or getattr(m, k, None) is not None:
                        setattr(m, k, None if v is None else v.clone())
                elif k not in ("num_labels", "multi_label") or getattr(m, k) != v:
                    setattr(m, k, v)
            m.train(snap["training"])
            m.bert.jointEmbeddings.train(snap["je_training"])
            m._seed, m._calls = snap["seed"]
            for k, v in (_overrides or {}).items():
                setattr(m, k, v)
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
        """Behind the backward pass of a training item: the whole gradient buffer -- on the clone, the spans of the frozen parameters
        zero-filled (``grad_mask``; see the module docstring) --, and for ``train`` the optimizer step."""
        f = self.model._flat
        g = res["grads"] = f.grads.clone()
        mask = grad_mask(self.model.__dict__.get("_tplan"))
        assert mask == f.frozen, "the storage's frozen set is not the one of the plan this step ran under"
        zero_spans(g, f.offset, f.numel, mask)
        if item[0] == "train":
            before = f.params.clone() if self.moves is not None else None
            res["norm"] = self.opt.clip_grad_norm_(self.max_norm).detach().clone()
            self.opt.step()
            self.sched.step()
            self.opt.zero_grad()
            self._after_step(res)
            if before is not None:
                from msa_amd.freeze import never_trainable
                moved = {n for n in f.order if f.numel[n] and not torch.equal(before[f.offset[n]:f.offset[n] + f.numel[n]], f.params[f.offset[n]:f.offset[n] + f.numel[n]])}
                still = {n for n, p in f.named.items() if not p.requires_grad or never_trainable(n)}
                self.moves.append((sorted(moved - still), sorted(moved & still)))
        return res

    # ---- a mutation
    def mutate(self, item):
        """A mutation item, at an optimizer-step boundary; the optimizer rule of the module docstring."""
        kind, shape, _seed, options = item
        assert kind in MUTATIONS and shape is None, item
        m = self.model
        if kind == "freeze":
            m.freeze(**options)
            return
        if kind == "unfreeze":
            m.unfreeze()
        elif kind == "add_lora":
            assert "seed" in options
            m.add_lora(**options)
        elif kind == "merge_lora":
            m.merge_lora()
        elif kind == "remove_lora":
            m.remove_lora()
        else:
            fb = base_frozen({n: p.requires_grad for n, p in m.named_parameters()})
            sd = m.lora_state_dict()
            m.remove_lora()
            m.load_lora_state_dict(sd, freeze_base=fb)
        self.rebuild_optimizer()

    def rebuild_optimizer(self):
        """A fresh AdamW on the model's parameters as they are now (unbound until its first use), the EMA restarted, the schedule re-bound
        at its position.  Returns the optimizer it replaces."""
        from msa_amd.optim import AdamW, LinearWarmupSchedule
        old, s = self.opt, self.sched
        self.opt = AdamW(self.model.parameters(), lr=self.lr, weight_decay=self.weight_decay, mode={0: "hf", 1: "torch"}[old.mode])
        self.opt.ema(old._ema_decay, warmup=old._ema_warmup)
        self.opt.lazy_zero, self.opt.grad_scale = old.lazy_zero, old.grad_scale
        self.sched = LinearWarmupSchedule(self.opt, s.warmup, s.total)
        self.sched.last_step = s.last_step
        self.sched._apply()
        return old

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


def twin(snap, cfg, build, overrides=None):
    """A fresh Session -- new model, new flat storage, new optimizer and schedule -- that holds exactly the snapshot's state: the model
    built, the adapters of the record added (``freeze_base=False``), the state dict loaded, every ``requires_grad`` flag set by name, and
    only then the flat storage and the optimizer.  ``overrides``: model switches set on top of the snapshot's ({"composite_layers": False})."""
    return Session(cfg, build, _snapshot=snap, max_norm=snap["max_norm"], _overrides=overrides)


def play(sess, script, enter=None, around=None, snapshots=True):
    """The long-lived run: every item in turn on ``sess``.  Returns (results, snapshots): snapshots[i] = the state in front of item i
    where item i is the first batch item behind an optimizer-step boundary (item 0, every item behind a ``train``, and the first item
    behind a run of mutations); a mutation's result is None.
    ``enter(i)``: a context manager for item i (a stream); ``around[i]``: (``around_step``, ``after_backward``) of item i."""
    results, snaps = [], {}
    for i, item in enumerate(script):
        with (enter(i) if enter is not None else contextlib.nullcontext()):
            if item[0] in MUTATIONS:
                sess.mutate(item)
                results.append(None)
                continue
            if snapshots and (i == 0 or script[i - 1][0] == "train" or script[i - 1][0] in MUTATIONS):
                snaps[i] = sess.snapshot()
                snaps[i]["max_norm"] = sess.max_norm
            results.append(sess.run(item, *(around or {}).get(i, ())))
    return results, snaps


def check_against_twins(results, snaps, script, cfg, build, overrides=None):
    """Every item of the long-lived run against a fresh twin of the last boundary in front of it.  The TRAINING items since that boundary
    are replayed on one twin that runs nothing else (an ``accumulate`` item together with the ``train`` item that consumes it, never the
    inference items in between); every inference item gets a twin of its own that replays the ``accumulate`` items in front of it (they
    move the dropout seed counter and the gradients, which an inference call must not read) and then the item.  Returns the number of
    items compared: the caller asserts it is the number of the script's batch items (mutations are not replayed: every snapshot is taken
    behind them).  ``overrides``: see ``twin``."""
    compared, lay = 0, None
    starts = sorted(snaps)
    for n, s0 in enumerate(starts):
        s1 = starts[n + 1] if n + 1 < len(starts) else len(script)
        t = twin(snaps[s0], cfg, build, overrides)
        lay = t.layout()
        acc = []
        for i in range(s0, s1):
            item = script[i]
            if item[0] in MUTATIONS:
                continue
            if item[0] in TRAINING:
                assert_same_bits(results[i], t.run(item), where(i, item) + " against its fresh twin", lay)
                acc.append(item)
            else:
                t2 = twin(snaps[s0], cfg, build, overrides)
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
