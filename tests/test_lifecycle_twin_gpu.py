"""The fine-tuning lifecycle of ONE long-lived model against fresh twins (tests/session_twin.py), bit for bit: parameters frozen and
released again, adapters added on one rank and later on another, saved and loaded, merged so that no encoder layer is trainable, removed
-- with the batch shape changing at every item and the inference paths in between (``ST.freeze_script`` / ``ST.lora_script``); and the same
with adapters on the dense seams (``ST.dense_lora_script``: all six targets behind steps, two micro-batches onto their gradients, reload,
merge, another rank without dense targets, then dense adapters alone on the top layer next to composite-path layers, ``predict`` through
the [CLS]-only top layer on gathered rows).

Deterministic mode, ``torch.equal`` throughout; every batch item of every script is compared and the count is asserted.  Two
configurations: F = tests/test_freeze_gpu.py's (hidden 128, four layers, the generic LayerNorm kernels) and B of
tests/test_step_stages_gpu.py (hidden 256, three layers, the lean ones).  What each test holds of the state that lives across steps:
DESIGN.md S3.4, "Across steps"; the optimizer rule behind a mutation and the one masked part of the gradient buffer:
tests/session_twin.py."""
import contextlib

import pytest
import torch

from tests import session_twin as ST
from tests.test_freeze_gpu import CFG as CFG_F
from tests.test_model_gpu import build
from tests.test_step_stages_gpu import CFG as _CFG_AB

pytestmark = pytest.mark.gpu

CFG = {"F": CFG_F, "B": _CFG_AB["B"]}
SCRIPTS = {"freeze": ST.freeze_script, "lora": ST.lora_script, "dense": ST.dense_lora_script}
_LONG = {}


@pytest.fixture(autouse=True)
def _deterministic():
    from msa_amd import ops
    was = ops.deterministic()
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(was)


def _script(cfg, name):
    return SCRIPTS[name](CFG[cfg]["layers"])


def _batch_items(script):
    return [it for it in script if it[0] not in ST.MUTATIONS]


def _prepare(cfg, script):
    for it in _batch_items(script):
        ST.batch(it[1], it[2], CFG[cfg])
    torch.cuda.synchronize()


def _long(cfg, name):
    """The long-lived run of a script at the default settings (composite layer path), played once per process: (script, results,
    snapshots).  Every optimizer step moved at least one trainable parameter and no frozen one; nothing is left behind."""
    key = (cfg, name)
    if key not in _LONG:
        script = _script(cfg, name)
        assert ST.misplaced_mutations(script) == []
        _prepare(cfg, script)
        s = ST.Session(CFG[cfg], build)
        s.moves = []
        assert not hasattr(s.model, "composite_layers") and not getattr(s.model, "async_prologue", False)
        assert ST.leftovers(s.model) == []
        results, snaps = ST.play(s, script)
        assert ST.leftovers(s.model) == []
        trains = [it for it in script if it[0] == "train"]
        assert len(s.moves) == len(trains) == {"freeze": 7, "lora": 7, "dense": 8}[name]
        for k, (moved, frozen_moved) in enumerate(s.moves):
            assert moved and not frozen_moved, (k, len(moved), frozen_moved[:3])
        if name == "dense":                                            # every step under adapters moved an adapter: trains 1, 2, 3 (all six
            for k in (1, 2, 3, 5, 6):                                  # targets), 5 (key), 6 (intermediate + ffn_output on the top layer)
                assert any(".lora_" in n for n in s.moves[k][0]), (k, s.moves[k][0][:3])
            assert any(".dense.lora_B" in n for n in s.moves[2][0]) and any("intermediate.dense.lora_B" in n for n in s.moves[6][0])
        assert [r is None for r in results] == [it[0] in ST.MUTATIONS for it in script]
        _LONG[key] = (script, results, snaps)
    return _LONG[key]


# ---------------------------------------------------------------------------------------------- 1. each script x each configuration
@pytest.mark.parametrize("name", ["freeze", "lora", "dense"])
@pytest.mark.parametrize("cfg", ["F", "B"])
def test_a_long_lived_model_equals_fresh_twins_over_its_fine_tuning_lifecycle(cfg, name):
    """Every batch item of the script on the long-lived model -- losses, scores, the gradient buffer (frozen spans masked on the clone),
    parameters, working copies, m, v, EMA, what predict / predict_tokens / predict_attention / the EMA swap return -- is that of a twin
    built fresh from the snapshot of the last boundary: the model with the snapshot's adapters and flags, a new flat storage, a new
    optimizer.  Behind a mutation other than ``freeze`` the snapshot holds an unbound optimizer (m / v / ema None)."""
    script, results, snaps = _long(cfg, name)
    n = len(_batch_items(script))
    assert n == {"freeze": 14, "lora": 13, "dense": 15}[name]
    behind_rebuild = [i for i in snaps if i and script[i - 1][0] in ST.MUTATIONS and script[i - 1][0] != "freeze"]
    assert behind_rebuild and all(snaps[i]["opt"]["m"] is None and snaps[i]["opt"]["ema"] is None and snaps[i]["opt"]["steps"] == 0 for i in behind_rebuild)
    kept = [i for i in snaps if i and script[i - 1][0] == "freeze"]
    assert all(snaps[i]["opt"]["m"] is not None and snaps[i]["opt"]["steps"] > 0 for i in kept) and (kept or name in ("lora", "dense"))
    compared = ST.check_against_twins(results, snaps, script, CFG[cfg], build)
    assert compared == n
    # the scripts' top layers, from the batches: sparse and dense each under "backward ends at the top layer" / under adapters
    names = list(snaps[0]["flags"])                                      # (item 0: a model without adapters)
    assert not any(".lora_" in k for k in names)
    facts = ST.lifecycle_facts(script, names, CFG[cfg]["layers"])
    under = facts["stop_is_top_layer_without_input_gradient"] if name == "freeze" else facts["adapters_on_frozen_base"] + facts["adapters_on_trainable_base"]
    assert {ST.top_layer_is_dense(script[i], CFG[cfg], "cuda") for i in under} == {False, True}
    if name == "dense":
        assert {ST.top_layer_is_dense(script[i], CFG[cfg], "cuda") for i in facts["dense_targets"]} == {False, True}
        assert facts["ffn_up_adapter"] and facts["dense_only_layer"] and facts["merge"] and facts["reload"] and facts["no_encoder_layer_trainable"]
        # the records the snapshots hold are the ones the names give: canonical target order, the twin's add_lora takes them as they are
        states = ST.lifecycle_states(script, names, CFG[cfg]["layers"])
        for i, sn in snaps.items():
            want = states[i][1]
            assert (sn["lora"] is None) == (want is None) and (want is None or {k: sn["lora"][k] for k in want} == want), (i, sn["lora"], want)


# ---------------------------------------------------------------------------------------------- 2. composite C call against per-launch twins
@pytest.mark.parametrize("name", ["freeze", "lora", "dense"])
def test_the_composite_layer_path_equals_per_launch_twins_over_the_lifecycle(name):
    """DESIGN: the composite C call of a layer's backward body is bit-identical to the per-launch path.  The long-lived run at its default
    settings (composite) against twins forced to ``composite_layers = False``, over the changing shapes of a whole script instead of one:
    ``mmbert_layer_bwd`` with ``dx == NULL`` at the layer where backward ends, its cached argument block across storages, and the seam
    to the adapter layers (which always take the per-launch body) -- in the ``dense`` script the layers that dense adapters force onto
    the per-launch body, alone on the top layer above composite layers, and back on the composite path behind ``remove_lora`` / ``merge_lora``."""
    script, results, snaps = _long("F", name)
    compared = ST.check_against_twins(results, snaps, script, CFG["F"], build, overrides={"composite_layers": False})
    assert compared == len(_batch_items(script))


# ---------------------------------------------------------------------------------------------- 3. the prologue on the input stream
def test_the_freeze_script_with_the_prologue_on_the_input_stream():
    """``model.async_prologue = True`` (the twins inherit the switch): static batches, complete before the first forward."""
    cfg = "B"
    script = _script(cfg, "freeze")
    _prepare(cfg, script)
    s = ST.Session(CFG[cfg], build, setup=lambda m: setattr(m, "async_prologue", True))
    assert s.model.async_prologue
    results, snaps = ST.play(s, script)
    assert ST.leftovers(s.model) == []
    assert all(sn["switches"].get("async_prologue") is True for sn in snaps.values())
    compared = ST.check_against_twins(results, snaps, script, CFG[cfg], build)
    assert compared == len(_batch_items(script)) == 14
    assert ST.leftovers(s.model) == []


# ---------------------------------------------------------------------------------------------- 4. two models, one process
def test_two_models_with_different_lifecycles_do_not_see_each_other():
    """Model F plays the freeze script, model B the adapter script, item by item in turn: they share the process-global caches (the fp32
    workspace the split-K GEMM, the grouped column sum and the adapter backward all take; slabs; the LayerNorm' workspace; the side
    streams).  Each is bit-equal to itself playing alone."""
    from msa_amd import ops
    plays = {"F": "freeze", "B": "lora"}
    alone = {k: _long(k, n) for k, n in plays.items()}
    s = {k: ST.Session(CFG[k], build) for k in plays}
    got = {k: [] for k in plays}
    for i in range(max(len(alone[k][0]) for k in plays)):
        for k in plays:
            script = alone[k][0]
            if i < len(script):
                got[k].extend(ST.play(s[k], script[i:i + 1], snapshots=False)[0])
    compared = 0
    for k in plays:
        script, want, _ = alone[k]
        lay = None
        for i, item in enumerate(script):
            if item[0] in ST.MUTATIONS:
                assert got[k][i] is None
                lay = None
                continue
            ST.assert_same_bits(got[k][i], want[i], f"model {k} beside the other, {ST.where(i, item)} -- against model {k} alone", lay)
            compared += 1
        assert ST.leftovers(s[k].model) == [], k
    assert compared == 14 + 13
    assert len({k[1] for k in ops._ws_cache}) >= 1 and len([k for k in ops._side_streams if k[0] == "heads"]) == 1


# ---------------------------------------------------------------------------------------------- 5. a user stream
def test_the_adapter_scripts_training_items_under_a_user_stream_equal_the_default_stream():
    """The mutations and training items of the adapter script under ONE non-default stream (model, storages and optimizers are built
    there too): bit-equal to the default stream."""
    from msa_amd import ops
    cfg = "B"
    script = [it for it in _script(cfg, "lora") if it[0] in ST.MUTATIONS or it[0] in ST.TRAINING]
    _prepare(cfg, script)
    want, _ = ST.play(ST.Session(CFG[cfg], build), script, snapshots=False)
    torch.cuda.synchronize()
    st, main = torch.cuda.Stream(), torch.cuda.current_stream()

    @contextlib.contextmanager
    def enter(i):
        with torch.cuda.stream(st):
            yield

    with torch.cuda.stream(st):
        st.wait_stream(main)
        sess = ST.Session(CFG[cfg], build)
    got, _ = ST.play(sess, script, enter=enter, snapshots=False)
    main.wait_stream(st)
    torch.cuda.synchronize()
    compared = 0
    for i, item in enumerate(script):
        if item[0] in ST.MUTATIONS:
            continue
        ST.assert_same_bits(got[i], want[i], f"one user stream, {ST.where(i, item)} -- against the default stream")
        compared += 1
    assert compared == 8
    assert ST.leftovers(sess.model) == []
    assert st.cuda_stream in {k[1] for k in ops._ws_cache}, "the adapter backward's workspace of the user stream"


# ---------------------------------------------------------------------------------------------- 6. the stale optimizer is refused
def _lora_then(what):
    def f(sess):
        sess.mutate(("add_lora", None, None, dict(r=4, alpha=8.0, targets=("query", "value"), freeze_base=True, seed=5)))
        sess.run(("train", (3, 20, 60, 40), 1202, {}))
        getattr(sess.model, what)()
    return f


def _unfreeze_behind_a_step(sess):
    sess.mutate(("freeze", None, None, dict(embeddings=True, layers=1)))
    sess.run(("train", (3, 20, 60, 40), 1202, {}))
    sess.model.unfreeze()


STALE = {"add_lora": lambda sess: sess.model.add_lora(r=8, targets=("key",), freeze_base=False, seed=5),
         "add_lora_dense": lambda sess: sess.model.add_lora(r=8, targets=("intermediate", "ffn_output"), freeze_base=False, seed=5), "merge_lora": _lora_then("merge_lora"),
         "remove_lora": _lora_then("remove_lora"), "unfreeze": _unfreeze_behind_a_step}


@pytest.mark.parametrize("case", sorted(STALE))
def test_the_optimizer_of_before_is_refused_and_writes_nothing(case):
    """Behind ``add_lora`` / ``merge_lora`` / ``remove_lora`` (the storage was dropped) and behind ``unfreeze`` after a step (one step count
    for all parameters), the optimizer built before raises at ``step()`` once the model has run again -- and neither its own buffers (m,
    v, EMA, step count, the storage it was bound to) nor the model's current storage were written."""
    s = ST.Session(CFG["B"], build)
    s.run(("train", (2, 12, 30, 30), 1201, {}))
    STALE[case](s)
    old, old_flat = s.opt, s.opt._flat
    assert old_flat is not None and old._steps >= 1
    out, _ = s.begin(("accumulate", (2, 12, 30, 30), 1203, {}))
    out[0].mean().backward()
    f = s.model._flat
    assert (f is old_flat) == (case == "unfreeze")
    if case == "add_lora_dense":
        assert any(".dense.lora_A" in n for n in f.order) and not any(".lora_" in n for n in old_flat.order)
    torch.cuda.synchronize()
    owned = dict(m=old._m, v=old._v, ema=old._ema, old_params=old_flat.params, old_half=old_flat.half, old_grads=old_flat.grads,
                 params=f.params, half=f.half, grads=f.grads, halfT=f.halfT)
    before = {k: t.clone() for k, t in owned.items()}
    steps, updates, stale = old._steps, old.ema_updates, set(f.stale)
    with pytest.raises((RuntimeError, NotImplementedError)):
        old.step()
    torch.cuda.synchronize()
    assert (old._steps, old.ema_updates) == (steps, updates) and set(f.stale) == stale
    ST.assert_same_bits({k: t.clone() for k, t in owned.items()}, before, f"behind the refused step() of the optimizer built before {case}")
    assert ST.leftovers(s.model) == []
