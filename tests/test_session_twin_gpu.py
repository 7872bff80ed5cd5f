"""One long-lived model against fresh twins (tests/session_twin.py), bit for bit, over changing batch shapes, interleaved modes,
inference between a forward pass and its backward pass, two models in one process and non-default streams; and, in the default
(non-deterministic) mode, recorded steps of a long-lived model against float64 (tests/step_stages.py).

The two small configurations of tests/test_step_stages_gpu.py (A: hidden 128, the generic LayerNorm kernels; B: hidden 256, the lean
ones).  Everything under (a) - (e) runs in deterministic mode and compares with ``torch.equal``; every item of every script is compared
and the count is asserted.  What each test holds of the cross-step state: DESIGN.md S3.4, "Across steps"."""
import contextlib

import pytest
import torch

from msa_amd.data import batch_to, synthetic_batch      # noqa: F401  (the batch helpers behind session_twin.batch)
from tests import session_twin as ST
from tests import step_stages as SS
from tests.test_model_gpu import _report, build
from tests.test_step_stages_gpu import CFG, expected_counts

pytestmark = pytest.mark.gpu

_PARITY = {}


@contextlib.contextmanager
def _deterministic(on=True):
    from msa_amd import ops
    was = ops.deterministic()
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(was)


def _all_dropouts_on(m):
    c = m.config
    assert m.training and m.bert.jointEmbeddings.training
    assert c.hidden_dropout_prob > 0 and c.attention_probs_dropout_prob > 0 and m.bert.jointEmbeddings.dropout_prob > 0


# ---------------------------------------------------------------------------------------------- (a) changing shapes, (g) leftovers
@pytest.mark.parametrize("prologue", ["default", "async"])
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_a_long_lived_model_equals_fresh_twins_over_changing_shapes(cfg, prologue):
    """The main script (growth past everything seen, shrinkage right behind the largest batch, repeats, another batch size at the same
    lengths, exchanged pair lengths, a sequence over 256 rows, one sample with labels on the pair rows, a batch without padding;
    two micro-batches of different shape per optimizer step), train mode with all three dropouts, AdamW with EMA, clipping and
    warm-up, short cuts and prologue at their defaults: at every optimizer-step boundary the long-lived run's losses, scores, whole
    gradient buffer, parameters, working copies, m, v and EMA are those of a twin built fresh from the previous boundary.
    ``async``: the same with ``model.async_prologue = True`` (the twins inherit the switch) -- the prologue's two alternating buffer
    sets are re-allocated only when too small, so the smaller batches run in the larger batches' buffers; the script keeps that
    switch's contract (static batches, complete before the first forward; every forward followed by its backward)."""
    script = ST.main_script()
    for it in script:
        ST.batch(it[1], it[2], CFG[cfg])
    torch.cuda.synchronize()
    with _deterministic():
        s = ST.Session(CFG[cfg], build, setup=(lambda m: setattr(m, "async_prologue", True)) if prologue == "async" else None)
        assert bool(getattr(s.model, "async_prologue", False)) == (prologue == "async")
        _all_dropouts_on(s.model)
        results, snaps = ST.play(s, script)
        assert sorted(snaps) == [0, 2, 4, 6, 8]
        assert ST.leftovers(s.model) == []
        steps = [r["params"] for r in results if "params" in r]
        assert len(steps) == 5 and all(not torch.equal(a, b) for a, b in zip(steps, steps[1:])), "the optimizer steps must move the parameters"
        compared = ST.check_against_twins(results, snaps, script, CFG[cfg], build)
        assert compared == len(script) == 10
        assert ST.leftovers(s.model) == []
        if prologue == "async":
            sizes = [ST.shape_facts(it[1])["prologue"] for it in script]
            for k in (0, 1):                 # each set as large as the largest batch it served (calls 1, 3, .. / 2, 4, ..), and no larger
                f, i = s.model._pro_bufs[k]
                mine = sizes[1 - k::2] if k else sizes[1::2]
                assert (f.numel(), i.numel()) == (max(x[0] for x in mine), max(x[1] for x in mine)), (k, f.numel(), i.numel())


# ---------------------------------------------------------------------------------------------- (b) modes interleaved
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_inference_between_train_steps_changes_nothing_and_sees_the_current_weights(cfg):
    """train, predict, train, predict_tokens, eval, ema_eval, predict_attention, train on one model, another shape at every item: every
    item's returned tensors are its fresh twin's -- the twin of a training item never ran the inference items in between (so none of
    them may move the dropout seed counter, the gradients, the prologue's buffers or the working copies), the twin of an inference
    item holds the weights of the last optimizer step (so the item read the refreshed copies, and the EMA swap came back bit for bit)."""
    script = ST.MODES_SCRIPT
    with _deterministic():
        s = ST.Session(CFG[cfg], build)
        results, snaps = ST.play(s, script)
        assert sorted(snaps) == [0, 1, 3]
        compared = ST.check_against_twins(results, snaps, script, CFG[cfg], build)
        assert compared == len(script) == 8
        assert not s.opt._swapped and ST.leftovers(s.model) == []
        # the averaged weights differ from the trained ones behind two steps: ema_eval really ran on other weights than eval would have
        assert not torch.equal(s.opt._ema, s.model._flat.params)


# ---------------------------------------------------------------------------------------------- (c) inference between forward and backward
X, X2, Y, Z = ("accumulate", (4, 24, 200, 130), 961, {}), ("accumulate", (3, 20, 60, 40), 962, {}), ("eval", (6, 30, 260, 90), 963, {}), \
    ("predict", (2, 12, 30, 30), 964, {})


@pytest.mark.parametrize("graphs", [1, 2], ids=["one_graph", "two_graphs"])
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_inference_between_a_forward_pass_and_its_backward_pass(cfg, graphs):
    """Behind one optimizer step: forward of X (and of X2: two graphs in flight) with grad, a no_grad eval forward of Y (a larger
    shape), predict on Z (a smaller one), then backward (of the sum).  Losses, scores and the whole gradient buffer are those of a twin
    that runs the forward passes and the backward pass with nothing in between; Y's and Z's results those of a twin that ran only them."""
    with _deterministic():
        s = ST.Session(CFG[cfg], build)
        s.run(("train", (5, 24, 200, 170), 960, {}))
        snap = s.snapshot()
        snap["max_norm"] = s.max_norm
        lay = s.layout()

        def passes(sess, between):
            outs, res = [], {}
            for k, item in enumerate((X, X2)[:graphs]):
                o, r = sess.begin(item, f"x{k}.")
                outs.append(o)
                res.update(r)
            mid = [sess.run(it) for it in between]
            loss = outs[0][0].mean() if graphs == 1 else outs[0][0].mean() + outs[1][0].mean()
            loss.backward()
            return sess.finish(X, res), mid

        got, mid = passes(s, (Y, Z))
        assert ST.leftovers(s.model) == []
        want, _ = passes(ST.twin(snap, CFG[cfg], build), ())
        assert len(got) == 11 * graphs + 1, sorted(got)                       # 10 returned tensors + the logits per pass, the gradients
        ST.assert_same_bits(got, want, f"forward x {graphs}, eval forward, predict, backward -- against forward x {graphs}, backward", lay)
        t2 = ST.twin(snap, CFG[cfg], build)
        for k, it in enumerate((Y, Z)):
            ST.assert_same_bits(mid[k], t2.run(it), ST.where(k, it) + " between forward and backward")


# ---------------------------------------------------------------------------------------------- (d) two models, one process
_TWO = {"A": [("train", s_, 970 + i, {}) for i, s_ in enumerate([(3, 20, 60, 40), (6, 30, 260, 90), (2, 12, 30, 30), (4, 24, 200, 130), (5, 24, 170, 200)])],
        "B": [("train", s_, 980 + i, {}) for i, s_ in enumerate([(5, 24, 200, 170), (2, 12, 30, 30), (6, 30, 260, 90), (3, 20, 60, 40), (4, 24, 200, 130)])]}


def test_two_models_in_one_process_do_not_see_each_other():
    """Model A (hidden 128) and model B (hidden 256), each long-lived with its own optimizer, share the process-global caches
    (LayerNorm' workspace, slabs, heads sync words, side streams): items 0 - 2 as whole steps in turn A, B, A, B, ... at changing shapes,
    item 3 as forward A, forward B, ONE backward of lossA + lossB, item 4 as forward A, forward B, backward A, backward B.  Every
    result of either model is bit-equal to the same model playing its five items alone."""
    with _deterministic():
        alone = {k: ST.play(ST.Session(CFG[k], build), _TWO[k], snapshots=False)[0] for k in ("A", "B")}
        s = {k: ST.Session(CFG[k], build) for k in ("A", "B")}
        got = {"A": [], "B": []}
        for i in range(3):
            for k in ("A", "B"):
                got[k].append(s[k].run(_TWO[k][i]))
        for i, joint in ((3, True), (4, False)):
            fw = {k: s[k].begin(_TWO[k][i]) for k in ("A", "B")}
            if joint:
                (fw["A"][0][0].mean() + fw["B"][0][0].mean()).backward()
            else:
                for k in ("A", "B"):
                    fw[k][0][0].mean().backward()
            for k in ("A", "B"):
                got[k].append(s[k].finish(_TWO[k][i], fw[k][1]))
        compared = 0
        for k in ("A", "B"):
            lay = s[k].layout()
            for i, item in enumerate(_TWO[k]):
                ST.assert_same_bits(got[k][i], alone[k][i], f"model {k} beside the other, {ST.where(i, item)} -- against model {k} alone", lay)
                compared += 1
        assert compared == 10
        for k in ("A", "B"):
            assert ST.leftovers(s[k].model) == [], k
            assert not torch.equal(got[k][3]["params"], got[k][4]["params"])
        from msa_amd import ops
        assert len([k for k in ops._side_streams if k[0] == "heads"]) == 1, "one heads side stream serves both models"


# ---------------------------------------------------------------------------------------------- (e) streams
@pytest.mark.parametrize("queue", [False, True], ids=["static_tiles", "tile_queue"])
def test_steps_under_user_streams_equal_the_default_stream(queue):
    """The first four items of the main script (a) under ONE non-default stream, (b) with the items in turn on TWO user streams,
    ``s_next.wait_stream(s_prev)`` between them: bit-equal to the run on the default stream, with the NT GEMM's dynamic tile queue off
    and on (one queue per stream, found and left zeroed)."""
    from msa_amd import ops
    script = ST.main_script(4)
    was = ops.dynamic_tile_queue
    try:
        ops.dynamic_tile_queue = queue
        with _deterministic():
            want, _ = ST.play(ST.Session(CFG["A"], build), script, snapshots=False)
            torch.cuda.synchronize()
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            for name, streams in (("one user stream", (s1, s1)), ("two user streams in turn", (s1, s2))):
                main = torch.cuda.current_stream()
                prev = [main]

                @contextlib.contextmanager
                def enter(i):
                    st = streams[i % 2]
                    st.wait_stream(prev[0])
                    prev[0] = st
                    with torch.cuda.stream(st):
                        yield

                with torch.cuda.stream(streams[0]):                 # (the model, its flat storage and its optimizer are built there too)
                    streams[0].wait_stream(main)
                    sess = ST.Session(CFG["A"], build)
                got, _ = ST.play(sess, script, enter=enter, snapshots=False)
                main.wait_stream(prev[0])
                torch.cuda.synchronize()
                lay = sess.layout()
                for i, item in enumerate(script):
                    ST.assert_same_bits(got[i], want[i], f"{name}, {ST.where(i, item)} -- against the default stream", lay)
                assert len(got) == len(script) == 4
                assert ST.leftovers(sess.model) == []
                # the steps really ran there: each user stream has per-stream state of its own in the process-global caches
                keyed = {k[1] for c in (ops._heads_sync, ops._slab_cache, ops._ws_cache, ops._lnd_cache) for k in c}
                assert {st.cuda_stream for st in streams} <= keyed, (name, keyed)
            if queue:
                used = {k[1] for k in ops._tile_queues}
                assert len(used) >= 3, "the default stream and both user streams have a tile queue of their own"
    finally:
        ops.dynamic_tile_queue = was


# ---------------------------------------------------------------------------------------------- (f) default mode, against float64
_RECORDED = {5: "item 6: the step_stages batch behind growth and shrinkage", 6: "item 7: one sample, labels on the pair rows",
             8: "item 9: a repeated shape"}


def _counts(L, cfg, item):
    """``expected_counts`` of tests/test_step_stages_gpu.py (short cuts on) for a script item, from the model's structure and the batch
    alone.  Its table is the step whose top encoder layer runs its backward on the few rows that carry a loss; the model takes that
    path when 4 (n + 3 B) <= ra (model._EncoderFn._sparse_rows; n = MLM-labelled rows, 3 B [CLS] rows, ra = the rows backward visits:
    per sequence max(unmasked keys, last labelled position + 1), the prologue's ``valid``), and the MLM head its few-row path when
    2 n <= rows.  Item 7 -- one sample, P == T, so the text labels are repeated on the pair rows: 40 rows -- has too many labelled rows
    for its few rows: its top layer runs the DENSE backward.  What the sparse top layer accounts for in the table then goes: its FFN-up
    input gradient is a plain NT GEMM instead of a split-K one, the gather of its 8 saved activations, the scatter back to full height
    and the query limit do not exist."""
    b = ST.batch(item[1], item[2], cfg)
    f = ST.shape_facts(item[1])
    B, T = b["input_ids"][0].shape
    am = b["attention_mask"]
    masks = [am[0] != 0] + [torch.cat((m[0] != 0, m[1][:, :, 0] != 0), 1) for m in am[1:]]
    n = ra = 0
    for mask, lab in zip(masks, b["masked_labels"]):
        assert mask.shape == lab.shape
        pos = torch.arange(1, mask.shape[1] + 1, device=mask.device)
        on = (lab >= 0) & (lab < cfg["vocab"])
        n += int(on.sum())
        ra += int(torch.maximum((mask * pos).amax(1), (on * pos).amax(1)).sum())
    assert ra <= f["rows"] and 2 * n <= f["rows"], "the MLM head's dense backward is not a case of this table"
    dense_top = 4 * (n + 3 * B) > ra
    c = expected_counts(L, True)
    if dense_top:
        c["gemm_nt"] += 1
        c["gemm_nt_splitk"] -= 1
        c["gather_rows"] -= 1
        del c["scatter_rows_zero"], c["attn_q_limit"], c["compact_rows"]
    return c, dense_top


def _judge(calls, m, case, L, cfg, item):
    """tests/test_step_stages_gpu.py::_judge for a step of the session: every launch inside its own family's bound (SS.recompute_all raises
    otherwise), the dataflow checks, every LayerNorm' call folded exactly once, the call counts, the tied decoder gradient."""
    per = SS.recompute_all(calls, m)
    print(case, {k: (n, round(w, 4)) for k, (n, w) in sorted(per.items())})
    passes, sites = SS.check_dataflow(calls, m)
    assert passes == {"fwd": 1, "bwd": 1}, passes
    assert sites == 3 * L + 1 + 2, sites
    got = {k: n for k, (n, _w) in per.items() if k != "ln_bwd_reduce"}
    folded = [id(x) for c in calls if c.op == "ln_bwd_reduce" for x in c.meta["calls"]]
    assert sorted(folded) == sorted(id(c) for c in calls if c.op == "ln_bwd"), "a LayerNorm' call folded twice or never"
    want, dense_top = _counts(L, cfg, item)
    assert got == want, (case, got, want)
    assert dense_top == (item[1][0] == 1), "of the recorded items, the one-sample batch alone runs the dense top-layer backward"
    tied = SS.check_tied_word_gradient(calls)
    assert len(tied) == 1, tied
    _PARITY[case] = {k: dict(calls=n, worst_ratio=w) for k, (n, w) in sorted(per.items())}
    _PARITY[case]["tied_word_gradient_both_producers"] = dict(calls=1, worst_ratio=max(tied))
    _report("session_twin_parity", _PARITY)
    return SS.check_accumulation(calls, SS.names_of(m))


@pytest.mark.parametrize("item", sorted(_RECORDED), ids=["item6", "item7", "item9"])
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_a_recorded_step_of_a_long_lived_model_is_within_its_reference_bounds(cfg, item):
    """The main script in the DEFAULT mode (fp32 atomics) on one long-lived model, per-launch path (``composite_layers = False``; all
    weight gradients in the one deferred call, as the timed shapes take it and tests/test_step_stages_gpu.py sets it), up to item 6, 7
    or 9, whose step is recorded and judged as a fresh model's step is -- every launch recomputed in float64 from its own recorded
    operands and inside its family's bound, the dataflow checks, the call counts -- behind five, six or eight earlier steps at other
    shapes and two to four optimizer steps.  (One case per recorded item: the float64 recomputation is what takes the time.)  The first
    backward behind an optimizer step overwrites the lazily dropped gradients, the second accumulates."""
    L = CFG[cfg]["layers"]
    script = ST.main_script(item + 1)

    def setup(m):
        m.composite_layers = False
        m.defer_wgrads = True

    lazy = [f"l{i}.g_{k}" for i in range(L) for k in ("Wqkv", "Wo", "W1", "W2")] + ["g_word_pad"]
    flags = {}
    with _deterministic(False):
        s = ST.Session(CFG[cfg], build, setup=setup)
        _all_dropouts_on(s.model)
        judge = lambda calls: flags.__setitem__(item, _judge(calls, s.model, f"{cfg} {_RECORDED[item]}", L, CFG[cfg], script[item]))
        results, _ = ST.play(s, script, around={item: (SS.record, judge)}, snapshots=False)
    assert sorted(flags) == [item] and len(results) == item + 1
    first = script[item][0] == "accumulate"                  # item 6 is the SECOND micro-batch of its step, items 7 and 9 the first
    assert first == (item != 5)
    for n in lazy:
        assert flags[item][n] == [not first], (item, n, flags[item][n])
    assert all(bool(torch.isfinite(r["out0"])) for r in results)
