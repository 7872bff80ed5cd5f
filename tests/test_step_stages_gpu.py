"""Every launch of a real training step recomputed in float64 from its own recorded operands (tests/step_stages.py), in situ: the
arguments the MODEL passes -- leading dimensions, row maps, row limits, split layouts, dropout sites, residuals, saved activations,
transposed weight copies, gradient buffers -- judged by each kernel family's own reference bound and by exact dataflow comparisons.

Two small configurations (A: hidden 128, the generic LayerNorm kernels; B: hidden 256, the lean ones; the composite test's batch: sequences
of 24 / 224 / 154 rows, unequal pair lengths, several 64-row query tiles, ragged last tiles, padded keys, few-row GEMMs in the sparse top
layer, split-K, two producers of the tied decoder gradient), eval and train mode, short cuts on and off, a second micro-batch, a step
behind an optimizer step.  The number of recomputed calls per op kind is asserted from the model's structure (``expected_counts``): a
path that stops going through a spied entry point fails.  The worst ratio to its bound per op kind and case is written through
``tests.test_model_gpu._report("step_stage_parity", ...)``: a record (a copy is kept as profiles/step_stage_parity.json), not a threshold."""
import pytest
import torch

from msa_amd.data import batch_to, synthetic_batch
from tests import step_stages as SS
from tests.test_model_gpu import _report, build

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFG = {"A": dict(hidden=128, layers=2, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0),
       "B": dict(hidden=256, layers=3, heads=4, intermediate=1024, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)}
_PARITY = {}


def _batch(seed=61):
    return batch_to(synthetic_batch(4, 24, 200, 130, dataset="mosei", vocab=4096, seed=seed), DEV)


def _model(cfg, train, shortcuts, seed=29):
    m = build(CFG[cfg], train=train)
    m.manual_seed(seed)
    m.composite_layers = False
    if shortcuts:
        m.defer_wgrads = True            # (what the timed shapes take by themselves: model._auto_defer_wgrads wants a full round of tiles)
    else:
        m.skip_padded_backward = m.sparse_top_layer_backward = m.sparse_mlm_backward = False
        m.defer_wgrads = False
    return m


def _step(m, batch):
    out, _logits = m(**batch)
    out[0].mean().backward()
    return out


def expected_counts(L, shortcuts, steps=1, side=True):
    """Launches per op kind of one forward + backward, from the model's structure (msa_amd/model.py): three passes, two of them joint
    (one pair projection each); per layer 4 + 4 NT GEMMs, 2 + 2 LayerNorms, attention forward and backward; the MLM head 2 + 2 NT GEMMs
    (the dense one: 3 + 2; the sparse one takes split-K for the vocabulary product), its LayerNorm and GELU'; the embedding LayerNorm in
    two launch groups (text pass | joint passes) forward and backward, the joint LayerNorm per joint pass.
    Short cuts on: the sparse top layer takes split-K for its FFN-up gradient, gathers its 8 saved activations, scatters two gradients
    back and asks for the query limit; the MLM head gathers its labelled rows; ALL weight gradients go out in one grouped call (the
    deferred dense ones, the top layer's, the MLM head's two).  Off: one grouped call per layer pair, the MLM head's two through gemm_tn.
    The deferred LayerNorm reduce is not counted here: its workspace grows with the first calls, each growth folds what it holds;
    ``_judge`` asserts that every LayerNorm' call is folded exactly once.
    The seam: one prologue call and one ``pack_i64`` (ids | token types | labels) per forward; the level-launch heads' forward in two
    calls with ``heads_side_stream`` (``side``: levels 1 - 6 prelaunched, level 7 behind the MLM head) and in one without, their backward
    in one call, in front of it ``heads_step_dmlm`` when the six levels go to the side stream; the sparse top layer builds its row list
    with one ``compact_rows``.  ``active_rows`` does not run: the labelled-row list is the prologue's."""
    on = shortcuts
    c = {"embed_gather": 1, "embed_scatter": 1, "pair_proj_fwd": 2, "pair_proj_bwd": 2, "ce_fwd": 1, "ce_bwd": 1, "gelu_bwd": 1,
         "attn_fwd": L, "attn_bwd": L,
         "ln_fwd": 2 * L + 1 + 2 + 2, "ln_bwd": 2 * L + 1 + 2 + 2,
         "gemm_nt": 8 * L + 2 + (1 if on else 2) - (1 if on else 0), "gemm_nt_splitk": 2 if on else 0,
         "gather_rows": 2 if on else 0, "scatter_rows_zero": 1 if on else 0, "attn_q_limit": 1 if on else 0,
         "gemm_tn": 0 if on else 2,
         "prologue": 1, "pack_i64": 1, "compact_rows": 1 if on else 0,
         "heads_step_fwd": 2 if side else 1, "heads_step_dmlm": 1 if side else 0, "heads_step_bwd": 1}
    c["gemm_tn_grouped"] = 1 if on else (L + 1) // 2
    return {k: v * steps for k, v in c.items() if v}


def _judge(calls, m, case, L, shortcuts, steps=1):
    per = SS.recompute_all(calls, m)
    print(case, {k: (n, round(w, 4)) for k, (n, w) in sorted(per.items())})
    passes, sites = SS.check_dataflow(calls, m)
    assert passes == {"fwd": steps, "bwd": steps}, passes
    got = {k: n for k, (n, _w) in per.items() if k != "ln_bwd_reduce"}
    folded = [id(x) for c in calls if c.op == "ln_bwd_reduce" for x in c.meta["calls"]]
    assert sorted(folded) == sorted(id(c) for c in calls if c.op == "ln_bwd"), "a LayerNorm' call folded twice or never"
    assert got == expected_counts(L, shortcuts, steps), (case, got, expected_counts(L, shortcuts, steps))
    tied = SS.check_tied_word_gradient(calls)                   # two producers per backward pass, against the float64 sum over both
    assert len(tied) == steps, tied
    _PARITY[case] = {k: dict(calls=n, worst_ratio=w) for k, (n, w) in sorted(per.items())}
    _PARITY[case]["tied_word_gradient_both_producers"] = dict(calls=steps, worst_ratio=max(tied))
    # (the heads' references' preconditions as this step met them, at the initialisation scale: a record -- tests/test_step_seam_gpu.py
    # chooses inputs that meet them and asserts them)
    _PARITY[case]["heads_preconditions"] = {k: min(c.meta["precondition"][k] for c in calls if k in c.meta.get("precondition", {}))
                                            for k in sorted({k for c in calls for k in c.meta.get("precondition", {})})}
    _report("step_stage_parity", _PARITY)
    return per, sites


@pytest.mark.parametrize("shortcuts", [True, False], ids=["shortcuts", "plain"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_every_launch_of_a_step_is_within_its_reference_bound(cfg, train, shortcuts):
    """Forward + ``out[0].mean().backward()``: every recorded launch of the embeddings, the trunk and the MLM head recomputed and inside
    its reference's bound, the dataflow checks, the call counts; train mode: all three dropouts on, L * 3 + 1 + 2 dropout sites seen."""
    L = CFG[cfg]["layers"]
    m = _model(cfg, train, shortcuts)
    batch = _batch()
    with SS.record(m) as calls:
        _step(m, batch)
    _per, sites = _judge(calls, m, f"{cfg} {'train' if train else 'eval'} {'shortcuts' if shortcuts else 'plain'}", L, shortcuts)
    assert sites == (3 * L + 1 + 2 if train else 0), sites


@pytest.mark.parametrize("cfg", ["A", "B"])
def test_a_second_micro_batch_accumulates_onto_the_first(cfg):
    """Behind an optimizer step (which drops the dense weights' and the tied table's gradients lazily), two micro-batches in train mode,
    short cuts on: the first backward's weight-gradient problems overwrite those buffers, the second's accumulate -- as recorded in
    the flags, and as the values say (each launch recomputed from the W0 it found)."""
    L = CFG[cfg]["layers"]
    from msa_amd.optim import AdamW
    m = _model(cfg, True, True)
    opt = AdamW(m.parameters(), lr=1e-3)
    _step(m, _batch(5))
    opt.step()
    with SS.record(m) as calls:
        _step(m, _batch(61))
        _step(m, _batch(62))
    _judge(calls, m, f"{cfg} two micro-batches", L, True, steps=2)
    flags = SS.check_accumulation(calls, SS.names_of(m))
    lazy = [f"l{i}.g_{k}" for i in range(L) for k in ("Wqkv", "Wo", "W1", "W2")] + ["g_word_pad"]
    for n in lazy:
        assert flags[n] == [False, True], (n, flags[n])
    assert flags["g_Wt"] == [True, True], flags["g_Wt"]          # (the MLM transform's gradient is zeroed by the optimizer itself)


@pytest.mark.parametrize("cfg", ["A", "B"])
def test_the_step_after_an_optimizer_step_reads_the_updated_copies(cfg):
    """A recorded step behind ``optimizer.step()``: the bf16 working copies the forward reads are the UPDATED parameters rounded to bf16
    and every ``W*T`` operand of backward their transpose (dataflow check 4) -- and they did change."""
    L = CFG[cfg]["layers"]
    from msa_amd.optim import AdamW
    m = _model(cfg, True, True)
    opt = AdamW(m.parameters(), lr=1e-2)
    _step(m, _batch(5))
    before = m._lw[0]["W1T"].clone()
    opt.step()
    with SS.record(m) as calls:
        _step(m, _batch(61))
    _judge(calls, m, f"{cfg} after optimizer.step", L, True)
    assert not torch.equal(before, m._lw[0]["W1T"])


def test_the_recorder_changes_nothing():
    """Deterministic mode, configuration A, train mode: losses and the whole flat gradient buffer of the step bit-identical with and
    without the recorder (the per-launch path both times)."""
    from msa_amd import ops
    was = ops.deterministic()
    res = []
    try:
        ops.set_deterministic(True)
        for rec in (False, True):
            m = _model("A", True, True)
            if rec:
                with SS.record(m):
                    out = _step(m, _batch())
            else:
                out = _step(m, _batch())
            torch.cuda.synchronize()
            res.append(([out[i].detach().clone() for i in (0, 4, 5, 6)], m._flat.grads.clone()))
    finally:
        ops.set_deterministic(was)
    for x, y in zip(res[0][0], res[1][0]):
        assert torch.equal(x, y), (float(x), float(y))
    assert torch.equal(res[0][1], res[1][1])
