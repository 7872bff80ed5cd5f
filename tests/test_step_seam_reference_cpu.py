"""The seam checks of tests/step_stages.py have teeth: a synthetic recorded seam on the CPU at configuration A (hidden 128), B = 4 -- the
step prologue as ``layout_ref.prologue_port`` writes it into one of two persistent buffer sets, an attention call that reads its key bias
and ``kv_len``, the top layer's ``ln2``, the heads' levels as ``heads_ref.restate(emu=True)`` computes them (levels 1 - 6, level 7,
``heads_step_dmlm``, the six backward levels), the MLM losses from ``rowwise_ref``'s cross-entropy emulation, ``ce_bwd``'s ``gscale``, the last
MLM product, ``compact_rows`` and the top layer's ``ln2_bwd`` -- chained through ``step_stages.synth`` with the hand-overs of the real step
(the compact one: labelled rows ‖ first_rows, the [CLS] rows the RNE bf16 of ``dfirst``; the dense one: torch's bf16 ``index_add_``).

The faithful chain passes ``check_seam``, ``recompute`` of every seam op and ``check_producers``; each single change of ``MUTATIONS`` fails,
caught by the check named in ``CAUGHT_BY``, and so does each ``Mutation`` tests/heads_ref.py exports, applied to the emulated levels.

For the value mutations the test also states what the end-to-end comparison would have said (``E2E_INSIDE`` / ``HEAD_E2E_INSIDE``: the
mutated chain's outputs -- the hand-over matrix, ``dfirst`` and the 22 gradients -- against the clean chain's by ``compare_gradients``' 4.5 %
relative error per tensor; measured, worst tensor):

    cls_row_truncated        one [CLS] row by truncation           inside  (0.003 %: today's suite lets it through)
    dfirst_sample0_to_row1   two samples' [CLS] gradients swapped  inside  (0.7 %: likewise)
    dfirst_v_s_swapped       passes v and s swapped                OUTSIDE (121 %)
    cls_added_twice          added twice on the dense path         OUTSIDE (99 %)

Of heads_ref's sixteen mutations five stay inside 4.5 % (``HEAD_E2E_INSIDE``); ``dmlm_over_three`` changes nothing at the step's three
passes (nmlm = 3) and is asserted to be no change."""
import types

import numpy as np
import pytest
import torch

from tests import heads_ref as HR
from tests import layout_ref as LR
from tests import rowwise_ref as R
from tests import step_stages as SS
from tests.test_step_stages_reference_cpu import _Lay

B, H, HEADS, T, PV, PS, V, LDV = 4, 128, 2, 6, 10, 8, 50, 64
LENS = [T, T + PV, T + PS]
SEQ = [S for S in LENS for _ in range(B)]                        # rows per sequence, pass by pass
TOKENS = sum(SEQ)
FIRST = [0] + [int(x) for x in np.cumsum(SEQ)[:-1]]
NSEQ = 3 * B
bf, f32 = torch.bfloat16, torch.float32

MUTATIONS = ("dfirst_v_s_swapped", "dfirst_sample0_to_row1", "cls_row_truncated", "cls_added_twice", "mlm_order_vts", "gscale_stale",
             "first_rows_off_by_one", "y_before_ln2", "grad_to_neighbour_view", "prior_ignored", "kv_len_short", "idx_last_row_missing",
             "prologue_previous_set")
CAUGHT_BY = {"dfirst_v_s_swapped": "compact hand-over", "dfirst_sample0_to_row1": "compact hand-over", "cls_row_truncated": "compact hand-over",
             "cls_added_twice": "dense hand-over", "mlm_order_vts": "mlm losses", "gscale_stale": "gscale", "first_rows_off_by_one": "heads first_rows",
             "y_before_ln2": "heads y", "grad_to_neighbour_view": "heads gradient views", "prior_ignored": "heads_step_bwd",
             "kv_len_short": "prologue: 1 int words differ", "idx_last_row_missing": "compact row list", "prologue_previous_set": "alternating buffers"}
E2E_INSIDE = {"cls_row_truncated": True, "dfirst_v_s_swapped": False, "dfirst_sample0_to_row1": True, "cls_added_twice": False}
HEAD_MUTATIONS = [HR.cpc_csum_dropped(1), HR.cpc_rsum_dropped(2), HR.softmax_over_columns(0), HR.positive_from_neighbour(), HR.beta_in_dS(),
                  HR.speech_labels_from_visual(), HR.drel_rows_shifted(), HR.gate_dP_w1_only(), HR.e_without_relu(), HR.pooler_tanh_grad(),
                  HR.label_tanh_grad_missing(), HR.grad_ignores_d("cpc_zv.net.bias"), HR.grad_overwritten("attn.bias"), HR.gbp_last_row_lost(),
                  HR.dmlm_over_three(), HR.last_granule_dropped()]
# the mutations whose worst output stays inside 4.5 % (measured: 4.4 %, 1.6 %, 2.5 %, 1.6 %, 2.4 %); every other one is outside (13 % and more)
HEAD_E2E_INSIDE = {HR.softmax_over_columns(0).name, HR.beta_in_dS().name, HR.drel_rows_shifted().name, HR.pooler_tanh_grad().name,
                   HR.gbp_last_row_lost().name}
NO_CHANGE = HR.dmlm_over_three().name                            # (dmlm = d alpha / 3 IS the step's formula at its three passes: nmlm = 3)


def _inputs(seed):
    """Masks, labels and logits of one step: text and pair masks with their padding at the end, one labelled row in every other
    sequence (never a [CLS] row), bf16 logits [tokens, LDV]."""
    g = torch.Generator().manual_seed(seed)
    segs = []
    for p in range(3):
        n = torch.randint(3, T + 1, (B,), generator=g)
        segs.append(((torch.arange(T)[None, :] < n[:, None]).float(), p, 0))
        if p:
            P = PV if p == 1 else PS
            n = torch.randint(2, P + 1, (B,), generator=g)
            segs.append(((torch.arange(P)[None, :] < n[:, None]).float(), p, T))
    labels = torch.full((TOKENS,), -100, dtype=torch.int64)
    for s, r0 in enumerate(FIRST):
        if s % 2 == 0:
            labels[r0 + 1 + (s // 2) % 2] = int(torch.randint(0, V, (1,), generator=g))
    logits = (torch.randn(TOKENS, LDV, generator=g) * 2.0).to(bf)
    return segs, labels, logits


def _t32(num):
    return num.v.to(f32)


def seam_chain(mut=None, dense=False, steps=1, head_mutation=None, num_labels=7):
    """(calls, model stub, {name: final tensor}) of ``steps`` synthetic seams under one change (None: the faithful chain)."""
    assert mut is None or mut in MUTATIONS
    case = HR.make_case(B, H, 3, num_labels=num_labels, nmlm=3, d=0.5)
    views = {n: case.prior[n].clone() for n in HR.PARAMS}         # the .grad views: they start at the prior, the steps accumulate
    model = types.SimpleNamespace(head_grad_views=views)
    params = {f: case.params[n] for f, n in SS.HEAD_PARAM.items()}
    sets = [(torch.zeros(NSEQ * 128 + 64), torch.zeros(5 * NSEQ + TOKENS + NSEQ + 3 + 29, dtype=torch.int32)) for _ in range(2)]   # (larger than the extent)
    lay = _Lay(SEQ, HEADS)
    first_rows = torch.tensor(FIRST, dtype=torch.int64)
    calls, out = [], {}
    y_prev = torch.randn(TOKENS, H, generator=torch.Generator().manual_seed(99)).to(bf)
    scal = dict(B=B, H=H, tanh_lo=1 if num_labels == 1 else 0, ncls=0, nmlm=3, alpha=float(np.float32(case.alpha)), beta=float(np.float32(case.beta)),
                ldy=H, loss_kind=0, huber_delta=0.0, label_smoothing=0.0, multi_label=0)

    def emit(op, a, write=None, writes=(), ret=None, stage=None, layer=None, record=None):
        """A call: ``a`` snapshot as the op found it, then ``write()`` runs (the "kernel"), then the operands ``writes`` / ``ret`` again."""
        c = SS.synth(op, a, meta=dict(stage=stage or op, layer=layer, record=record))
        if write is not None:
            write()
        c.post = {k: SS._snap(a[k]) for k in writes}
        c.ret = SS._snap(ret() if callable(ret) else ret)
        calls.append(c)
        return c
    for step in range(steps):
        segs, labels, logits = _inputs(10 + step)
        # ---- the prologue into one of the two persistent sets, and an attention call that reads its outputs
        fb, ib = sets[0 if mut == "prologue_previous_set" else step % 2]
        ref = LR.prologue_port([(m.numpy(), p, o) for m, p, o in segs], LENS, B, labels.numpy(), V)
        wf, wi, _mask = SS.prologue_words(ref, TOKENS, False)
        n = int(ref["words"][NSEQ])
        if mut == "kv_len_short" and step == 0:
            wi = wi.copy()
            wi[5] -= 1
        fl, ints = fb[:wf.size], ib[:wi.size]
        pr = dict(key_bias=fl, kv_len=ints[:NSEQ], valid=ints[NSEQ:2 * NSEQ], idx=ints[5 * NSEQ:5 * NSEQ + TOKENS], words=ints[5 * NSEQ + TOKENS:],
                  all_f=fl, all_i=ints)

        def write_pro():
            fl.copy_(torch.from_numpy(wf))
            ints.copy_(torch.from_numpy(wi.astype(np.int32)))
        emit("prologue", dict(segs=segs, pass_lens=LENS, B=B, labels=labels, vocab=V, device=None, bufs=(fb, ib), rowset=False), write_pro,
             writes=("bufs",), ret=lambda: pr)
        emit("attn_fwd", dict(key_bias=pr["key_bias"], kv_len=pr["kv_len"], layout=lay), layer=0)
        # ---- the top layer's ln2 leaves y; its [CLS] rows are the case's (bf16-representable) rows
        y = y_prev.clone()                                        # (the region holds something else until ln2 writes it)
        y_new = torch.randn(TOKENS, H, generator=torch.Generator().manual_seed(50 + step)).to(bf)
        y_new[first_rows] = case.first.to(bf)
        too_early = SS._snap(y)
        emit("ln_fwd", dict(x=y_prev), lambda: y.copy_(y_new), ret=lambda: (y, None, None), stage="ln2", layer=0)
        rows_h = first_rows.clone()
        if mut == "first_rows_off_by_one":
            rows_h[5] += 1
        # ---- the MLM losses (rowwise_ref's emulation), then the heads' levels (heads_ref's emulation) on the recorded rows
        bounds = torch.tensor([0] + [int(x) for x in np.cumsum([B * S for S in LENS])], dtype=torch.int32)
        ce = R.ce_fwd(logits, labels, V, bounds, 3, emu=True)
        loss = ce["loss"].to(f32)
        case.mlm = loss[[1, 0, 2]].clone() if mut == "mlm_order_vts" else loss.clone()
        case.prior = {} if (mut == "prior_ignored" and step == 1) else {k: v.clone() for k, v in views.items()}
        em = HR.restate(case, emu=True, mutation=head_mutation)
        outs = {k: torch.zeros_like(_t32(em[k])) for k in ("loss", "aux", "out5", "logits", "t_rel", "rel")}
        base = dict(params, y=y, first_rows=rows_h, ap=case.ap_v, ap2=case.ap_s, sent=case.sent, **scal, **outs)
        rec = 1000 + step

        def write_outs(keys):
            for k in keys:
                outs[k].copy_(_t32(em[k]).reshape(outs[k].shape))
        c16 = emit("heads_step_fwd", dict(base, lo=1, hi=6), lambda: write_outs(SS.HEAD_FWD_FINAL), writes=SS.HEAD_FWD_FINAL, record=rec)
        emit("ce_fwd", dict(logits=logits, V=V, labels=labels, seg_bounds=bounds, nseg=3, smoothing=0.0), ret=(loss, torch.ones(4), ce["row_lse"].to(f32)))
        c7 = emit("heads_step_fwd", dict(base, lo=7, hi=7, mlm=case.mlm), lambda: write_outs(("loss", "aux", "out5")),
                  writes=("loss", "aux", "out5") + SS.HEAD_FWD_FINAL, record=rec)
        if mut == "y_before_ln2":                                 # the prelaunched levels read the region before ln2 had written it
            c16.a["y"].t, c16.a["y"]._cpu = too_early.t, None
        # ---- backward: dmlm in-stream, the six levels beside it
        gv = {g: views[nm] for g, nm in SS.HEAD_GRADS.items()}
        if mut == "grad_to_neighbour_view":
            gv["gWq0"], gv["gWq1"] = gv["gWq1"], gv["gWq0"]
        dmlm, scratch, dfirst = torch.full((3,), 0.25), torch.zeros(3), torch.zeros(3 * B, H)
        stale = dmlm.clone()
        bw = dict(base, mlm=case.mlm, dloss=torch.tensor([case.d], dtype=f32), dfirst=dfirst, **gv)
        emit("heads_step_dmlm", dict(bw, dmlm=dmlm, lo=1, hi=6), lambda: dmlm.copy_(_t32(em["dmlm"])), writes=("dmlm",), record=rec)

        def write_bwd():
            dfirst.copy_(_t32(em["dfirst"]))
            scratch.copy_(_t32(em["dmlm"]))
            for nm in HR.PARAMS:
                views[nm].copy_(_t32(em[nm]))
        emit("heads_step_bwd", dict(bw, dmlm=scratch, lo=1, hi=6), write_bwd, writes=("dfirst", "dmlm") + tuple(SS.HEAD_GRADS), record=rec)
        emit("ce_bwd", dict(logits=logits, V=V, labels=labels, seg_bounds=bounds, nseg=3, gscale=stale if mut == "gscale_stale" else dmlm, rows=None),
             ret=torch.zeros(2, LDV).to(bf))
        # ---- the hand-over to the trunk's backward
        idx = pr["idx"][:n]
        df = dfirst.clone()
        dfb = SS.bf16_rne(df)
        g = torch.Generator().manual_seed(70 + step)
        nothing = torch.zeros(1, 1).to(bf)
        if dense:
            dy = torch.zeros(TOKENS, H, dtype=bf)
            emit("gemm_nt", dict(A=nothing, B=nothing), lambda: dy.copy_((torch.randn(TOKENS, H, generator=g) * 0.01).to(bf)), ret=lambda: dy, stage="mlm_dy")
            for _ in range(2 if mut == "cls_added_twice" else 1):
                dy.index_add_(0, first_rows, dfb)
            emit("ln_bwd", dict(dy=dy, dy_rows=None), stage="ln2_bwd", layer=0)
            out["hand-over"] = dy.float()
        else:
            dy_all = torch.zeros(n + 3 * B, H, dtype=bf)
            emit("gemm_nt", dict(A=nothing, B=nothing), lambda: dy_all[:n].copy_((torch.randn(n, H, generator=g) * 0.01).to(bf)), ret=lambda: dy_all[:n],
                 stage="mlm_dy")
            tail = dfb.clone()
            if mut == "dfirst_v_s_swapped":
                tail = torch.cat((dfb[:B], dfb[2 * B:], dfb[B:2 * B]))
            elif mut == "dfirst_sample0_to_row1":
                tail[1], tail[0] = dfb[0], dfb[1]
            elif mut == "cls_row_truncated":
                tail[3] = torch.from_numpy((LR.f32_bits(df[3].numpy()) >> 16).astype(np.uint16).view(np.int16)).view(bf)
            dy_all[n:] = tail                                     # (the converting copy: no recorded launch)
            rows = idx[:n - 1] if mut == "idx_last_row_missing" else idx
            want = torch.cat((rows.long(), first_rows))
            emit("compact_rows", dict(rows=rows, extra=first_rows, row_map=None, inverse=None), ret=(want, want.int()))
            emit("ln_bwd", dict(dy=dy_all, dy_rows=None), stage="ln2_bwd", layer=0)
            out["hand-over"] = dy_all.float()
        out["dfirst"] = df
        y_prev = y
    out.update({nm: views[nm].clone() for nm in HR.PARAMS})
    for i, c in enumerate(calls):
        c.index = i
    return calls, model, out


def harness(calls, model):
    """The seam's exact checks, every seam op recomputed, the producers (with the hand-over's expectation)."""
    expect, ran = SS.check_seam(calls, model)
    for c in calls:
        if c.op in SS.SEAM_OPS:
            SS.recompute(c)
    SS.check_producers(calls, expect)
    return ran


def _worst_rel(out, clean):
    return max(float((out[k].double() - clean[k].double()).norm() / clean[k].double().norm().clamp(min=1e-300)) for k in clean)


@pytest.fixture(scope="module")
def clean():
    return {(d, nl): seam_chain(dense=d, num_labels=nl)[2] for d, nl in ((False, 7), (True, 7), (False, 1))}


def test_the_faithful_chains_pass():
    calls, model, _ = seam_chain()
    ran = harness(calls, model)
    assert ran == {"prologue consumers": 1, "heads y": 2, "heads first_rows": 2, "heads forward finals": 1, "mlm losses": 1, "dmlm twice": 1,
                   "heads gradient views": 1, "gscale": 1, "compact row list": 1, "compact hand-over": 1}, ran
    assert SS.preconditions(calls)["kink_ratio"] >= HR.KINK
    calls, model, _ = seam_chain(dense=True)
    assert harness(calls, model)["dense hand-over"] == 1
    calls, model, _ = seam_chain(steps=2)                         # the second micro-batch accumulates onto the first, the buffer sets alternate
    ran = harness(calls, model)
    assert ran["alternating buffers"] == 1 and ran["compact hand-over"] == 2
    calls, model, _ = seam_chain(num_labels=1)
    harness(calls, model)


@pytest.mark.parametrize("mut", MUTATIONS)
def test_each_single_change_fails_the_check_named_for_it(clean, mut):
    dense = mut == "cls_added_twice"
    steps = 2 if mut in ("prior_ignored", "prologue_previous_set") else 1
    calls, model, out = seam_chain(mut, dense=dense, steps=steps)
    with pytest.raises(AssertionError, match=CAUGHT_BY[mut]):
        harness(calls, model)
    if mut in E2E_INSIDE:
        worst = _worst_rel(out, clean[(dense, 7)])
        print(f"\n{mut}: worst relative error of an output {worst:.3g}")
        assert (worst < 0.045) == E2E_INSIDE[mut], (mut, worst)


@pytest.mark.parametrize("j", range(len(HEAD_MUTATIONS)), ids=[m.name for m in HEAD_MUTATIONS])
def test_each_mutation_of_the_emulated_levels_fails_the_recomputation(clean, j):
    m = HEAD_MUTATIONS[j]
    nl = 1 if m.name == HR.label_tanh_grad_missing().name else 7
    calls, model, out = seam_chain(head_mutation=m, num_labels=nl)
    worst = _worst_rel(out, clean[(False, nl)])
    print(f"\nE2E {m.name!r}: {worst:.3g}")
    if m.name == NO_CHANGE:
        assert worst == 0.0
        harness(calls, model)
        return
    with pytest.raises(AssertionError, match="heads_step_(fwd|bwd|dmlm)"):
        harness(calls, model)
    assert (worst < 0.045) == (m.name in HEAD_E2E_INSIDE), (m.name, worst)
