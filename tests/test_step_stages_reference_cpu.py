"""The step-stage harness (tests/step_stages.py) has teeth: a synthetic "recorded step" on the CPU -- the references' emulations
(``emu=True``: the kernels' documented roundings) chained into one encoder layer, forward and backward in the sparse top-layer form, plus
the MLM head, at configuration A (hidden 128, 2 heads, intermediate 512, vocabulary 4096), one short and one ragged sequence (24 and 77
rows, 18 and 60 of them keys), train mode -- passes ``recompute`` and ``check_dataflow`` as it is, and fails them under each single
change of ``MUTATIONS``: the wiring mistakes the end-to-end bounds let through.

For the mutations that are NOT an exact-comparison failure the test also states what the end-to-end comparison would have said: the
mutated chain's final gradients against the clean chain's, by ``compare_gradients``' 4.5 % relative error per gradient
(``E2E_INSIDE``; measured, worst gradient):

    gelu_1pct  GELU' scaled by 1 %                 inside  (0.5 %: today's suite lets it through)
    u_is_g     aux stored after the activation     OUTSIDE (11 %: gelu'(gelu(v)) is far from gelu'(v) on the FFN-up weight gradient)
    acc_flag   accumulate flag ignored             OUTSIDE (96 %: what the buffer held before -- the first micro-batch's gradient -- is lost)

For the two that exceed 4.5 % on their own the harness proves nothing new (the end-to-end test sees them as well); they stay in the list as
checks of the recomputation itself.

``gelu_bwd_ref``'s bound is validated here by its emulation (largest ratio 0.5).

The adapter launches have chains of their own below: ``lora_chain`` (Q/K/V adapters, the grouped column sum) and ``dense_chain`` (the
dense-seam adapters between the GEMMs they follow) -- the faithful chains pass, every mutation of tests/lora_ref.py / tests/lora_dense_ref.py
applied to what the "kernels" computed fails the recomputation, every wiring change fails the exact check named for it."""
import types

import pytest
import torch

from tests import attention_ref as A
from tests import gemm_ref as G
from tests import layout_ref as LR
from tests import rowwise_ref as R
from tests import step_stages as SS

H, HEADS, I, V = 128, 2, 512, 4096
LENS, VALID = [24, 77], [18, 60]
M = sum(LENS)
LABELLED = [3, 7, 30, 41, 55]
CLS_ROWS = [0, 24]
EPS = 1e-12
bf, f32 = torch.bfloat16, torch.float32

MUTATIONS = ("resid_z1", "dh_swapped", "u_is_g", "saved_altered", "ln2_stats_to_ln1", "stale_W1T", "acc_flag", "shared_stream",
             "rows_shifted", "gelu_1pct", "kv_short")
E2E_INSIDE = {"u_is_g": False, "gelu_1pct": True, "acc_flag": False}
CAUGHT_BY = {"resid_z1": "z2 residual = y1", "dh_swapped": "pre_drop is not the forward's triple", "u_is_g": "gemm_nt aux",
             "saved_altered": "ln1_bwd.* operand x: 1 of", "ln2_stats_to_ln1": "ln1_bwd mean", "stale_W1T": "W1T is not the transpose",
             "acc_flag": "gemm_tn_grouped problem 1 W", "shared_stream": "two dropout sites share a stream",
             "rows_shifted": "x_rows is not the row list", "gelu_1pct": "stage du.*gemm_nt out", "kv_short": r"kv_len\[1\] = 59"}


class _Lay:
    """What step_stages snapshots of an ops.SeqLayout."""

    def __init__(self, lens, heads):
        self.lens, self.heads = list(lens), heads
        starts, bases, bst, s, e, bp = [], [], [], 0, 0, 0
        for n in lens:
            starts.append(s)
            bases.append(e)
            bst.append(bp)
            s += n
            e = (e + heads * n * ((n + 3) // 4 * 4) + 3) // 4 * 4
            bp += (n + 127) // 128 * 128
        self.seq_start = torch.tensor(starts, dtype=torch.int32)
        self.bias_start = torch.tensor(bst, dtype=torch.int32)
        self.elem_base_host = bases


class _Deferred:
    items = ()

    def flush(self):
        pass


class _Inverse:
    def __init__(self, rows, nrows, stamp=7):
        import numpy as np
        self.table = torch.from_numpy(LR.stamp_table_ref(np.zeros(nrows, dtype=np.int64), rows.numpy(), stamp))
        self.stamp, self.nlist = stamp, rows.numel()


def _drop(seed, site, stream_of=None):
    thr = LR.dropout_thr16(0.1)
    return (LR.rng_stream(seed, site if stream_of is None else stream_of), thr, 1.0 / (1.0 - thr / 65536.0))


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc                     # noqa: E731
    lw = {}
    for n, (r, c) in dict(Wqkv=(3 * H, H), Wo=(H, H), W1=(I, H), W2=(H, I)).items():
        lw[n] = rn(r, c, sc=0.05).to(bf)
        lw[n + "T"] = lw[n].t().contiguous()
        lw["g_" + n] = rn(r, c, sc=0.05)                                          # (a first micro-batch's gradient: the launches accumulate)
    for n, c in dict(bqkv=3 * H, bo=H, b1=I, b2=H).items():
        lw[n] = rn(c, sc=0.1)
        lw["g_" + n] = rn(c, sc=0.1)
    for n in ("ln1", "ln2"):
        lw[n + "_g"], lw[n + "_b"] = 1.0 + rn(H, sc=0.1), rn(H, sc=0.1)
        lw["g_" + n + "_g"], lw["g_" + n + "_b"] = rn(H, sc=0.1), rn(H, sc=0.1)
    w = dict(Wt=rn(H, H, sc=0.05).to(bf), word_h=rn(V, H, sc=0.05).to(bf), bt=rn(H, sc=0.1), pred_bias=rn(V, sc=0.1),
             mlm_ln_g=1.0 + rn(H, sc=0.1), mlm_ln_b=rn(H, sc=0.1))
    w["WtT"], w["wordT"] = w["Wt"].t().contiguous(), w["word_h"].t().contiguous()
    w.update(g_Wt=rn(H, H, sc=0.05), g_bt=rn(H, sc=0.1), g_word_pad=rn(V, H, sc=0.01), g_pred_bias=rn(V, sc=0.01),
             g_mlm_ln_g=rn(H, sc=0.1), g_mlm_ln_b=rn(H, sc=0.1))
    return types.SimpleNamespace(_lw=[lw], _w=w)


def _b16(x):
    return x.to(bf)


def run_chain(mut=None):
    """(calls, model stub, final gradients) of the chain under one mutation (None: the faithful chain)."""
    assert mut is None or mut in MUTATIONS
    model = _params()
    lw, w = model._lw[0], model._w
    if mut == "stale_W1T":                                    # the transposed copy of BEFORE an optimizer step
        lw["W1T"] = _b16(lw["W1T"].float() * (1.0 + 2.0 ** -6))
    g = torch.Generator().manual_seed(1)
    x = _b16(torch.randn(M, H, generator=g))
    lay = _Lay(LENS, HEADS)
    seq = torch.repeat_interleave(torch.arange(len(LENS)), torch.tensor(LENS))
    pos = torch.cat([torch.arange(n) for n in LENS])
    key_bias = torch.where(pos < torch.tensor(VALID)[seq], 0.0, A.MASKED).float()
    kv_len = torch.tensor(VALID, dtype=torch.int32)
    if mut == "kv_short":
        kv_len[1] -= 1
    labels = torch.full((M,), -100, dtype=torch.int64)
    labels[LABELLED] = torch.randint(1000, V, (len(LABELLED),), generator=g)
    bounds = torch.tensor([0, LENS[0], M], dtype=torch.int32)
    d_att, d_h1 = _drop(11, 0), _drop(11, 1)
    d_h2 = _drop(11, 2, stream_of=1 if mut == "shared_stream" else None)
    calls = []

    def emit(op, a, compute, writes=()):
        """Snapshot the operands, run the emulation, record what it returned / wrote."""
        c = SS.Call(op, {k: SS._snap(v) for k, v in a.items()})
        ret = compute()
        c.ret = SS._snap(ret)
        c.post = {k: SS._snap(a[k]) for k in writes if a.get(k) is not None}
        calls.append(c)
        return ret

    def keep(n, cols, d):
        return SS.flat_mask(n * cols, d).view(n, cols)

    def nt(A_, B_, bias=None, gelu=False, aux=None, resid=None, gelu_bwd_u=None, drop=None, mutation=None, scale_out=1.0):
        a = dict(A=A_, B=B_, out=None, bias=bias, gelu=gelu, aux=aux, resid=resid, gelu_bwd_u=gelu_bwd_u, alpha=1.0, alpha_dev=None, drop=drop,
                 out_f32=False)

        def compute():
            r = G.nt(A_, B_, bias=bias, gelu=gelu, resid=resid, keep=keep(A_.shape[0], B_.shape[0], drop) if drop else None,
                     drop_scale=drop[2] if drop else 1.0, gelu_u=gelu_bwd_u, emu=True, mutation=mutation)
            if aux is not None:
                aux.copy_(r["aux"])
            return _b16(r["out"] * scale_out)
        return emit("gemm_nt", a, compute, writes=("aux",))

    def splitk(A_, B_, resid=None):
        return emit("gemm_nt_splitk", dict(A=A_, B=B_, out=None, resid=resid), lambda: _b16(G.splitk(A_, B_, resid=resid, emu=True)["out"]))

    def ln_fwd(x_, gam, bet):
        def compute():
            r = R.ln_fwd(x_, gam, bet, EPS, emu=True)
            return _b16(r["y"]), r["mean"].to(f32), r["rstd"].to(f32)
        return emit("ln_fwd", dict(x=x_, gamma=gam, beta=bet, eps=EPS, M=None, out=None, in_rows=None, out_rows=None, drop=None, stats=True,
                                   drop_row0=0), compute)

    sums = []

    def ln_bwd(dy, x_, mean, rstd, gam, dgam, dbet, x_rows=None, pre_drop=None, site_rows=None):
        dx2 = torch.empty(mean.numel(), H, dtype=bf) if pre_drop else None
        a = dict(dy=dy, x=x_, mean=mean, rstd=rstd, gamma=gam, dgamma=dgam, dbeta=dbet, M=None, dx=None, dx2=dx2, dy_rows=None, x_rows=x_rows,
                 dx_rows=None, post_drop=None, pre_drop=pre_drop, dbias2=None, drop_rows=x_rows if pre_drop else None, deferred=_Deferred(),
                 dy_row_limit=0)

        def compute():
            r = R.ln_bwd(dy, x_, mean, rstd, gam, x_rows=x_rows, drop_rows=a["drop_rows"], dx2=dx2 is not None,
                         pre_keep=keep(site_rows, H, pre_drop) if pre_drop else None, pre_scale=pre_drop[2] if pre_drop else 1.0, emu=True)
            if dx2 is not None:
                dx2.copy_(r["dx2"])
            sums.append((dgam, dbet, r["dgamma"], r["dbeta"]))
            return _b16(r["dx"])
        out = emit("ln_bwd", a, compute, writes=("dx2",))
        sums[-1] += (calls[-1],)
        return out, (dx2 if dx2 is not None else out)

    def attn(qkv, dctx=None, ctx=None, lse=None, q_limit=None):
        bias = torch.where(pos >= kv_len.long()[seq], torch.tensor(-1.0e30, dtype=torch.float64), key_bias.double())
        masks = SS.attn_masks(SS._snap(lay), d_att)
        if dctx is None:
            def compute():
                r = A.emulate(qkv, bias, LENS, HEADS, masks, d_att[2])
                return _b16(r["ctx"]), r["lse"].to(f32)
            return emit("attn_fwd", dict(qkv=qkv, key_bias=key_bias, layout=lay, H=H, drop=d_att, ctx=None, lse=None, kv_len=kv_len), compute)

        def compute():
            r = A.emulate(qkv, bias, LENS, HEADS, masks, d_att[2], dctx)
            return _b16(torch.cat((r["dq"], r["dk"], r["dv"]), 1))
        return emit("attn_bwd", dict(qkv=qkv, ctx=ctx, dctx=dctx, lse=lse, key_bias=key_bias, layout=lay, H=H, drop=d_att, dqkv=None, kv_len=kv_len,
                                     q_limit=q_limit), compute)

    def gather(srcs, idx):
        return emit("gather_rows", dict(srcs=list(srcs), idx32=idx), lambda: [t[idx.long()].clone() for t in srcs])

    def tn_grouped(probs, mutation=None):
        a = dict(problems=probs, accumulate=[True] * len(probs), alpha=1.0)

        def compute():
            for (A_, B_, W, b), r in zip(probs, G.tn_grouped(probs, a["accumulate"], emu=True, mutation=mutation)):
                W.copy_(r["W"])
                b.copy_(r["bias"])
        emit("gemm_tn_grouped", a, compute, writes=("problems",))

    # ---- forward: one encoder layer ...
    qkv = nt(x, lw["Wqkv"], bias=lw["bqkv"])
    actx, lse = attn(qkv)
    z1 = nt(actx, lw["Wo"], bias=lw["bo"], resid=x, drop=d_h1)
    y1, m1, r1 = ln_fwd(z1, lw["ln1_g"], lw["ln1_b"])
    u = torch.empty(M, I, dtype=bf)
    gg = nt(y1, lw["W1"], bias=lw["b1"], gelu=True, aux=u, mutation=G.aux_after_activation() if mut == "u_is_g" else None)
    z2 = nt(gg, lw["W2"], bias=lw["b2"], resid=z1 if mut == "resid_z1" else y1, drop=d_h2)
    y2, m2, r2 = ln_fwd(z2, lw["ln2_g"], lw["ln2_b"])
    # ---- ... and the MLM head over all rows (the caller wants the scores), backward over the labelled rows
    pre = torch.empty(M, H, dtype=bf)
    t0 = nt(y2, w["Wt"], bias=w["bt"], gelu=True, aux=pre)
    t, mt, rt = ln_fwd(t0, w["mlm_ln_g"], w["mlm_ln_b"])
    logits = nt(t, w["word_h"], bias=w["pred_bias"])

    def ce_f():
        r = R.ce_fwd(logits, labels, V, bounds, 2, emu=True)
        cnt = torch.tensor([sum(1 for i in LABELLED if bounds[s] <= i < bounds[s + 1]) for s in range(2)] + [1, 1], dtype=torch.float64)
        return r["loss"].to(f32), (1.0 / cnt.clamp(min=1)).to(f32), r["row_lse"].to(f32)
    loss, inv, row_lse = emit("ce_fwd", dict(logits=logits, V=V, labels=labels, seg_bounds=bounds, nseg=2, smoothing=0.0), ce_f)
    if mut == "saved_altered":                                 # a saved activation overwritten between its production and its use
        z1[5, 9] = z1[5, 9] * 1.5 + 1.0
    idx = torch.tensor(LABELLED, dtype=torch.int32)
    gs = torch.tensor([1.0, 0.5])
    dl = torch.empty(idx.numel(), V, dtype=bf)

    def ce_b():
        for j, v in R.ce_bwd(logits, labels, V, bounds, 2, gs, row_lse, rows=idx, emu=True):
            dl[j] = _b16(v)
        return dl
    emit("ce_bwd", dict(logits=logits, V=V, labels=labels, seg_bounds=bounds, nseg=2, inv=inv, gscale=gs, lse=row_lse, dlogits=dl, rows=idx,
                        smoothing=0.0), ce_b, writes=("dlogits",))
    t_c, t0_c, pre_c, y_c, mt_c, rt_c = gather([t, t0, pre, y2, mt, rt], idx)
    dt = splitk(dl, w["wordT"])
    dt0, _ = ln_bwd(dt, t0_c, mt_c, rt_c, w["mlm_ln_g"], w["g_mlm_ln_g"], w["g_mlm_ln_b"])
    dpre = emit("gelu_bwd", dict(dy=dt0, u=pre_c, du=None), lambda: _b16(SS.gelu_bwd_ref(dt0, pre_c, emu=True)))
    dyl = nt(dpre, w["WtT"])
    # the compact hand-over: labelled rows' gradients, then the [CLS] rows' (from the other heads: given)
    R32 = torch.tensor(LABELLED + CLS_ROWS, dtype=torch.int32)
    dy_c = torch.cat((dyl, _b16(torch.randn(len(CLS_ROWS), H, generator=g) * 0.01)))
    # ---- backward of the layer, sparse top-layer form (model._EncoderFn._last_layer_sparse)
    rinv = _Inverse(R32.long(), M)
    m2_c, r2_c, u_c, m1_c, r1_c, y1_c, g_c, actx_c = gather([m2, r2, u, m1, r1, y1, gg, actx], R32 + 1 if mut == "rows_shifted" else R32)
    b_h2, b_h1 = (d_h1, d_h2) if mut == "dh_swapped" else (d_h2, d_h1)
    dz2_c, dz2d_c = ln_bwd(dy_c, z2, m2_c, r2_c, lw["ln2_g"], lw["g_ln2_g"], lw["g_ln2_b"], x_rows=R32, pre_drop=b_h2, site_rows=M)
    du_c = nt(dz2d_c, lw["W2T"], gelu_bwd_u=u_c, scale_out=1.01 if mut == "gelu_1pct" else 1.0)
    dy1_c = splitk(du_c, lw["W1T"], resid=dz2_c)
    st1 = (m2_c, r2_c) if mut == "ln2_stats_to_ln1" else (m1_c, r1_c)
    dz1_c, dz1d_c = ln_bwd(dy1_c, z1, st1[0], st1[1], lw["ln1_g"], lw["g_ln1_g"], lw["g_ln1_b"], x_rows=R32, pre_drop=b_h1, site_rows=M)
    dctx_c = nt(dz1d_c, lw["WoT"])

    def scat():
        outs = [torch.zeros(M, H, dtype=bf), torch.zeros(M, H, dtype=bf)]
        for o, s in zip(outs, (dctx_c, dz1_c)):
            o[R32.long()] = s
        return outs
    dctx, dz1 = emit("scatter_rows_zero", dict(srcs=[dctx_c, dz1_c], inverse=rinv, nrows=M), scat)
    st = lay.seq_start.long()
    sq = torch.searchsorted(st, R32.long(), right=True) - 1
    qlim = emit("attn_q_limit", dict(rows32=R32, layout=lay),
                lambda: torch.zeros(len(LENS), dtype=torch.long).scatter_reduce_(0, sq, R32.long() - st[sq] + 1, "amax").int())
    dqkv = attn(qkv, dctx, actx, lse, qlim)
    dx = nt(dqkv, lw["WqkvT"], resid=dz1)
    # ---- every weight gradient in one grouped call (deferred + late), then the one LayerNorm reduce
    tn_grouped([(dqkv, x, lw["g_Wqkv"], lw["g_bqkv"]), (du_c, y1_c, lw["g_W1"], lw["g_b1"]), (dz2d_c, g_c, lw["g_W2"], lw["g_b2"]),
                (dz1d_c, actx_c, lw["g_Wo"], lw["g_bo"]), (dl, t_c, w["g_word_pad"], w["g_pred_bias"]), (dpre, y_c, w["g_Wt"], w["g_bt"])],
               mutation=G.grouped_ignores_accumulate(1) if mut == "acc_flag" else None)
    red = SS.Call("ln_bwd_reduce", dict(pre=[(SS._snap(s[0]), SS._snap(s[1])) for s in sums], H=H))
    red.meta["calls"] = [s[4] for s in sums]
    for dgam, dbet, sg, sb, _c in sums:
        dgam.copy_((dgam.double() + sg).to(f32))
        dbet.copy_((dbet.double() + sb).to(f32))
    red.post["grads"] = [(SS._snap(s[0]), SS._snap(s[1])) for s in sums]
    calls.append(red)
    for i, c in enumerate(calls):
        c.index = i
    grads = {k: v.clone() for k, v in list(lw.items()) + list(w.items()) if k.startswith("g_")}
    grads["dx"] = dx.float()
    return calls, model, grads


def harness(calls, model):
    per = SS.recompute_all(calls, model)
    SS.check_dataflow(calls, model)
    return per


@pytest.fixture(scope="module")
def clean():
    return run_chain(None)


def test_the_faithful_chain_passes(clean):
    calls, model, _ = clean
    per = harness(calls, model)
    want = {"gemm_nt": 10, "gemm_nt_splitk": 2, "gemm_tn_grouped": 1, "attn_fwd": 1, "attn_bwd": 1, "attn_q_limit": 1, "ln_fwd": 3, "ln_bwd": 3,
            "ln_bwd_reduce": 1, "gelu_bwd": 1, "ce_fwd": 1, "ce_bwd": 1, "gather_rows": 2, "scatter_rows_zero": 1}
    assert {k: n for k, (n, _w) in per.items()} == want
    print({k: round(w, 3) for k, (_n, w) in per.items()})
    assert all(w <= 1.0 for _n, w in per.values())
    # an emulation sits well inside its reference's bound (about half: one bf16 rounding of the output)
    assert 0.3 < per["gemm_nt"][1] < 0.8 and 0.3 < per["gelu_bwd"][1] < 0.8, per


def test_gelu_bwd_bound_is_calibrated_by_its_emulation():
    """The one new reference: its emulation (fp32 product, one bf16 rounding) against the float64 value, on a grid of u over [-6, 6]
    and gradients over 2^+-12 -- largest ratio about 0.5 (the bf16 rounding of the output), a GELU' off by 1 % fails."""
    g = torch.Generator().manual_seed(3)
    u = _b16(torch.linspace(-6, 6, 4096).repeat(4))
    dy = _b16(torch.randn(u.numel(), generator=g) * torch.exp2(torch.randint(-12, 13, (u.numel(),), generator=g).float()))
    ref = SS.gelu_bwd_ref(dy, u)
    r = G.ratios(SS.gelu_bwd_ref(dy, u, emu=True).reshape(1, -1), ref)
    assert 0.4 < r.elem <= 0.55 and r.norm <= 0.55, (r.elem, r.norm)
    bad = G.ratios(_b16(SS.gelu_bwd_ref(dy, u, emu=True).double() * 1.01).reshape(1, -1), ref)
    assert bad.worst > 1.0, bad


@pytest.mark.parametrize("mut", MUTATIONS)
def test_each_single_change_fails_the_harness(clean, mut):
    """One change to the chain at a time (see ``run_chain``): the residual of the FFN-down epilogue from z1; d_h1 / d_h2 swapped in
    backward only; the saved u replaced by g; a saved activation altered between production and use; LayerNorm 2's statistics handed to
    LayerNorm 1's backward; W1T left at the values from before the optimizer step; a weight-gradient problem ignoring its accumulate flag;
    two dropout sites sharing a stream; the sparse top layer's row list shifted by one; GELU' scaled by 1 %; kv_len one key short on one
    sequence.  Each fails ``recompute`` or ``check_dataflow``; for the three that are no exact-comparison failure, the end-to-end
    4.5 % comparison of the final gradients is asserted as well (``E2E_INSIDE``: u_is_g and acc_flag exceed it on their own, so the
    harness proves nothing new for those two -- module docstring)."""
    calls, model, grads = run_chain(mut)
    with pytest.raises(AssertionError, match=CAUGHT_BY[mut]):
        harness(calls, model)
    if mut in E2E_INSIDE:
        ref = clean[2]
        worst = max(float((grads[k].double() - ref[k].double()).norm() / ref[k].double().norm()) for k in ref)
        print(mut, "worst end-to-end relative error of a gradient:", round(worst, 4))
        assert (worst < 0.045) == E2E_INSIDE[mut], (mut, worst)
        assert worst > 0.0


# ------------------------------------------------------------------------------------------------ the adapter and column-sum launches
from tests import lora_ref as LO                             # noqa: E402
from tests.test_lora_reference_cpu import MUTATIONS as LORA_MUTATIONS            # noqa: E402

LM, LR_, LT = 257, 8, ("query", "value")                     # (tests/test_lora_reference_cpu.py's mutation case: 257 rows, H = 128, r = 8, q + v)
COLSUM_ROWS = 200                                            # rows of the column-sum problem; a dropped row block = its last 32


def lora_chain(mutation=None, colsum_rows=COLSUM_ROWS, stray=None):
    """The three new launches as a recorded chain on the CPU, outputs from the references' emulations: ``lora_qkv_fwd`` (in place on the
    qkv a gemm left, h kept), ``lora_qkv_bwd`` reading that h (a row slice of it, as the model passes it), accumulating onto the adapter
    gradients, and ``colsum_grouped`` of a bias gradient -- all gradients views of ONE flat buffer laid out by ``offset`` / ``numel``.
    ``mutation``: a tests/lora_ref.py Mutation applied to what the "kernels" computed; ``colsum_rows``: the rows the column sum really
    summed; ``stray``: a parameter name whose span the column sum writes instead of its own.  Returns (calls, flat buffer, offset, numel)."""
    inp = LO.inputs(LM, H, LR_, LT, "real", 4242 + LR_)
    s = 16.0 / LR_
    names = [f"{t}.lora_{m}" for t in LT for m in ("A", "B")] + ["bqkv", "ln.weight", "ln.bias"]
    numel = {n: LR_ * H for n in names[:4]}
    numel.update({"bqkv": 3 * H, "ln.weight": H, "ln.bias": H})
    offset, off = {}, 0
    for n in names:
        offset[n] = off
        off = (off + numel[n] + 255) // 256 * 256 + (256 if n == "bqkv" else 0)            # (a block of padding behind the bias)
    flat = torch.randn(off, generator=torch.Generator().manual_seed(9)) * 0.01
    view = lambda n, shape: flat[offset[n]:offset[n] + numel[n]].view(shape)                 # noqa: E731
    gA = {t: view(f"{t}.lora_A", (LR_, H)) for t in LT}
    gB = {t: view(f"{t}.lora_B", (H, LR_)) for t in LT}
    calls = []
    # forward
    qkv = inp["qkv"].clone()
    hbuf = torch.zeros(LM + 7, len(LT) * LR_, dtype=bf)
    a = dict(x=inp["x"], qkv=qkv, A=inp["A"], B=inp["B"], targets=LT, scale=s, h_out=hbuf[:LM])
    pre = {k: SS._snap(v) for k, v in a.items()}
    e = LO.fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], LT, s, emu=True, mutation=mutation)
    qkv.copy_(e["qkv"].val.to(bf))
    hbuf[:LM].copy_(e["h"].val.to(bf))
    calls.append(SS.Call("lora_qkv_fwd", pre, {"qkv": SS._snap(qkv), "h_out": SS._snap(hbuf[:LM])}, SS._snap(qkv)))
    # backward
    a = dict(dqkv=inp["dqkv"], x=inp["x"], h=hbuf[:LM], A=inp["A"], B=inp["B"], gA=gA, gB=gB, targets=LT, scale=s, dres=inp["dres"], accumulate=True,
             workspace=None)
    pre = {k: SS._snap(v) for k, v in a.items()}
    e = LO.bwd(inp["dqkv"], inp["x"], hbuf[:LM], inp["A"], inp["B"], LT, s, dres=inp["dres"], gA0={t: g.clone() for t, g in gA.items()},
               gB0={t: g.clone() for t, g in gB.items()}, accumulate=True, emu=True, mutation=mutation)
    for t in LT:
        gA[t].copy_(e["dA"][t].val.float())
        gB[t].copy_(e["dB"][t].val.float())
    calls.append(SS.Call("lora_qkv_bwd", pre, {"gA": SS._snap(gA), "gB": SS._snap(gB)}, SS._snap(e["dres"].val.to(bf))))
    # the bias gradient of the frozen Wqkv: the column sum of dqkv's first rows
    X = inp["dqkv"][:COLSUM_ROWS]
    out = view(stray, (-1,))[:3 * H] if stray == "bqkv" else (view("bqkv", (3 * H,)) if stray is None else flat[offset[stray]:offset[stray] + 3 * H])
    a = dict(problems=[(X, out)], accumulate=True, alpha=1.0, alpha_dev=None)
    pre = {k: SS._snap(v) for k, v in a.items()}
    out.add_(X[:colsum_rows].float().sum(0))
    calls.append(SS.Call("colsum_grouped", pre, {"problems": SS._snap([(X, out)])}, None))
    for i, c in enumerate(calls):
        c.index = i
        c.meta.update(stage=c.op, layer=None)
    return calls, flat, offset, numel


def test_the_chain_through_the_adapter_and_column_sum_launches_passes():
    calls, flat, offset, numel = lora_chain()
    per = SS.recompute_all(calls)
    assert {k: n for k, (n, _w) in per.items()} == {"lora_qkv_fwd": 1, "lora_qkv_bwd": 1, "colsum_grouped": 1}
    print({k: round(w, 3) for k, (_n, w) in per.items()})
    assert 0.2 < per["lora_qkv_fwd"][1] <= 0.55 and 0.2 < per["lora_qkv_bwd"][1] <= 0.55 and per["colsum_grouped"][1] <= 0.5, per
    SS.check_producers(calls)                                   # backward read the h forward wrote, bit for bit


@pytest.mark.parametrize("name", list(LORA_MUTATIONS))
def test_each_adapter_mutation_fails_the_recomputation(name):
    """tests/lora_ref.py's six mutations (a rank column dropped, s off by 2^-6, q and v swapped, the last partial row block skipped, a
    partial sum left out of the fold, accumulate ignored), each applied to what the chain's adapter launches computed."""
    calls, *_ = lora_chain(LORA_MUTATIONS[name][0]())
    with pytest.raises(AssertionError, match="lora_qkv_(fwd|bwd)"):
        SS.recompute_all(calls)


def test_a_dropped_row_block_of_the_column_sum_fails():
    calls, *_ = lora_chain(colsum_rows=COLSUM_ROWS - 32)
    with pytest.raises(AssertionError, match=r"colsum_grouped problem 0 \(200 x 384\)"):
        SS.recompute_all(calls)


def test_a_backward_that_reads_another_h_than_forward_wrote_fails_the_producer_check():
    calls, *_ = lora_chain()
    h = calls[1].a["h"]
    h.t.view(torch.int16)[5, 3] += 1
    h._cpu = None
    with pytest.raises(AssertionError, match="lora_qkv_bwd.* operand h: 1 of"):
        SS.check_producers(calls)


def test_a_write_into_a_frozen_span_trips_the_check():
    """``check_frozen_writes``: the chain's writes lie in trainable spans (the adapters, the bias) -- fine while the LayerNorm is what is
    frozen, a failure as soon as the bias is, or as the column sum lands in the frozen LayerNorm's span; padding is nobody's span."""
    plan = lambda *frozen: types.SimpleNamespace(frozen=frozenset(frozen), layers={}, word_table=False)      # noqa: E731
    model = _params()
    names = SS.names_of(model)
    wg = SS.synth("gemm_tn_grouped", dict(problems=[(torch.zeros(4, H, dtype=bf), torch.zeros(4, H, dtype=bf), model._w["g_Wt"], model._w["g_bt"])],
                                          accumulate=True, alpha=1.0), post=dict(problems=[(model._w["g_Wt"], model._w["g_bt"])]))
    wg.meta.update(stage="gemm_tn_grouped", layer=None)
    calls, flat, offset, numel = lora_chain()
    assert SS.check_frozen_writes(calls + [wg], names, plan("ln.weight", "ln.bias"), 1, flat, offset, numel) == 5     # 2 x 2 adapter gradients, the bias
    with pytest.raises(AssertionError, match=r"colsum_grouped.* writes elements \[\d+, \d+\) of the gradient buffer: the span of the frozen bqkv"):
        SS.check_frozen_writes(calls + [wg], names, plan("bqkv"), 1, flat, offset, numel)
    with pytest.raises(AssertionError, match="lora_qkv_bwd.*the span of the frozen value.lora_B"):
        SS.check_frozen_writes(calls + [wg], names, plan("value.lora_B"), 1, flat, offset, numel)
    stray, flat2, *_ = lora_chain(stray="ln.weight")
    with pytest.raises(AssertionError, match="the span of the frozen ln.weight"):
        SS.check_frozen_writes(stray + [wg], names, plan("ln.weight", "ln.bias"), 1, flat2, offset, numel)
    # the weight-gradient problems written are exactly the plan's: the MLM transform alone here; a missing or an extra one fails
    with pytest.raises(AssertionError, match=r"missing \['g_Wt'\]"):
        SS.check_frozen_writes(calls, names, plan("ln.weight"), 1, flat, offset, numel)
    full = types.SimpleNamespace(frozen=frozenset({"ln.weight"}), layers={0: dict(w1="full", w2="none", qkv="bias", o="none")}, word_table=True)
    assert SS.expected_wgrad_problems(full, 1) == {"l0.g_W1", "g_Wt", "g_word_pad"}
    assert SS.expected_wgrad_problems(None, 2) == {f"l{i}.g_{k}" for i in (0, 1) for k in ("W1", "W2", "Wqkv", "Wo")} | {"g_Wt", "g_word_pad"}
    with pytest.raises(AssertionError, match=r"missing \['g_word_pad', 'l0.g_W1'\]"):
        SS.check_frozen_writes(calls + [wg], names, full, 1, flat, offset, numel)


def test_the_frozen_form_of_the_sequence_check():
    """``check_sequence`` with a plan: forward all L layers, backward L-1 .. stop, no ``dx`` where backward ends without an embedding
    stage, the adapter stages directly behind ``qkv`` / ``attn_bwd`` -- and each deviation fails."""
    def calls_of(seq):
        out = []
        for st, l in seq:
            c = SS.Call(st, {})
            c.meta.update(stage=st, layer=l)
            out.append(c)
        return out
    L = 3
    fwd = lambda lora=(): [(s, l) for l in range(L) for s in (SS._with(SS.FWD_LAYER, "qkv", "lora_fwd") if l in lora else SS.FWD_LAYER)]      # noqa: E731
    dense = lambda l, lora=(), dx=True: [(s, l) for s in SS._with(SS._with(SS.BWD_DENSE, "attn_bwd", "lora_bwd") if l in lora else SS.BWD_DENSE, None, None, drop=None if dx else "dx")]      # noqa: E731
    assert SS.check_sequence(calls_of(fwd() + dense(2) + dense(1, dx=False)), L, stop=1, no_dx=True) == {"fwd": 1, "bwd": 1}
    assert SS.check_sequence(calls_of(fwd((0, 1, 2)) + dense(2, (2,)) + dense(1, (1,)) + dense(0, (0,), dx=False)), L, 0, True, (0, 1, 2)) == {"fwd": 1, "bwd": 1}
    assert SS.check_sequence(calls_of(fwd((2,)) + dense(2, (2,)) + dense(1) + dense(0)), L, 0, False, (2,)) == {"fwd": 1, "bwd": 1}
    assert SS.check_sequence(calls_of(fwd()), L, stop=3, no_dx=True) == {"fwd": 1, "bwd": 0}
    for bad, kw in ((fwd() + dense(2) + dense(1), dict(stop=1, no_dx=True)),                        # an input gradient where backward ends
                    (fwd() + dense(2) + dense(1, dx=False) + dense(0, dx=False), dict(stop=1, no_dx=True)),     # a layer below stop runs
                    (fwd() + dense(2), dict(stop=3, no_dx=True)),                                  # a layer runs though none is trainable
                    (fwd((2,)) + dense(2) + dense(1) + dense(0), dict(lora_layers=(2,))),           # the adapter backward is missing
                    (fwd() + dense(2, (2,)) + dense(1) + dense(0), dict(lora_layers=(2,)))):        # the adapter forward is missing
        with pytest.raises(AssertionError):
            SS.check_sequence(calls_of(bad), L, **kw)


# ------------------------------------------------------------------------------------------------ the dense-seam adapter launches
from tests import lora_dense_ref as DR                       # noqa: E402
from tests.test_lora_dense_reference_cpu import MUTATIONS as DENSE_MUTATIONS     # noqa: E402

DM, DRA, DRANK = 257, 249, 4                                 # (tests/test_lora_dense_reference_cpu.py's mutation case: 257 rows, (K, N) = (128, 512); backward on 249)
DROWS = [0, 3, 17, 64, 65, 127, 128, 200, 248] + list(range(20, 48))            # the rows of the gathered launch (37: no multiple of 16)
DENSE_TARGETS = ("intermediate", "ffn_output")               # (K, N) = (128, 512) and (512, 128): K != N both ways
WIRING = ("triple", "gelu_u", "fresh_dx", "no_aux")


def dense_chain(mutation=None, wiring=None):
    """The FFN half of one encoder layer with dense-seam adapters as a recorded chain on the CPU, the adapters' outputs from
    tests/lora_dense_ref.py's emulation, the launches around them from the other references' emulations: LayerNorm 1, the FFN-up GEMM
    (bias only), ``lora_dense_fwd`` in GELU mode writing ``aux`` and h, the FFN-down GEMM with residual and a live dropout triple,
    ``lora_dense_fwd`` in ADD mode with that triple; backward on the leading 249 rows: the ``du`` GEMM, ``lora_dense_bwd`` with ``gelu_u`` =
    that ``aux``, ``dx`` in place and ``h`` a row slice; a gather, the split-K ``dy1`` GEMM on the gathered rows and ``lora_dense_bwd`` with
    ``h=None`` -- the adapter gradients views of ONE flat buffer laid out by ``offset`` / ``numel`` (they hold an earlier micro-batch's
    values: the launches accumulate).  ``mutation``: a tests/lora_dense_ref.py Mutation applied to what the adapter "kernels" computed;
    ``wiring``: ``triple`` (the ADD-mode adapter gets another triple than its GEMM), ``gelu_u`` (another buffer than the du GEMM's),
    ``fresh_dx`` (dx is a copy, not the GEMM's output), ``no_aux`` (the GELU-mode launch is handed no ``aux``: backward reads a buffer nobody
    wrote).  Returns (calls, model stub, flat buffer, offset, numel)."""
    assert wiring is None or wiring in WIRING
    model = _params()
    lw = model._lw[0]
    g = torch.Generator().manual_seed(21)
    s = 16.0 / DRANK
    dims = {"intermediate": (H, I), "ffn_output": (I, H)}
    names = [f"{t}.lora_{m}" for t in DENSE_TARGETS for m in ("A", "B")] + ["b2"]
    numel = {f"{t}.lora_{m}": DRANK * (dims[t][0] if m == "A" else dims[t][1]) for t in DENSE_TARGETS for m in ("A", "B")}
    numel["b2"] = H
    offset, off = {}, 0
    for n in names:
        offset[n] = off
        off = (off + numel[n] + 255) // 256 * 256
    flat = torch.randn(off, generator=torch.Generator().manual_seed(9)) * 0.01
    view = lambda n, shape: flat[offset[n]:offset[n] + numel[n]].view(shape)                 # noqa: E731
    dl = dict(targets=DENSE_TARGETS, r=DRANK, scale=s, A={}, B={}, gA={}, gB={}, pA={}, pB={})
    for k, t in enumerate(DENSE_TARGETS):
        K, N = dims[t]
        inp = DR.inputs(8, K, N, DRANK, "real", 6000 + k)
        dl["A"][t], dl["B"][t] = inp["A"], inp["B"]
        dl["gA"][t], dl["gB"][t] = view(f"{t}.lora_A", (DRANK, K)), view(f"{t}.lora_B", (N, DRANK))
        dl["pA"][t] = types.SimpleNamespace(requires_grad=True, grad=dl["gA"][t])
        dl["pB"][t] = types.SimpleNamespace(requires_grad=True, grad=dl["gB"][t])
    lw["lora_dense"] = dl
    calls = []

    def emit(op, a, compute, writes=()):
        c = SS.Call(op, {k: SS._snap(v) for k, v in a.items()})
        ret = compute()
        c.ret = SS._snap(ret)
        c.post = {k: SS._snap(a[k]) for k in writes if a.get(k) is not None}
        calls.append(c)
        return ret

    def nt(A_, B_, bias=None, resid=None, gelu_bwd_u=None, drop=None):
        a = dict(A=A_, B=B_, out=None, bias=bias, gelu=False, aux=None, resid=resid, gelu_bwd_u=gelu_bwd_u, alpha=1.0, alpha_dev=None, drop=drop,
                 out_f32=False)
        keep = SS.flat_mask(A_.shape[0] * B_.shape[0], drop).view(A_.shape[0], B_.shape[0]) if drop else None
        return emit("gemm_nt", a, lambda: _b16(G.nt(A_, B_, bias=bias, resid=resid, keep=keep, drop_scale=drop[2] if drop else 1.0,
                                                     gelu_u=gelu_bwd_u, emu=True)["out"]))

    def dense_fwd(t, x_, y_, mode, drop=None, aux=None, h_out=None):
        a = dict(x=x_, y=y_, A=dl["A"][t], B=dl["B"][t], scale=s, mode=mode, drop=drop, aux=aux, h_out=h_out)

        def compute():
            e = DR.fwd(x_, y_, dl["A"][t], dl["B"][t], s, mode, drop=drop, emu=True, mutation=mutation)
            y_.copy_(_b16(e["y"].val))
            if aux is not None:
                aux.copy_(_b16(e["aux"].val))
            if h_out is not None:
                h_out.copy_(_b16(e["h"].val))
            return y_
        return emit("lora_dense_fwd", a, compute, writes=("y", "aux", "h_out"))

    def dense_bwd(t, dy, x_, h, dx, gelu_u=None):
        gA, gB = dl["gA"][t], dl["gB"][t]
        a = dict(dy=dy, x=x_, h=h, A=dl["A"][t], B=dl["B"][t], gA=gA, gB=gB, scale=s, dx=dx, gelu_u=gelu_u, accumulate=True, workspace=None)

        def compute():
            e = DR.bwd(dy, x_, h, dl["A"][t], dl["B"][t], s, dx=dx, gelu_u=gelu_u, gA0=gA.clone(), gB0=gB.clone(), accumulate=True, emu=True,
                       mutation=mutation)
            dx.copy_(_b16(e["dx"].val))
            gA.copy_(e["dA"].val.float())
            gB.copy_(e["dB"].val.float())
            return dx
        return emit("lora_dense_bwd", a, compute, writes=("dx", "gA", "gB"))

    d_h2 = _drop(11, 2)
    z1 = _b16(torch.randn(DM, H, generator=g))
    # ---- forward
    y1 = emit("ln_fwd", dict(x=z1, gamma=lw["ln1_g"], beta=lw["ln1_b"], eps=EPS, M=None, out=None, in_rows=None, out_rows=None, drop=None, stats=True,
                             drop_row0=0), lambda: (lambda r: (_b16(r["y"]), r["mean"].to(f32), r["rstd"].to(f32)))(R.ln_fwd(z1, lw["ln1_g"], lw["ln1_b"], EPS, emu=True)))[0]
    gg = nt(y1, lw["W1"], bias=lw["b1"])
    u = torch.zeros(DM, I, dtype=bf)
    h_i, h_f = torch.zeros(DM + 7, DRANK, dtype=bf), torch.zeros(DM + 7, DRANK, dtype=bf)
    dense_fwd("intermediate", y1, gg, DR.GELU, aux=None if wiring == "no_aux" else u, h_out=h_i[:DM])
    z2 = nt(gg, lw["W2"], bias=lw["b2"], resid=y1, drop=d_h2)
    dense_fwd("ffn_output", gg, z2, DR.ADD, drop=_drop(11, 5) if wiring == "triple" else d_h2, h_out=h_f[:DM])
    # ---- backward on the leading rows
    dz2d = _b16(torch.randn(DRA, H, generator=g) * 0.05)
    dz2 = _b16(torch.randn(len(DROWS), H, generator=g) * 0.05)
    du = nt(dz2d, lw["W2T"], gelu_bwd_u=u[:DRA])
    dense_bwd("ffn_output", dz2d, gg[:DRA], h_f[:DRA], du.clone() if wiring == "fresh_dx" else du, gelu_u=u.clone()[:DRA] if wiring == "gelu_u" else u[:DRA])
    idx = torch.tensor(DROWS, dtype=torch.int32)
    y1_c, du_c = emit("gather_rows", dict(srcs=[y1[:DRA], du], idx32=idx), lambda: [t[idx.long()].clone() for t in (y1[:DRA], du)])
    dy1_c = emit("gemm_nt_splitk", dict(A=du_c, B=lw["W1T"], out=None, resid=dz2), lambda: _b16(G.splitk(du_c, lw["W1T"], resid=dz2, emu=True)["out"]))
    dense_bwd("intermediate", du_c, y1_c, None, dy1_c)
    for i, c in enumerate(calls):
        c.index = i
        c.meta["pass"] = 1
    SS.annotate(calls, model)
    return calls, model, flat, offset, numel


def test_the_chain_through_the_dense_adapter_launches_passes():
    """The faithful chain: every launch recomputed (measured on this chain: lora_dense_fwd 0.497, lora_dense_bwd 0.490 -- one bf16 rounding
    of an output, half its bound), the producer check (backward read the h, the aux and the dx their producers left, bit for bit), the new
    wiring check on all four adapter launches, check 5 with the ADD-mode adapter counted to its GEMM's site."""
    calls, model, *_ = dense_chain()
    assert [(c.meta["stage"], c.meta["layer"]) for c in calls] == [("ln1", 0), ("g", 0), ("lora_g", 0), ("z2", 0), ("lora_z2", 0), ("du", 0), ("lora_du", 0),
                                                                   ("gather_rows2", None), ("dy1", 0), ("lora_dy1", 0)]
    per = SS.recompute_all(calls)
    assert {k: n for k, (n, _w) in per.items()} == {"ln_fwd": 1, "gemm_nt": 3, "gemm_nt_splitk": 1, "gather_rows": 1, "lora_dense_fwd": 2, "lora_dense_bwd": 2}
    print({k: round(w, 3) for k, (_n, w) in per.items()})
    assert all(w <= 1.0 for _n, w in per.values())
    assert 0.2 < per["lora_dense_fwd"][1] <= 0.55 and 0.2 < per["lora_dense_bwd"][1] <= 0.55, per
    SS.check_producers(calls)
    assert SS.check_dense_adapter_wiring(calls, model) == 4
    assert SS.check_dropout_sites(calls) == 1                   # (z2 and lora_z2: one site)
    assert calls[9].a["h"] is None and calls[6].a["h"].shape[0] == DRA < calls[4].a["h_out"].shape[0]


@pytest.mark.parametrize("name", list(DENSE_MUTATIONS))
def test_each_dense_adapter_mutation_fails_the_recomputation(name):
    """tests/lora_dense_ref.py's mutations (the delta not masked, the mask indexed by the pitch, drop_scale left out, GELU before the delta,
    aux after GELU, gelu' missing or from the neighbouring row, s off by 2^-6, the last row block skipped, a fold slab skipped, accumulate
    ignored, the contraction stopping at min(K, N) -- the chain holds K < N and K > N), each applied to what the chain's adapter launches
    computed."""
    make = DENSE_MUTATIONS[name][0]
    mut = DR.mask_by_pitch(H + 8) if name.startswith("mask indexed") else make()          # (the ADD launch of the chain has N = 128)
    calls, *_ = dense_chain(mut)
    with pytest.raises(AssertionError, match="lora_dense_(fwd|bwd)"):
        SS.recompute_all(calls)


def test_each_wiring_change_of_the_dense_adapters_fails_its_check():
    """The adapter's triple differs from its GEMM's (each launch still recomputes from its OWN triple: only check 5 sees it, and the wiring
    check); ``gelu_u`` is another buffer than the du GEMM's; ``dx`` is a fresh buffer; the GELU-mode launch is handed no ``aux`` (every launch
    still recomputes from what it read, and the producer check knows no writer of the buffer: only the wiring check names the mistake);
    backward reads another h than forward wrote; gB lands in a frozen span."""
    calls, model, *_ = dense_chain(wiring="triple")
    assert all(w <= 1.0 for _n, w in SS.recompute_all(calls).values())
    with pytest.raises(AssertionError, match=r"dropout site \(1, 0, 'z2'\): forward and backward carry different triples"):
        SS.check_dropout_sites(calls)
    with pytest.raises(AssertionError, match=r"layer 0 lora_z2\): drop .* is not the GEMM's"):
        SS.check_dense_adapter_wiring(calls, model)
    calls, model, *_ = dense_chain(wiring="gelu_u")
    assert all(w <= 1.0 for _n, w in SS.recompute_all(calls).values())
    SS.check_producers(calls)                                   # (the copy holds the same bits: only the address says it is another buffer)
    with pytest.raises(AssertionError, match=r"layer 0 lora_du\) gelu_u = the GEMM's gelu_bwd_u"):
        SS.check_dense_adapter_wiring(calls, model)
    calls, model, *_ = dense_chain(wiring="fresh_dx")
    with pytest.raises(AssertionError, match=r"layer 0 lora_du\) dx = what the GEMM returned"):
        SS.check_dense_adapter_wiring(calls, model)
    calls, model, *_ = dense_chain(wiring="no_aux")
    assert all(w <= 1.0 for _n, w in SS.recompute_all(calls).values())
    SS.check_producers(calls)                                   # (no recorded call ever wrote u: nothing to compare with)
    with pytest.raises(AssertionError, match="layer 0 du: backward reads a pre-activation, yet the layer's intermediate adapter was handed no aux"):
        SS.check_dense_adapter_wiring(calls, model)
    calls, model, flat, offset, numel = dense_chain()
    h = calls[6].a["h"]
    h.t.view(torch.int16)[5, 3] += 1
    h._cpu = None
    with pytest.raises(AssertionError, match=r"lora_dense_bwd, lora_du\) operand h: 1 of"):
        SS.check_producers(calls)
    # gB in a frozen span
    plan = lambda *frozen: types.SimpleNamespace(frozen=frozenset(frozen), layers={}, word_table=False)      # noqa: E731
    names = SS.names_of(model)
    wg = SS.synth("gemm_tn_grouped", dict(problems=[(torch.zeros(4, H, dtype=bf), torch.zeros(4, H, dtype=bf), model._w["g_Wt"], model._w["g_bt"])],
                                          accumulate=True, alpha=1.0), post=dict(problems=[(model._w["g_Wt"], model._w["g_bt"])]))
    wg.meta.update(stage="gemm_tn_grouped", layer=None)
    calls, model, flat, offset, numel = dense_chain()
    assert SS.check_frozen_writes(calls + [wg], names, plan("b2"), 1, flat, offset, numel) == 4              # gA and gB of two launches
    with pytest.raises(AssertionError, match=r"lora_dense_bwd, stage lora_du layer 0\) writes elements \[\d+, \d+\) of the gradient buffer: the span of the frozen ffn_output.lora_B"):
        SS.check_frozen_writes(calls + [wg], names, plan("ffn_output.lora_B"), 1, flat, offset, numel)
    with pytest.raises(AssertionError, match="stage lora_dy1 layer 0.*the span of the frozen intermediate.lora_A"):
        SS.check_frozen_writes(calls + [wg], names, plan("intermediate.lora_A"), 1, flat, offset, numel)


def test_the_sequence_check_with_dense_adapter_stages():
    """``check_sequence`` with an adapter record: on an adapted layer every present target's stage sits directly behind z1 / g / z2 in
    forward and behind du / dy1 / dctx in backward -- for a subset of the targets, a subset of the layers, in the dense and in both
    sparse top-layer forms; a missing forward stage, a missing backward stage, a swapped order, and an adapter launch on no layer fail."""
    def calls_of(seq):
        out = []
        for st, l in seq:
            c = SS.Call({"lora_z1": "lora_dense_fwd", "lora_dctx": "lora_dense_bwd"}.get(st, st), {})
            c.meta.update(stage=st, layer=l)
            out.append(c)
        return out
    L = 3
    rec = lambda targets, layers: dict(r=4, alpha=8.0, targets=targets, layers=layers)          # noqa: E731
    assert SS.adapter_stages(rec(("query", "ffn_output"), (1,))) == {1: (True, ("ffn_output",))}
    assert SS.adapter_stages((0, 2)) == {0: (True, ()), 2: (True, ())} and SS.adapter_stages(None) == {}

    def fwd(ad):
        return [(s, l) for l in range(L) for s in SS._fwd_form(ad.get(l))]

    def bwd(ad, l, form=SS.BWD_DENSE, dx=True):
        f = SS._bwd_form(form, ad.get(l))
        return [(s, l if s not in ("gather_rows8", "gather_rows1", "scatter_rows_zero", "attn_q_limit") else None) for s in f if dx or s != "dx"]
    all6 = rec(("query", "key", "value", "attention_output", "intermediate", "ffn_output"), (0, 1, 2))
    ad = SS.adapter_stages(all6)
    assert SS._fwd_form(ad[0]) == ("qkv", "lora_fwd", "attn_fwd", "z1", "lora_z1", "ln1", "g", "lora_g", "z2", "lora_z2", "ln2")
    assert SS._bwd_form(SS.BWD_DENSE, ad[0]) == ("ln2_bwd", "du", "lora_du", "dy1", "lora_dy1", "ln1_bwd", "dctx", "lora_dctx", "attn_bwd", "lora_bwd", "dx")
    for form in (SS.BWD_DENSE,) + SS.BWD_TOP_SPARSE:
        seq = fwd(ad) + bwd(ad, 2, form) + bwd(ad, 1) + bwd(ad, 0, dx=False)
        assert SS.check_sequence(calls_of(seq), L, 0, True, all6) == {"fwd": 1, "bwd": 1}
    # a subset of the targets on a subset of the layers, without Q/K/V adapters, next to plain layers
    sub = rec(("intermediate", "ffn_output"), (2,))
    ad2 = SS.adapter_stages(sub)
    good = fwd(ad2) + bwd(ad2, 2, SS.BWD_TOP_SPARSE[0]) + bwd(ad2, 1) + bwd(ad2, 0)
    assert SS._fwd_form(ad2[2]) == ("qkv", "attn_fwd", "z1", "ln1", "g", "lora_g", "z2", "lora_z2", "ln2") and SS._fwd_form(ad2.get(1)) == SS.FWD_LAYER
    assert SS.check_sequence(calls_of(good), L, 0, False, sub) == {"fwd": 1, "bwd": 1}
    assert SS.check_sequence(calls_of(fwd(ad2)), L, 0, False, sub, backward=False) == {"fwd": 1, "bwd": 0}
    swap = lambda seq, a, b: [(b if s == a else a if s == b else s, l) for s, l in seq]        # noqa: E731
    for bad in ([x for x in good if x[0] != "lora_g"],                                         # a missing forward stage
                [x for x in good if x[0] != "lora_dy1"],                                       # a missing backward stage
                swap(good, "lora_du", "du"),                                                   # the adapter in front of its GEMM
                swap(good, "lora_du", "lora_dy1"),                                             # two adapters exchanged
                good + [("lora_g", 2)]):                                                       # a stray adapter launch behind the step
        with pytest.raises(AssertionError):
            SS.check_sequence(calls_of(bad), L, 0, False, sub)
    with pytest.raises(AssertionError, match="a forward pass without backward"):
        SS.check_sequence(calls_of(fwd(ad2) + bwd(ad2, 2)), L, 0, False, sub, backward=False)
    with pytest.raises(AssertionError, match="a dense adapter launch on no layer"):
        SS.check_sequence(calls_of(good[:4] + [("lora_z1", None)] + good[4:]), L, 0, False, sub)
