"""The float64 references of the loss options (``model.set_loss_options``) and the scale-aware checks of the kernels behind them.

Not a test module (pytest does not collect it): ``from tests import loss_options_ref as LR``.

Vocabulary cross-entropy with label smoothing (csrc/rowwise.hip, ``ce_row_kernel<.., .., true>`` behind ``mmbert_ce_fwd_smooth`` /
``mmbert_ce_bwd_smooth``): tests/rowwise_ref.py's ``ce_fwd`` / ``ce_bwd`` with the smoothing term added, on the same bf16-rounded
logits and with the fp32 value of eps the C ABI receives.  For a labelled row (0 <= y < V), segment s, count_s labelled rows:

    loss_i        = lse_i - (1 - eps) x[i, y] - (eps / V) sum_{c < V} x[i, c]          loss[s] = sum_i loss_i / count_s
    dlogits[i, c] = (exp(x[i, c] - lse_i) - (1 - eps) [c = y] - eps / V) gscale[s] / count_s     for c < V

and exactly 0 on the pad columns V .. ldv, on unlabelled rows and where gscale is 0; an empty segment's loss is 0.  These are
``torch.nn.functional.cross_entropy(label_smoothing=eps, ignore_index=-100)``'s values and autograd gradients
(tests/test_loss_options_reference_cpu.py compares them in float64).

The check is rowwise_ref's (``check``: elementwise and normwise, ``exact`` values bit for bit) with its constants C_OUT, C_ACC,
TAU_OUT, TAU_ACC untouched.  The error models are rowwise_ref's with, by its stated conventions,

    loss     the row's model gains the new row sum's, by the ``sums`` rule:  acc_s = (eps / V) 4 sum_{c < V} |x_c|
             (loss acc = sum_i (acc_lse_i + acc_s_i) / count + 8 sqrt(count) |loss|)
    dlogits  acc gains |gscale / count| eps / V on the columns c < V

``emu=True`` follows the kernel: the lse through ``rowwise_ref._lse_emu``; the row sum per thread over its 8-column chunks in
ascending order, the lane tree, the four waves in order; the loss term fma(-eps/V, sum, fma(-(1 - eps), x_y, lse)) * inv_count in
fp32 with 1 - eps and eps / V rounded to fp32 on the host; the terms of a segment added in row order; the backward
(exp2((x - lse) log2 e) - (1 - eps) [c = y] - eps / V) * (inv_count * gscale) rounded to bf16.  It takes value-only mutations
(``Mutation``), with which the CPU test shows that the bounds are tight.

The heads' label-loss options (csrc/heads_coop.hip, forward level 7) follow in the second half of this file, with their own header.

Calibration.  The largest ratios (elementwise, normwise) the emulation reached (tests/test_loss_options_reference_cpu.py) and the
MI355X reached (tests/test_ce_smooth_gpu.py: the 36 cases of ``ce_cases()`` plus deterministic mode; tests/test_heads_loss_options_gpu.py:
12 class-head, 32 regression cases and the exact-zero case, both operand forms), under rowwise_ref's / heads_ref's constants as they are:

    cross-entropy   emulation      MI355X            heads          emulation      MI355X
    loss            0.09  0.21     0.10  0.20        losses         0.45  0.77     0.41  0.80
    row_lse         0.14  0.06     0.26  0.07        logits/rel     0.29  0.36     0.55  0.60
    dlogits         0.50  0.33     0.50  0.38        dfirst         0.36  0.34     0.43  0.43
                                                     parameters     0.36  0.50     0.54  0.50

The label head's own outputs on the MI355X: label loss (aux) 0.35 0.35, classifier1_2 weight 0.26 0.17, bias 0.13 0.21.  The heads'
largest, 0.80, is the joint loss's normwise ratio (one element: |error| against TAU-scaled terms) at B = 15, H = 16 under Huber with
tanh; nothing exceeds 1, so no model was widened.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import mmbert_oracle as O
from tests import heads_cls_ref as HCR
from tests import heads_ref as HR
from tests import rowwise_ref as R
from tests.heads_cls_ref import mm_seq, _first_argmax
from tests.heads_ref import Num, KINK, PARAMS, GATES, CPCS, NW, cat, tanh, exp, log, sqrt, relu, mm, rowdot, colsum, rowmax, _tree_sum  # noqa: F401
from tests.rowwise_ref import (Ref, Mutation, check, ratios, _hook, _f32, _c32, _bf, _ref, _seq, seg_of_rows, logits_rows,  # noqa: F401
                               C_OUT, C_ACC, TAU_OUT, TAU_ACC, U_BF16, U_F32, EPS24, CE_MAXC, IGNORE)


def eps32(eps) -> float:
    """The smoothing as the kernel receives it: the C ABI's float."""
    return _c32(float(eps))


# ------------------------------------------------------------------------------------------------ mutations (value-only, on the emulation)
def bwd_eps_over_v_dropped():
    return Mutation("eps/V dropped in the backward", {"bwd_eov": lambda x, ctx: 0.0})


def bwd_eps_over_v_on_pad():
    return Mutation("eps/V subtracted on the pad columns", {"bwd_eov_cols": lambda V, ctx: ctx["ldv"]})


def rowsum_over_ldv():
    return Mutation("sum of x over ldv instead of V", {"sum_cols": lambda V, ctx: ctx["ldv"]})


def one_minus_eps_missing():
    return Mutation("(1 - eps) missing on the label term", {"one_minus": lambda x, ctx: 1.0})


def smoothing_on_unlabelled_rows():
    return Mutation("the smoothing term on an unlabelled row", {"smooth_rows": lambda ok, ctx: torch.ones_like(ok)})


CE_MUTATIONS = (bwd_eps_over_v_dropped, bwd_eps_over_v_on_pad, rowsum_over_ldv, one_minus_eps_missing, smoothing_on_unlabelled_rows)


# ------------------------------------------------------------------------------------------------ cross-entropy, forward
def _rowsum_emu(Xb, ncols):
    """ce_row_kernel<0, .., true>'s row sum on rows Xb [R, ldv] (float64 of bf16): per thread over its chunks, lane tree, waves in order."""
    Rn, ldv = Xb.shape
    x = torch.where((torch.arange(ldv) < ncols)[None, :], Xb, torch.zeros_like(Xb))
    P = x.new_zeros(Rn, CE_MAXC * 256 * 8)
    P[:, :ldv] = x
    P = P.view(Rn, CE_MAXC, 256, 8)
    sx = x.new_zeros(Rn, 256)
    for c in range(CE_MAXC):
        for q in range(8):
            sx = _f32(sx + P[:, c, :, q])
    w = sx.view(Rn, 4, 64)
    while w.shape[-1] > 1:
        h = w.shape[-1] // 2
        w = _f32(w[..., :h] + w[..., h:])
    w = w[..., 0]
    return _f32(_f32(_f32(w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])


def ce_fwd(L, labels, V, bounds, nseg, eps, *, chunk=512, emu=False, mutation=None):
    """mmbert_ce_fwd_smooth: rowwise_ref.ce_fwd (same arguments and return value) with the smoothing term.  eps = 0 IS rowwise_ref.ce_fwd."""
    e = eps32(eps)
    base = R.ce_fwd(L, labels, V, bounds, nseg, chunk=chunk, emu=emu)
    if e == 0.0 and mutation is None:
        return base
    M = labels.numel()
    seg = seg_of_rows(M, bounds, nseg)
    ok = (labels >= 0) & (labels < V)
    count = torch.zeros(nseg, dtype=torch.long).index_add_(0, seg, ok.long())
    inv = 1.0 / count.clamp(min=1).to(torch.float64)
    rows_s = _hook(mutation, "smooth_rows", ok)                          # the rows that get a loss term
    act = torch.nonzero(rows_s).flatten()
    xlab = torch.zeros(M, dtype=torch.float64)
    sumx = torch.zeros(M, dtype=torch.float64)
    sabs = torch.zeros(M, dtype=torch.float64)
    for a in range(0, act.numel(), chunk):
        rows = act[a:a + chunk]
        Xb = logits_rows(L, rows)
        ldv = Xb.shape[1]
        lab = labels[rows]
        xl = Xb.gather(1, lab.clamp(0, ldv - 1)[:, None])[:, 0]
        xlab[rows] = torch.where(ok[rows], xl, torch.zeros_like(xl))
        ncols = _hook(mutation, "sum_cols", V, ldv=ldv)
        if emu:
            sumx[rows] = _rowsum_emu(Xb, ncols)
        else:
            sumx[rows] = Xb[:, :ncols].sum(1)
            sabs[rows] = Xb[:, :ncols].abs().sum(1)
    if emu:
        lse = base["row_lse"]
        ome = _hook(mutation, "one_minus", _c32(1.0 - e))
        eov = _c32(e / V)
        inner = _f32(lse - ome * xlab)                                   # fma(-(1 - eps), x_y, lse)
        inner = torch.where(ok, inner, torch.zeros_like(inner))          # (an unlabelled row under the mutation: no lse, no label)
        terms = _f32(_f32(inner - eov * sumx) * _f32(inv)[seg])
        terms = torch.where(rows_s, terms, torch.zeros_like(terms))
        loss = torch.stack([_seq([terms[i] for i in act[seg[act] == s].tolist()], torch.zeros((), dtype=torch.float64)) for s in range(nseg)])
        return {"loss": loss, "row_lse": lse}
    lse = base["lse64"]
    terms = torch.where(ok, (lse - (1.0 - e) * xlab - (e / V) * sumx) * inv[seg], torch.zeros_like(lse))
    loss = torch.zeros(nseg, dtype=torch.float64).index_add_(0, seg, terms)
    row_acc = base["row_lse"].acc + (e / V) * 4.0 * sabs
    lacc = torch.zeros(nseg, dtype=torch.float64).index_add_(0, seg, torch.where(ok, row_acc * inv[seg], torch.zeros_like(row_acc)))
    lacc = lacc + 8.0 * count.to(torch.float64).sqrt() * loss.abs()
    exact = torch.where(count == 0, torch.zeros_like(loss), torch.full_like(loss, float("nan")))
    return {"loss": _ref(loss, lacc, 0.0, U_F32, None, exact), "row_lse": base["row_lse"], "count": count, "lse64": lse}


# ------------------------------------------------------------------------------------------------ cross-entropy, backward
def ce_bwd(L, labels, V, bounds, nseg, gscale, lse32, eps, *, rows=None, chunk=512, count=None):
    """mmbert_ce_bwd_smooth on the labelled rows: rowwise_ref.ce_bwd's (out_rows, Ref) chunks with the smoothing term in the value and
    |gscale / count| eps / V in the accuracy model (columns c < V)."""
    e = eps32(eps)
    M = labels.numel()
    seg = seg_of_rows(M, bounds, nseg)
    ok = (labels >= 0) & (labels < V)
    if count is None:
        count = torch.zeros(nseg, dtype=torch.long).index_add_(0, seg, ok.long())
    inv = 1.0 / count.clamp(min=1).to(torch.float64)
    src = torch.arange(M) if rows is None else rows.long()
    for j, ref in R.ce_bwd(L, labels, V, bounds, nseg, gscale, lse32, rows=rows, chunk=chunk, count=count):
        if e == 0.0:
            yield j, ref
            continue
        i = src[j]
        ldv = ref.val.shape[1]
        col = torch.arange(ldv)
        sc = (inv[seg[i]] * gscale.to(torch.float64)[seg[i]])[:, None]
        on = (col[None, :] == labels[i][:, None]).to(torch.float64)
        valid = (col < V).to(torch.float64)[None, :]
        val = ref.val + sc * (e * on - (e / V) * valid)
        acc = ref.acc + sc.abs() * (e / V) * valid
        yield j, _ref(val, acc, 0.0, U_BF16, None, ref.exact)


def ce_bwd_emu(L, labels, V, bounds, nseg, gscale, lse32, eps, *, rows=None, ldd=None, mutation=None):
    """The emulated kernel's whole output [n, ldd] bf16 (n = M, or len(rows)): every row it writes, zeros where it writes zeros."""
    e = eps32(eps)
    M = labels.numel()
    seg = seg_of_rows(M, bounds, nseg)
    ok = (labels >= 0) & (labels < V)
    count = torch.zeros(nseg, dtype=torch.long).index_add_(0, seg, ok.long())
    inv = _f32(1.0 / count.clamp(min=1).to(torch.float64))
    src = torch.arange(M) if rows is None else rows.long()
    Xb = logits_rows(L, src)
    ldv = Xb.shape[1]
    out = torch.zeros(src.numel(), ldd or ldv, dtype=torch.bfloat16)
    col = torch.arange(ldv)
    lz = lse32.to(torch.float64)[src]
    lab = labels[src]
    on = col[None, :] == lab[:, None]
    sc = _f32(inv[seg[src]] * _f32(gscale.to(torch.float64))[seg[src]])
    L2E = _c32(1.0 / math.log(2.0))
    pr = _f32(torch.exp2(_f32(_f32(Xb - lz[:, None]) * L2E)))
    pr = torch.where(col[None, :] < V, pr, torch.zeros_like(pr))
    ome = _hook(mutation, "one_minus", _c32(1.0 - e))
    eov = _hook(mutation, "bwd_eov", _c32(e / V))
    pr = torch.where(on, _f32(pr - ome), pr)
    ecols = _hook(mutation, "bwd_eov_cols", V, ldv=ldv)
    pr = torch.where(col[None, :] < ecols, _f32(pr - eov), pr)
    val = _bf(_f32(pr * sc[:, None]))
    written = _hook(mutation, "smooth_rows", ok[src])                    # rows that get the arithmetic above (the others: zeros)
    val = torch.where(written[:, None], val, torch.zeros_like(val))
    out[:, :ldv] = val.to(torch.bfloat16)
    return out


def ce_check_bwd(dl, L, labels, V, bounds, nseg, gscale, lse32, eps, *, rows=None, count=None, what="", worst=None, gathered_from=None):
    """The whole check of a backward output ``dl`` [n, >= ldv] (any device): labelled rows against ``ce_bwd`` through rowwise_ref.check,
    every other row bit-for-bit zero (pad columns and zero-gscale rows through the reference's ``exact``).  Returns (elem, norm)."""
    n = rows.numel() if rows is not None else labels.numel()
    src = torch.arange(n) if rows is None else rows.long()
    labelled = (labels[src] >= 0) & (labels[src] < V)
    el = nm = 0.0
    for j, ref in ce_bwd(L, labels, V, bounds, nseg, gscale, lse32, eps, rows=rows, count=count):
        got = dl[j.to(dl.device)][:, :ref.val.shape[1]]
        r = check(got, ref, f"{what} dlogits", gathered=True)
        el, nm = max(el, r.elem), max(nm, r.norm)
    zero_rows = dl[(~labelled).to(dl.device)].contiguous()
    bad = int((zero_rows.view(torch.int16) != 0).sum())
    assert bad == 0, f"{what}: {bad} elements of unlabelled rows of dlogits are not exactly zero"
    if worst is not None:
        w = worst["ce dlogits"]
        w[0], w[1] = max(w[0], el), max(w[1], nm)
    return el, nm


# ------------------------------------------------------------------------------------------------ the cases of tests/test_ce_smooth_gpu.py
CE_M = 40
CE_SHAPES = ((30522, 30592), (1000, 1000), (13, 16))
CE_EPS = (0.1, 0.5)
CE_SEGS = ((1, None), (3, None), (4, 2))                                 # (nseg, the empty segment)
CE_GS = (0.5, -2.0, 0.0, 1.25)                                           # gscale per segment: a zero and a negative one from nseg 3 on


def ce_bounds(M, nseg, empty=None):
    b = [0] + [M * (s + 1) // nseg for s in range(nseg)]
    if empty is not None:
        b[empty + 1] = b[empty]
    return torch.tensor(b, dtype=torch.int32)


def ce_inputs(V, ldv, nseg, empty, seed, dtype=torch.bfloat16, M=CE_M):
    """tests/test_rowwise_gpu.py's generator at (V, ldv), on the CPU: pads 4 above the row max, every third row uniform, every fifth
    labelled row peaked; half of the rows labelled, rows 0 .. 2 with the ignored labels V, ldv - 1 (V - 1 + 1 without a pad) and -1,
    rows 3 .. with the columns at the chunk and thread edges, the rest of the unlabelled rows -100."""
    lab = R.ce_labels(M, V, ldv, seed, frac=0.5, edge=False)
    full = R.ce_labels(max(M, 64), V, ldv, seed, frac=0.5, edge=True)    # its first rows: the odd labels, then the edge columns
    n_odd = 3 if ldv > V else 2
    edge = full[n_odd:]
    edge = edge[(edge >= 0) & (edge < V)]
    k = min(int(edge.numel()), M // 3)
    pick = edge[torch.linspace(0, edge.numel() - 1, k).round().long()] if k else edge
    lab[:3] = torch.tensor([V, ldv - 1 if ldv > V else V, -1])
    lab[3:3 + k] = pick
    X = R.ce_logits(M, V, ldv, seed, kind="mixed", dtype=torch.float32)
    X = R.make_peaked(X, lab, V, torch.arange(0, M, 5))
    if ldv > V:
        X[:, V:] = X[:, :V].max(1, keepdim=True).values + 4.0
    return X.to(dtype), lab, ce_bounds(M, nseg, empty)


def ce_cases():
    """(V, ldv, eps, dtype, nseg, empty, seed) of every case the GPU test runs."""
    out = []
    for si, (V, ldv) in enumerate(CE_SHAPES):
        for eps in CE_EPS:
            for dtype in (torch.bfloat16, torch.float32):
                for nseg, empty in CE_SEGS:
                    out.append((V, ldv, eps, dtype, nseg, empty, 100 * si + 10 * nseg + int(eps * 10)))
    return out


def ce_compact_rows(lab, V):
    """The compact backward's row list: the labelled rows in order, then rows 0 and 2 (ignored labels: V and -1)."""
    act = torch.nonzero((lab >= 0) & (lab < V)).flatten()
    return torch.cat([act, torch.tensor([0, 2])]).int()


# ================================================================================================ the label loss's options (csrc/heads_coop.hip)
# The heads' float64 reference and restatement with the label term of forward level 7 replaced: tests/heads_ref.py's regression head
# with L1 / Huber, tests/heads_cls_ref.py's class head with class weights and label smoothing.  ``reference`` is float64 autograd
# through the oracle's pinned pieces with torch's own loss call as the label term; ``restate`` is heads_cls_ref.restate's text (itself
# heads_ref.restate's) with level 7's new statements, on the same ``Num`` arithmetic and the same constants:
#
#   regression   d = v - y (v = the logit, through tanh when tanh_lo);  L1: sum_b |d| / B, seed sign(d) / B tanh';  Huber(delta):
#                0.5 d^2 / B where |d| <= delta else delta (|d| - 0.5 delta) / B, seed d / B or delta sign(d) / B, times tanh'
#   class head   W = sum_b w[y_b] and SW = sum_c w_c as sequential sums (samples / classes in order), k1 = (1 - eps) / W, k2 = eps / (C W),
#                term_b = k1 w[y_b] (lse_b - l[b, y_b]) + k2 sum_c w_c (lse_b - l[b, c])   (wave butterflies, the waves' partials in order)
#                dlo[b, k] = k1 w[y_b] (p[b, k] - [k == y_b]) + k2 (SW p[b, k] - w_k)
#
# L1 and Huber have kinks: every generated case keeps |d| (L1) and ||d| - delta| (Huber) at least KINK (heads_ref's 64) logit bounds
# away from them on every sample (``loss_kink_ratio``); ``make_regression_case`` re-seeds until that holds.
KINDS = ("mse", "l1", "huber")


@dataclass
class Opts:
    kind: str = "mse"
    delta: float = 1.0
    eps: float = 0.0
    weight: torch.Tensor | None = None        # fp32 [C]

    @property
    def default(self):
        return self.kind == "mse" and self.eps == 0.0 and self.weight is None


def _is_cls(c) -> bool:
    return getattr(c, "C", 0) > 0


# ------------------------------------------------------------------------------------------------ mutations (value-only, on the restatement)
def weights_not_normalised():
    return Mutation("weights not normalised by W", {"W": lambda W, ctx: torch.ones_like(W)})


def W_taken_as_B():
    return Mutation("W taken as B", {"W": lambda W, ctx: torch.full_like(W, float(ctx["B"]))})


def sum_w_replaced_by_C():
    return Mutation("sum_c w_c replaced by C", {"SW": lambda S, ctx: torch.full_like(S, float(ctx["C"]))})


def l1_seed_without_tanh():
    return Mutation("L1 seed without tanh'", {"dlo_tanh": lambda x, ctx: 1.0})


def huber_delta_squared():
    return Mutation("Huber using delta^2", {"delta_out": lambda d, ctx: d * d})


def sign_zero_is_one():
    return Mutation("sign(0) = 1", {"sign": lambda s, ctx: torch.where(ctx["d"] == 0, torch.ones_like(s), s)})


def heads_one_minus_eps_missing():
    return Mutation("(1 - eps) missing on the label term", {"one_minus": lambda x, ctx: 1.0})


# ------------------------------------------------------------------------------------------------ the autograd reference
def reference(c, o: Opts) -> dict:
    """float64 autograd through the oracle's pieces (heads_cls_ref.reference's assembly) with torch's loss call as the label term."""
    p = {k: v.detach().to(torch.float64).clone().requires_grad_(k in PARAMS) for k, v in c.params.items()}
    first = c.first.detach().to(torch.float64).clone().requires_grad_(True)
    B, beta = c.B, _c32(c.beta)
    pooled = torch.tanh(O._linear(first, p, "bert.pooler.dense"))
    v_rel, s_rel = O._linear(first[B:2 * B], p, "cls.align"), O._linear(first[2 * B:], p, "cls.align")
    v_ap = F.cross_entropy(v_rel.view(-1, 2), c.ap_v.view(-1).long())
    s_ap = F.cross_entropy(s_rel.view(-1, 2), c.ap_s.view(-1).long())
    pt, pv, ps = pooled[:B], pooled[B:2 * B], pooled[2 * B:]

    def gate(x, vname):
        a = F.relu(O._linear(torch.cat((x, x), dim=1), p, "attn"))
        return O._linear(a, p, vname)
    fused = torch.cat((pt * gate(pt, "vt"), pv * gate(pv, "vv"), ps * gate(ps, "vs")), dim=1)
    temp = O._linear(fused, p, "classifier1_1")
    logits = O._linear(temp, p, "classifier1_2")
    nce = O.cpc(p, "cpc_zt", pt, temp) + O.cpc(p, "cpc_zv", pv, temp) + O.cpc(p, "cpc_za", ps, temp)
    ap = (v_ap + s_ap) / 2.0
    pred = None
    if _is_cls(c):
        w = None if o.weight is None else o.weight.to(torch.float64)
        label = F.cross_entropy(logits, c.y.view(-1).long(), weight=w, label_smoothing=_c32(o.eps))
        pred = _first_argmax(logits.detach())
        out_logits = logits
    else:
        out_logits = torch.tanh(logits) if c.num_labels == 1 else logits
        v, t = out_logits.view(-1), c.sent.to(torch.float64).view(-1)
        if o.kind == "l1":
            label = F.l1_loss(v, t)
        elif o.kind == "huber":
            label = F.huber_loss(v, t, delta=_c32(o.delta))
        else:
            label = F.mse_loss(v, t)
    heads = ap + label - beta * nce
    mlm, joint = None, heads
    if c.nmlm:
        mlm = c.mlm.detach().to(torch.float64).clone().requires_grad_(True)
        joint = _c32(c.alpha) * mlm.mean() + heads
    joint.backward(torch.tensor(_c32(c.d), dtype=torch.float64))
    with torch.no_grad():
        t_rel = O._linear(pt, p, "cls.seq_relationship")
        rel = torch.cat((v_rel, s_rel)).detach()
    out = dict(loss=joint.detach().reshape(1), aux=torch.stack([ap, label, nce]).detach(),
               out5=torch.stack([ap, label, nce, heads, joint]).detach(), logits=out_logits.detach(), t_rel=t_rel, rel=rel,
               dfirst=first.grad, dmlm=None if mlm is None else mlm.grad)
    if pred is not None:
        out["pred"] = pred
    for n in PARAMS:
        out[n] = c.prior.get(n, torch.zeros_like(c.params[n])).to(torch.float64) + p[n].grad
    return out


# ------------------------------------------------------------------------------------------------ the restatement
def _seq_sum(x: Num) -> Num:
    """One thread adds the elements of a vector in order (W over the samples, sum_c w_c over the classes)."""
    v = x.v.reshape(-1)
    if x.emu:
        s = torch.zeros((), dtype=torch.float64)
        for q in v:
            s = _f32(s + q)
    else:
        s = v.sum()
    e = HR.F_SUM * v.abs().sum() + (x.e.reshape(-1) ** 2).sum().sqrt() + s.abs()
    return Num(s.reshape(()), e.reshape(()), x.emu)


def _where(m, a: Num, b: Num) -> Num:
    return Num(torch.where(m, a.v, b.v), torch.where(m, a.e, b.e), a.emu)


def restate(c, o: Opts, emu=False, mutation=None) -> dict:
    """heads_ref.restate / heads_cls_ref.restate with level 7's label term as the options state it (see above): every output as a Num
    (``pred`` an int64 tensor for a class head).  With default options the values are those restatements'."""
    mut = mutation
    cls = _is_cls(c)
    B, H, R = c.B, c.H, 3 * c.B

    def inp(t):
        return Num(t.detach().to(torch.float64).clone(), None, emu)
    p = {k: inp(v) for k, v in c.params.items()}
    X = inp(c.first)
    beta, alpha, d = _c32(c.beta), _c32(c.alpha), _c32(c.d)

    def cst(x):
        return _c32(x) if emu else x

    # ---- forward (heads_ref.restate, unchanged up to the label term)
    P = tanh(mm(X, p["bert.pooler.dense.weight"].T) + p["bert.pooler.dense.bias"].v)
    rel = mm(X[B:], p["cls.align.weight"].T) + p["cls.align.bias"]
    Wat = p["attn.weight"]
    Wsum = Wat[:, :H] + Wat[:, H:]
    Apre = mm(P, Wsum.T) + p["attn.bias"]
    t_rel = mm(P[:B], p["cls.seq_relationship.weight"].T) + p["cls.seq_relationship.bias"]
    A = relu(Apre)
    vrows = cat([Num(p[f"{GATES[m]}.weight"].v.expand(B, H).clone(), None, emu) for m in range(3)])
    vb = torch.cat([p[f"{GATES[m]}.bias"].v.expand(B) for m in range(3)])
    g = rowdot(A, vrows) + vb
    nx = sqrt(rowdot(P, P))
    Cc = cat([P[m * B:(m + 1) * B] * g[m * B:(m + 1) * B].reshape(B, 1) for m in range(3)], 1)
    T = mm(Cc, p["classifier1_1.weight"].T) + p["classifier1_1.bias"]
    XP = cat([mm(T, p[f"{CPCS[m]}.weight"].T) + p[f"{CPCS[m]}.bias"] for m in range(3)])
    Wc2 = p["classifier1_2.weight"]
    lo = mm(T, Wc2.T) + p["classifier1_2.bias"]                  # [B, C] raw, or [B, 1]
    ny = sqrt(rowdot(XP, XP))
    wgt = cst(-beta / B)
    eye = torch.eye(B, dtype=torch.float64)
    dS, rsum, csum, nce_parts = [], [], [], []
    for m in range(3):
        sl = slice(m * B, (m + 1) * B)
        S = mm(P[sl], XP[sl].T) / (nx[sl].reshape(B, 1) * ny[sl].reshape(1, B))
        mx = rowmax(S)
        ex = exp(S - mx)
        se = rowdot(ex, Num(torch.ones_like(ex.v), None, emu), width=1)
        sm = ex / se.reshape(B, 1)
        ds = wgt * (sm - Num(eye, None, emu))
        dS.append(ds)
        rsum.append(rowdot(ds, S, width=1))
        csum.append(colsum(ds * S, parts=NW))
        diag = Num((S.v * eye).sum(1), (S.e * eye).sum(1), emu)
        term = (mx.reshape(B) + log(se) - diag) / float(B)
        nce_parts.append(colsum(term.reshape(B, 1), parts=NW).reshape(1))
    nce = nce_parts[0] + nce_parts[1] + nce_parts[2]
    y2 = torch.cat([c.ap_v, c.ap_s]).to(torch.float64)
    a0, a1 = rel[:, 0], rel[:, 1]
    mxr = Num(torch.maximum(a0.v, a1.v), torch.maximum(a0.e, a1.e), emu)
    lse2 = mxr + log(exp(a0 - mxr) + exp(a1 - mxr))
    sc = cst(0.5 / B)
    picked = Num(torch.where(y2 > 0, a1.v, a0.v), torch.where(y2 > 0, a1.e, a0.e), emu)
    ce = _tree_sum((lse2 - picked) * sc)
    drel = cat([((exp(a0 - lse2) - (y2 == 0).double()) * sc).reshape(2 * B, 1), ((exp(a1 - lse2) - (y2 == 1).double()) * sc).reshape(2 * B, 1)], 1)

    # ---- level 7's label term
    pred = None
    if cls:
        C = c.C
        logits = lo
        y = c.y.view(-1).long().clamp(0, C - 1)
        onehot = F.one_hot(y, C).to(torch.float64)
        mxl = rowmax(lo)
        sx = colsum(exp(lo - mxl).T)
        lse = mxl.reshape(B) + log(sx)
        pick = Num(lo.v.gather(1, y[:, None]).reshape(B), lo.e.gather(1, y[:, None]).reshape(B), emu)
        soft = exp(lo - lse.reshape(B, 1))
        pred = _first_argmax(lo.v)
        if o.eps == 0.0 and o.weight is None:
            se_l = _tree_sum((lse - pick) / float(B))
            dlo = (soft - Num(onehot, None, emu)) / float(B)
        else:
            e32 = eps32(o.eps)
            wv = torch.ones(C, dtype=torch.float64) if o.weight is None else o.weight.to(torch.float64)
            wN = Num(wv.clone(), None, emu)
            wy = Num(wv[y], None, emu)
            W = _seq_sum(wy)
            W = W.with_v(_hook(mut, "W", W.v, B=B))
            SW = _seq_sum(wN)
            SW = SW.with_v(_hook(mut, "SW", SW.v, C=C))
            ome = _hook(mut, "one_minus", cst(1.0 - e32))
            k1 = Num(torch.tensor(ome, dtype=torch.float64), None, emu) / W
            k2 = Num(torch.tensor(e32, dtype=torch.float64), None, emu) / (float(C) * W)
            a1_ = k1 * wy                                                       # [B]
            smc = mm_seq(lse.reshape(B, 1) - lo, wN.reshape(C, 1)).reshape(B)    # sum_c w_c (lse_b - l[b, c]), classes in order
            se_l = _tree_sum(a1_ * (lse - pick) + k2 * smc)
            dlo = a1_.reshape(B, 1) * (soft - Num(onehot, None, emu)) + k2 * (SW * soft - wN.reshape(1, C))
    else:
        tanh_lo = c.num_labels == 1
        logits = tanh(lo) if tanh_lo else lo
        vlo = logits.reshape(B)
        dd = vlo - Num(c.sent.to(torch.float64), None, emu)
        dtanh = (1.0 - vlo * vlo) if tanh_lo else 1.0
        if o.kind != "mse":
            dtanh = _hook(mut, "dlo_tanh", dtanh)
        if o.kind == "mse":
            se_l = _tree_sum(dd * dd / float(B))
            dlo = (2.0 * dd / float(B) * dtanh).reshape(B, 1)
        else:
            ad = Num(dd.v.abs(), dd.e, emu)
            sg = Num(_hook(mut, "sign", torch.sign(dd.v), d=dd.v), None, emu)
            if o.kind == "l1":
                se_l = _tree_sum(ad / float(B))
                gsd = sg
            else:
                dl = _c32(o.delta)
                dl_out = _hook(mut, "delta_out", dl)
                inside = ad.v <= dl
                se_l = _tree_sum(_where(inside, 0.5 * dd * dd / float(B), dl_out * (ad - 0.5 * dl_out) / float(B)))
                gsd = _where(inside, dd, dl_out * sg)
            dlo = (gsd / float(B) * dtanh).reshape(B, 1)
    heads = ce + se_l - beta * nce
    if c.nmlm:
        ms = colsum(Num(c.mlm.to(torch.float64).reshape(-1, 1), None, emu)).reshape(1)
        joint = alpha * (ms / float(c.nmlm)) + heads
    else:
        joint = heads
    out = dict(loss=joint, aux=cat([ce.reshape(1), se_l.reshape(1), nce]), out5=cat([ce.reshape(1), se_l.reshape(1), nce, heads, joint]),
               logits=logits, t_rel=t_rel, rel=rel)
    if cls:
        out["pred"] = pred

    # ---- backward (heads_cls_ref.restate / heads_ref.restate, unchanged: dlo keeps its shape and meaning)
    def acc(name, s):
        prior = Num(c.prior.get(name, torch.zeros_like(c.params[name])).to(torch.float64), None, emu)
        out[name] = prior + d * s.reshape(prior.v.shape)

    dPc, dXP = [], []
    for m in range(3):
        sl = slice(m * B, (m + 1) * B)
        XPn = XP[sl] / ny[sl].reshape(B, 1)
        Xn = P[sl] / nx[sl].reshape(B, 1)
        cx = P[sl] / nx[sl].reshape(B, 1) * rsum[m].reshape(B, 1)
        cy = XP[sl] / ny[sl].reshape(B, 1) * csum[m].reshape(B, 1)
        dPc.append((mm(dS[m], XPn, "wave") - cx) / nx[sl].reshape(B, 1))
        dXP.append((mm(dS[m].T, Xn, "wave") - cy) / ny[sl].reshape(B, 1))
    dPc, dXPc = cat(dPc), cat(dXP, 1)
    Wq = cat([p[f"{CPCS[m]}.weight"] for m in range(3)])
    dT = mm(dXPc, Wq) + (mm_seq(dlo, Wc2) if cls else dlo * Wc2)
    for m in range(3):
        acc(f"{CPCS[m]}.weight", mm(dXP[m].T, T, "wave"))
        acc(f"{CPCS[m]}.bias", colsum(dXP[m]))
    dC = mm(dT, p["classifier1_1.weight"])
    acc("classifier1_1.weight", mm(dT.T, Cc, "wave"))
    acc("classifier1_1.bias", colsum(dT))
    acc("classifier1_2.weight", mm_seq(dlo.T, T) if cls else colsum(dlo * T))
    acc("classifier1_2.bias", colsum(dlo))
    dCr = cat([dC[:, m * H:(m + 1) * H] for m in range(3)])
    dg = rowdot(dCr, P)
    dP0 = dCr * g.reshape(R, 1) + dPc
    mask = (Apre.v > 0).to(torch.float64)
    dA = Num(mask, None, emu) * (dg.reshape(R, 1) * vrows)
    E = dg.reshape(R, 1) * A
    dP = mm(dA, Wsum) + dP0
    dpre = dP * (1.0 - P * P)
    gA = mm(dA.T, P, "wave")
    acc("attn.weight", cat([gA, gA], 1))
    acc("attn.bias", colsum(dA))
    for m in range(3):
        sl = slice(m * B, (m + 1) * B)
        acc(f"{GATES[m]}.weight", colsum(E[sl]))
        acc(f"{GATES[m]}.bias", colsum(dg[sl].reshape(B, 1)))
    Wal = p["cls.align.weight"]
    dal = drel[:, 0:1] * Wal[0:1] + drel[:, 1:2] * Wal[1:2]
    dfirst0 = mm(dpre, p["bert.pooler.dense.weight"])
    out["dfirst"] = d * cat([dfirst0[:B], dfirst0[B:] + dal])
    acc("bert.pooler.dense.weight", mm(dpre.T, X, "wave"))
    acc("bert.pooler.dense.bias", colsum(dpre))
    acc("cls.align.weight", mm(drel.T, X[B:], "wave"))
    acc("cls.align.bias", colsum(drel))
    out["dmlm"] = Num(torch.full((c.nmlm,), d, dtype=torch.float64), None, emu) * cst(alpha / c.nmlm) if c.nmlm else None
    return out


def expected(c, o: Opts, ref=None, bounds=None) -> dict:
    """name -> Ref: the autograd value with the restatement's acc (heads_ref.expected / heads_cls_ref.expected under the options)."""
    ref = reference(c, o) if ref is None else ref
    bounds = restate(c, o) if bounds is None else bounds
    out = {}
    for k in HR.OUTPUTS:
        if ref.get(k) is None:
            continue
        out[k] = Ref(ref[k].reshape(bounds[k].v.shape), bounds[k].e, 0.0, U_F32)
    if _is_cls(c):
        out["pred"] = ref["pred"]
    return out


def check_all(got: dict, exp: dict, what="", worst=None):
    if "pred" in exp:
        HCR.check_all(got, exp, what, worst)
    else:
        HR.check_all(got, exp, what, worst)


def emulated(c, o: Opts, mutation=None) -> dict:
    """The emulation's outputs as plain tensors (what a kernel would hand to ``check_all``)."""
    r = restate(c, o, emu=True, mutation=mutation)
    return {k: (v.v if isinstance(v, Num) else v) for k, v in r.items() if v is not None}


def loss_kink_ratio(c, o: Opts, exp=None) -> float:
    """min over the samples of the distance of d = logit - target from the loss's kink (L1: 0; Huber: +-delta) in units of the logit's
    elementwise bound.  inf for a loss without a kink."""
    if _is_cls(c) or o.kind == "mse":
        return math.inf
    lg = (expected(c, o) if exp is None else exp)["logits"]
    bound = HCR.logit_bound(lg).reshape(-1)
    dv = (lg.val.reshape(-1) - c.sent.to(torch.float64)).abs()
    dist = dv if o.kind == "l1" else (dv - _c32(o.delta)).abs()
    return float((dist / bound).min())


# ------------------------------------------------------------------------------------------------ the cases of tests/test_heads_loss_options_gpu.py
CLS_SHAPES = ((1, 16, 2), (2, 80, 6), (17, 768, 6), (128, 256, 16))
CLS_VARIANTS = ("weights", "smoothing", "both")
REG_B, REG_H = (1, 15, 33, 128), (16, 768)
HUBER_DELTA = 0.5


def class_weights_for(C, seed):
    g = torch.Generator().manual_seed(9000 + seed)
    return torch.exp(0.7 * torch.randn(C, generator=g)).to(torch.float32)


def cls_case(i):
    """(case, Opts) number i of the class head: CLS_SHAPES x CLS_VARIANTS."""
    (B, H, C), var = CLS_SHAPES[i // 3], CLS_VARIANTS[i % 3]
    c = HCR.make_case(B, H, 800 + i, C, alpha=0.6, beta=0.7, nmlm=(0, 3, 256)[i % 3], d=HCR.DS[i % 3])
    o = Opts(eps=0.1 if var != "weights" else 0.0, weight=class_weights_for(C, i) if var != "smoothing" else None)
    return c, o


def make_regression_case(B, H, seed, o: Opts, **kw):
    """heads_ref.make_case re-seeded (seed + 1000, ...) until loss_kink_ratio >= KINK: no sample is ever left out of a comparison."""
    for attempt in range(50):
        c = HR.make_case(B, H, seed + 1000 * attempt, **kw)
        if loss_kink_ratio(c, o) >= KINK:
            return c
    raise AssertionError(f"no case with loss_kink_ratio >= {KINK} for B={B} H={H} seed={seed}")


def reg_cases():
    """(B, H, tanh_lo, kind) of every regression case."""
    return [(B, H, t, k) for B in REG_B for H in REG_H for t in (0, 1) for k in ("l1", "huber")]


def reg_case(i):
    B, H, t, k = reg_cases()[i]
    o = Opts(kind=k, delta=HUBER_DELTA)
    c = make_regression_case(B, H, 600 + i, o, num_labels=1 if t else 7, alpha=0.6, beta=0.7, nmlm=(0, 3, 256)[i % 3], d=HCR.DS[i % 3])
    return c, o


def exact_zero_case(B=16, H=64, bias=0.375):
    """classifier1_2.weight = 0 and bias b: every logit is exactly b; the targets equal b on the even samples (d = 0 exactly: the L1
    seed there must be exactly 0, sign(0) = 0 as torch), b -+ 1 on the others."""
    c = HR.make_case(B, H, 4242, num_labels=7, alpha=0.6, beta=0.7, nmlm=3, d=1.0)
    c.params["classifier1_2.weight"] = torch.zeros(1, H)
    c.params["classifier1_2.bias"] = torch.tensor([bias])
    t = torch.full((B,), bias)
    t[1::4] += 1.0
    t[3::4] -= 1.0
    c.sent = t
    return c, Opts(kind="l1")
