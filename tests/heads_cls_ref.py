"""The float64 reference of the pretraining heads with a C-CLASS label head (csrc/heads_coop.hip, ``ncls`` = C in 2 .. 16) and the
scale-aware check of their outputs: tests/heads_ref.py with a [C, H] ``classifier1_2``, the label term replaced by the mean C-way
cross-entropy (REF:MMBertForPretraining.py:438-443) and the predicted class per sample.

Not a test module (pytest does not collect it): ``from tests import heads_cls_ref as HCR``.

The oracle cannot state this objective (``fusion_objective`` ends in ``mse_loss``) and the reference never builds a C-wide layer, so
``reference(case)`` assembles it in float64 autograd from the oracle's own pinned pieces: ``O._linear``, ``O.cpc``, the gate
expression of ``fusion_objective``, the pooler / align / 2-way CE lines of ``heads_from_cls`` -- and ``F.cross_entropy(logits, y)``
as the label term.  Outputs as heads_ref's, ``logits`` [B, C] raw, plus ``pred`` [B]: the index of the largest float64 logit.

``restate(case, emu=False, mutation=None)`` is heads_ref.restate's text with the class head's four pieces in place of the
regression head's, on the same ``Num`` values (value + accumulated fp32 magnitude) with the SAME constants (``C_OUT``, ``C_ACC``,
``F_SUM``, ``F_FN``, ``TAU_ACC``) -- the bound is derived, not chosen:

    lo = T Wc2^T + bc2  [B, C]                                  (one workgroup tile, as every K = H product)
    lse_b = max_c lo + log(sum_c exp(lo - max))                 (one thread per sample, classes in order)
    label = sum_b (lse_b - lo[b, y_b]) / B                      (wave butterflies, the waves' partials in order)
    dlo[b, c] = (exp(lo[b, c] - lse_b) - [c == y_b]) / B
    dT += dlo Wc2         gWc2 += d dlo^T T         gbc2 += d colsum(dlo)          (sequential sums: classes / samples in order)

``emu=True`` rounds to fp32 in that order (exp / log correctly rounded; the hardware's are widened through F_FN, as in heads_ref).
Pass = every ratio of ``heads_ref.check`` <= 1 and ``pred`` equal on EVERY sample.

``make_case``: ``heads_ref.make_case`` plus ``classifier1_2.weight`` ~ N(0, (2 / sqrt(H))^2) [C, H], bias 0.1 N(0, 1), labels
uniform in [0, C) with every class present when B >= C.  So that no sample has to be left out of the ``pred`` comparison, every
generated case satisfies ``gap_ratio(case) >= KINK`` (64): each sample's gap between its two largest float64 logits is at least 64
times the larger of those two logits' bounds; the generator re-seeds until it holds (the CPU test asserts it on every case the GPU
test uses).

Calibration (tests/test_heads_cls_reference_cpu.py: every case there; tests/test_heads_cls_gpu.py on an MI355X: 18 + 4 cases).
Largest ratios (elementwise, normwise):

    output       emulation      MI355X
    losses       0.21  0.34     0.32  0.34
    logits/rel   0.22  0.25     0.46  0.44
    dfirst       0.19  0.15     0.42  0.40
    parameters   0.22  0.19     0.51  0.49

The class head's own outputs on the MI355X: logits 0.23 0.28, label loss (aux) 0.32 0.25, classifier1_2 weight 0.18 0.14, bias 0.09
0.07; ``pred`` equal to the float64 argmax on all 985 samples.  The largest, 0.51, is the elementwise ratio of the align weight
gradient at B = 128, H = 256, C = 16 in the model's form -- an output the class head does not touch.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import mmbert_oracle as O
from tests import heads_ref as HR
from tests.gemm_ref import Mutation, _hook, _f32, _c32
from tests.heads_ref import (Num, PARAMS, GATES, CPCS, NW, KINK, cat, tanh, exp, log, sqrt, relu, mm, rowdot, colsum, rowmax,  # noqa: F401
                             _tree_sum, ratios, check, Ref, U_F32, C_OUT, EPS24, F_SUM)

OUTPUTS = HR.OUTPUTS                     # + "pred", compared exactly
C_ACC = 1.0                              # (rowwise_ref's: the factor of 2^-24 acc in the elementwise bound)


@dataclass
class Case(HR.Case):
    C: int = 2
    y: torch.Tensor | None = None        # int64 [B] class labels


# ------------------------------------------------------------------------------------------------ the autograd reference
def reference(c: Case) -> dict:
    """float64 autograd through the oracle's pieces: every output as a float64 CPU tensor (dmlm None without MLM losses), pred int64."""
    p = {k: v.detach().to(torch.float64).clone().requires_grad_(k in PARAMS) for k, v in c.params.items()}
    first = c.first.detach().to(torch.float64).clone().requires_grad_(True)
    B, beta = c.B, _c32(c.beta)
    pooled = torch.tanh(O._linear(first, p, "bert.pooler.dense"))                      # heads_from_cls
    v_rel, s_rel = O._linear(first[B:2 * B], p, "cls.align"), O._linear(first[2 * B:], p, "cls.align")
    v_ap = F.cross_entropy(v_rel.view(-1, 2), c.ap_v.view(-1).long())
    s_ap = F.cross_entropy(s_rel.view(-1, 2), c.ap_s.view(-1).long())
    pt, pv, ps = pooled[:B], pooled[B:2 * B], pooled[2 * B:]

    def gate(x, vname):                                                                # fusion_objective :407-409
        a = F.relu(O._linear(torch.cat((x, x), dim=1), p, "attn"))
        return O._linear(a, p, vname)
    fused = torch.cat((pt * gate(pt, "vt"), pv * gate(pv, "vv"), ps * gate(ps, "vs")), dim=1)
    temp = O._linear(fused, p, "classifier1_1")
    logits = O._linear(temp, p, "classifier1_2")                                       # [B, C]  (REF :314, :415)
    nce = O.cpc(p, "cpc_zt", pt, temp) + O.cpc(p, "cpc_zv", pv, temp) + O.cpc(p, "cpc_za", ps, temp)
    ap = (v_ap + s_ap) / 2.0
    label = F.cross_entropy(logits, c.y.view(-1).long())                               # REF :438-441
    heads = ap + label - beta * nce
    mlm = None
    joint = heads
    if c.nmlm:
        mlm = c.mlm.detach().to(torch.float64).clone().requires_grad_(True)
        joint = _c32(c.alpha) * mlm.mean() + heads
    joint.backward(torch.tensor(_c32(c.d), dtype=torch.float64))
    with torch.no_grad():
        t_rel = O._linear(pt, p, "cls.seq_relationship")
        rel = torch.cat((v_rel, s_rel)).detach()
    out = dict(loss=joint.detach().reshape(1), aux=torch.stack([ap, label, nce]).detach(),
               out5=torch.stack([ap, label, nce, heads, joint]).detach(), logits=logits.detach(), t_rel=t_rel, rel=rel,
               dfirst=first.grad, dmlm=None if mlm is None else mlm.grad, pred=_first_argmax(logits.detach()))
    for n in PARAMS:
        out[n] = c.prior.get(n, torch.zeros_like(c.params[n])).to(torch.float64) + p[n].grad
    return out


def _first_argmax(x):
    """Index of the largest element per row, the lowest index on an exact tie."""
    top = x == x.max(1, keepdim=True).values
    return (top.to(torch.int64).cumsum(1) == 0).sum(1)


# ------------------------------------------------------------------------------------------------ mutations (value-only, on the restatement)
def softmax_over_batch():
    return Mutation("softmax over the batch axis", {"cls_softmax": lambda x, ctx: torch.softmax(ctx["lo"], 0)})


def onehot_dropped():
    return Mutation("one-hot term dropped", {"onehot": lambda x, ctx: x * 0})


def inv_b_dropped():
    return Mutation("1/B dropped in dlo", {"invB": lambda x, ctx: 1.0})


def dT_row0_only():
    return Mutation("dT through row 0 of Wc2 for every class", {"Wc2_dT": lambda W, ctx: W[0:1].expand_as(W).clone()})


def gWc2_rows_permuted():
    return Mutation("gWc2 rows permuted", {"gWc2": lambda g, ctx: torch.roll(g, 1, 0)})


def gbc2_last_class_lost():
    def f(g, ctx):
        g = g.clone()
        g[-1] = 0
        return g
    return Mutation("gbc2 last class lost", {"gbc2": f})


def label_cast_to_zero():
    return Mutation("label read as a float cast to 0", {"y": lambda y, ctx: y * 0})


def pred_second_largest():
    def f(pred, ctx):
        lo = ctx["lo"].clone()
        lo.scatter_(1, pred[:, None], -math.inf)
        return _first_argmax(lo)
    return Mutation("pred = the second largest", {"pred": f})


# ------------------------------------------------------------------------------------------------ sequential sums (one thread, operands in order)
def mm_seq(A: Num, B: Num) -> Num:
    """A [R, K] @ B [K, N] as one thread per output element: an fp32 running sum of fused multiply-adds over k in order (the class
    sums of dT, the sample sums of gWc2); the bound's form is heads_ref.mm's."""
    a, b = A.v, B.v
    if A.emu:
        v = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float64)
        for k in range(a.shape[1]):
            v = _f32(v + a[:, k:k + 1] * b[k:k + 1])
    else:
        v = a @ b
    e = F_SUM * (a.abs() @ b.abs()) + (a * a @ (B.e * B.e) + (A.e * A.e) @ (b * b)).sqrt() + v.abs()
    return Num(v, e, A.emu)


# ------------------------------------------------------------------------------------------------ the restatement
def restate(c: Case, emu=False, mutation=None) -> dict:
    """heads_ref.restate with the class head (see the module docstring): every output as a Num, ``pred`` as an int64 tensor."""
    mut = mutation
    B, H, R, C = c.B, c.H, 3 * c.B, c.C

    def inp(t):
        return Num(t.detach().to(torch.float64).clone(), None, emu)
    p = {k: inp(v) for k, v in c.params.items()}
    X = inp(c.first)
    beta, alpha, d = _c32(c.beta), _c32(c.alpha), _c32(c.d)

    def cst(x):
        return _c32(x) if emu else x

    # ---- forward (heads_ref.restate, unchanged up to the label head)
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
    Wc2 = p["classifier1_2.weight"]                             # [C, H]
    lo = mm(T, Wc2.T) + p["classifier1_2.bias"]                 # [B, C] raw
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

    # ---- the class head: C-way log-sum-exp per sample, the label loss, its seed, the predicted class
    y = _hook(mut, "y", c.y.view(-1).long()).clamp(0, C - 1)
    onehot = _hook(mut, "onehot", F.one_hot(y, C).to(torch.float64))
    mxl = rowmax(lo)                                             # [B, 1] (exact)
    sx = colsum(exp(lo - mxl).T)                                 # classes in order
    lse = mxl.reshape(B) + log(sx)
    pick = Num(lo.v.gather(1, y[:, None]).reshape(B), lo.e.gather(1, y[:, None]).reshape(B), emu)
    se_l = _tree_sum((lse - pick) / float(B))
    soft = exp(lo - lse.reshape(B, 1))
    soft = soft.with_v(_hook(mut, "cls_softmax", soft.v, lo=lo.v))
    dlo = (soft - Num(onehot, None, emu)) / _hook(mut, "invB", float(B))
    pred = _hook(mut, "pred", _first_argmax(lo.v), lo=lo.v)
    heads = ce + se_l - beta * nce
    if c.nmlm:
        ms = colsum(Num(c.mlm.to(torch.float64).reshape(-1, 1), None, emu)).reshape(1)
        joint = alpha * (ms / float(c.nmlm)) + heads
    else:
        joint = heads
    out = dict(loss=joint, aux=cat([ce.reshape(1), se_l.reshape(1), nce]), out5=cat([ce.reshape(1), se_l.reshape(1), nce, heads, joint]),
               logits=lo, t_rel=t_rel, rel=rel, pred=pred)

    # ---- backward
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
    Wd = Wc2.with_v(_hook(mut, "Wc2_dT", Wc2.v))
    dT = mm(dXPc, Wq) + mm_seq(dlo, Wd)                          # dT[b, n] = sum_m dXP_m Wq_m + sum_c dlo[b, c] Wc2[c, n]
    for m in range(3):
        acc(f"{CPCS[m]}.weight", mm(dXP[m].T, T, "wave"))
        acc(f"{CPCS[m]}.bias", colsum(dXP[m]))
    dC = mm(dT, p["classifier1_1.weight"])
    acc("classifier1_1.weight", mm(dT.T, Cc, "wave"))
    acc("classifier1_1.bias", colsum(dT))
    gW = mm_seq(dlo.T, T)                                        # [C, H]: samples in order
    acc("classifier1_2.weight", gW.with_v(_hook(mut, "gWc2", gW.v)))
    gb = colsum(dlo)
    acc("classifier1_2.bias", gb.with_v(_hook(mut, "gbc2", gb.v)))
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


# ------------------------------------------------------------------------------------------------ bounds
def expected(c: Case, ref=None, bounds=None) -> dict:
    """name -> Ref (the autograd value with the restatement's acc, float64, no emulation); "pred" -> the int64 classes."""
    ref = reference(c) if ref is None else ref
    bounds = restate(c) if bounds is None else bounds
    out = {}
    for k in OUTPUTS:
        if ref.get(k) is None:
            continue
        out[k] = Ref(ref[k].reshape(bounds[k].v.shape), bounds[k].e, 0.0, U_F32)
    out["pred"] = ref["pred"]
    return out


def check_all(got: dict, exp: dict, what="", worst=None):
    """heads_ref.check_all; ``pred`` is compared exactly, on every sample."""
    got = dict(got)
    pred = got.pop("pred", None)
    if pred is not None:
        bad = (pred.detach().cpu().reshape(-1).long() != exp["pred"]).nonzero().flatten().tolist()
        assert not bad, f"{what} pred: samples {bad[:8]} differ from the float64 argmax"
    HR.check_all(got, {k: v for k, v in exp.items() if k != "pred"}, what, worst)


def logit_bound(exp_logits: Ref):
    """The elementwise bound of heads_ref.check on the logits: C_OUT 2^-23 |ref| + C_ACC 2^-24 acc."""
    return C_OUT * U_F32 * exp_logits.val.abs() + C_ACC * EPS24 * exp_logits.acc


def gap_ratio(c: Case, exp=None) -> float:
    """min over the samples of (largest - second largest float64 logit) / (the larger of those two logits' bounds)."""
    lg = (expected(c) if exp is None else exp)["logits"]
    top, idx = lg.val.topk(2, dim=1)
    bound = logit_bound(lg).gather(1, idx).max(1).values
    return float(((top[:, 0] - top[:, 1]) / bound).min())


# ------------------------------------------------------------------------------------------------ inputs
def make_case(B, H, seed, C, **kw) -> Case:
    """heads_ref.make_case(B, H, seed, **kw) with a C-class head: classifier1_2.weight ~ N(0, (2 / sqrt(H))^2) [C, H], bias 0.1 N(0, 1),
    labels uniform in [0, C) with every class present when B >= C; re-seeded (seed + 1000, ...) until gap_ratio >= KINK."""
    kw.pop("num_labels", None)
    for attempt in range(50):
        s = seed + 1000 * attempt
        base = HR.make_case(B, H, s, num_labels=7, **kw)
        g = torch.Generator().manual_seed(s * 7919 + C)
        fields = {k: getattr(base, k) for k in ("B", "H", "first", "params", "ap_v", "ap_s", "alpha", "beta", "mlm", "d", "prior")}
        c = Case(sent=None, num_labels=C, C=C, **fields)
        c.params["classifier1_2.weight"] = torch.randn(C, H, generator=g) * (2.0 / math.sqrt(H))
        c.params["classifier1_2.bias"] = torch.randn(C, generator=g) * 0.1
        if c.prior:
            c.prior["classifier1_2.weight"] = torch.randn(C, H, generator=g) * 0.1
            c.prior["classifier1_2.bias"] = torch.randn(C, generator=g) * 0.1
        y = torch.randint(0, C, (B,), generator=g)
        if B >= C:
            y[torch.randperm(B, generator=g)[:C]] = torch.arange(C)
        c.y = y
        if gap_ratio(c) >= KINK:
            return c
    raise AssertionError(f"no case with gap_ratio >= {KINK} for B={B} H={H} C={C} seed={seed}")


# ------------------------------------------------------------------------------------------------ the cases of tests/test_heads_cls_gpu.py: (B, H, C) -- every B with two H, every C with at least three B
GPU_STEP = [(1, 16, 2), (1, 768, 3), (2, 80, 6), (2, 1024, 16), (15, 256, 2), (15, 16, 3), (16, 768, 6), (16, 80, 16), (17, 1024, 2),
            (17, 256, 3), (33, 80, 6), (33, 768, 16), (64, 16, 2), (64, 1024, 6), (127, 768, 6), (127, 80, 3), (128, 256, 16), (128, 16, 2)]
GPU_MODEL_FORM = [(1, 80, 2), (17, 768, 6), (33, 1024, 3), (128, 256, 16)]
DS = (1.0, -0.37, 2.0 ** 10)
NMLM = (0, 3, 256)


def gpu_step_case(i):
    B, H, C = GPU_STEP[i]
    return make_case(B, H, 500 + i, C, alpha=0.6, beta=0.7 if i % 5 else 1.3, nmlm=NMLM[(i // 3) % 3], d=DS[i % 3],
                         ap=("mixed", "zeros", "ones", "mixed")[i % 4])


def gpu_model_form_case(i):
    B, H, C = GPU_MODEL_FORM[i]
    return make_case(B, H, 70 + B, C, alpha=0.8, beta=0.6, nmlm=3, d=-0.37)
