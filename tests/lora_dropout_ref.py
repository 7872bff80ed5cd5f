"""A float64 reference for the adapter kernels under the dropout of their INPUT (csrc/lora.hip: mmbert_lora_qkv_fwd_drop / _bwd_drop,
mmbert_lora_dense_fwd_drop / _bwd_drop) and the scale-aware check of their outputs.

Not a test module (pytest does not collect it): ``from tests import lora_dropout_ref as XR``.  The pattern is tests/lora_ref.py's and
tests/lora_dense_ref.py's, whose helpers, input families and constants it takes; the mask comes from tests/rng_ref.py alone.

The mask.  ``in_drop`` = (stream, thr16, c), c = 1 / (1 - thr16 / 65536) as the fp32 value the kernel gets.  Element (m, k) of a seam input
of LOGICAL width K is kept iff rng_ref.keep_at(stream, row(m) * K + k, thr16), the index a 64-bit integer (the pair counter wraps mod 2^32
inside keep_at); row(m) = m, or rows[m] where a row list is given (the dense backward on gathered rows).  ``Kp`` is that 0 / 1 matrix; the
q / k / v adapters of a call share it.  thr16 = 0: Kp = 1, c is not applied, and every function below equals lora_ref's / lora_dense_ref's.

``emu=False`` is the reference, float64 with no intermediate rounding (s = scale):

    fwd   h  = c * (Kp . x) A^T                  y  = y + s * h B^T            (the epilogues of the seam as they are: GEMM mask / GELU)
    bwd   g  = c * dy B                          dx = dx + s * Kp . (g A)      [* gelu'(u) on the FFN-down seam]
          dA = [dA +] s * g^T (Kp . x)           dB = [dB +] s * dy^T h        (h: the bf16 tensor forward wrote, or recomputed)

``emu=True`` adds the kernels' documented roundings to those of the two older references: a dropped element of x is +0 (a select: a NaN
there does not travel); c is ONE fp32 multiply on the finished fp32 accumulator of h and of g, before their bf16 rounding; an element of
dx / dres that the mask dropped keeps the bits of dx_old / dres_in (``Ref.exact``).

``check(got, ref)`` is the older references' bound,

    |got - ref| <= C_OUT * u_out * |ref| + C_ACC * 2^-24 * acc + C_MID * 2^-9 * mid + extra,        C_OUT = 2, C_ACC = 0.75, C_MID = 4,

with ``acc`` and ``mid`` taken on the MASKED operands and with c folded in: sqrt(K) c |Kp . x| |A|^T under h, c sqrt(N) |dy| |B| under g,
and so on through every product they feed.

Calibration (tests/test_lora_dropout_reference_cpu.py): emu=True against emu=False over M in {1, 65, 257}; q / k / v at H in {64, 768};
dense at (K, N) in {(64, 64), (128, 832), (832, 128)}; r in {4, 8, 16}; p in {0.1, 0.5} and thr16 = 1; lora_ref.DISTS.  Rule: the largest
error / bound is at most 0.5.  Measured (the CPU test prints the table):

    output            real    cancel   scaled   zeros         output               real    cancel   scaled   zeros
    qkv: h            0.494   0.496    0.494    0.494         dense: h             0.497   0.492    0.497    0.497
    qkv: qkv          0.491   0.493    0.494    0.493         dense: y (ADD)       0.486   0.494    0.492    0.494
    qkv: dres         0.480   0.493    0.493    0.486         dense: y (ADD, p=.1) 0.487   0.496    0.494    0.493
    qkv: dA           0.410   0.387    0.452    0.232         dense: aux           0.486   0.494    0.492    0.494
    qkv: dB           0.210   0.210    0.236    0.131         dense: y (GELU)      0.488   0.497    0.497    0.489
                                                              dense: dx            0.490   0.496    0.489    0.495
                                                              dense: dx (gelu')    0.495   0.496    0.494    0.497
                                                              dense: dA            0.407   0.456    0.465    0.230
                                                              dense: dB            0.210   0.210    0.249    0.124

(y (ADD, p=.1): with the GEMM's own output mask on top of the input mask.)  The extra fp32 multiply by c stays inside: its
2^-24 |c * accumulator| is at most a 1 / sqrt(K) fraction of what ``acc`` already grants the accumulation itself (sqrt(K) c |Kp . x| |A|^T),
so no term was added and no constant enlarged.  The smallest margin of a mutation is in the CPU test's docstring.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import gemm_ref as G
from tests import lora_dense_ref as DR
from tests import lora_ref as LR
from tests import rng_ref as RNG
from tests.gemm_ref import GELUP_ABS, GELU_ABS, gelu64, gelu_grad64
from tests.lora_ref import DISTS, Mutation, _abs, _hook, _prod, _token_sum

C_OUT, C_ACC, C_MID = LR.C_OUT, LR.C_ACC, LR.C_MID
U_BF16, U_F32, EPS24, U_MID = LR.U_BF16, LR.U_F32, LR.EPS24, LR.U_MID
ADD, GELU = DR.ADD, DR.GELU
Ref, ratio, check = DR.Ref, DR.ratio, DR.check
walk = LR.walk

_f32, _bf, _c32 = G._f32, G._bf, G._c32

SITES = {"qkv": 3, "attention_output": 4, "intermediate": 5, "ffn_output": 6}      # layer i: 8 * i + offset


def in_drop(p, seed, site):
    """(stream, thr16, c) as ops.make_drop forms it, from tests/rng_ref.py alone; p <= 0: (0, 0, 1.0)."""
    t = RNG.thr16(p)
    return (RNG.rng_stream(seed, site), t, RNG.drop_scale(t)) if t else (0, 0, 1.0)


def in_drop_thr(thr16, seed, site):
    return (RNG.rng_stream(seed, site), int(thr16), RNG.drop_scale(int(thr16)))


# ------------------------------------------------------------------------------------------------ the mask
def keep_matrix(M, K, drop, rows=None, *, mutation=None, what="x", target=None):
    """[M, K] float64 0 / 1.  ``rows``: the site row of every local row (any integer sequence; None: the identity)."""
    stream, thr16, _ = drop if drop is not None else (0, 0, 1.0)
    if not thr16:
        return torch.ones(M, K, dtype=torch.float64)
    r = np.arange(M, dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.int64).astype(np.uint64)
    r = _hook(mutation, "site_rows", r, M=M, given=rows is not None)
    pitch = _hook(mutation, "mask_pitch", K)
    idx = r[:, None] * np.uint64(pitch) + np.arange(K, dtype=np.uint64)[None, :]
    idx = _hook(mutation, "mask_index", idx)
    stream = _hook(mutation, "stream", stream, what=what, target=target)
    return torch.from_numpy(RNG.keep_at(stream, idx, thr16).astype(np.float64))


def _c(drop, mutation, stage):
    """c as the kernel applies it (fp32), 1 without a mask."""
    if drop is None or not drop[1]:
        return 1.0
    return _hook(mutation, stage, _c32(drop[2]))


def _masked(x64, Kp):
    return torch.where(Kp > 0, x64, torch.zeros_like(x64))           # a select: a NaN in a dropped element does not travel


def _times_c(acc, c, emu):
    """The finished accumulator times c: one fp32 multiply."""
    if c == 1.0:
        return acc
    return _f32(acc * c) if emu else acc * c


# ------------------------------------------------------------------------------------------------ mutations (on the mask and on c)
def mask_by_pitch(ld):
    return Mutation(f"mask indexed by row * {ld} (the row pitch) instead of K", {"mask_pitch": lambda K, ctx: ld})


def mask_of_next_row():
    return Mutation("mask of row m + 1", {"site_rows": lambda r, ctx: r + np.uint64(1)})


def halves_swapped():
    return Mutation("even / odd halves of a pair swapped", {"mask_index": lambda idx, ctx: idx ^ np.uint64(1)})


def c_left_out_of_h():
    return Mutation("c left out of h", {"c_h": lambda c, ctx: 1.0})


def c_left_out_of_g():
    return Mutation("c left out of g", {"c_g": lambda c, ctx: 1.0})


def no_mask_in_dA():
    return Mutation("no mask in dA", {"keep_dA": lambda k, ctx: torch.ones_like(k)})


def no_mask_in_dx():
    return Mutation("no mask in dx", {"keep_dx": lambda k, ctx: torch.ones_like(k)})


def dropped_dx_rounded():
    """The dropped element goes through the update with a zero product, bf16(fma(s, 0, old)), instead of keeping its bits: the same VALUE
    for every finite old, another sign for old = -0 -- the CPU test looks at the sign bit."""
    return Mutation("dropped dx elements rounded instead of kept", {"dropped_rounded": lambda f, ctx: True})


def rows_ignored():
    return Mutation("rows ignored", {"site_rows": lambda r, ctx: np.arange(ctx["M"], dtype=np.uint64) if ctx["given"] else r})


def per_target_site(seed, layer=0):
    """q / k / v each with a site of its own (8 * layer + 3 + its index through the free offsets) instead of the shared one."""
    def f(stream, ctx):
        t = ctx.get("target")
        if t is None or t == "query":
            return stream
        return RNG.rng_stream(seed, 8 * layer + 7 + 8 * LR.TARGETS.index(t))
    return Mutation("a per-target site for q / k / v", {"stream": f})


# ------------------------------------------------------------------------------------------------ q / k / v
def qkv_fwd(x, qkv, A, B, targets, scale, drop=None, *, emu=False, mutation=None):
    """mmbert_lora_qkv_fwd_drop on CPU tensors.  Returns {"qkv": Ref [M, 3H], "h": Ref [M, ntargets * r]} as lora_ref.fwd does."""
    names = LR._names(targets)
    M, H = x.shape
    s = _c32(scale)
    c = _c(drop, mutation, "c_h")
    r = A[names[0]].shape[0]
    x64 = x.to(torch.float64)
    out = qkv.to(torch.float64).clone()
    acc, mid = torch.zeros_like(out), torch.zeros_like(out)
    exact = torch.ones(out.shape, dtype=torch.bool)
    hv, ha = [], []
    for t in names:
        k = LR.TARGETS.index(t)
        xm = _masked(x64, keep_matrix(M, H, drop, mutation=mutation, target=t))
        At, Bt = A[t].to(torch.float64), B[t].to(torch.float64)
        h = _times_c(_prod(xm, At, emu), c, emu)
        hb = _bf(h) if emu else h
        d = _prod(hb, Bt, emu)
        old = out[:, k * H:(k + 1) * H]
        v = s * d + old
        hs = abs(c) * _abs(xm, A[t])
        acc[:, k * H:(k + 1) * H] = old.abs() + abs(s) * (math.sqrt(r) * _abs(hb, Bt) + math.sqrt(H) * (hs @ Bt.abs().t()))
        mid[:, k * H:(k + 1) * H] = abs(s) * _abs(hb, Bt)
        out[:, k * H:(k + 1) * H] = _bf(_f32(v)) if emu else v
        exact[:, k * H:(k + 1) * H] = False
        hv.append(hb)
        ha.append(math.sqrt(H) * hs)
    hcat, hacc = torch.cat(hv, 1), torch.cat(ha, 1)
    return {"qkv": Ref(out, acc, mid, U_BF16, 0.0, exact), "h": Ref(hcat, hacc, torch.zeros_like(hacc), U_BF16)}


def _keep_old(new, old, Kp, mutation, s, emu):
    """The masked update: ``new`` where the mask kept the element, the bits of ``old`` where it dropped it."""
    if _hook(mutation, "dropped_rounded", False):
        dropped = s * torch.zeros_like(old) + old                    # fma(s, +0, old): -0 becomes +0
        return torch.where(Kp > 0, new, _bf(_f32(dropped)) if emu else dropped)
    return torch.where(Kp > 0, new, old)


def qkv_bwd(dqkv, x, h, A, B, targets, scale, drop=None, *, dres=None, gA0=None, gB0=None, accumulate=True, emu=False, mutation=None):
    """mmbert_lora_qkv_bwd_drop on CPU tensors; h [M, ntargets * r] bf16 as forward wrote it (None: recomputed, emulated).  Returns what
    lora_ref.bwd returns."""
    names = LR._names(targets)
    M, H = x.shape
    s = _c32(scale)
    c = _c(drop, mutation, "c_g")
    r = A[names[0]].shape[0]
    if h is None:
        h = qkv_fwd(x, torch.zeros(M, 3 * H, dtype=torch.bfloat16), A, B, targets, 1.0, drop, emu=True, mutation=mutation)["h"].val
    res = {"dA": {}, "dB": {}}
    d = torch.zeros(M, H, dtype=torch.float64)
    d_acc, d_mid = torch.zeros_like(d), torch.zeros_like(d)
    x64 = x.to(torch.float64)
    Kp = keep_matrix(M, H, drop, mutation=mutation, target="query")          # (the shared mask: the input gradient is ONE chain over the targets)
    for ti, t in enumerate(names):
        k = LR.TARGETS.index(t)
        At, Bt = A[t].to(torch.float64), B[t].to(torch.float64)
        dq = dqkv[:, k * H:(k + 1) * H].to(torch.float64)
        g = _times_c(_prod(dq, Bt.t(), emu), c, emu)
        gb = _bf(g) if emu else g
        gs = abs(c) * _abs(dq, Bt.t())
        d = d + gb @ At
        if emu:
            d = _f32(d)
        d_acc += math.sqrt(r) * (gb.abs() @ At.abs()) + math.sqrt(H) * (gs @ At.abs())
        d_mid += gb.abs() @ At.abs()
        ht = h[:, ti * r:(ti + 1) * r].to(torch.float64)
        xm = _masked(x64, _hook(mutation, "keep_dA", keep_matrix(M, H, drop, mutation=mutation, target=t)))
        for key, C, S, old in (("dA", gb, xm, gA0), ("dB", dq, ht, gB0)):
            tot = _token_sum(C, S, emu, None)
            o = old[t].to(torch.float64) if (old is not None and accumulate) else torch.zeros_like(tot)
            v = s * tot
            v = _f32(_f32(v) + o) if emu else v + o
            a = o.abs() + abs(s) * math.sqrt(max(M, 1)) * (C.abs().t() @ S.abs())
            m = torch.zeros_like(a)
            if key == "dA":
                a = a + abs(s) * math.sqrt(H) * (gs.t() @ xm.abs())
                m = abs(s) * (gb.abs().t() @ xm.abs())
            res[key][t] = Ref(v, a, m, U_F32)
    if dres is not None:
        old = dres.to(torch.float64)
        Kd = _hook(mutation, "keep_dx", Kp)
        v = s * d + old
        new = _bf(_f32(v)) if emu else v
        res["dres"] = Ref(_keep_old(new, old, Kd, mutation, s, emu), old.abs() + abs(s) * d_acc * Kd, abs(s) * d_mid * Kd, U_BF16, 0.0, Kp == 0)
    return res


# ------------------------------------------------------------------------------------------------ the dense seams
def _dense_h(x64, A64, drop, rows, emu, mutation, K):
    Kp = keep_matrix(x64.shape[0], K, drop, rows, mutation=mutation)
    xm = _masked(x64, Kp)
    c = _c(drop, mutation, "c_h")
    h = _times_c(_prod(xm, A64, emu), c, emu)
    return (_bf(h) if emu else h), math.sqrt(K) * abs(c) * _abs(xm, A64)


def dense_fwd(x, y, A, B, scale, mode=ADD, *, drop=None, in_drop=None, emu=False, mutation=None):
    """mmbert_lora_dense_fwd_drop on CPU tensors; ``drop`` the GEMM's own output triple, ``in_drop`` the input's.  Returns what
    lora_dense_ref.fwd returns."""
    M, K = x.shape
    N, r = B.shape
    s = _c32(scale)
    A64, B64 = A.to(torch.float64), B.to(torch.float64)
    hb, hacc = _dense_h(x.to(torch.float64), A64, in_drop, None, emu, mutation, K)
    p = _prod(hb, B64, emu)
    pa = math.sqrt(r) * _abs(hb, B64) + hacc @ B64.abs().t()
    pm = _abs(hb, B64)
    old = y.to(torch.float64)
    res = {"h": Ref(hb, hacc, torch.zeros_like(hacc), U_BF16)}
    if mode == ADD:
        stream, thr16, dscale = drop if drop is not None else (0, 0, 1.0)
        cy = _c32(dscale)
        keep = DR.keep_mask(M, N, stream, thr16) if thr16 else torch.ones(M, N, dtype=torch.float64)
        sc = _c32(s * cy) if emu else s * cy
        v = sc * p * keep + old
        out = _bf(_f32(v)) if emu else v
        res["y"] = Ref(out, old.abs() + abs(sc) * keep * pa, abs(sc) * keep * pm, U_BF16, 0.0, keep == 0)
        return res
    w = s * p + old
    if emu:
        w = _f32(w)
    acc, mid = old.abs() + abs(s) * pa, abs(s) * pm
    g = gelu64(w)
    if emu:
        g = _f32(g)
    lip = DR._lip(w, acc, mid)
    res["aux"] = Ref(_bf(w) if emu else w, acc, mid, U_BF16)
    res["y"] = Ref(_bf(g) if emu else g, lip * acc, lip * mid, U_BF16, GELU_ABS)
    return res


def dense_bwd(dy, x, h, A, B, scale, *, in_drop=None, rows=None, dx=None, gelu_u=None, gA0=None, gB0=None, accumulate=True, emu=False,
              mutation=None):
    """mmbert_lora_dense_bwd_drop on CPU tensors; h [M, r] bf16 as forward wrote it (None: recomputed under the mask of ``rows``); ``rows``:
    the site row of every local row.  Returns what lora_dense_ref.bwd returns."""
    M, K = x.shape
    N, r = B.shape
    s = _c32(scale)
    c = _c(in_drop, mutation, "c_g")
    A64, B64, x64, dy64 = A.to(torch.float64), B.to(torch.float64), x.to(torch.float64), dy.to(torch.float64)
    if h is None:
        h = _dense_h(x64, A64, in_drop, rows, True, mutation, K)[0]
    h64 = h.to(torch.float64)
    g = _times_c(_prod(dy, B64.t(), emu), c, emu)
    gb = _bf(g) if emu else g
    gs = abs(c) * _abs(dy, B64.t())
    Kp = keep_matrix(M, K, in_drop, rows, mutation=mutation)
    xm = _masked(x64, _hook(mutation, "keep_dA", Kp))
    res = {}
    for key, C, S, old in (("dA", gb, xm, gA0), ("dB", dy64, h64, gB0)):
        tot = _token_sum(C, S, emu, None)
        o = old.to(torch.float64) if (old is not None and accumulate) else torch.zeros_like(tot)
        v = s * tot
        v = _f32(_f32(v) + o) if emu else v + o
        a = o.abs() + abs(s) * math.sqrt(max(M, 1)) * (C.abs().t() @ S.abs())
        m = torch.zeros_like(a)
        if key == "dA":
            a = a + abs(s) * math.sqrt(N) * (gs.t() @ xm.abs())
            m = abs(s) * (gb.abs().t() @ xm.abs())
        res[key] = Ref(v, a, m, U_F32)
    if dx is not None:
        old = dx.to(torch.float64)
        Kd = _hook(mutation, "keep_dx", Kp)
        q = gb @ A64
        if emu:
            q = _f32(q)
        qa = math.sqrt(r) * (gb.abs() @ A64.abs()) + math.sqrt(N) * (gs @ A64.abs())
        qm = gb.abs() @ A64.abs()
        extra = 0.0
        if gelu_u is not None:
            gp = gelu_grad64(gelu_u.to(torch.float64))
            extra = GELUP_ABS * abs(s) * q.abs() * Kd
            q = _f32(q * _f32(gp)) if emu else q * gp
            qa, qm = gp.abs() * qa, gp.abs() * qm
        v = s * q + old
        new = _bf(_f32(v)) if emu else v
        res["dx"] = Ref(_keep_old(new, old, Kd, mutation, s, emu), old.abs() + abs(s) * qa * Kd, abs(s) * qm * Kd, U_BF16, extra, Kp == 0)
    return res
