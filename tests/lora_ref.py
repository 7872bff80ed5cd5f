"""A float64 reference for the adapter kernels (csrc/lora.hip) and a scale-aware check of their outputs.

Not a test module (pytest does not collect it): ``from tests import lora_ref as LR``.  The pattern is tests/gemm_ref.py's.

``fwd`` / ``bwd`` with ``emu=False`` are the reference: plain float64 torch on the CPU, on the same bf16 inputs (x, qkv, dqkv, dres, h,
A, B) and the same fp32 scale and fp32 gradient buffers the kernels get, with NO intermediate rounding:

    fwd   h_t = x . A_t^T                         qkv_t = qkv_t + s * h_t . B_t^T
    bwd   g_t = dqkv_t . B_t                      dres_out = dres_in + s * sum_t g_t . A_t
          dA_t = [dA_t +] s * g_t^T . x           dB_t = [dB_t +] s * dqkv_t^T . h_t        (h: the bf16 tensor forward wrote)

``emu=True`` is the emulation with the kernels' documented roundings: products of bf16 values exact in fp32, summed in 32-term blocks
(the K step of v_mfma_f32_16x16x32_bf16) into an fp32 accumulator; h and g rounded to bf16; the rank-r product in fp32 (one block); the
update fma(s, product, old) rounded to fp32 and then to bf16; the token sums over 128-token slabs (four 32-token blocks each, the last
one partial) as fp32 partial sums, folded in ascending slab order into one fp32 sum, times s, plus the old gradient.  It exists only to
calibrate the bounds below on the CPU.

``check(got, ref)`` asserts, for every element,

    |got - ref| <= C_OUT * u_out * |ref| + C_ACC * 2^-24 * acc + C_MID * 2^-9 * mid

u_out = 2^-8 (bf16 outputs: h, qkv, dres) or 2^-23 (fp32: dA, dB); ``acc`` = the magnitude the fp32 sums run over: sqrt(K) |.| . |.|^T of
every contraction (K = H, r or the token count) that feeds the element, and what the epilogue adds (|qkv|, |dres|, the old gradient);
``mid`` = what the bf16 rounding of the rank-r intermediate can move: s (|h| . |B_t|^T) for qkv, s sum_t |g_t| . |A_t| for dres,
s |g_t|^T . |x| for dA, nothing for h and dB (their inputs are given).

Calibration (tests/test_lora_reference_cpu.py): ``emu=True`` against ``emu=False`` over M in {1, 63, 65, 257, 1153}, H in {64, 128, 768},
r in {4, 8, 16}, the three target sets, on the realistic, cancellation-heavy, 2^+-20-scaled and zero-row inputs.  Rule: the constants are
twice what the emulation needs, i.e. its largest ratio error / bound is 0.5 (the margin tests/gemm_ref.py keeps).  With

    C_OUT = 2, C_ACC = 0.75, C_MID = 4

the largest ratios are

    output     real    cancel   scaled   zeros          output     real    cancel   scaled   zeros
    h          0.498   0.492    0.498    0.498          dres       0.490   0.496    0.493    0.494
    qkv        0.487   0.495    0.496    0.494          dA         0.465   0.396    0.465    0.184
                                                        dB         0.211   0.211    0.211    0.142

A bf16 value rounds by up to u = 2^-8 of itself (half an ulp just above a power of two): C_OUT = 2 is that at ratio 0.5, and the bf16
rows reach it on every input family.  The rounding of h / g is the same u = 2^-8 = 2 * 2^-9 of every entry, all entries aligned in the
worst case, so C_MID = 4 (with C_MID = 2 the emulation reached 0.83 on qkv).  C_ACC is gemm_ref's; the fp32 outputs stay inside with it.

The smallest margin of a mutation is recorded in the CPU test's docstring.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

from tests import gemm_ref as G

C_OUT, C_ACC, C_MID = 2.0, 0.75, 4.0
U_BF16, U_F32, EPS24, U_MID = G.U_BF16, G.U_F32, G.EPS24, 2.0 ** -9
TARGETS = ("query", "key", "value")
SLAB, BLOCK = 128, 32
NAN_BF16, NAN_F32 = G.NAN_BF16, G.NAN_F32

_f32, _bf, _c32 = G._f32, G._bf, G._c32


@dataclass
class Mutation:
    """A value-only perturbation applied inside ``fwd`` / ``bwd``: ``hooks[stage](value, ctx)`` replaces the value of a stage
    (stages: A (one target's matrix), scale, adapters (the {name: (A, B)} map), token_rows, fold_slabs, accumulate)."""
    name: str
    hooks: dict = field(default_factory=dict)


def _hook(mut, stage, x, **ctx):
    if mut is None or stage not in mut.hooks:
        return x
    return mut.hooks[stage](x, ctx)


def drop_rank_column(target, k):
    def f(A, ctx):
        if ctx["target"] != target:
            return A
        A = A.clone()
        A[k] = 0
        return A
    return Mutation(f"rank column {k} of {target} dropped", {"A": f})


def scale_off(factor=1.0 + 2.0 ** -6):
    return Mutation(f"s x {factor}", {"scale": lambda s, ctx: s * factor})


def swap_q_v():
    def f(ad, ctx):
        ad = dict(ad)
        ad["query"], ad["value"] = ad["value"], ad["query"]
        return ad
    return Mutation("query and value adapters swapped", {"adapters": f})


def skip_last_row_block():
    """The last (partial) 32-token block left out of the token sums."""
    return Mutation("last partial row block skipped", {"token_rows": lambda M, ctx: (M - 1) // BLOCK * BLOCK})


def skip_fold_slab(slab):
    return Mutation(f"partial sum {slab} left out of the fold", {"fold_slabs": lambda ids, ctx: [i for i in ids if i != slab]})


def ignore_accumulate():
    return Mutation("accumulate ignored", {"accumulate": lambda a, ctx: not a})


@dataclass
class Ref:
    val: torch.Tensor      # float64: the exact output (or, from emu=True, the emulated one)
    acc: torch.Tensor      # float64: magnitude under the fp32 sums (times 2^-24 in the bound)
    mid: torch.Tensor      # float64: magnitude under the bf16 rounding of h / g (times 2^-9)
    u_out: float
    exact: torch.Tensor | None = None      # bool: elements that must equal ``val`` bit for bit (untargeted thirds)


def _names(targets):
    names = [targets] if isinstance(targets, str) else list(targets)
    assert names and all(t in TARGETS for t in names)
    return [t for t in TARGETS if t in names]


def _prod(X, W, emu):
    """X [M, K] . W [N, K]^T"""
    return G._product(X.to(torch.float64), W.to(torch.float64), emu, BLOCK)


def _abs(X, W):
    return X.to(torch.float64).abs() @ W.to(torch.float64).abs().t()


def fwd(x, qkv, A, B, targets, scale, *, emu=False, mutation=None):
    """mmbert_lora_qkv_fwd on CPU tensors.  Returns {"qkv": Ref [M, 3H], "h": Ref [M, ntargets * r]}; untargeted thirds come back as they are
    (acc = mid = 0: they must keep their bits)."""
    names = _names(targets)
    M, H = x.shape
    ad = _hook(mutation, "adapters", {t: (A[t], B[t]) for t in names})
    s = _hook(mutation, "scale", _c32(scale))
    r = ad[names[0]][0].shape[0]
    out = qkv.to(torch.float64).clone()
    acc, mid = torch.zeros_like(out), torch.zeros_like(out)
    exact = torch.ones(out.shape, dtype=torch.bool)
    hv, ha = [], []
    for t in names:
        k = TARGETS.index(t)
        At = _hook(mutation, "A", ad[t][0].to(torch.float64), target=t)
        Bt = ad[t][1].to(torch.float64)
        h = _prod(x, At, emu)
        hb = _bf(h) if emu else h
        d = _prod(hb, Bt, emu)
        old = out[:, k * H:(k + 1) * H]
        v = s * d + old
        hs = _abs(x, ad[t][0])
        acc[:, k * H:(k + 1) * H] = old.abs() + abs(s) * (math.sqrt(r) * _abs(hb, Bt) + math.sqrt(H) * (hs @ Bt.abs().t()))
        mid[:, k * H:(k + 1) * H] = abs(s) * _abs(hb, Bt)
        out[:, k * H:(k + 1) * H] = _bf(_f32(v)) if emu else v
        exact[:, k * H:(k + 1) * H] = False
        hv.append(hb)
        ha.append(math.sqrt(H) * hs)
    hcat, hacc = torch.cat(hv, 1), torch.cat(ha, 1)
    return {"qkv": Ref(out, acc, mid, U_BF16, exact), "h": Ref(hcat, hacc, torch.zeros_like(hacc), U_BF16)}


def _token_sum(C, S, emu, mutation):
    """sum over tokens m of C[m, :]^T S[m, :] -> [C cols, S cols], in the kernels' order when ``emu``; returns (sum, slab count)."""
    M = C.shape[0]
    rows = _hook(mutation, "token_rows", M)
    nslab = (M + SLAB - 1) // SLAB
    C64, S64 = C.to(torch.float64), S.to(torch.float64)
    parts = []
    for q in range(nslab):
        lo, hi = q * SLAB, min(rows, (q + 1) * SLAB)
        p = torch.zeros(C.shape[1], S.shape[1], dtype=torch.float64)
        for b0 in range(lo, max(lo, hi), BLOCK):
            b1 = min(b0 + BLOCK, hi)
            p = p + C64[b0:b1].t() @ S64[b0:b1]
            if emu:
                p = _f32(p)
        parts.append(p)
    tot = torch.zeros(C.shape[1], S.shape[1], dtype=torch.float64)
    for q in _hook(mutation, "fold_slabs", list(range(nslab))):
        tot = tot + parts[q]
        if emu:
            tot = _f32(tot)
    return tot


def bwd(dqkv, x, h, A, B, targets, scale, *, dres=None, gA0=None, gB0=None, accumulate=True, emu=False, mutation=None):
    """mmbert_lora_qkv_bwd on CPU tensors; h [M, ntargets * r] bf16 as forward wrote it; gA0 / gB0 = {name: fp32 old gradient}.
    Returns {"dres": Ref [M, H] (if dres is given), "dA": {name: Ref [r, H]}, "dB": {name: Ref [H, r]}}."""
    names = _names(targets)
    M, H = x.shape
    ad = _hook(mutation, "adapters", {t: (A[t], B[t]) for t in names})
    s = _hook(mutation, "scale", _c32(scale))
    accumulate = _hook(mutation, "accumulate", bool(accumulate))
    r = ad[names[0]][0].shape[0]
    res = {"dA": {}, "dB": {}}
    d = torch.zeros(M, H, dtype=torch.float64)
    d_acc, d_mid = torch.zeros_like(d), torch.zeros_like(d)
    x64 = x.to(torch.float64)
    for ti, t in enumerate(names):
        k = TARGETS.index(t)
        At = _hook(mutation, "A", ad[t][0].to(torch.float64), target=t)
        Bt = ad[t][1].to(torch.float64)
        dq = dqkv[:, k * H:(k + 1) * H].to(torch.float64)
        g = _prod(dq, Bt.t(), emu)                                   # [M, r]
        gb = _bf(g) if emu else g
        gs = _abs(dq, Bt.t())
        d = d + gb @ At                                              # (one MFMA chain over the targets: one fp32 accumulator)
        if emu:
            d = _f32(d)
        d_acc += math.sqrt(r) * (gb.abs() @ At.abs()) + math.sqrt(H) * (gs @ At.abs())
        d_mid += gb.abs() @ At.abs()
        ht = h[:, ti * r:(ti + 1) * r].to(torch.float64)
        for key, C, S, old in (("dA", gb, x64, gA0), ("dB", dq, ht, gB0)):
            tot = _token_sum(C, S, emu, mutation)
            o = old[t].to(torch.float64) if (old is not None and accumulate) else torch.zeros_like(tot)
            v = s * tot
            if emu:
                v = _f32(_f32(v) + o)
            else:
                v = v + o
            a = o.abs() + abs(s) * math.sqrt(max(M, 1)) * (C.abs().t() @ S.abs())
            m = torch.zeros_like(a)
            if key == "dA":
                a = a + abs(s) * math.sqrt(H) * (gs.t() @ x64.abs())
                m = abs(s) * (gb.abs().t() @ x64.abs())
            res[key][t] = Ref(v, a, m, U_F32)
    if dres is not None:
        old = dres.to(torch.float64)
        v = s * d + old
        res["dres"] = Ref(_bf(_f32(v)) if emu else v, old.abs() + abs(s) * d_acc, abs(s) * d_mid, U_BF16)
    return res


def identity(dW, A, B, dq, x, h, scale):
    """The model-level gradient identity for one target: with dW [H, H] = dq^T . x as the weight-gradient kernel wrote it (fp32),
    dB = s dW A^T and dA = s B^T dW in float64.  Against them the adapter kernels' gradients differ by the bf16 rounding of h (dB) and of
    g (dA) -- ``mid`` -- and by the fp32 sums over the tokens on both sides -- ``acc``.  dq [M, H], x [M, H], h [M, r] bf16; A [r, H], B [H, r]."""
    s = _c32(scale)
    M = dq.shape[0]
    dW64, A64, B64 = dW.to(torch.float64), A.to(torch.float64), B.to(torch.float64)
    dq64, x64, h64 = dq.to(torch.float64).abs(), x.to(torch.float64).abs(), h.to(torch.float64).abs()
    g = (dq.to(torch.float64) @ B64).abs()
    tn = dq64.t() @ x64                                              # |dq|^T |x|: what the weight gradient's own fp32 sum runs over
    rt = math.sqrt(max(M, 1))
    vb = s * dW64 @ A64.t()
    vb_mid = abs(s) * (dq64.t() @ h64)
    vb_acc = abs(s) * rt * (dq64.t() @ h64 + tn @ A64.abs().t())
    va = s * B64.t() @ dW64
    va_mid = abs(s) * (g.t() @ x64)
    va_acc = abs(s) * rt * (g.t() @ x64 + B64.abs().t() @ tn)
    return {"dA": Ref(va, va_acc, va_mid, U_F32), "dB": Ref(vb, vb_acc, vb_mid, U_F32)}


def ratio(got, ref: Ref) -> float:
    """The largest error / bound over the elements (<= 1 passes; an element that differs where the bound is 0, or a NaN, is inf)."""
    g = got.detach().to(torch.float64).cpu().reshape(ref.val.shape) if torch.is_tensor(got) else got.val
    err = (g - ref.val).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    bound = C_OUT * ref.u_out * ref.val.abs() + C_ACC * EPS24 * ref.acc + C_MID * U_MID * ref.mid
    if ref.exact is not None:
        bound = torch.where(ref.exact, torch.zeros_like(bound), bound)
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.nan_to_num(q, nan=math.inf, posinf=math.inf)
    return float(q.max()) if q.numel() else 0.0


def check(got, ref: Ref, what=""):
    q = ratio(got, ref)
    assert q <= 1.0, f"{what}: error / bound = {q:.3g}"
    return q


def walk(res):
    """(label, Ref) over a result of fwd / bwd."""
    for k, v in res.items():
        if isinstance(v, dict):
            for t, r in v.items():
                yield f"{k}[{t}]", r
        else:
            yield k, v


DISTS = ("real", "cancel", "scaled", "zeros")


def inputs(M, H, r, targets, dist, seed, bscale=0.02):
    """x [M, H], qkv / dqkv [M, 3H], dres [M, H] bf16; A {name: [r, H]}, B {name: [H, r]} bf16; gA0 / gB0 fp32 (CPU).
    real: N(0, 1) activations, kaiming-uniform-sized A, N(0, bscale) B; cancel: rows of x / dqkv with a large common offset against
    mean-free rows of A / columns of B (|h| << |x| . |A|); scaled: per-token powers of two over 2^+-20 on x, dqkv, qkv and dres;
    zeros: real with all-zero token rows and one all-zero rank row of A / column of B."""
    names = _names(targets)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, qkv, dqkv, dres = rn(M, H), rn(M, 3 * H), rn(M, 3 * H) * 0.05, rn(M, H) * 0.05
    A = {t: (torch.rand(r, H, generator=g) * 2 - 1) / math.sqrt(H) for t in names}
    B = {t: rn(H, r) * bscale for t in names}
    if dist == "cancel":
        off = lambda n: (2.0 + 6.0 * torch.rand(M, 1, generator=g)) * torch.sign(rn(M, 1)) * torch.ones(1, n)
        x = off(H) + 0.05 * x
        dqkv = 0.05 * off(3 * H) + 0.05 * dqkv
        A = {t: a - a.mean(1, keepdim=True) for t, a in A.items()}
        B = {t: b - b.mean(0, keepdim=True) for t, b in B.items()}
    elif dist == "scaled":
        e = lambda: torch.exp2(torch.randint(-20, 21, (M, 1), generator=g).float())
        x, dqkv = x * e(), dqkv * e()
        qkv, dres = qkv * e(), dres * e()
    elif dist == "zeros":
        z = torch.unique(torch.tensor([0, M // 2, M - 1]))
        x[z] = 0
        dqkv[z] = 0
        x[::37] = 0
        for t in names:
            A[t][r - 1] = 0
            B[t][:, 0] = 0
    elif dist != "real":
        raise ValueError(dist)
    bf = torch.bfloat16
    gA0 = {t: rn(r, H) * 0.01 for t in names}
    gB0 = {t: rn(H, r) * 0.01 for t in names}
    return dict(x=x.to(bf), qkv=qkv.to(bf), dqkv=dqkv.to(bf), dres=dres.to(bf), A={t: a.to(bf) for t, a in A.items()},
                B={t: b.to(bf) for t, b in B.items()}, gA0=gA0, gB0=gB0)


def forward_h(inp, targets, emu=True):
    """The bf16 h forward writes (emulated), as backward's input."""
    return fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], targets, 1.0, emu=emu)["h"].val.to(torch.bfloat16)
