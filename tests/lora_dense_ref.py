"""A float64 reference for the dense-seam adapter kernels (csrc/lora.hip: mmbert_lora_dense_fwd / _bwd) and a scale-aware check.

Not a test module (pytest does not collect it): ``from tests import lora_dense_ref as DR``.  The pattern is tests/lora_ref.py's; the
dropout generator comes from tests/rng_ref.py and the float64 GELU with its absolute error terms from tests/gemm_ref.py.

``fwd`` / ``bwd`` with ``emu=False`` are the reference: plain float64 on the CPU, on the same bf16 inputs and fp32 scalars the kernels get,
with NO intermediate rounding (s = scale, x [M, K], y / dy [M, N], A [r, K], B [N, r]):

    fwd ADD    h = x . A^T      y = y + s * c * (h . B^T),  c(m, n) = drop_scale where keep(stream, m * N + n, thr16), else 0
    fwd GELU   w = y + s * (h . B^T)      aux = w      y = gelu(w)
    bwd        g = dy . B       dx = dx + s * (g . A) [* gelu'(u)]      dA = [dA +] s * g^T . x      dB = [dB +] s * dy^T . h

``emu=True`` is the emulation with the kernels' documented roundings: products of bf16 values exact in fp32, summed in 32-term blocks in
ascending k into one fp32 accumulator (the column chunks change nothing); h and g rounded to bf16; the rank-r product in fp32; s * c ONE
fp32 product; the update fma(.., product, old) rounded to fp32 and then to bf16; aux = bf16(w), y = bf16(fp32 gelu(w)); the gelu' factor an
fp32 value times the fp32 rank-r product; the token sums as in tests/lora_ref.py (128-token slabs, ascending fold).

``check(got, ref)`` asserts, for every element,

    |got - ref| <= C_OUT * u_out * |ref| + C_ACC * 2^-24 * acc + C_MID * 2^-9 * mid + extra

with lora_ref's meaning of ``acc`` (what the fp32 sums run over, what the epilogue adds) and ``mid`` (what the bf16 rounding of h / g can
move).  ``extra`` is the absolute error of the device GELU (gemm_ref.GELU_ABS on y of the GELU mode) or of gelu' (GELUP_ABS times
|s (g . A)| on dx).  Behind the GELU, acc and mid of w are carried with the Lipschitz factor min(1.13, |gelu'(w)| + 0.8 d), d the bound
on w itself (|gelu''| <= 0.8: first order alone is not a bound where gelu' ~ 0).  Elements the dropout dropped must keep their bits.

Calibration (tests/test_lora_dense_reference_cpu.py): emu=True against emu=False over M in {1, 63, 65, 129, 257}, (K, N) in {(64, 64),
(64, 256), (256, 64), (128, 512)}, r in {4, 8, 16}, on lora_ref.DISTS.  Rule: the emulation stays within HALF the bound.  With lora_ref's

    C_OUT = 2, C_ACC = 0.75, C_MID = 4

unchanged, the largest ratios are

    output        real    cancel   scaled   zeros         output        real    cancel   scaled   zeros
    h             0.495   0.491    0.495    0.495         dx            0.489   0.495    0.491    0.495
    y (ADD)       0.483   0.495    0.494    0.495         dx (gelu')    0.496   0.493    0.489    0.492
    y (ADD, p=.1) 0.486   0.496    0.492    0.494         dA            0.409   0.326    0.444    0.149
    aux           0.483   0.495    0.494    0.495         dB            0.210   0.210    0.214    0.131
    y (GELU)      0.487   0.497    0.494    0.489

(the CPU test prints the table it measures; the bf16 rows reach 0.5 by construction -- half an ulp just above a power of two is u = 2^-8
of the value -- and none needs a larger constant).  The smallest margin of a mutation is recorded in the CPU test's docstring.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from tests import gemm_ref as G
from tests import lora_ref as LR
from tests import rng_ref as RNG
from tests.gemm_ref import GELU_ABS, GELUP_ABS, gelu64, gelu_grad64
from tests.lora_ref import DISTS, Mutation, _abs, _hook, _prod, _token_sum

C_OUT, C_ACC, C_MID = 2.0, 0.75, 4.0
U_BF16, U_F32, EPS24, U_MID = G.U_BF16, G.U_F32, G.EPS24, 2.0 ** -9
NAN_BF16, NAN_F32 = G.NAN_BF16, G.NAN_F32
ADD, GELU = 0, 1
TARGETS = ("attention_output", "intermediate", "ffn_output")
ROWS = 16                                  # token rows of one wave's MFMA block

_f32, _bf, _c32 = G._f32, G._bf, G._c32


@dataclass
class Ref:
    val: torch.Tensor      # float64: the exact output (or, from emu=True, the emulated one)
    acc: torch.Tensor      # float64: magnitude under the fp32 sums (times 2^-24 in the bound)
    mid: torch.Tensor      # float64: magnitude under the bf16 rounding of h / g (times 2^-9)
    u_out: float
    extra: torch.Tensor | float = 0.0      # absolute term (the device GELU / gelu')
    exact: torch.Tensor | None = None      # bool: elements that must equal ``val`` bit for bit (dropped by the mask)


# ------------------------------------------------------------------------------------------------ mutations
def delta_not_masked():
    return Mutation("the delta is not masked", {"keep": lambda k, ctx: torch.ones_like(k)})


def mask_by_pitch(ldy):
    return Mutation(f"mask indexed by m * ldy + n, ldy = {ldy}", {"mask_pitch": lambda n, ctx: ldy})


def no_drop_scale():
    return Mutation("drop_scale left out", {"drop_scale": lambda c, ctx: 1.0})


def gelu_before_delta():
    return Mutation("GELU applied before the delta is added", {"gelu_first": lambda f, ctx: True})


def aux_after_gelu():
    return Mutation("aux stored after GELU", {"aux_after": lambda f, ctx: True})


def no_gelu_grad():
    return Mutation("gelu' missing from the input gradient", {"gelup": lambda gp, ctx: torch.ones_like(gp)})


def gelu_grad_neighbour_row():
    return Mutation("gelu' read from the neighbouring row", {"U": lambda u, ctx: torch.roll(u, 1, 0)})


def scale_off(factor=1.0 + 2.0 ** -6):
    return Mutation(f"s x {factor}", {"scale": lambda s, ctx: s * factor})


def skip_last_row_block():
    """The last 16-row block is left out: its rows of y / dx keep their values, the token sums do not see them."""
    f = lambda M, ctx: (M - 1) // ROWS * ROWS
    return Mutation("last 16-row block skipped", {"live_rows": f, "token_rows": f})


def skip_fold_slab(slab):
    return LR.skip_fold_slab(slab)


def ignore_accumulate():
    return LR.ignore_accumulate()


def contraction_stops_at_min():
    return Mutation("the contraction stops at min(K, N)", {"contract_len": lambda n, ctx: min(ctx["K"], ctx["N"])})


# ------------------------------------------------------------------------------------------------ the generator
def keep_mask(M, N, stream, thr16, pitch=None):
    """[M, N] float64 0 / 1: keep(stream, m * pitch + n, thr16) of tests/rng_ref.py; pitch = N is what the GEMM and the adapter kernel use."""
    pitch = N if pitch is None else pitch
    idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(pitch) + np.arange(N, dtype=np.uint64)[None, :]
    return torch.from_numpy(RNG.keep_at(stream, idx, thr16).astype(np.float64))


def keep_rate_ok(keep, thr16, sigmas=5.0):
    """The reference's own keep rate on a test shape against the binomial spread of tests/rng_ref.py's generator (p = thr16 / 65536 per
    element, two elements per hash word: independent halves): |rate - (1 - p)| <= sigmas * sqrt(p (1 - p) / n)."""
    n = keep.numel()
    p = thr16 / 65536.0
    return abs(float(keep.mean()) - (1.0 - p)) <= sigmas * math.sqrt(p * (1.0 - p) / n) and 0 < float(keep.sum()) < n


# ------------------------------------------------------------------------------------------------ forward
def _h(x, A, emu, mutation, K, N):
    kl = _hook(mutation, "contract_len", K, K=K, N=N)
    h = _prod(x[:, :kl], A[:, :kl], emu)
    return (_bf(h) if emu else h), math.sqrt(K) * _abs(x, A)


def _lip(w, acc, mid):
    d = C_ACC * EPS24 * acc + C_MID * U_MID * mid
    return torch.clamp(gelu_grad64(w).abs() + 0.8 * d, max=1.13)


def fwd(x, y, A, B, scale, mode=ADD, *, drop=None, emu=False, mutation=None):
    """mmbert_lora_dense_fwd on CPU tensors; ``drop`` = (stream, thr16, drop_scale) or None.  Returns {"y": Ref, "h": Ref[, "aux": Ref]}."""
    M, K = x.shape
    N, r = B.shape
    s = _hook(mutation, "scale", _c32(scale))
    live = _hook(mutation, "live_rows", M)
    A64, B64 = A.to(torch.float64), B.to(torch.float64)
    hb, hacc = _h(x, A64, emu, mutation, K, N)
    p = _prod(hb, B64, emu)
    pa = math.sqrt(r) * _abs(hb, B64) + hacc @ B64.abs().t()
    pm = _abs(hb, B64)
    old = y.to(torch.float64)
    res = {"h": Ref(hb, hacc, torch.zeros_like(hacc), U_BF16)}
    rows = (torch.arange(M) < live)[:, None]
    if mode == ADD:
        stream, thr16, dscale = drop if drop is not None else (0, 0, 1.0)
        c = _hook(mutation, "drop_scale", _c32(dscale))
        keep = keep_mask(M, N, stream, thr16, _hook(mutation, "mask_pitch", N)) if thr16 else torch.ones(M, N, dtype=torch.float64)
        exact = keep == 0
        keep = _hook(mutation, "keep", keep)
        sc = _c32(s * c) if emu else s * c
        v = sc * p * keep + old
        out = _bf(_f32(v)) if emu else v
        out = torch.where(rows, out, old)
        res["y"] = Ref(out, old.abs() + abs(sc) * keep * pa, abs(sc) * keep * pm, U_BF16, 0.0, exact)
        return res
    w = s * p + old
    if emu:
        w = _f32(w)
    acc, mid = old.abs() + abs(s) * pa, abs(s) * pm
    if _hook(mutation, "gelu_first", False):
        g = gelu64(old) + s * p
    else:
        g = gelu64(w)
    if emu:
        g = _f32(g)
    aux = g if _hook(mutation, "aux_after", False) else w
    lip = _lip(w, acc, mid)
    res["aux"] = Ref(torch.where(rows, _bf(aux) if emu else aux, old), acc, mid, U_BF16)
    res["y"] = Ref(torch.where(rows, _bf(g) if emu else g, old), lip * acc, lip * mid, U_BF16, GELU_ABS)
    return res


# ------------------------------------------------------------------------------------------------ backward
def bwd(dy, x, h, A, B, scale, *, dx=None, gelu_u=None, gA0=None, gB0=None, accumulate=True, emu=False, mutation=None):
    """mmbert_lora_dense_bwd on CPU tensors; h [M, r] bf16 as forward wrote it (None: recomputed); gA0 / gB0 the old fp32 gradients.
    Returns {"dA": Ref [r, K], "dB": Ref [N, r][, "dx": Ref [M, K]]}."""
    M, K = x.shape
    N, r = B.shape
    s = _hook(mutation, "scale", _c32(scale))
    accumulate = _hook(mutation, "accumulate", bool(accumulate))
    live = _hook(mutation, "live_rows", M)
    A64, B64, x64, dy64 = A.to(torch.float64), B.to(torch.float64), x.to(torch.float64), dy.to(torch.float64)
    if h is None:
        h = _h(x, A64, True, mutation, K, N)[0]
    h64 = h.to(torch.float64)
    nl = _hook(mutation, "contract_len", N, K=K, N=N)
    g = _prod(dy[:, :nl], B64[:nl].t(), emu)
    gb = _bf(g) if emu else g
    gs = _abs(dy, B64.t())
    res = {}
    for key, C, S, old in (("dA", gb, x64, gA0), ("dB", dy64, h64, gB0)):
        tot = _token_sum(C, S, emu, mutation)
        o = old.to(torch.float64) if (old is not None and accumulate) else torch.zeros_like(tot)
        v = s * tot
        v = _f32(_f32(v) + o) if emu else v + o
        a = o.abs() + abs(s) * math.sqrt(max(M, 1)) * (C.abs().t() @ S.abs())
        m = torch.zeros_like(a)
        if key == "dA":
            a = a + abs(s) * math.sqrt(N) * (gs.t() @ x64.abs())
            m = abs(s) * (gb.abs().t() @ x64.abs())
        res[key] = Ref(v, a, m, U_F32)
    if dx is not None:
        old = dx.to(torch.float64)
        q = gb @ A64
        if emu:
            q = _f32(q)
        qa = math.sqrt(r) * (gb.abs() @ A64.abs()) + math.sqrt(N) * (gs @ A64.abs())
        qm = gb.abs() @ A64.abs()
        extra = 0.0
        if gelu_u is not None:
            U = _hook(mutation, "U", gelu_u.to(torch.float64))
            gp = _hook(mutation, "gelup", gelu_grad64(U))
            extra = GELUP_ABS * abs(s) * q.abs()
            q = _f32(q * _f32(gp)) if emu else q * gp
            qa, qm = gp.abs() * qa, gp.abs() * qm
        v = s * q + old
        out = _bf(_f32(v)) if emu else v
        out = torch.where((torch.arange(M) < live)[:, None], out, old)
        res["dx"] = Ref(out, old.abs() + abs(s) * qa, abs(s) * qm, U_BF16, extra)
    return res


def identity(dW, A, B, dy, x, h, scale):
    """lora_ref.identity for a projection K -> N: with dW [N, K] = dy^T . x as the weight-gradient kernel wrote it (fp32), dB = s dW A^T and
    dA = s B^T dW in float64; bounds as there (the bf16 rounding of h and g under ``mid``, the fp32 token sums on both sides under ``acc``)."""
    r = LR.identity(dW, A, B, dy, x, h, scale)
    return {k: Ref(v.val, v.acc, v.mid, v.u_out) for k, v in r.items()}


# ------------------------------------------------------------------------------------------------ the check
def ratio(got, ref: Ref) -> float:
    """The largest error / bound over the elements (<= 1 passes; an element that differs where the bound is 0, or a NaN, is inf)."""
    g = got.detach().to(torch.float64).cpu().reshape(ref.val.shape) if torch.is_tensor(got) else got.val
    err = (g - ref.val).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    bound = C_OUT * ref.u_out * ref.val.abs() + C_ACC * EPS24 * ref.acc + C_MID * U_MID * ref.mid + ref.extra
    if ref.exact is not None:
        bound = torch.where(ref.exact, torch.zeros_like(bound), bound)
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.nan_to_num(q, nan=math.inf, posinf=math.inf)
    return float(q.max()) if q.numel() else 0.0


def check(got, ref: Ref, what=""):
    q = ratio(got, ref)
    assert q <= 1.0, f"{what}: error / bound = {q:.3g}"
    return q


def inputs(M, K, N, r, dist, seed, bscale=0.02):
    """x / dx / u [M, K], y / dy [M, N] bf16; A [r, K], B [N, r] bf16; gA0 [r, K], gB0 [N, r] fp32 (CPU).  The families are lora_ref.inputs':
    real: N(0, 1) activations, kaiming-uniform-sized A, N(0, bscale) B; cancel: rows of x / dy with a large common offset against mean-free
    rows of A / columns of B; scaled: per-token powers of two over 2^+-20 on x, dy, y and dx; zeros: real with all-zero token rows and one
    all-zero rank row of A / column of B.  u (the saved pre-activation) stays N(0, 1.5): it only enters through gelu'."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, y, dy, dx, u = rn(M, K), rn(M, N), rn(M, N) * 0.05, rn(M, K) * 0.05, rn(M, K) * 1.5
    A = (torch.rand(r, K, generator=g) * 2 - 1) / math.sqrt(K)
    B = rn(N, r) * bscale
    if dist == "cancel":
        off = lambda n: (2.0 + 6.0 * torch.rand(M, 1, generator=g)) * torch.sign(rn(M, 1)) * torch.ones(1, n)
        x = off(K) + 0.05 * x
        dy = 0.05 * off(N) + 0.05 * dy
        A = A - A.mean(1, keepdim=True)
        B = B - B.mean(0, keepdim=True)
    elif dist == "scaled":
        e = lambda: torch.exp2(torch.randint(-20, 21, (M, 1), generator=g).float())
        x, dy = x * e(), dy * e()
        y, dx = y * e(), dx * e()
    elif dist == "zeros":
        z = torch.unique(torch.tensor([0, M // 2, M - 1]))
        x[z] = 0
        dy[z] = 0
        x[::37] = 0
        A[r - 1] = 0
        B[:, 0] = 0
    elif dist != "real":
        raise ValueError(dist)
    bf = torch.bfloat16
    return dict(x=x.to(bf), y=y.to(bf), dy=dy.to(bf), dx=dx.to(bf), u=u.to(bf), A=A.to(bf), B=B.to(bf), gA0=rn(r, K) * 0.01, gB0=rn(N, r) * 0.01)


def forward_h(inp, emu=True):
    """The bf16 h forward writes (emulated), as backward's input."""
    return fwd(inp["x"], inp["y"], inp["A"], inp["B"], 1.0, emu=emu)["h"].val.to(torch.bfloat16)
