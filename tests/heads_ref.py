"""A float64 reference for the pretraining heads (csrc/heads_coop.hip, csrc/heads.hip) and a scale-aware check of their outputs.

Not a test module (pytest does not collect it): ``from tests import heads_ref as HR``.

``reference(case)`` is the truth: the oracle's own golden-pinned objective (``oracle.heads_from_cls`` -> ``fusion_objective``, ``cpc``;
``cls.seq_relationship`` on the text pooled rows for ``t_rel``) evaluated in float64 with autograd, on the fp32 rows and parameters
the kernels get, plus ``alpha * mean(mlm)`` when there are MLM losses.  The upstream gradient ``d`` scales every gradient, and every
parameter gradient is added onto the case's prior gradient.  Outputs: loss, aux (ap, label, nce), out5 (ap, label, nce, heads,
joint), logits, t_rel, rel, dfirst, dmlm and the 22 head parameters' gradients (``PARAMS``).

``restate(case, emu=False)`` restates the same forward and the backward formulas written in the header of csrc/heads_coop.hip
with values of class ``Num``: a value and, per element, the magnitude its fp32 arithmetic works at (``acc``, in units of 2^-24):

    product / sum     acc = F_SUM sum|a b| + sqrt(sum (|a| acc_b)^2 + (acc_a |b|)^2) + |out|
    + - * /  sqrt      first-order running error of the operands, added in quadrature, plus |out| (one rounding)
    tanh exp log       |f'(x)| acc_x + F_FN |f(x)|  (+ F_FN for log: hardware logf has an absolute error near 1)
    relu               acc_x where x > 0 (the inputs keep every |Apre| KINK bounds away from 0: ``kink_ratio``)

so the batch softmax, the cosine rows x / |x|, the CEs and every gradient carry the error their operands bring.  With ``emu=False``
the values are plain float64 and equal the autograd reference to ~1e-12 (the CPU test asserts it): the bounds describe the pinned
objective.  ``emu=True`` is the emulation, for calibration only: the same operations with fp32 roundings in the kernels' documented
order -- workgroup tiles with K split over 16 waves in 16-deep granules, each MFMA a fp32 add of 4 products, the wave partials added
in wave order; wave tiles (short inner dimension) one MFMA chain; row pieces per lane (float4 loads) and ``wave_sum``'s xor
butterfly (lane i with lane i + 32 first, then 16, ... 1); column sums in row order; fp32 exp / log / tanh correctly rounded (hardware's are widened through F_FN).  It takes value-only
mutations (``Mutation``) that the CPU test uses to show the bounds are tight.

``check(got, ref)`` is rowwise_ref's: for every element  |got - ref| <= C_OUT 2^-23 |ref| + C_ACC 2^-24 acc,  and normwise per row
(per sample for dfirst, per output feature for a weight gradient), there with TAU_ACC = 0.5 in place of 0.25: every element of a
row of gWp or of rel carries the same operand's error, so a row's errors add coherently (MI355X: normwise 1.27 / 2 at 0.25).

Calibration (tests/test_heads_reference_cpu.py: every case there).  Largest ratios (elementwise, normwise) the emulation reached,
and the MI355X over tests/test_heads_gpu.py, with

    C_OUT = 2, C_ACC = 1, F_SUM = 2, F_FN = 4

    output       emulation      MI355X
    losses       0.14  0.20     0.36  0.58
    logits/rel   0.22  0.25     0.62  0.68
    dfirst       0.25  0.19     0.53  0.46
    parameters   0.33  0.30     0.64  0.85

MI355X per output (elementwise, normwise): loss 0.30 0.58, aux 0.36 0.37, out5 0.36 0.34, dmlm 0.30 0.34, logits 0.21 0.36,
t_rel 0.51 0.39, rel 0.62 0.68, dfirst 0.53 0.46; pooler W 0.64 0.85, b 0.50 0.29; align W 0.46 0.46, b 0.27 0.20; attn W
0.56 0.33, b 0.49 0.38; vt / vv / vs W 0.30 0.26, b 0.14 0.24; classifier1_1 W 0.52 0.29, b 0.26 0.17; classifier1_2 W 0.27
0.18, b 0.10 0.19; cpc_z* W 0.34 0.34, b 0.34 0.29.  The largest, 0.85, is the pooler weight gradient's normwise ratio in the
19-launch form at B = 32, H = 64 (atomics); the largest of the level-launch form is the same gradient's elementwise 0.64 at
B = 128, H = 16.

Independent rounding errors of a product's operands add in quadrature: propagated as absolute sums, the bounds grow by about
sqrt(K) per dense layer and sit 10^3 - 10^4 above what the emulation reaches, too loose to see a dropped CPC term.  The hardware
reaches more than the emulation (the emulation's exp / log / tanh are correctly rounded, the hardware's v_exp_f32 / v_log_f32 are
not; the 19-launch form adds 64-deep chunks with atomics): its largest normwise ratio, 0.85, leaves less than the factor 2 the emulation has.

The smallest margin of a mutation is recorded in the CPU test's docstring.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

from oracle import mmbert_oracle as O
from tests.gemm_ref import Mutation, _hook, _f32, _c32  # noqa: F401  (Mutation re-exported for the tests)
from tests import rowwise_ref as _RW
from tests.rowwise_ref import Ref, Ratios, U_F32, C_OUT, TAU_OUT, EPS24  # noqa: F401

F_SUM = 2.0                   # accumulation: units of 2^-24 per unit of sum|a b|
F_FN = 4.0                    # fp32 tanh / exp / log: units of 2^-24 of their result (hardware: a few ulp)
TAU_ACC = 0.5                 # normwise: a row of a weight gradient shares its operand's error (coherent), unlike rowwise_ref's rows
KINK = 64.0                   # |Apre| >= KINK * 2^-24 acc(Apre) on every generated input
NW = 16                       # waves per workgroup (csrc/heads_coop.hip HC_WAVES)

MOD = ("t", "v", "s")
GATES = ("vt", "vv", "vs")
CPCS = ("cpc_zt.net", "cpc_zv.net", "cpc_za.net")
PARAMS = (["bert.pooler.dense.weight", "bert.pooler.dense.bias", "cls.align.weight", "cls.align.bias", "attn.weight", "attn.bias"]
          + [f"{g}.{w}" for g in GATES for w in ("weight", "bias")]
          + ["classifier1_1.weight", "classifier1_1.bias", "classifier1_2.weight", "classifier1_2.bias"]
          + [f"{c}.{w}" for c in CPCS for w in ("weight", "bias")])
FWD_ONLY = ("cls.seq_relationship.weight", "cls.seq_relationship.bias")
OUTPUTS = ("loss", "aux", "out5", "logits", "t_rel", "rel", "dfirst", "dmlm") + tuple(PARAMS)


# ------------------------------------------------------------------------------------------------ the case
@dataclass
class Case:
    B: int
    H: int
    first: torch.Tensor              # fp32 [3B, H] (bf16-representable: the model's form reads the same rows from a bf16 matrix)
    params: dict                     # name -> fp32 CPU tensor (PARAMS + FWD_ONLY)
    ap_v: torch.Tensor               # int64 [B]
    ap_s: torch.Tensor               # int64 [B]
    sent: torch.Tensor               # fp32 [B]
    num_labels: int = 7
    alpha: float = 1.0
    beta: float = 1.0
    mlm: torch.Tensor | None = None  # fp32 [nmlm]
    d: float = 1.0
    prior: dict = field(default_factory=dict)   # name -> fp32 prior gradient (zeros where missing)

    @property
    def nmlm(self):
        return 0 if self.mlm is None else self.mlm.numel()


# ------------------------------------------------------------------------------------------------ the autograd reference
class _Sent64:
    """The sentiment targets as fusion_objective reads them (``sentiment.view(-1).float()``), kept in float64: the fp32 values exactly,
    without an fp32 target in a float64 graph."""

    def __init__(self, t):
        self.t = t.to(torch.float64)

    def view(self, *shape):
        return _Sent64(self.t.view(*shape))

    def float(self):
        return self.t


def reference(c: Case) -> dict:
    """float64 autograd through the oracle: every output as a float64 CPU tensor (dmlm None without MLM losses)."""
    p = {k: v.detach().to(torch.float64).clone().requires_grad_(k in PARAMS) for k, v in c.params.items()}
    first = c.first.detach().to(torch.float64).clone().requires_grad_(True)
    cfg = dict(beta=_c32(c.beta), num_labels=c.num_labels)
    heads, ap, label, nce, logits = O.heads_from_cls(p, cfg, first, c.ap_v, c.ap_s, _Sent64(c.sent))
    B = c.B
    mlm = None
    joint = heads
    if c.nmlm:
        mlm = c.mlm.detach().to(torch.float64).clone().requires_grad_(True)
        joint = _c32(c.alpha) * mlm.mean() + heads
    joint.backward(torch.tensor(_c32(c.d), dtype=torch.float64))
    with torch.no_grad():
        pooled = torch.tanh(O._linear(first, p, "bert.pooler.dense"))
        t_rel = O._linear(pooled[:B], p, "cls.seq_relationship")
        rel = O._linear(first[B:], p, "cls.align")
    out = dict(loss=joint.detach().reshape(1), aux=torch.stack([ap, label, nce]).detach(),
               out5=torch.stack([ap, label, nce, heads, joint]).detach(), logits=logits.detach().reshape(B, 1), t_rel=t_rel, rel=rel,
               dfirst=first.grad, dmlm=None if mlm is None else mlm.grad)
    for n in PARAMS:
        out[n] = c.prior.get(n, torch.zeros_like(c.params[n])).to(torch.float64) + p[n].grad
    return out


# ------------------------------------------------------------------------------------------------ mutations (value-only, on the restatement)
def cpc_csum_dropped(m):
    """The -XPn o csum term of dXP dropped in modality m."""
    return Mutation(f"dXP without -XPn o csum ({MOD[m]})", {"dXP_corr": lambda x, ctx: x * 0 if ctx["m"] == m else x})


def cpc_rsum_dropped(m):
    """The -Xn o rsum term of dPc dropped in modality m."""
    return Mutation(f"dPc without -Xn o rsum ({MOD[m]})", {"dPc_corr": lambda x, ctx: x * 0 if ctx["m"] == m else x})


def softmax_over_columns(m):
    return Mutation(f"softmax over columns ({MOD[m]})", {"softmax": lambda x, ctx: torch.softmax(ctx["S"], 0) if ctx["m"] == m else x})


def positive_from_neighbour():
    return Mutation("positive term from the neighbouring sample", {"eye": lambda e, ctx: torch.roll(e, 1, 1)})


def beta_in_dS(f=1.0 + 2.0 ** -6):
    return Mutation("beta x (1 + 2^-6) in dS", {"beta_dS": lambda b, ctx: b * f})


def speech_labels_from_visual():
    return Mutation("ap2 ignored", {"ap_s": lambda s, ctx: ctx["ap_v"]})


def drel_rows_shifted():
    return Mutation("drel of the rows >= B shifted by one sample", {"drel_rows": lambda x, ctx: torch.roll(x, 1, 0)})


def gate_dP_w1_only():
    return Mutation("gate dP through W1 only", {"W_dP": lambda W, ctx: ctx["W1"]})


def e_without_relu():
    return Mutation("E = dg Apre", {"E": lambda E, ctx: ctx["dg"][:, None] * ctx["Apre"]})


def pooler_tanh_grad(f=1.0 + 2.0 ** -6):
    return Mutation("pooler tanh' x (1 + 2^-6)", {"tanh_pool": lambda x, ctx: x * f})


def label_tanh_grad_missing():
    return Mutation("label loss without tanh' (1 label)", {"dlo_tanh": lambda x, ctx: 1.0})


def grad_ignores_d(name):
    return Mutation(f"{name} ignores d", {"d_of": lambda d, ctx: 1.0 if ctx["name"] == name else d})


def grad_overwritten(name):
    return Mutation(f"{name} overwritten", {"prior": lambda v, ctx: v * 0 if ctx["name"] == name else v})


def gbp_last_row_lost():
    def f(x, ctx):
        x = x.clone()
        x[-1] = 0
        return x
    return Mutation("last row lost in gbp", {"gbp_rows": f})


def dmlm_over_three():
    return Mutation("dmlm = d alpha / 3", {"nmlm": lambda n, ctx: 3})


def last_granule_dropped():
    return Mutation("last K granule of the pooler dropped", {"drop_last_granule": lambda f, ctx: True})


# ------------------------------------------------------------------------------------------------ values with a running error
class Num:
    """A float64 value ``v`` and the magnitude ``e`` (units of 2^-24) its fp32 evaluation works at; ``emu``: values rounded to fp32."""
    __slots__ = ("v", "e", "emu")

    def __init__(self, v, e=None, emu=False):
        self.v, self.e, self.emu = v, (torch.zeros_like(v) if e is None else e), emu

    def _out(self, v, e):
        v = _f32(v) if self.emu else v
        return Num(v, e + v.abs(), self.emu)

    @staticmethod
    def _lift(x, like):
        return x if isinstance(x, Num) else Num(torch.as_tensor(x, dtype=torch.float64), None, like.emu)

    def __add__(self, o):
        o = Num._lift(o, self)
        return self._out(self.v + o.v, _q(self.e, o.e))
    __radd__ = __add__

    def __sub__(self, o):
        o = Num._lift(o, self)
        return self._out(self.v - o.v, _q(self.e, o.e))

    def __rsub__(self, o):
        return Num._lift(o, self) - self

    def __mul__(self, o):
        o = Num._lift(o, self)
        return self._out(self.v * o.v, _q(self.v.abs() * o.e, self.e * o.v.abs()))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Num._lift(o, self)
        q = self.v / o.v
        return self._out(q, _q(self.e, q.abs() * o.e) / o.v.abs())

    def __neg__(self):
        return Num(-self.v, self.e, self.emu)

    def __getitem__(self, i):
        return Num(self.v[i], self.e[i], self.emu)

    @property
    def T(self):
        return Num(self.v.t(), self.e.t(), self.emu)

    def reshape(self, *s):
        return Num(self.v.reshape(*s), self.e.reshape(*s), self.emu)

    def with_v(self, v):
        return Num(v, self.e, self.emu)


def _q(a, b):
    """Independent errors add in quadrature."""
    return (a * a + b * b).sqrt()


def cat(xs, dim=0):
    return Num(torch.cat([x.v for x in xs], dim), torch.cat([x.e for x in xs], dim), xs[0].emu)


def _fn(x, f, df, absolute=0.0):
    v = f(x.v)
    v = _f32(v) if x.emu else v
    return Num(v, df(x.v).abs() * x.e + F_FN * v.abs() + absolute + v.abs(), x.emu)


def tanh(x):
    return _fn(x, torch.tanh, lambda t: 1.0 - torch.tanh(t) ** 2)


def exp(x):
    return _fn(x, torch.exp, torch.exp)


def log(x):
    return _fn(x, torch.log, lambda t: 1.0 / t, absolute=F_FN)


def sqrt(x):
    v = torch.sqrt(x.v)
    return x._out(v, x.e / (2.0 * v).clamp_min(1e-300))


def relu(x):
    pos = (x.v > 0).to(torch.float64)
    return Num(x.v * pos, x.e * pos, x.emu)


# ------------------------------------------------------------------------------------------------ products and sums
def _chain(A, B, start=None):
    """A [R, K] x B [K, C] as one MFMA chain: per 16-deep granule q, four steps j = 0 .. 3, each an fp32 add of the exact sum of the
    four products k = 16 q + 4 g + j (g = 0 .. 3: the four lane groups) onto the accumulator."""
    K = A.shape[-1]
    Kp = (K + 15) // 16 * 16
    if Kp != K:
        A = torch.nn.functional.pad(A, (0, Kp - K))
        B = torch.nn.functional.pad(B, (0, 0, 0, Kp - K))
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float64) if start is None else start
    for q in range(Kp // 16):
        a = A[:, 16 * q:16 * q + 16].reshape(-1, 4, 4)
        b = B[16 * q:16 * q + 16].reshape(4, 4, -1)
        s = torch.einsum("rgj,gjc->jrc", a, b)
        for j in range(4):
            acc = _f32(acc + s[j])
    return acc


def _emu_wg(A, B, drop_last=False):
    """One 16 x 16 tile per workgroup (hc_wg_tile): K split over 16 waves in 16-deep granules (gpw = ceil(granules / 16) each), each
    wave an MFMA chain over its granules, the 16 partials added in wave order onto 0."""
    K = A.shape[1]
    gran = K // 16
    gpw = (gran + NW - 1) // NW
    if drop_last:
        A = A.clone()
        A[:, (gran - 1) * 16:] = 0.0
    tot = None
    for w in range(NW):
        g0, g1 = w * gpw, min(w * gpw + gpw, gran)
        part = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float64)
        if g0 < g1:
            part = _chain(A[:, g0 * 16:g1 * 16], B[g0 * 16:g1 * 16])
        tot = part if tot is None else _f32(tot + part)
    return tot


def _emu_wave(A, B):
    """One 16 x 16 tile per wave (hc_wave_tile): one MFMA chain over the (short) inner dimension."""
    return _chain(A, B)


def mm(A: Num, B: Num, kind="wg", drop_last=False) -> Num:
    """A [R, K] @ B [K, C]; kind: "wg" (workgroup tile, K % 16 == 0) or "wave" (wave tile, any K)."""
    a, b = A.v, B.v
    if A.emu:
        v = _emu_wg(a, b, drop_last) if kind == "wg" else _emu_wave(a, b)
    else:
        v = a @ b
    e = F_SUM * (a.abs() @ b.abs()) + (a * a @ (B.e * B.e) + (A.e * A.e) @ (b * b)).sqrt() + v.abs()
    return Num(v, e, A.emu)


def rowdot(A: Num, B: Num, width=4) -> Num:
    """sum_k A[r, k] B[r, k] as a wave per row: lane l takes ``width`` consecutive k at width l + 64 width i, an fp32 running sum
    (i, then the components), then wave_sum's xor butterfly over the 64 lanes (i with i + 32 first)."""
    a, b = A.v, B.v
    prod = a * b
    if A.emu:
        R, K = prod.shape
        Kp = (K + 64 * width - 1) // (64 * width) * (64 * width)
        pp = torch.nn.functional.pad(prod, (0, Kp - K)).reshape(R, Kp // (64 * width), 64, width)
        acc = torch.zeros(R, 64, dtype=torch.float64)
        for i in range(pp.shape[1]):
            for j in range(width):
                acc = _f32(acc + pp[:, i, :, j])
        while acc.shape[1] > 1:
            h = acc.shape[1] // 2
            acc = _f32(acc[:, :h] + acc[:, h:])
        v = acc[:, 0]
    else:
        v = prod.sum(1)
    e = F_SUM * (a.abs() * b.abs()).sum(1) + ((a * B.e) ** 2 + (A.e * b) ** 2).sum(1).sqrt() + v.abs()
    return Num(v, e, A.emu)


def colsum(X: Num, parts=1) -> Num:
    """sum over rows (axis 0): one thread per column, rows in order; ``parts`` > 1: row b goes to partial b % parts (a wave each), the
    partials added in order."""
    x = X.v
    if X.emu:
        ps = []
        for q in range(parts):
            acc = torch.zeros(x.shape[1:], dtype=torch.float64)
            for r in range(q, x.shape[0], parts):
                acc = _f32(acc + x[r])
            ps.append(acc)
        v = ps[0]
        for q in ps[1:]:
            v = _f32(v + q)
    else:
        v = x.sum(0)
    e = F_SUM * x.abs().sum(0) + (X.e ** 2).sum(0).sqrt() + v.abs()
    return Num(v, e, X.emu)


def rowmax(X: Num) -> Num:
    v, i = X.v.max(1, keepdim=True)
    return Num(v, X.e.max(1, keepdim=True).values, X.emu)


# ------------------------------------------------------------------------------------------------ the restatement
def restate(c: Case, emu=False, mutation=None, terms=None) -> dict:
    """The forward and the hand-derived backward of csrc/heads_coop.hip on Num values (see the module docstring).  Returns every
    output as a Num; ``terms`` (a dict): the norms of the separate terms of the multi-term sums, for the inputs' sanity check."""
    mut = mutation
    B, H, R = c.B, c.H, 3 * c.B

    def inp(t):
        return Num(t.detach().to(torch.float64).clone(), None, emu)
    p = {k: inp(v) for k, v in c.params.items()}
    X = inp(c.first)
    beta, alpha, d = _c32(c.beta), _c32(c.alpha), _c32(_hook(mut, "d", c.d))

    def cst(x):                                                 # a constant the kernel forms in fp32
        return _c32(x) if emu else x

    # ---- forward
    pre = mm(X, p["bert.pooler.dense.weight"].T, drop_last=_hook(mut, "drop_last_granule", False)) + p["bert.pooler.dense.bias"].v
    P = tanh(pre)
    rel = mm(X[B:], p["cls.align.weight"].T) + p["cls.align.bias"]
    Wat = p["attn.weight"]
    Wsum = Wat[:, :H] + Wat[:, H:]                              # cat(x, x): x (W1 + W2)^T, added in the operand loader
    Apre = mm(P, Wsum.T) + p["attn.bias"]
    t_rel = mm(P[:B], p["cls.seq_relationship.weight"].T) + p["cls.seq_relationship.bias"]
    A = relu(Apre)
    vrows = cat([Num(p[f"{GATES[m]}.weight"].v.expand(B, H).clone(), None, emu) for m in range(3)])
    vb = torch.cat([p[f"{GATES[m]}.bias"].v.expand(B) for m in range(3)])
    g = rowdot(A, vrows) + vb                                    # [R]
    nx = sqrt(rowdot(P, P))
    C = cat([P[m * B:(m + 1) * B] * g[m * B:(m + 1) * B].reshape(B, 1) for m in range(3)], 1)      # [B, 3H]
    T = mm(C, p["classifier1_1.weight"].T) + p["classifier1_1.bias"]
    XP = cat([mm(T, p[f"{CPCS[m]}.weight"].T) + p[f"{CPCS[m]}.bias"] for m in range(3)])            # [R, H]
    lo = mm(T, p["classifier1_2.weight"].T) + p["classifier1_2.bias"]                              # [B, 1]
    tanh_lo = c.num_labels == 1
    logits = tanh(lo) if tanh_lo else lo
    ny = sqrt(rowdot(XP, XP))
    wgt = cst(-_hook(mut, "beta_dS", beta) / B)
    eye = _hook(mut, "eye", torch.eye(B, dtype=torch.float64))
    dS, rsum, csum, nce_parts = [], [], [], []
    for m in range(3):
        sl = slice(m * B, (m + 1) * B)
        S = mm(P[sl], XP[sl].T) / (nx[sl].reshape(B, 1) * ny[sl].reshape(1, B))
        mx = rowmax(S)
        ex = exp(S - mx)
        se = rowdot(ex, Num(torch.ones_like(ex.v), None, emu), width=1)
        sm = ex / se.reshape(B, 1)
        sm = sm.with_v(_hook(mut, "softmax", sm.v, m=m, S=S.v))
        ds = wgt * (sm - Num(eye, None, emu))
        dS.append(ds)
        rsum.append(rowdot(ds, S, width=1))
        csum.append(colsum(ds * S, parts=NW))
        diag = Num((S.v * eye).sum(1), (S.e * eye).sum(1), emu)
        term = (mx.reshape(B) + log(se) - diag) / float(B)
        nce_parts.append(colsum(term.reshape(B, 1), parts=NW).reshape(1))
    nce = nce_parts[0] + nce_parts[1] + nce_parts[2]
    # alignment CE and the label loss
    ap_v, ap_s = c.ap_v, _hook(mut, "ap_s", c.ap_s, ap_v=c.ap_v)
    y = torch.cat([ap_v, ap_s]).to(torch.float64)
    a0, a1 = rel[:, 0], rel[:, 1]
    mxr = Num(torch.maximum(a0.v, a1.v), torch.maximum(a0.e, a1.e), emu)
    lse = mxr + log(exp(a0 - mxr) + exp(a1 - mxr))
    sc = cst(0.5 / B)
    picked = Num(torch.where(y > 0, a1.v, a0.v), torch.where(y > 0, a1.e, a0.e), emu)
    ce_terms = (lse - picked) * sc
    ce = _tree_sum(ce_terms)
    drel = cat([((exp(a0 - lse) - (y == 0).double()) * sc).reshape(2 * B, 1), ((exp(a1 - lse) - (y == 1).double()) * sc).reshape(2 * B, 1)], 1)
    vlo = logits.reshape(B)
    dd = vlo - Num(c.sent.to(torch.float64), None, emu)
    se_l = _tree_sum(dd * dd / float(B))
    dtanh = (1.0 - vlo * vlo) if tanh_lo else 1.0
    dtanh = _hook(mut, "dlo_tanh", dtanh)
    dlo = (2.0 * dd / float(B) * dtanh).reshape(B, 1)
    heads = ce + se_l - beta * nce
    if c.nmlm:
        ms = colsum(Num(c.mlm.to(torch.float64).reshape(-1, 1), None, emu)).reshape(1)
        joint = alpha * (ms / float(c.nmlm)) + heads
    else:
        joint = heads
    out = dict(loss=joint, aux=cat([ce.reshape(1), se_l.reshape(1), nce]), out5=cat([ce.reshape(1), se_l.reshape(1), nce, heads, joint]),
               logits=logits, t_rel=t_rel, rel=rel)

    # ---- backward (d applied where a result leaves)
    def acc(name, s):
        prior = Num(c.prior.get(name, torch.zeros_like(c.params[name])).to(torch.float64), None, emu)
        prior = prior.with_v(_hook(mut, "prior", prior.v, name=name))
        dn = _c32(_hook(mut, "d_of", d, name=name))
        out[name] = prior + dn * s.reshape(prior.v.shape)

    dPc, dXP = [], []
    for m in range(3):
        sl = slice(m * B, (m + 1) * B)
        XPn = XP[sl] / ny[sl].reshape(B, 1)
        Xn = P[sl] / nx[sl].reshape(B, 1)
        cx = P[sl] / nx[sl].reshape(B, 1) * rsum[m].reshape(B, 1)
        cy = XP[sl] / ny[sl].reshape(B, 1) * csum[m].reshape(B, 1)
        cx = cx.with_v(_hook(mut, "dPc_corr", cx.v, m=m))
        cy = cy.with_v(_hook(mut, "dXP_corr", cy.v, m=m))
        a_ = mm(dS[m], XPn, "wave")
        b_ = mm(dS[m].T, Xn, "wave")
        if terms is not None:
            terms.setdefault("dPc", []).append((a_.v.norm(), cx.v.norm()))
            terms.setdefault("dXP", []).append((b_.v.norm(), cy.v.norm()))
        dPc.append((a_ - cx) / nx[sl].reshape(B, 1))
        dXP.append((b_ - cy) / ny[sl].reshape(B, 1))
    dPc, dXPc = cat(dPc), cat(dXP, 1)                           # [R, H], [B, 3H]
    Wq = cat([p[f"{CPCS[m]}.weight"] for m in range(3)])        # [3H, H]
    Wc2 = p["classifier1_2.weight"]                             # [1, H]
    dT = mm(dXPc, Wq) + dlo * Wc2
    if terms is not None:
        terms["dT"] = [(dXPc.v[:, m * H:(m + 1) * H] @ Wq.v[m * H:(m + 1) * H]).norm() for m in range(3)] + [(dlo.v * Wc2.v).norm()]
    for m in range(3):
        acc(f"{CPCS[m]}.weight", mm(dXP[m].T, T, "wave"))
        acc(f"{CPCS[m]}.bias", colsum(dXP[m]))
    dC = mm(dT, p["classifier1_1.weight"])                      # [B, 3H]
    acc("classifier1_1.weight", mm(dT.T, C, "wave"))
    acc("classifier1_1.bias", colsum(dT))
    acc("classifier1_2.weight", colsum(dlo * T))
    acc("classifier1_2.bias", colsum(dlo))
    dCr = cat([dC[:, m * H:(m + 1) * H] for m in range(3)])     # [R, H]: row m B + b = dC[b, m H ...]
    dg = rowdot(dCr, P)
    dP0 = dCr * g.reshape(R, 1) + dPc
    mask = (Apre.v > 0).to(torch.float64)
    dA = Num(mask, None, emu) * (dg.reshape(R, 1) * vrows)
    E = dg.reshape(R, 1) * A
    E = E.with_v(_hook(mut, "E", E.v, dg=dg.v, Apre=Apre.v))
    Wb = Wsum
    Wb = Wb.with_v(_hook(mut, "W_dP", Wb.v, W1=Wat.v[:, :H]))
    dPA = mm(dA, Wb)
    dP = dPA + dP0
    if terms is not None:
        terms["dP"] = [(dCr.v * g.v.reshape(R, 1)).norm(), dPc.v.norm(), dPA.v.norm()]
    dtp = 1.0 - P * P
    dtp = dtp.with_v(_hook(mut, "tanh_pool", dtp.v))
    dpre = dP * dtp
    gA = mm(dA.T, P, "wave")
    acc("attn.weight", cat([gA, gA], 1))
    acc("attn.bias", colsum(dA))
    for m in range(3):
        sl = slice(m * B, (m + 1) * B)
        acc(f"{GATES[m]}.weight", colsum(E[sl]))
        acc(f"{GATES[m]}.bias", colsum(dg[sl].reshape(B, 1)))
    Wal = p["cls.align.weight"]
    drel_f = drel.with_v(_hook(mut, "drel_rows", drel.v))
    dal = drel_f[:, 0:1] * Wal[0:1] + drel_f[:, 1:2] * Wal[1:2]   # [2B, H]
    dfirst0 = mm(dpre, p["bert.pooler.dense.weight"])
    if terms is not None:
        terms["dfirst"] = [dfirst0.v.norm(), dal.v.norm()]
        terms["loss"] = [ce.v.abs(), se_l.v.abs(), (beta * nce.v).abs()]
    dfirst = cat([dfirst0[:B], dfirst0[B:] + dal])
    out["dfirst"] = d * dfirst
    acc("bert.pooler.dense.weight", mm(dpre.T, X, "wave"))
    dpre_b = dpre.with_v(_hook(mut, "gbp_rows", dpre.v))
    acc("bert.pooler.dense.bias", colsum(dpre_b))
    acc("cls.align.weight", mm(drel.T, X[B:], "wave"))
    acc("cls.align.bias", colsum(drel))
    if c.nmlm:
        nm = _hook(mut, "nmlm", c.nmlm)
        out["dmlm"] = Num(torch.full((c.nmlm,), d, dtype=torch.float64), None, emu) * cst(alpha / nm)
    else:
        out["dmlm"] = None
    return out


def _tree_sum(x: Num) -> Num:
    """One element per thread (i < 2B <= 256): wave_sum's xor butterfly per 64 threads, then the 16 waves' partials in order."""
    n = x.v.shape[0]
    npad = (n + 63) // 64 * 64
    v = torch.nn.functional.pad(x.v, (0, npad - n)).reshape(-1, 64)
    if x.emu:
        while v.shape[1] > 1:
            h = v.shape[1] // 2
            v = _f32(v[:, :h] + v[:, h:])
        v = v[:, 0]
        s = v[0]
        for q in v[1:]:
            s = _f32(s + q)
    else:
        s = x.v.sum()
    e = F_SUM * x.v.abs().sum() + (x.e ** 2).sum().sqrt() + s.abs()
    return Num(s.reshape(()), e.reshape(()), x.emu)


# ------------------------------------------------------------------------------------------------ bounds
def ratios(got, ref: Ref) -> Ratios:
    """rowwise_ref.ratios, with the normwise term at TAU_ACC: the largest elementwise and per-row normwise ratios (<= 1 passes)."""
    r = _RW.ratios(got, ref)
    g = got.detach().to(torch.float64).cpu().reshape(ref.val.shape)
    val, acc = ref.val, ref.acc
    if val.dim() == 1:
        g, val, acc = g[None, :], val[None, :], acc[None, :]
    err = (g - val).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, 1e300), err)
    en, rn = (err ** 2).sum(1).sqrt(), (val ** 2).sum(1).sqrt()
    rmax = val.abs().max(1).values
    n_eff = torch.where(rmax > 0, (rn / rmax) ** 2, torch.ones_like(rn))
    nb = (TAU_OUT + C_OUT / n_eff.sqrt()) * ref.u_out * rn + TAU_ACC * EPS24 * (acc ** 2).sum(1).sqrt()
    qn = torch.where(en == 0, torch.zeros_like(en), en / nb)
    norm = float(torch.nan_to_num(qn, nan=math.inf, posinf=math.inf).max()) if qn.numel() else 0.0
    return Ratios(r.elem, norm, r.exact_bad, r.where)


def check(got, ref: Ref, what=""):
    r = ratios(got, ref)
    assert r.elem <= 1.0 and r.norm <= 1.0, f"{what}: elementwise ratio {r.elem:.3g} (worst at {r.where}), normwise {r.norm:.3g}"
    return r


def expected(c: Case, ref=None, bounds=None) -> dict:
    """name -> Ref: the autograd value with the restatement's acc (float64, no emulation)."""
    ref = reference(c) if ref is None else ref
    bounds = restate(c) if bounds is None else bounds
    out = {}
    for k in OUTPUTS:
        if ref.get(k) is None:
            continue
        v = ref[k].reshape(bounds[k].v.shape) if ref[k].numel() == bounds[k].v.numel() else ref[k]
        out[k] = Ref(v, bounds[k].e, 0.0, U_F32)
    return out


def check_all(got: dict, exp: dict, what="", worst=None):
    """check() every output in ``got`` (name -> tensor) against ``exp``; ``worst`` (dict output name -> [elem, norm, case of the
    largest elem, case of the largest norm]) collects the ratios."""
    for k, t in got.items():
        r = check(t.reshape(exp[k].val.shape), exp[k], f"{what} {k}")
        if worst is not None:
            w = worst.setdefault(k, [0.0, 0.0, "", ""])
            if r.elem > w[0]:
                w[0], w[2] = r.elem, what
            if r.norm > w[1]:
                w[1], w[3] = r.norm, what


def _group(k):
    if k in ("loss", "aux", "out5", "dmlm"):
        return "losses"
    if k in ("logits", "t_rel", "rel"):
        return "logits/rel"
    return "dfirst" if k == "dfirst" else "parameters"


def kink_ratio(c: Case) -> float:
    """min over Apre of |Apre| / (2^-24 acc): the inputs keep it >= KINK, so that fp32 and float64 agree on relu's side."""
    b = _apre(c)
    return float((b.v.abs() / (b.e * 2.0 ** -24)).min())


def _apre(c):
    p = {k: Num(c.params[k].to(torch.float64)) for k in ("bert.pooler.dense.weight", "bert.pooler.dense.bias", "attn.weight", "attn.bias")}
    X = Num(c.first.to(torch.float64))
    P = tanh(mm(X, p["bert.pooler.dense.weight"].T) + p["bert.pooler.dense.bias"].v)
    W = p["attn.weight"]
    return mm(P, (W[:, :c.H] + W[:, c.H:]).T) + p["attn.bias"]


# ------------------------------------------------------------------------------------------------ inputs
def make_case(B, H, seed, *, num_labels=7, alpha=0.6, beta=0.7, nmlm=3, d=1.0, ap="mixed", prior=True, features=True) -> Case:
    """Head weights at a scale where every term of every output counts (asserted by the CPU test); ``features``: a tiny-norm sample
    (all three rows x 2^-10: x / |x| of the pooled and the projected rows), a duplicate sample, saturating pooler rows (x 8);
    ``ap``: "mixed" (speech labels the complement of the visual ones), "zeros", "ones".  Rows whose Apre comes within KINK bounds
    of 0 are redrawn."""
    g = torch.Generator().manual_seed(seed)
    R = 3 * B

    def w(o, i, s):
        return torch.randn(o, i, generator=g) * (s / math.sqrt(i))

    def b(n, s):
        return torch.randn(n, generator=g) * s
    p = {"bert.pooler.dense.weight": w(H, H, 1.0), "bert.pooler.dense.bias": b(H, 1e-3),
         "cls.align.weight": w(2, H, 1.0), "cls.align.bias": b(2, 0.3),
         "cls.seq_relationship.weight": w(2, H, 1.0), "cls.seq_relationship.bias": b(2, 0.3),
         "attn.weight": w(H, 2 * H, 1.0), "attn.bias": (0.1 + b(H, 0.5).abs()) * torch.sign(b(H, 1.0)),
         "classifier1_1.weight": w(H, 3 * H, 1.0), "classifier1_1.bias": b(H, 1e-3),
         "classifier1_2.weight": w(1, H, 0.5 if num_labels == 1 else 1.0), "classifier1_2.bias": b(1, 0.1)}
    for m in range(3):
        p[f"{GATES[m]}.weight"] = w(1, H, 2.0)
        p[f"{GATES[m]}.bias"] = b(1, 0.5)
        p[f"{CPCS[m]}.weight"] = w(H, H, 1.0)
        p[f"{CPCS[m]}.bias"] = b(H, 1e-3)
    scale = torch.ones(R, 1)
    dup = None
    if features and B >= 3:
        tiny, sat = B - 2, 0
        scale[[tiny, B + tiny, 2 * B + tiny]] = 2.0 ** -10
        scale[[sat, B + 1 if B > 1 else sat]] = 8.0
        dup = (1, B - 1)                                        # sample B - 1 repeats sample 1
    base = torch.randn(R, H, generator=g)

    def rows():
        x = base * scale
        if dup is not None:
            for m in range(3):
                x[m * B + dup[1]] = x[m * B + dup[0]]
        return x.to(torch.bfloat16).float()
    c = Case(B, H, rows(), p, None, None, None, num_labels, alpha, beta, None, d)
    for _ in range(100):
        a = _apre(c)
        bad = ((a.v.abs() / (a.e * 2.0 ** -24)) < KINK).any(1).nonzero().flatten().tolist()
        if not bad:
            break
        for r in bad:
            if dup is not None and r % B == dup[1]:
                r = (r // B) * B + dup[0]
            base[r] = torch.randn(H, generator=g)
        c.first = rows()
    assert kink_ratio(c) >= KINK
    ap_v = torch.randint(0, 2, (B,), generator=g)
    if ap == "zeros":
        ap_v = torch.zeros(B, dtype=torch.long)
    elif ap == "ones":
        ap_v = torch.ones(B, dtype=torch.long)
    c.ap_v, c.ap_s = ap_v, (1 - ap_v if ap == "mixed" else ap_v.clone())
    c.sent = torch.rand(B, generator=g) * 6 - 3                 # outside tanh's range for the 1-label head
    if nmlm:
        c.mlm = torch.rand(nmlm, generator=g) * 4 + 5
    if prior:
        c.prior = {n: torch.randn(p[n].shape, generator=g) * 0.1 for n in PARAMS}
    return c
