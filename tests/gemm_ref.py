"""A float64 reference for the GEMM kernels (csrc/gemm.hip) and a scale-aware check of their outputs.

Not a test module (pytest does not collect it): ``from tests import gemm_ref as G``.

``nt`` / ``splitk`` / ``tn`` / ``colsum`` with ``emu=False`` are the reference: plain float64 torch on the CPU, on the same bf16
inputs (and the same fp32 alpha, bias and fp32 W) the kernels get:

    gemm_nt        out = epi(alpha * alpha_dev * A . B^T)   epi in: plain | +bias | gelu(+bias) with aux = the pre-activation |
                   (+bias) * keep * drop_scale + R | + R | * gelu'(U) | fp32 out | +bias, fp32 out
    gemm_nt_splitk out = A . B^T (+ R)
    gemm_tn        W = [W0 +] alpha * A^T . B          bias = bias0 + alpha * colsum(A)
    colsum         out = out0 + alpha * colsum(X)

Each returns ``Ref`` objects: the exact value, the rounding scale ``S = |alpha| |A| . |B|^T`` (float64), the magnitude of what the
fp32 epilogue adds (``E``: |bias|, |R|, |W0| ...), the exact value an output must take where it is known bit for bit (rows of A or
columns of B that are all zero: ``exact``, NaN elsewhere) and the output tile the check groups by.  Dropout comes in as the keep
mask the library exports (``ops.dropout_mask``).  At large M the reference is evaluated on a subset of rows (``row_subset``).

``emu=True`` is the emulation: the same operations with the kernels' documented roundings -- bf16 products exact in fp32, summed in
32-term blocks (the K step of v_mfma_f32_16x16x32_bf16) into an fp32 accumulator, alpha and the epilogue in fp32, the final bf16
rounding; the TN path over 32-token blocks per split, split slabs added in split order; split-K slabs added in order.  It exists only
to calibrate the bounds below on the CPU.

``check(got, ref)`` asserts, for every compared element,

    elementwise   |got - ref| <= C_OUT * u_out * |ref| + C_ACC * 2^-24 * acc + extra
    normwise      ||got - ref||_T <= TAU_OUT * u_out * ||ref||_T + TAU_ACC * 2^-24 * ||acc||_T + ||extra||_T     per output tile T

with u_out = 2^-8 (bf16 out) or 2^-23 (fp32 out), acc = sqrt(K) * S + E (for GELU: |gelu'(v)| (sqrt(K) S + |bias|); for GELU':
|gelu'(U)| sqrt(K) S), extra = the erf approximation (GELU_ABS; GELU' GELUP_ABS * |v|), and the tile the kernel ran
(``ops.gemm_nt_describe``: 128 x 128 or 128 / 192 / 224 / 256 x 256; TN: 256 x 256).  Where ``exact`` is set the output must equal it.

Calibration (tests/test_gemm_reference_cpu.py; every case there): ``emulate`` against ``reference`` over every operation and
epilogue, K = 64 ... 3072 (split-K to 30 592, TN over 33 ... 4129 tokens with 1, 2, 3 and 8 splits), on the realistic,
cancellation-heavy, 2^+-20-scaled and zero-row inputs.  Largest ratios the emulation reached (elementwise / normwise) with

    C_OUT = 2, C_ACC = 0.75, TAU_OUT = 0.8, TAU_ACC = 0.2

    op                        elementwise  normwise        op                   elementwise  normwise
    plain, bias, resid(+drop)  0.50         0.51            fp32 out (+bias)      0.21         0.14
    GELU out / aux             0.50         0.52            split-K (+resid)      0.50         0.49
    GELU'                      0.50         0.49            TN W / bias           0.52 / 0.12  0.13
    colsum                     0.27         0.06

Two things the emulation forced.  A bf16 output rounds by up to u = 2^-8 of its value, so C_OUT is 2 for a ratio of 0.5.  A tile
whose norm sits in a few elements (the 2^+-20 inputs, corner tiles of 2 x 8) cannot average its roundings, so the normwise rounding
term is (TAU_OUT + C_OUT / sqrt(n_eff)) u ||ref||_T with n_eff = ||ref||_T^2 / max|ref|_T^2: TAU_OUT on large tiles, about the
elementwise bound on a tile of one element.  And every split slab (TN) or partial sum (colsum's row blocks, added by atomics) is one
more fp32 rounding onto W0 / bias0 / out0: that term counts ``splits`` times.  The GELU terms are twice the floors the kernels'
single-transcendental erf forms reach on a dense grid (tests/test_kernels_gpu.py::test_gelu_and_its_derivative_on_a_dense_grid:
5.7e-7 and 4.1e-6).

The smallest margin of a mutation is recorded in the CPU test's docstring.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

C_OUT, C_ACC = 2.0, 0.75
TAU_OUT, TAU_ACC = 0.8, 0.2
GELU_ABS, GELUP_ABS = 1.2e-6, 8.2e-6
U_BF16, U_F32 = 2.0 ** -8, 2.0 ** -23
EPS24 = 2.0 ** -24
CUS = 256                     # MI355X compute units (the split-K plan of the emulation)

NAN_BF16 = 0x7FC5             # canary patterns: quiet NaNs with a payload no kernel writes
NAN_F32 = 0x7FC5A5A5


def _f32(x):
    return x.to(torch.float32).to(torch.float64)


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float64)


def _c32(v):
    """A Python float as the kernel receives it (fp32)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def gelu_grad64(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------ mutations
@dataclass
class Mutation:
    """A value-only perturbation applied inside ``reference`` or ``emulate``: ``hooks[stage](x, ctx)`` replaces the value of a stage
    (stages: A, B, alpha, bias, keep, resid_scaled, U, aux_after, tn_rows, tn_bias_alpha, acc_flags)."""
    name: str
    hooks: dict = field(default_factory=dict)


def _hook(mut, stage, x, **ctx):
    if mut is None or stage not in mut.hooks:
        return x
    return mut.hooks[stage](x, ctx)


def drop_k_tile(row_tile, k_tile, bm):
    """One 64-deep K tile left out for the rows of one row tile."""
    def f(A, ctx):
        A = A.clone()
        A[row_tile * bm:(row_tile + 1) * bm, k_tile * 64:(k_tile + 1) * 64] = 0
        return A
    return Mutation(f"drop K tile {k_tile} of row tile {row_tile}", {"A": f})


def drop_k_term_last_row(k):
    """One K term left out of the last row (the last row of a partial tile)."""
    def f(A, ctx):
        A = A.clone()
        A[-1, k] = 0
        return A
    return Mutation(f"drop K term {k} of the last row", {"A": f})


def alpha_scale(factor=1.0 + 2.0 ** -6):
    return Mutation(f"alpha x {factor}", {"alpha": lambda a, ctx: a * factor})


def bias_shift(col_tile, bn):
    """The bias read one column to the right in one column tile."""
    def f(b, ctx):
        lo, hi = col_tile * bn, min((col_tile + 1) * bn, b.numel())
        b2 = b.clone()
        b2[lo:hi] = b[(torch.arange(lo, hi) + 1).clamp(max=b.numel() - 1)]
        return b2
    return Mutation(f"bias one column right in column tile {col_tile}", {"bias": f})


def keep_row_shift():
    """The dropout keep index off by one row (row m uses the bits of row m + 1)."""
    return Mutation("dropout keep index + one row", {"keep": lambda k, ctx: torch.roll(k, -1, 0)})


def resid_scaled():
    """The dropout scale applied to the residual as well."""
    return Mutation("dropout scale on the residual", {"resid_scaled": lambda x, ctx: True})


def gelu_u_neighbour():
    """GELU' reading U from the neighbouring row."""
    return Mutation("GELU' U from the next row", {"U": lambda U, ctx: torch.roll(U, -1, 0)})


def aux_after_activation():
    return Mutation("aux stored after GELU", {"aux_after": lambda x, ctx: True})


def tn_row_lost_at_split(split_boundary_row):
    """TN: one token row lost at a split boundary (the first row of split 1)."""
    def f(X, ctx):
        X = X.clone()
        X[split_boundary_row] = 0
        return X
    return Mutation(f"TN token row {split_boundary_row} lost", {"tn_rows": f})


def tn_bias_without_alpha():
    return Mutation("TN bias sum without alpha", {"tn_bias_alpha": lambda a, ctx: 1.0})


def grouped_ignores_accumulate(problem):
    def f(flags, ctx):
        flags = list(flags)
        flags[problem] = not flags[problem]
        return flags
    return Mutation(f"grouped TN problem {problem} ignores its accumulate flag", {"acc_flags": f})


def splitk_last_split_dropped(M, N, K):
    """Split-K: the last (shorter) split left out."""
    zs, per = splitk_plan(M, N, K)
    lo = (zs - 1) * per * 64

    def f(A, ctx):
        A = A.clone()
        A[:, lo:] = 0
        return A
    return Mutation(f"split-K last split (K {lo}..{K}) dropped", {"A": f})


# ------------------------------------------------------------------------------------------------ products
def _product(A, B, emu, block=32):
    """A [R, K] x B [N, K]^T.  Reference: float64.  Emulation: 32-term blocks summed exactly and rounded into an fp32 accumulator."""
    A64, B64 = A.to(torch.float64), B.to(torch.float64)
    if not emu:
        return A64 @ B64.t()
    K = A.shape[1]
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float64)
    for k0 in range(0, K, block):
        acc = _f32(acc + A64[:, k0:k0 + block] @ B64[:, k0:k0 + block].t())
    return acc


def _scale(A, B):
    return A.to(torch.float64).abs() @ B.to(torch.float64).abs().t()


@dataclass
class Ref:
    val: torch.Tensor                 # float64 [R, C]: the exact output on ``rows``
    acc: torch.Tensor                 # float64 [R, C]: accumulation / fp32-epilogue magnitude (times 2^-24 in the bound)
    extra: torch.Tensor | float       # absolute term (erf approximation)
    u_out: float
    tile: tuple                       # (rows, columns) of the output tile the kernel ran
    rows: torch.Tensor | None = None  # int64 [R]: output rows compared (None: all)
    exact: torch.Tensor | None = None # float64 [R, C]: the bit-exact value (NaN: none)
    cols: torch.Tensor | None = None  # int64 [C]: output columns compared (None: all)


def _rows(rows, M):
    return torch.arange(M) if rows is None else rows


def nt(A, B, *, bias=None, gelu=False, resid=None, keep=None, drop_scale=1.0, gelu_u=None, alpha=1.0, alpha_dev=None,
       out_f32=False, rows=None, tile=(128, 128), emu=False, mutation=None):
    """mmbert_gemm_nt on CPU tensors (A [M,K] bf16, B [N,K] bf16, bias [N] fp32, resid / gelu_u [M,N] bf16, keep [M,N] 0/1).
    Returns {"out": Ref[, "aux": Ref]} (aux: the GELU form's pre-activation), or the emulated tensors with ``emu``."""
    M, K = A.shape
    N = B.shape[0]
    r = _rows(rows, M)
    Af = _hook(mutation, "A", A.to(torch.float64))
    Bf = _hook(mutation, "B", B.to(torch.float64))
    a = _c32(alpha) * (_c32(float(alpha_dev)) if alpha_dev is not None else 1.0)
    if emu:
        a = _c32(a)                                                  # (the kernel multiplies the two in fp32)
    a = _hook(mutation, "alpha", a)
    R32 = _f32 if emu else (lambda x: x)
    Ar = Af[r]
    P = _product(Ar, Bf, emu)
    S = abs(a) * _scale(A[r], B)
    v = R32(P * a)
    E = torch.zeros_like(v)
    res = {}
    exact = torch.full_like(v, float("nan"))
    zero = (A[r].to(torch.float64).abs().sum(1) == 0)[:, None] | (B.to(torch.float64).abs().sum(1) == 0)[None, :]
    out_exact = not gelu and not (bias is not None and keep is not None)
    b = None
    if bias is not None:
        b = _hook(mutation, "bias", bias.to(torch.float64))
        v = R32(v + b[None, :])
        E = E + b.abs()[None, :]
    acc = math.sqrt(K) * S + E
    extra = 0.0
    if gelu:
        aux_v = v
        g = gelu64(v)
        if emu:
            g = _f32(gelu64(v))
        accg = gelu_grad64(v).abs() * acc
        if _hook(mutation, "aux_after", False):
            aux_v = g
        res["aux"] = Ref(_bf(aux_v) if emu else aux_v, acc, 0.0, U_BF16, tile, rows,
                         torch.where(zero, _bf(v.new_zeros(v.shape) + (b[None, :] if b is not None else 0)), exact))
        v, acc, extra = g, accg, GELU_ABS
    if gelu_u is not None:
        U = _hook(mutation, "U", gelu_u.to(torch.float64))[r]
        gp = gelu_grad64(U)
        extra = GELUP_ABS * v.abs()
        acc = gp.abs() * acc
        v = R32(v * (_f32(gp) if emu else gp))
    if resid is not None:
        Rr = resid.to(torch.float64)[r]
        if keep is not None:
            kp = _hook(mutation, "keep", keep.to(torch.float64))[r]
            s = _c32(drop_scale)
            v = R32(R32(v * s) * kp)
            acc = acc * s * kp
            if _hook(mutation, "resid_scaled", False):
                Rr = Rr * s
        v = R32(v + Rr)
        acc = acc + Rr.abs()
    val = v if out_f32 else (_bf(v) if emu else v)
    if emu:
        return {k: (x.val if isinstance(x, Ref) else x) for k, x in {**res, "out": val}.items()}
    if out_exact:
        z = torch.zeros_like(v)
        if b is not None:
            z = z + b[None, :]
        if resid is not None:
            z = _f32(z + resid.to(torch.float64)[r])
        exact = torch.where(zero, z if out_f32 else _bf(z), exact)
    res["out"] = Ref(val, acc, extra, U_F32 if out_f32 else U_BF16, tile, rows, exact)
    return res


def splitk_plan(M, N, K, cus=CUS):
    """(workgroups along K, K tiles per workgroup) of mmbert_gemm_nt_splitk."""
    tiles, kt = ((M + 127) // 128) * ((N + 127) // 128), K // 64
    splits = max(1, min((2 * cus + tiles - 1) // tiles, kt // 4))
    per = (kt + splits - 1) // splits
    return (kt + per - 1) // per, per


def splitk(A, B, *, resid=None, rows=None, emu=False, mutation=None):
    """mmbert_gemm_nt_splitk: A . B^T (+ R), bf16 out."""
    M, K = A.shape
    N = B.shape[0]
    r = _rows(rows, M)
    Af = _hook(mutation, "A", A.to(torch.float64))[r]
    Bf = B.to(torch.float64)
    if emu:
        zs, per = splitk_plan(M, N, K)
        v = None
        for z in range(zs):
            k0, k1 = z * per * 64, min(K, (z + 1) * per * 64)
            part = _product(Af[:, k0:k1], Bf[:, k0:k1], True)
            v = part if v is None else _f32(v + part)
    else:
        v = Af @ Bf.t()
    acc = math.sqrt(K) * _scale(A[r], B)
    exact = torch.full_like(v, float("nan"))
    zero = (A[r].to(torch.float64).abs().sum(1) == 0)[:, None] | (B.to(torch.float64).abs().sum(1) == 0)[None, :]
    if resid is not None:
        Rr = resid.to(torch.float64)[r]
        v = _f32(v + Rr) if emu else v + Rr
        acc = acc + Rr.abs()
        exact = torch.where(zero, Rr, exact)
    else:
        exact = torch.where(zero, torch.zeros_like(v), exact)
    if emu:
        return {"out": _bf(v)}
    return {"out": Ref(v, acc, 0.0, U_BF16, (128, 128), rows, exact)}


def tn_rows_per_split(M, splits):
    return (((M + splits - 1) // splits) + 31) // 32 * 32


def tn(A, B, *, W0=None, bias0=None, with_bias=False, alpha=1.0, alpha_dev=None, accumulate=True, cols=None, splits=1, emu=False,
       mutation=None):
    """mmbert_gemm_tn on CPU tensors: A [M,N] bf16, B [M,K] bf16, W0 [N,K] fp32 (used when ``accumulate``), bias0 [N] fp32.
    ``cols``: the W rows (output rows n) compared.  ``splits``: the kernel's token split (mmbert_gemm_tn_workspace), i.e. the number
    of fp32 additions onto W0 and bias0, and the emulation's split.  Returns {"W": Ref[, "bias": Ref]}."""
    M, N = A.shape
    K = B.shape[1]
    n = _rows(cols, N)
    A64 = _hook(mutation, "tn_rows", A.to(torch.float64))[:, n]
    B64 = _hook(mutation, "tn_rows", B.to(torch.float64))
    a = _c32(alpha) * (_c32(float(alpha_dev)) if alpha_dev is not None else 1.0)
    a = _hook(mutation, "alpha", a)
    ab = _hook(mutation, "tn_bias_alpha", a)
    At, Bt = A64.t().contiguous(), B64.t().contiguous()
    res = {}
    if emu:
        rps = tn_rows_per_split(M, splits)
        parts, bparts = [], []
        for s in range(splits):
            m0, m1 = s * rps, min(M, (s + 1) * rps)
            if m0 >= m1:
                continue
            parts.append(_f32(_product(At[:, m0:m1], Bt[:, m0:m1], True) * a))
            bparts.append(_f32(_product(At[:, m0:m1], torch.ones(1, m1 - m0, dtype=torch.float64), True)[:, 0] * ab))
        W = parts[0]
        if accumulate:
            W = _f32(W + W0.to(torch.float64)[n])
        for p in parts[1:]:
            W = _f32(W + p)
        res["W"] = W
        if with_bias:
            bb = _f32(bias0.to(torch.float64)[n] + bparts[0])
            for p in bparts[1:]:
                bb = _f32(bb + p)
            res["bias"] = bb
        return res
    W = a * (At @ Bt.t())
    acc = math.sqrt(M) * abs(a) * (A.to(torch.float64)[:, n].abs().t() @ B.to(torch.float64).abs())
    zero = (A.to(torch.float64)[:, n].abs().sum(0) == 0)[:, None] | (B.to(torch.float64).abs().sum(0) == 0)[None, :]
    base = torch.zeros_like(W)
    if accumulate:
        base = W0.to(torch.float64)[n]
        W = W + base
        acc = acc + splits * base.abs()                       # (every split's slab is one more fp32 addition onto W0)
    res["W"] = Ref(W, acc, 0.0, U_F32, (256, 256), cols, torch.where(zero, base, torch.full_like(W, float("nan"))), None)
    if with_bias:
        b0 = bias0.to(torch.float64)[n]
        col = A64.sum(0)
        bv = b0 + ab * col
        bacc = math.sqrt(M) * abs(a) * A.to(torch.float64)[:, n].abs().sum(0) + splits * b0.abs()
        bz = A.to(torch.float64)[:, n].abs().sum(0) == 0
        res["bias"] = Ref(bv[:, None], bacc[:, None], 0.0, U_F32, (256, 1), cols,
                          torch.where(bz, b0, torch.full_like(b0, float("nan")))[:, None])
    return res


def tn_grouped(problems, accumulate, *, alpha=1.0, cols=None, emu=False, mutation=None):
    """mmbert_gemm_tn_grouped_rows: problems = [(A, B, W0, bias0 or None)] (CPU), ``accumulate``: one flag per problem.  ``cols``:
    per problem the W rows compared (or None).  The token axis is never split when rows differ; the emulation takes one split."""
    flags = _hook(mutation, "acc_flags", list(accumulate))
    out = []
    for i, (A, B, W0, b0) in enumerate(problems):
        out.append(tn(A, B, W0=W0, bias0=b0, with_bias=b0 is not None, alpha=alpha, accumulate=flags[i],
                      cols=None if cols is None else cols[i], emu=emu))
    return out


def colsum_adds(M, N, deterministic):
    """How many partial sums mmbert_colsum adds onto out (one per row block of its grid)."""
    if deterministic:
        return 1
    gx = (N // 8 + 63) // 64
    gy = (2048 + gx - 1) // gx
    rows = max(32, (M + gy - 1) // gy)
    return (M + rows - 1) // rows


def colsum(X, out0, *, alpha=1.0, alpha_dev=None, adds=1, emu=False):
    """mmbert_colsum: out0 + alpha * colsum(X); ``adds``: the partial sums added onto out0 (``colsum_adds``).  The emulation: 32-row
    blocks in fp32."""
    M, N = X.shape
    ones = torch.ones(M, 1, dtype=torch.bfloat16)
    r = tn(X, ones, W0=out0[:, None], alpha=alpha, alpha_dev=alpha_dev, accumulate=True, splits=adds, emu=emu)
    if emu:
        return {"out": r["W"][:, 0]}
    w = r["W"]
    return {"out": Ref(w.val, w.acc, 0.0, U_F32, (512, 1), None, w.exact)}


# ------------------------------------------------------------------------------------------------ row subsets
def row_subset(M, bm, seed, seeded=16):
    """Rows of an M-row output the reference is evaluated on: per row tile of ``bm`` rows the first and the last, ``seeded`` rows
    (one per residue mod 16 when seeded == 16: every MFMA lane row of a 16-row fragment group), and every row of a partial last tile."""
    g = torch.Generator().manual_seed(seed)
    out = []
    tiles = (M + bm - 1) // bm
    for t in range(tiles):
        m0, m1 = t * bm, min(M, (t + 1) * bm)
        if m1 - m0 < bm:
            out.append(torch.arange(m0, m1))
            continue
        out.append(torch.tensor([m0, m1 - 1]))
        groups = bm // 16
        j = torch.randint(0, groups, (seeded,), generator=g)
        out.append(m0 + 16 * j + torch.arange(seeded) % 16)
    return torch.unique(torch.cat(out))


# ------------------------------------------------------------------------------------------------ the check
@dataclass
class Ratios:
    elem: float
    norm: float
    exact_bad: int
    where: tuple

    @property
    def worst(self):
        return max(self.elem, self.norm, math.inf if self.exact_bad else 0.0)


def ratios(got, ref: Ref) -> Ratios:
    """The largest elementwise and normwise ratios error / bound (<= 1 passes) and the count of exact-value misses."""
    g = got.detach()
    if g.dim() == 1:
        g = g[:, None]
    if ref.rows is not None:
        g = g[ref.rows.to(g.device)]
    if ref.cols is not None:
        g = g[:, ref.cols.to(g.device)]
    g = g.to(torch.float64).cpu().reshape(ref.val.shape)
    err = (g - ref.val).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    bound = C_OUT * ref.u_out * ref.val.abs() + C_ACC * EPS24 * ref.acc + ref.extra
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.nan_to_num(q, nan=math.inf, posinf=math.inf)
    at = int(q.argmax())
    elem = float(q.max()) if q.numel() else 0.0
    # normwise per output tile
    R, C = ref.val.shape
    rows = _rows(ref.rows, R)
    cols = _rows(ref.cols, C)
    tr, tc = ref.tile
    rt, ct = rows // tr, cols // tc
    nct = int(ct.max()) + 1
    tid = (rt[:, None] * nct + ct[None, :]).reshape(-1)
    ntile = int(tid.max()) + 1

    def tsum(x):
        x = x.reshape(-1) if torch.is_tensor(x) else torch.full((R * C,), float(x), dtype=torch.float64)
        return torch.zeros(ntile, dtype=torch.float64).index_add_(0, tid, x * x).sqrt()
    en = torch.nan_to_num(tsum(torch.where(torch.isinf(err), torch.full_like(err, 1e300), err)), nan=math.inf, posinf=math.inf)
    rn = tsum(ref.val)
    rmax = torch.zeros(ntile, dtype=torch.float64).scatter_reduce_(0, tid, ref.val.abs().reshape(-1), "amax")
    n_eff = torch.where(rmax > 0, (rn / rmax) ** 2, torch.ones_like(rn))       # how many elements carry the tile's norm
    nb = (TAU_OUT + C_OUT / n_eff.sqrt()) * ref.u_out * rn + TAU_ACC * EPS24 * tsum(ref.acc) + tsum(ref.extra)
    qn = torch.where(en == 0, torch.zeros_like(en), en / nb)
    qn = torch.nan_to_num(qn, nan=math.inf, posinf=math.inf)
    norm = float(qn.max())
    bad = 0
    if ref.exact is not None:
        m = ~torch.isnan(ref.exact)
        bad = int((g[m] != ref.exact[m]).sum())
    return Ratios(elem, norm, bad, (int(rows[at // C]), int(cols[at % C])))


def check(got, ref: Ref, what=""):
    """Assert ``got`` (the kernel's whole output, any device) within the bounds of ``ref``; returns the Ratios."""
    r = ratios(got, ref)
    assert r.exact_bad == 0, f"{what}: {r.exact_bad} elements differ from their exact value"
    assert r.elem <= 1.0 and r.norm <= 1.0, f"{what}: elementwise ratio {r.elem:.3g} (worst at row, col {r.where}), normwise {r.norm:.3g}"
    return r


# ------------------------------------------------------------------------------------------------ test inputs
DISTS = ("real", "cancel", "scaled", "zeros")


def operands(M, N, K, dist, seed, wscale=0.02):
    """A [M,K], B [N,K] bf16 (CPU).  real: N(0,1) activations x N(0, wscale) weights; cancel: rows of A with a large common offset
    against rows of B that sum to ~0 (|ref| << S); scaled: per-row / per-column powers of two over 2^+-20; zeros: real with all-zero
    rows of A and of B (exact-zero outputs)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(N, K, generator=g) * wscale
    if dist == "cancel":
        off = (2.0 + 6.0 * torch.rand(M, 1, generator=g)) * torch.sign(torch.randn(M, 1, generator=g))
        A = off + 0.05 * A
        B = B - B.mean(1, keepdim=True)
    elif dist == "scaled":
        A = A * torch.exp2(torch.randint(-20, 21, (M, 1), generator=g).float())
        B = B * torch.exp2(torch.randint(-20, 21, (N, 1), generator=g).float())
    elif dist == "zeros":
        A[torch.unique(torch.tensor([0, M // 2, M - 1]))] = 0
        A[::37] = 0
        B[torch.unique(torch.tensor([0, N // 3, N - 1]))] = 0
    elif dist != "real":
        raise ValueError(dist)
    return A.to(torch.bfloat16), B.to(torch.bfloat16)


def epilogue_inputs(M, N, seed, need=("bias", "R", "U")):
    """bias [N] fp32, R and U [M,N] bf16 (None where not in ``need``)."""
    g = torch.Generator().manual_seed(seed)
    bias = torch.randn(N, generator=g)
    R = torch.randn(M, N, generator=g).to(torch.bfloat16) if "R" in need else None
    U = torch.randn(M, N, generator=g).to(torch.bfloat16) if "U" in need else None
    return bias, R, U


class Canary:
    """An output / aux / W view inside a larger buffer filled with a NaN bit pattern: ``pre`` rows before, ``post`` rows after,
    ``pad`` columns of padding per row (ldc = cols + pad).  ``flat=True``: a contiguous [rows, cols] view in a 1-D buffer with ``pre``
    / ``post`` elements around it (the W views inside the flat gradient buffer).  ``intact()``: every element outside the view still
    holds the pattern bit for bit."""

    def __init__(self, rows, cols, dtype, device, pre=0, post=0, pad=0, flat=False, fill=None):
        self.dtype, self.shape, self.flat = dtype, (rows, cols), flat
        itype, pat = (torch.int16, NAN_BF16) if dtype == torch.bfloat16 else (torch.int32, NAN_F32)
        self.itype, self.pat = itype, pat
        if flat:
            self.buf = torch.full((pre + rows * cols + post,), pat, dtype=itype, device=device).view(dtype)
            self.view = self.buf[pre:pre + rows * cols].view(rows, cols)
            self.inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=device)
            self.inside[pre:pre + rows * cols] = True
        else:
            self.buf = torch.full((pre + rows + post, cols + pad), pat, dtype=itype, device=device).view(dtype)
            self.view = self.buf[pre:pre + rows, :cols]
            self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=device)
            self.inside[pre:pre + rows, :cols] = True
        if fill is not None:
            self.view.copy_(fill)

    def damaged(self):
        """How many elements outside the view lost the pattern."""
        bits = self.buf.view(self.itype)
        return int(((bits != self.pat) & ~self.inside).sum())

    def intact(self, what=""):
        n = self.damaged()
        assert n == 0, f"{what}: {n} elements outside the output changed"
