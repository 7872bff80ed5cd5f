"""A float64 reference for the LayerNorm and cross-entropy kernels (csrc/layernorm.hip, csrc/rowwise.hip) and a scale-aware check of their outputs.

Not a test module (pytest does not collect it): ``from tests import rowwise_ref as R``.

``ln_fwd`` / ``ln_bwd`` / ``ce_fwd`` / ``ce_bwd`` with ``emu=False`` are the reference: plain float64 torch on the CPU, on the same
bf16 rows and fp32 parameters the kernels get (LayerNorm backward: the fp32 mean / rstd the forward left, as the kernel reads them;
cross-entropy: fp32 logits enter rounded to bf16, as the kernel rounds them):

    ln_fwd   y[out_row(i)] = ((x[in_row(i)] - mu) rsqrt(var + eps) gamma + beta) * keep[i + drop_row0] * dscale
             mean[i] = mu, rstd[i] = rsqrt(var + eps)               (biased variance)
    ln_bwd   g = dy[dy_row(i)] * post_keep[drop_row(i)] * post_scale          (0 where dy_row(i) >= dy_row_limit > 0)
             xhat = (x[x_row(i)] - mean) rstd,  dx = rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat))  -> dx[dx_row(i)]
             dx2 = dx * pre_keep[drop_row(i)] * pre_scale,  dgamma += sum g xhat,  dbeta += sum g,  dbias2 += sum dx2 (fp32 values)
    ce_fwd   per segment s: loss[s] = sum_{i in s, 0 <= label < V} (lse_i - logit_i,label) / max(1, count_s)  (0 when count_s = 0)
             row_lse[i] = logsumexp(logit_i,0..V-1) on labelled rows, 0 elsewhere
    ce_bwd   dlogits[i, c] = (softmax_c - [c = label]) * gscale[s] / count_s for c < V on labelled rows; 0 everywhere else

Dropout enters as the keep masks the library exports (``ops.dropout_mask``).  Each returns ``Ref`` objects: the exact value, the
magnitude its fp32 arithmetic works at (``acc``), an absolute term (``extra``), and the value an element must take bit for bit
where it is known (``exact``: dropped elements, unlabelled rows, pad columns; NaN elsewhere).

``emu=True`` is the emulation: the same operations with the kernels' documented fp32 roundings.  LayerNorm: per-lane partial sums
(two accumulators per lane, even / odd element, over the row's 256-column chunks), a pairwise tree over the 64 lanes, mean times
fp32(1/H), centred variance by fma, rsqrt of (variance + eps), xhat by fma, fma forms of the outputs, bf16 stores (RNE), and the
gamma / beta / bias sums per wave over its rows, per workgroup over its waves, then the reduce's slices added onto the gradient.
Cross-entropy: max, __expf as exp2(x * fp32(log2 e)) summed per thread over its 8-column chunks, a lane tree, the four waves in
order, __logf as log2 * fp32(ln 2), loss terms added in row order.  It exists only to calibrate the bounds below on the CPU, and
it takes value-only mutations (``Mutation``) that the CPU test uses to show the bounds are tight.

``check(got, ref)`` asserts, for every compared element,

    elementwise   |got - ref| <= C_OUT * u_out * |ref| + C_ACC * 2^-24 * acc + extra
    normwise      ||got - ref||_G <= (TAU_OUT + C_OUT / sqrt(n_eff)) u_out ||ref||_G + TAU_ACC * 2^-24 ||acc||_G + ||extra||_G

over groups G (a row of a matrix output, the whole of a vector output), n_eff = ||ref||_G^2 / max|ref|_G^2 as in gemm_ref, and
u_out = 2^-8 (bf16) or 2^-23 (fp32).  Where ``exact`` is set the output must equal it.  The ``acc`` models, with the mean's error
bound E_m = C_ACC 2^-24 acc_mean:

    mean    acc = 2 mean|x| + |mu|
    rstd    acc = rstd (4 + 6 var / (var + eps)),  extra = rstd E_m^2 / (var + eps)   (a centring off by E_m adds E_m^2 to var)
    y       acc = keep dscale (|gamma| (4 |xhat| + rstd acc_mean + |xhat| acc_rstd / rstd) + |beta|)
    dx      acc = rstd (4 |g gamma| + 4 mean|g gamma| + a_xh |m2| + |xhat| mean(|g gamma| a_xh)),  a_xh = |xhat| + |mean| rstd
    sums    acc = 4 sum_i |term_i| + adds |out0|      (dgamma: term = g a_xh; dbeta: g; dbias2: dx2, plus sum_i acc_dx2)
    lse     acc = 2 |lse| + 12 + 4 sum_c p_c |x_c - max|
    loss    acc = sum_i acc_lse_i / count + 8 sqrt(count) |loss|
    dlogits acc = |gscale / count| (p (|x - lse| + |lse| + 14) + [c = label])

Calibration (tests/test_rowwise_reference_cpu.py; every case there): LayerNorm at H = 64, 128, 200, 256, 768, 1024, eps 1e-12
and 1e-5, on the realistic and the mixed inputs (rows with a mean of 64 sigma, constant rows, tiny-variance rows, rows scaled by
2^+-20, one outlier), every backward form, 5000 rows over three backward trips; cross-entropy at V = 30 522 / ldv = 30 592 and
V = 1000 on scaled, peaked, uniform and mixed rows, bf16 pads above the row max, dense and compact.  Largest ratios the emulation
reached, and the MI355X over tests/test_rowwise_gpu.py (elementwise / normwise), with

    C_OUT = 2, C_ACC = 1, TAU_OUT = 0.8, TAU_ACC = 0.25

    output     emulation      MI355X            output     emulation      MI355X
    y          0.50  0.47     0.50  0.49        loss       0.05  0.11     0.19  0.43
    mean       0.19  0.07     0.19  0.09        row_lse    0.18  0.16     0.66  0.11
    rstd       0.18  0.16     0.25  0.22        dlogits    0.50  0.27     0.50  0.31
    dx, dx2    0.50  0.47     0.50  0.48
    dgamma     0.19  0.17     0.31  0.44
    dbeta      0.17  0.14     0.11  0.11
    dbias2     0.10  0.09     0.22  0.21

Two things the emulation forced, and one the hardware did.  A bf16 output rounds by up to 2^-8 of its value, so C_OUT is 2 for
a ratio of 0.5, as in gemm_ref.  A constant row's mean may be off by an fp32 ulp (sum * fp32(1/H)), which at eps = 1e-12 makes xhat
as large as rstd ulp(mu): the y bound carries rstd acc_mean and the rstd bound the E_m^2 / (var + eps) term.  (The fp32 outputs
(mean, rstd, the gradient sums, row_lse, the losses) carry the tight checks: an unbiased variance moves y by 0.17 bf16 ulp at
H = 768 but rstd by ~2600 fp32 ulps.)  On the MI355X, v_exp_f32 / v_log_f32 and the atomics' arrival order cost more than the
emulation's correctly rounded exp2 / log2 and row-order sums (row_lse 0.87, the losses' and dgamma's normwise 0.79 / 0.87 under
half the constants above): the lse, loss and sum models are twice what the emulation alone needs.

The smallest margin of a mutation is recorded in the CPU test's docstring.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

from tests.gemm_ref import Canary, NAN_BF16, NAN_F32, _bf, _c32, _f32  # noqa: F401  (re-exported for the tests)

C_OUT, C_ACC = 2.0, 1.0
TAU_OUT, TAU_ACC = 0.8, 0.25
U_BF16, U_F32 = 2.0 ** -8, 2.0 ** -23
EPS24 = 2.0 ** -24

LN_MAXV = 4                  # csrc/common.h: 4 chunks x 256 columns
CE_MAXC = 16                 # csrc/rowwise.hip: register chunks of ce_row_kernel (16 x 256 threads x 8 columns)
IGNORE = -100


# ------------------------------------------------------------------------------------------------ launch geometry (csrc/layernorm.hip, csrc/rowwise.hip)
def grid_for(work, per_block, cap):
    return max(1, min(cap, (work + per_block - 1) // per_block))


def ln_lean(H):
    return H % 256 == 0 and H <= LN_MAXV * 256


def ln_bwd_geometry(M, H):
    """(workgroups, waves per workgroup) of mmbert_ln_bwd: the lean kernel 8 waves x <= 256 workgroups, the generic one 4 x <= 1024."""
    return (grid_for(M, 8, 256), 8) if ln_lean(H) else (grid_for(M, 4, 1024), 4)


def ln_bwd_block_of_row(M, H):
    """The workgroup that sums row i's gamma / beta / bias terms: row i runs on wave i mod (workgroups x waves)."""
    nb, wpb = ln_bwd_geometry(M, H)
    return (torch.arange(M) % (nb * wpb)) // wpb


def seg_of_rows(M, bounds, nseg):
    """Segment of every row as the kernels find it (rows at or past bounds[s] for s = 1 .. nseg-1 move on)."""
    i = torch.arange(M)
    s = torch.zeros(M, dtype=torch.long)
    for q in range(1, nseg):
        s += (i >= int(bounds[q])).long()
    return s


# ------------------------------------------------------------------------------------------------ mutations
@dataclass
class Mutation:
    """A value-only perturbation of the emulation: ``hooks[stage](x, ctx)`` replaces the value of a stage."""
    name: str
    hooks: dict = field(default_factory=dict)


def _hook(mut, stage, x, **ctx):
    if mut is None or stage not in mut.hooks:
        return x
    return mut.hooks[stage](x, ctx)


def unbiased_variance():
    return Mutation("unbiased variance", {"var_div": lambda d, ctx: ctx["H"] - 1})


def eps_outside_sqrt():
    return Mutation("eps outside the square root", {"eps_outside": lambda x, ctx: True})


def _neighbour_col(v):
    return torch.cat([v[1:], v[-1:]])


def gamma_neighbour():
    return Mutation("gamma from the neighbouring column", {"gamma": lambda g, ctx: _neighbour_col(g)})


def beta_neighbour():
    return Mutation("beta from the neighbouring column", {"beta": lambda b, ctx: _neighbour_col(b)})


def drop_row_plus_one():
    return Mutation("dropout row + 1", {"drop_row": lambda r, ctx: r + 1})


def no_m2_term():
    return Mutation("xhat * mean(g gamma xhat) term dropped", {"m2": lambda m, ctx: torch.zeros_like(m)})


def dbias2_unmasked():
    return Mutation("dbias2 from the unmasked gradient", {"ad": lambda ad, ctx: ctx["o"]})


def dbias2_pair_first():
    """Both elements of a pair take the first one's value in dbias2 (the second still masked by its own keep bit)."""
    def f(ad, ctx):
        o2, keep = ctx["o2"], ctx["keep"]
        first = o2[:, 0::2].repeat_interleave(2, dim=1)[:, :o2.shape[1]]
        return torch.where(keep > 0, first, torch.zeros_like(first))
    return Mutation("dbias2 pair takes its first element", {"ad": f})


def workgroup_partial_missing(block):
    return Mutation(f"workgroup {block}'s partial missing from the reduce", {"wg_total": lambda t, ctx: t if ctx["b"] != block else t * 0})


def lse_over_pad():
    return Mutation("pad columns V..ldv in the LSE", {"lse_cols": lambda V, ctx: ctx["ldv"]})


def label_neighbour(offset):
    what = "column" if offset == 1 else "chunk"
    return Mutation(f"label logit from the neighbouring {what}", {"lab_col": lambda c, ctx: (c + offset).clamp(max=ctx["ldv"] - 1)})


def count_out_of_range_labels():
    return Mutation("labels >= V counted in inv_count", {"count_valid": lambda ok, ctx: ctx["labels"] >= 0})


def count_ignored_labels():
    return Mutation("ignored labels (-100, -1) counted in inv_count", {"count_valid": lambda ok, ctx: ctx["labels"] < ctx["V"]})


def boundary_row_previous_segment():
    def f(seg, ctx):
        b, M = ctx["bounds"], seg.numel()
        seg = seg.clone()
        for q in range(1, ctx["nseg"]):
            if int(b[q]) < M:
                seg[int(b[q])] -= 1
        return seg
    return Mutation("a boundary row in the previous segment", {"seg": f})


def no_minus_one():
    return Mutation("no -1 at the label", {"onehot": lambda x, ctx: 0.0})


def gscale_neighbour():
    return Mutation("the neighbouring segment's gscale", {"gscale": lambda g, ctx: torch.roll(g, -1)})


def compact_lse_of_j():
    return Mutation("compact backward reads row j's LSE", {"lse_row": lambda r, ctx: torch.arange(r.numel()).clamp(max=ctx["M"] - 1)})


# ------------------------------------------------------------------------------------------------ fp32 helpers of the emulation
def _lanes(X, H):
    """[M, H] -> [M, NV, 64, 4] (zero columns past H): lane l holds columns c*256 + 4l .. 4l+3 of chunk c."""
    NV = (H + 255) // 256
    Xp = X.new_zeros(X.shape[0], NV * 256)
    Xp[:, :H] = X
    return Xp.view(X.shape[0], NV, 64, 4)


def _lane_acc(A, B=None):
    """Per lane, two fp32 accumulators (even / odd element) over the chunks and the two pairs, added at the end; with B, fma(A, B, acc)."""
    M, NV = A.shape[0], A.shape[1]
    acc = [A.new_zeros(M, 64), A.new_zeros(M, 64)]
    for c in range(NV):
        for k in range(2):
            for e in range(2):
                t = A[:, c, :, 2 * k + e] if B is None else A[:, c, :, 2 * k + e] * B[:, c, :, 2 * k + e]
                acc[e] = _f32(acc[e] + t)
    return _f32(acc[0] + acc[1])


def _tree(v):
    """Pairwise fp32 tree over the last axis (64 lanes: DPP pairs, quads, half rows, rows, then the row broadcasts)."""
    while v.shape[-1] > 1:
        v = _f32(v[..., 0::2] + v[..., 1::2])
    return v[..., 0]


def _seq(parts, start=None):
    """fp32 sum of parts[0], parts[1], ... in order (onto ``start``)."""
    t = start
    for p in parts:
        t = p if t is None else _f32(t + p)
    return t


# ------------------------------------------------------------------------------------------------ reference objects
@dataclass
class Ref:
    val: torch.Tensor                  # float64 [R, C] or [R]: the exact output (rows in launch order)
    acc: torch.Tensor                  # float64, same shape: fp32 working magnitude (times 2^-24 in the bound)
    extra: torch.Tensor | float        # absolute term
    u_out: float
    rows: torch.Tensor | None = None   # int64 [R]: the output rows the kernel writes, in launch order (None: 0 .. R-1)
    exact: torch.Tensor | None = None  # float64: the bit-exact value (NaN: none)


def _ref(val, acc, extra, u, rows=None, exact=None):
    return Ref(val, acc, extra, u, rows, exact)


def _keep_rows(keep, rows, H, mut=None):
    """keep [site rows, H] (0/1) -> the rows ``rows`` (after the drop-row mutation), as float64."""
    r = _hook(mut, "drop_row", rows)
    return keep.to(torch.float64)[r.clamp(max=keep.shape[0] - 1)]


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def ln_fwd(x, gamma, beta, eps, *, M=None, in_rows=None, out_rows=None, keep=None, dscale=1.0, drop_row0=0, emu=False, mutation=None):
    """mmbert_ln_fwd on CPU tensors: x [*, H] bf16, gamma / beta [H] fp32, keep [site rows, H] 0/1 (the exported mask of the site;
    launch row i uses row i + drop_row0).  Returns {"y": Ref, "mean": Ref, "rstd": Ref} (y rows: ``out_rows`` or 0 .. M-1), or the
    emulated tensors with ``emu``."""
    H = x.shape[1]
    if M is None:
        M = in_rows.numel() if in_rows is not None else x.shape[0]
    src = torch.arange(M) if in_rows is None else in_rows.long()
    X = x.to(torch.float64)[src]
    gam = _hook(mutation, "gamma", gamma.to(torch.float64))
    bet = _hook(mutation, "beta", beta.to(torch.float64))
    e32 = _c32(eps)
    ds = _c32(dscale)
    kp = _keep_rows(keep, torch.arange(M) + drop_row0, H, mutation) if keep is not None else None
    if emu:
        T = _lanes(X, H)
        valid = _lanes(torch.ones(1, H, dtype=torch.float64), H)[0] > 0
        invH = _c32(1.0 / H)
        mean = _f32(_tree(_lane_acc(T)) * invH)
        D = torch.where(valid, _f32(T - mean[:, None, None, None]), torch.zeros_like(T))
        Q = _tree(_lane_acc(D, D))
        div = _hook(mutation, "var_div", H, H=H)
        var = _f32(Q * _c32(1.0 / div))
        if _hook(mutation, "eps_outside", False):
            rstd = _f32(1.0 / _f32(var.sqrt() + e32))
        else:
            rstd = _f32(1.0 / _f32(var + e32).sqrt())
        Dh = D.reshape(M, -1)[:, :H]
        Y = _f32(_f32(Dh * rstd[:, None]) * gam[None, :] + bet[None, :])
        if kp is not None:
            Y = _bf(_f32(Y * ds)) * kp
        else:
            Y = _bf(Y)
        return {"y": Y, "mean": mean, "rstd": rstd}
    mu = X.mean(1)
    d = X - mu[:, None]
    var = (d * d).mean(1)
    rstd = 1.0 / (var + e32).sqrt()
    xh = d * rstd[:, None]
    y = xh * gamma.to(torch.float64)[None, :] + beta.to(torch.float64)[None, :]
    mabs = X.abs().mean(1)
    acc_mean = 2.0 * mabs + mu.abs()
    Em = C_ACC * EPS24 * acc_mean
    r_acc = rstd * (4.0 + 6.0 * var / (var + e32))
    r_extra = rstd * Em * Em / (var + e32)
    g = gamma.to(torch.float64).abs()[None, :]
    acc_y = g * (4.0 * xh.abs() + (rstd * acc_mean)[:, None] + xh.abs() * (r_acc / rstd)[:, None]) + beta.to(torch.float64).abs()[None, :]
    exact = torch.full_like(y, float("nan"))
    if kp is not None:
        y, acc_y = y * kp * ds, acc_y * kp * ds
        exact = torch.where(kp == 0, torch.zeros_like(y), exact)
    return {"y": _ref(y, acc_y, 0.0, U_BF16, None if out_rows is None else out_rows.long(), exact),
            "mean": _ref(mu, acc_mean, 0.0, U_F32),
            "rstd": _ref(rstd, r_acc, r_extra, U_F32)}


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_bwd(dy, x, mean, rstd, gamma, *, M=None, dy_rows=None, x_rows=None, dx_rows=None, drop_rows=None, dy_row_limit=0,
           post_keep=None, post_scale=1.0, pre_keep=None, pre_scale=1.0, dx2=False, dbias2=False, dgamma0=None, dbeta0=None,
           dbias20=None, adds=1, emu=False, mutation=None):
    """mmbert_ln_bwd on CPU tensors: dy [*, H] / x [*, H] bf16, mean / rstd [M] fp32 (the forward's), gamma [H] fp32; keeps [site rows,
    H] 0/1 indexed by the dropout row (``drop_rows`` or i); ``dx2`` / ``dbias2``: the second output / the bias sum are produced;
    dgamma0 / dbeta0 / dbias20: the gradients' values before the call; ``adds``: fp32 additions onto them (the reduce's slices, or 1
    per call in deferred / ordered mode).  Returns {"dx": Ref (rows dx_rows), "dx2", "dgamma", "dbeta", "dbias2"}."""
    H = x.shape[1]
    if M is None:
        M = mean.numel()
    i = torch.arange(M)
    xr = i if x_rows is None else x_rows.long()
    dr = i if dy_rows is None else dy_rows.long()
    has = torch.ones(M, dtype=torch.bool) if dy_row_limit <= 0 else dr < dy_row_limit
    X = x.to(torch.float64)[xr]
    DY = torch.where(has[:, None], dy.to(torch.float64)[dr.clamp(max=dy.shape[0] - 1)], torch.zeros(M, H, dtype=torch.float64))
    m, r = mean.to(torch.float64)[:M], rstd.to(torch.float64)[:M]
    gam = _hook(mutation, "gamma", gamma.to(torch.float64))
    drow = i if drop_rows is None else drop_rows.long()
    pk = _keep_rows(post_keep, drow, H, mutation) if post_keep is not None else None
    qk = _keep_rows(pre_keep, drow, H, mutation) if (pre_keep is not None and dx2) else None
    ps, qs = _c32(post_scale), _c32(pre_scale)
    z = torch.zeros(H, dtype=torch.float64)
    g0, b0, d0 = [(v.to(torch.float64) if v is not None else z) for v in (dgamma0, dbeta0, dbias20)]
    if emu:
        nmr = _f32(-m * r)
        XH = _f32(X * r[:, None] + nmr[:, None])
        DV = DY if pk is None else _f32(DY * pk * ps)
        G = _f32(DV * gam[None, :])
        invH = _c32(1.0 / H)
        m1 = _f32(_tree(_lane_acc(_lanes(G, H))) * invH)
        m2 = _f32(_tree(_lane_acc(_lanes(G, H), _lanes(XH, H))) * invH)
        m2 = _hook(mutation, "m2", m2)
        c1, c2 = _f32(-m1 * r), _f32(-m2 * r)
        O = _f32(XH * c2[:, None] + _f32(G * r[:, None] + c1[:, None]))
        out = {"dx": _bf(O)}
        AD = O
        if dx2:
            if qk is not None:
                O2 = _f32(O * qs)
                out["dx2"] = _bf(O2) * qk
                AD = O2 * qk
                AD = _hook(mutation, "ad", AD, o=O, o2=O2, keep=qk)
            else:
                out["dx2"] = out["dx"]
        nb, wpb = ln_bwd_geometry(M, H)
        stride = nb * wpb

        def colsum(C, fma_with=None, start=z):
            # per wave over its rows (trips), per workgroup over its waves, then 8 reduce slices of the workgroups added onto start
            trips = (M + stride - 1) // stride
            P = C.new_zeros(trips * stride, H)
            P[:M] = C if fma_with is None else C * fma_with
            P = P.view(trips, stride, H)
            w = _seq([P[t] for t in range(trips)])
            wg = _seq([w.view(nb, wpb, H)[:, q] for q in range(wpb)])
            wg = torch.stack([_hook(mutation, "wg_total", wg[b], b=b) for b in range(nb)])
            per = (nb + 7) // 8
            sl = [_seq([wg[b] for b in range(z0 * per, min(nb, (z0 + 1) * per))]) for z0 in range(8) if z0 * per < nb]
            return _seq(sl, start)
        out["dgamma"] = colsum(DV, XH, g0)
        out["dbeta"] = colsum(DV, None, b0)
        if dbias2:
            out["dbias2"] = colsum(AD, None, d0)
        return out
    xh = (X - m[:, None]) * r[:, None]
    g = DY if pk is None else DY * pk * ps
    gg = g * gamma.to(torch.float64)[None, :]
    m1, m2 = gg.mean(1), (gg * xh).mean(1)
    dx = r[:, None] * (gg - m1[:, None] - xh * m2[:, None])
    a_xh = xh.abs() + (m.abs() * r)[:, None]
    acc_dx = r[:, None] * (4.0 * gg.abs() + 4.0 * gg.abs().mean(1, keepdim=True) + a_xh * m2.abs()[:, None]
                           + xh.abs() * (gg.abs() * a_xh).mean(1, keepdim=True))
    nan = torch.where(has[:, None], torch.full_like(dx, float("nan")), torch.zeros_like(dx))     # (a missing dy row: dx = 0 exactly)
    out = {"dx": _ref(dx, acc_dx, 0.0, U_BF16, None if dx_rows is None else dx_rows.long(), nan)}
    d2, acc2 = dx, acc_dx
    if dx2:
        ex2 = nan
        if qk is not None:
            d2, acc2 = dx * qk * qs, acc_dx * qk * qs
            ex2 = torch.where(qk == 0, torch.zeros_like(d2), nan)
        out["dx2"] = _ref(d2, acc2, 0.0, U_BF16, None, ex2)

    def vec(v0, terms, a):
        return _ref(v0 + terms.sum(0), 4.0 * a + adds * v0.abs(), 0.0, U_F32)
    out["dgamma"] = vec(g0, g * xh, (g.abs() * a_xh).sum(0))
    out["dbeta"] = vec(b0, g, g.abs().sum(0))
    if dbias2:
        out["dbias2"] = _ref(d0 + d2.sum(0), 4.0 * d2.abs().sum(0) + acc2.sum(0) + adds * d0.abs(), 0.0, U_F32)
    return out


# ------------------------------------------------------------------------------------------------ cross-entropy
def logits_rows(L, rows):
    """Rows of the logits as float64 after the kernel's load (fp32 logits rounded to bf16)."""
    t = L(rows) if callable(L) else L[rows]
    return t.to(torch.bfloat16).to(torch.float64)


def _lse_emu(Xb, V, lse_cols):
    """ce_row_kernel's forward on rows Xb [R, ldv] (float64 of bf16): max, per-thread __expf sums, lane tree, waves in order, __logf."""
    R, ldv = Xb.shape
    cols = torch.arange(ldv)
    ok = cols < lse_cols
    mx = torch.where(ok[None, :], Xb, torch.full_like(Xb, -math.inf)).max(1).values
    L2E, LN2 = _c32(1.0 / math.log(2.0)), _c32(math.log(2.0))
    e = _f32(torch.exp2(_f32(_f32(Xb - mx[:, None]) * L2E)))
    e = torch.where(ok[None, :], e, torch.zeros_like(e))
    P = e.new_zeros(R, CE_MAXC * 256 * 8)
    P[:, :ldv] = e
    P = P.view(R, CE_MAXC, 256, 8)                                   # [row, register chunk c, thread, r]: column (c*256 + tid)*8 + r
    se = e.new_zeros(R, 256)
    for c in range(CE_MAXC):
        for q in range(8):
            se = _f32(se + P[:, c, :, q])
    w = se.view(R, 4, 64)
    while w.shape[-1] > 1:                                             # xor shuffles 32, 16, ... 1
        h = w.shape[-1] // 2
        w = _f32(w[..., :h] + w[..., h:])
    w = w[..., 0]
    tot = _f32(_f32(_f32(w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])
    return _f32(mx + _f32(_f32(torch.log2(tot)) * LN2))


def ce_fwd(L, labels, V, bounds, nseg, *, chunk=512, emu=False, mutation=None):
    """mmbert_ce_fwd: L = logits [M, ldv] (CPU, bf16 or fp32) or a callable rows -> CPU rows of them (the caller's chunked
    copy); labels [M] int64; bounds [nseg + 1].  The reference reads only labelled rows, ``chunk`` at a time.  Returns {"loss": Ref
    [nseg], "row_lse": Ref [M], "count": int64 [nseg]} (emu: {"loss", "row_lse"} tensors)."""
    M = labels.numel()
    ldv = L.shape[1] if not callable(L) else None
    seg = _hook(mutation, "seg", seg_of_rows(M, bounds, nseg), bounds=bounds, nseg=nseg)
    ok = (labels >= 0) & (labels < V)
    okc = _hook(mutation, "count_valid", ok, labels=labels, V=V)
    count = torch.zeros(nseg, dtype=torch.long).index_add_(0, seg, okc.long())
    inv = 1.0 / count.clamp(min=1).to(torch.float64)
    inv32 = _f32(inv)
    act = torch.nonzero(ok).flatten()
    lse = torch.zeros(M, dtype=torch.float64)
    lse_acc = torch.zeros(M, dtype=torch.float64)
    xlab = torch.zeros(M, dtype=torch.float64)
    for a in range(0, act.numel(), chunk):
        rows = act[a:a + chunk]
        Xb = logits_rows(L, rows)
        ldv = Xb.shape[1]
        lab = labels[rows]
        lc = _hook(mutation, "lab_col", lab, ldv=ldv)
        xlab[rows] = Xb.gather(1, lc[:, None])[:, 0]
        ncols = _hook(mutation, "lse_cols", V, ldv=ldv)
        if emu:
            lse[rows] = _lse_emu(Xb, V, ncols)
            continue
        Xv = Xb[:, :ncols]
        mx = Xv.max(1).values
        z = torch.logsumexp(Xv, 1)
        p = torch.exp(Xv - z[:, None])
        lse[rows] = z
        lse_acc[rows] = 2.0 * z.abs() + 12.0 + 4.0 * (p * (Xv - mx[:, None]).abs()).sum(1)
    if emu:
        terms = torch.where(ok, _f32(_f32(lse - xlab) * inv32[seg]), torch.zeros_like(lse))
        loss = torch.stack([_seq([terms[i] for i in act[seg[act] == s].tolist()], torch.zeros((), dtype=torch.float64))
                            for s in range(nseg)])
        return {"loss": loss, "row_lse": lse}
    terms = torch.where(ok, (lse - xlab) * inv[seg], torch.zeros_like(lse))
    loss = torch.zeros(nseg, dtype=torch.float64).index_add_(0, seg, terms)
    lacc = torch.zeros(nseg, dtype=torch.float64).index_add_(0, seg, lse_acc * inv[seg])
    lacc = lacc + 8.0 * count.to(torch.float64).sqrt() * loss.abs()
    lse_exact = torch.where(ok, torch.full_like(lse, float("nan")), torch.zeros_like(lse))
    return {"loss": _ref(loss, lacc, 0.0, U_F32, None, torch.where(count == 0, torch.zeros_like(loss), torch.full_like(loss, float("nan")))),
            "row_lse": _ref(lse, lse_acc, 0.0, U_F32, None, lse_exact), "count": count, "lse64": lse}


def ce_bwd(L, labels, V, bounds, nseg, gscale, lse32, *, rows=None, chunk=512, count=None, emu=False, mutation=None):
    """mmbert_ce_bwd, evaluated on the labelled rows only.  lse32: the forward's row_lse (fp32, as the kernel reads it); ``rows``: the
    compact form's row list (output row j = row rows[j]).  Yields (out_rows, Ref [n, ldv]) chunks: out_rows are the dlogits rows the
    chunk compares (every other output row must be exactly zero); the emulation yields (out_rows, tensor)."""
    M = labels.numel()
    seg = _hook(mutation, "seg", seg_of_rows(M, bounds, nseg), bounds=bounds, nseg=nseg)
    ok = (labels >= 0) & (labels < V)
    if count is None:
        count = torch.zeros(nseg, dtype=torch.long).index_add_(0, seg, ok.long())
    inv = 1.0 / count.clamp(min=1).to(torch.float64)
    gs = _hook(mutation, "gscale", gscale.to(torch.float64))
    src = torch.arange(M) if rows is None else rows.long()             # output row j reads row src[j]
    lse_src = src if rows is None else _hook(mutation, "lse_row", src, M=M)
    outj = torch.nonzero(ok[src]).flatten()
    for a in range(0, outj.numel(), chunk):
        j = outj[a:a + chunk]
        i = src[j]
        Xb = logits_rows(L, i)
        ldv = Xb.shape[1]
        lab = labels[i]
        col = torch.arange(ldv)
        s = seg[i]
        lz = lse32.to(torch.float64)[lse_src[j]]
        on = (col[None, :] == lab[:, None]).to(torch.float64)
        oh = _hook(mutation, "onehot", 1.0)
        if emu:
            sc = _f32(_f32(inv[s]) * _f32(gs[s]))
            L2E = _c32(1.0 / math.log(2.0))
            pr = _f32(torch.exp2(_f32(_f32(Xb - lz[:, None]) * L2E)))
            pr = torch.where(col[None, :] < V, pr, torch.zeros_like(pr))
            pr = torch.where(on > 0, _f32(pr - oh), pr)
            yield j, _bf(_f32(pr * sc[:, None]))
            continue
        sc = inv[s] * gs[s]
        p = torch.where(col[None, :] < V, torch.exp(Xb - lz[:, None]), torch.zeros_like(Xb))
        val = (p - on) * sc[:, None]
        acc = sc.abs()[:, None] * (p * ((Xb - lz[:, None]).abs() + lz.abs()[:, None] + 14.0) + on)
        exact = torch.where(col[None, :] >= V, torch.zeros_like(val), torch.full_like(val, float("nan")))
        if float(gscale.abs().min()) == 0:
            exact = torch.where((sc == 0)[:, None], torch.zeros_like(val), exact)
        yield j, _ref(val, acc, 0.0, U_BF16, None, exact)


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


def ratios(got, ref: Ref, gathered=False) -> Ratios:
    """The largest elementwise and normwise ratios error / bound (<= 1 passes) and the count of exact-value misses.  ``got``: the
    kernel's whole output (rows picked by ``ref.rows``), or, with ``gathered``, already in the reference's row order."""
    g = got.detach()
    if ref.rows is not None and not gathered:
        g = g[ref.rows.to(g.device)]
    g = g.to(torch.float64).cpu().reshape(ref.val.shape)
    val = ref.val
    vec = val.dim() == 1
    if vec:
        g, val = g[None, :], val[None, :]
    acc = ref.acc[None, :] if vec else ref.acc
    extra = ref.extra
    if torch.is_tensor(extra):
        extra = extra[None, :] if vec else extra[:, None] if extra.dim() == 1 else extra
    err = (g - val).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    bound = C_OUT * ref.u_out * val.abs() + C_ACC * EPS24 * acc + extra
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.nan_to_num(q, nan=math.inf, posinf=math.inf)
    at = int(q.argmax()) if q.numel() else 0
    elem = float(q.max()) if q.numel() else 0.0

    def nrm(x):
        x = x if torch.is_tensor(x) else torch.full_like(val, float(x))
        return (x.expand_as(val) ** 2).sum(1).sqrt()
    en = nrm(torch.where(torch.isinf(err), torch.full_like(err, 1e300), err))
    rn = nrm(val)
    rmax = val.abs().max(1).values
    n_eff = torch.where(rmax > 0, (rn / rmax) ** 2, torch.ones_like(rn))
    nb = (TAU_OUT + C_OUT / n_eff.sqrt()) * ref.u_out * rn + TAU_ACC * EPS24 * nrm(acc) + nrm(extra)
    qn = torch.where(en == 0, torch.zeros_like(en), en / nb)
    norm = float(torch.nan_to_num(qn, nan=math.inf, posinf=math.inf).max()) if qn.numel() else 0.0
    bad = 0
    if ref.exact is not None:
        ex = ref.exact[None, :] if vec else ref.exact
        m = ~torch.isnan(ex)
        bad = int((g[m] != ex[m]).sum())
    C = val.shape[1]
    return Ratios(elem, norm, bad, (at // C, at % C) if not vec else (at,))


def check(got, ref: Ref, what="", gathered=False):
    """Assert ``got`` within the bounds of ``ref``; returns the Ratios."""
    r = ratios(got, ref, gathered)
    assert r.exact_bad == 0, f"{what}: {r.exact_bad} elements differ from their exact value"
    assert r.elem <= 1.0 and r.norm <= 1.0, f"{what}: elementwise ratio {r.elem:.3g} (worst at {r.where}), normwise {r.norm:.3g}"
    return r


def still_canary(t, mask=None, what=""):
    """Every element of ``t`` (where ``mask``, a row mask or an element mask, is True) still holds the canary NaN bit for bit."""
    bits = t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    pat = NAN_BF16 if t.dtype == torch.bfloat16 else NAN_F32
    if mask is not None:
        bits = bits[mask.to(bits.device)]
    n = int((bits != pat).sum())
    assert n == 0, f"{what}: {n} elements the kernel must leave alone were written"


def canary_vec(n, dtype, device, pre=16, post=16, fill=None):
    """A length-n vector inside a canary buffer (``Canary`` flat form)."""
    return Canary(1, n, dtype, device, pre=pre, post=post, flat=True, fill=None if fill is None else fill.reshape(1, n))


# ------------------------------------------------------------------------------------------------ test inputs
LN_DISTS = ("real", "mixed")
ROW_KINDS = ("normal", "offset64", "constant", "tiny", "scaled_up", "scaled_down", "outlier")


def ln_inputs(M, H, dist, seed):
    """x [M, H] bf16, gamma / beta [H] fp32, dy [M, H] bf16 (CPU).  real: per-column offsets of a residual stream (N(0, 0.5) per
    column) plus N(0, 1) rows with row scales in [0.5, 2]; mixed: rows cycling through ROW_KINDS -- normal, a mean of 64 standard
    deviations, constant, tiny variance (sigma 1e-3: var ~ eps 1e-5 matters), scaled by 2^+20 / 2^-20, one outlier of 100 sigma."""
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(M, H, generator=g)
    off = 0.5 * torch.randn(H, generator=g)
    x = off[None, :] + Z * (0.5 + 1.5 * torch.rand(M, 1, generator=g))
    if dist == "mixed":
        x = Z.clone()
        kind = torch.arange(M) % len(ROW_KINDS)
        mu = torch.randn(M, 1, generator=g)
        x = torch.where((kind == 1)[:, None], mu * 64.0 + Z, x)
        x = torch.where((kind == 2)[:, None], mu.expand(M, H), x)
        x = torch.where((kind == 3)[:, None], 0.3 + 1e-3 * Z, x)
        x = torch.where((kind == 4)[:, None], Z * 2.0 ** 20, x)
        x = torch.where((kind == 5)[:, None], Z * 2.0 ** -20, x)
        out = Z.clone()
        out[:, H // 3] = 100.0
        x = torch.where((kind == 6)[:, None], out, x)
    elif dist != "real":
        raise ValueError(dist)
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g)
    beta = 0.1 * torch.randn(H, generator=g)
    dy = torch.randn(M, H, generator=g)
    return x.to(torch.bfloat16), gamma, beta, dy.to(torch.bfloat16)


def ce_labels(M, V, ldv, seed, frac=0.3, edge=True):
    """Labels [M] int64: ``frac`` of the rows labelled uniformly, the rest -100; with ``edge`` the first rows carry labels in the pad
    (V, ldv-1) and -1 (all ignored), then the columns where a chunk or thread walk goes wrong (0, V-1, 8k-1 / 8k, 2048k +- 1)."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, V, (M,), generator=g)
    lab[torch.rand(M, generator=g) >= frac] = IGNORE
    if edge:
        cols = [0, V - 1, 7, 8, 15, 16, 8 * (V // 16) - 1, 8 * (V // 16), 8 * (V // 8) - 1, 8 * (V // 8)]
        cols += [c for k in range(1, V // 2048 + 1) for c in (2048 * k - 1, 2048 * k, 2048 * k + 1)]
        cols = [c for c in cols if 0 <= c < V]
        odd = [V, ldv - 1, -1] if ldv > V else [V, -1]
        e = torch.tensor(odd + cols, dtype=torch.long)[:M]
        lab[:e.numel()] = e
    return lab


def ce_logits(M, V, ldv, seed, kind="scaled", device="cpu", dtype=torch.bfloat16):
    """Logits [M, ldv]: scaled N(0, 3); peaked: the row's label column (computed by the caller) raised later; uniform: all equal
    per row.  Pad columns V..ldv hold a value 4 above the row's max (they must change nothing)."""
    g = torch.Generator(device=device).manual_seed(seed)
    X = torch.randn(M, ldv, generator=g, device=device) * 3.0
    if kind == "uniform":
        X = X[:, :1].expand(M, ldv).clone()
    elif kind == "mixed":
        X[1::3] = X[1::3, :1]
    elif kind != "scaled":
        raise ValueError(kind)
    if ldv > V:
        X[:, V:] = X[:, :V].max(1, keepdim=True).values + 4.0
    return X.to(dtype)


def make_peaked(X, labels, V, rows, height=40.0):
    """Raise the label logit of ``rows`` (labelled ones) far above the rest: p_label ~ 1."""
    r = rows[(labels[rows] >= 0) & (labels[rows] < V)]
    X[r.to(X.device), labels[r].to(X.device)] = (X[r.to(X.device), :V].max(1).values.float() + height).to(X.dtype)
    return X
