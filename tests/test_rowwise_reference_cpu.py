"""tests/rowwise_ref.py on the CPU: the emulation of the LayerNorm and cross-entropy kernels' fp32 roundings passes ``check`` with
about a factor 2 to spare on every calibration case, and every value-only mutation of the emulation fails it.

Largest emulation ratio over every case: 0.50 (bf16 outputs y, dx, dx2, dlogits: the half-ulp rounding of the store); every fp32
output stays at or below 0.19 (the table in tests/rowwise_ref.py).

Smallest margin of a mutation (error / bound of the mutated emulation; > 1 fails): 128, the missing -1 at the label (a peaked row's
label gradient is (p - 1) scale ~ 0: the mutant's p scale is 128 bounds away).  Next: the neighbouring segment's gscale 386, an
unbiased variance 781 (rstd), then 1e4 ... 1e9 (gamma / beta / label from the neighbouring column or chunk, a lost workgroup
partial, the m2 term, dbias2 unmasked or from the pair's first element, the boundary row, counted ignored or >= V labels, pad
columns in the LSE, the compact form's LSE row, eps outside the square root); a dropout row off by one fails the exact zeros.
"""
import math

import pytest
import torch

from tests import rowwise_ref as R

torch.set_num_threads(min(16, torch.get_num_threads()))

EMU_LIMIT = 0.6            # the emulation's ratios stay below this (about half the bound)
MIN_MARGIN = 3.0
V, LDV = 30522, 30592      # the model's vocabulary and its padded row (vpad)


def _keep(rows, H, seed, p=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(rows, H, generator=g) >= p).to(torch.uint8)


def _scale(p=0.1):
    thr = int(p * 65536 + 0.5)
    return 1.0 / (1.0 - thr / 65536.0)


def _worst(emu, ref, keys=None):
    out = {}
    for k in keys or ref:
        if k in ref and k in emu and isinstance(ref[k], R.Ref):
            out[k] = R.ratios(emu[k], ref[k], gathered=True)
    return out


def _assert_emu(qs, name):
    for k, q in qs.items():
        assert q.exact_bad == 0 and q.elem <= EMU_LIMIT and q.norm <= EMU_LIMIT, (name, k, q)


# ------------------------------------------------------------------------------------------------ LayerNorm
FWD_CASES = [(H, eps, dist, drop) for H in (64, 128, 200, 256, 768, 1024) for eps in (1e-12, 1e-5) for dist in R.LN_DISTS
             for drop in (False, True)]


@pytest.mark.parametrize("H,eps,dist,drop", FWD_CASES)
def test_emulation_passes_ln_fwd(H, eps, dist, drop):
    M = 140
    x, gamma, beta, _ = R.ln_inputs(M, H, dist, seed=H)
    kw = dict(keep=_keep(M + 5, H, 3), dscale=_scale(), drop_row0=5) if drop else {}
    ref = R.ln_fwd(x, gamma, beta, eps, **kw)
    emu = R.ln_fwd(x, gamma, beta, eps, emu=True, **kw)
    _assert_emu(_worst(emu, ref), (H, eps, dist, drop))


BWD_FORMS = {"FFF": (False, False, False, False), "TFF": (True, False, False, False), "FTT": (False, True, True, True),
             "FTF": (False, True, False, True), "TTT": (True, True, True, True), "dbias2 without dx2": (False, False, False, True)}


def bwd_case(M, H, eps, dist, form, seed=1, mutation=None, maps=False):
    post, dx2, pre, dbias2 = BWD_FORMS[form]
    x, gamma, beta, dy = R.ln_inputs(M, H, dist, seed=seed)
    f = R.ln_fwd(x, gamma, beta, eps, emu=True)
    mean, rstd = f["mean"].float(), f["rstd"].float()
    g = torch.Generator().manual_seed(seed + 1)
    kw = dict(dx2=dx2, dbias2=dbias2, dgamma0=torch.randn(H, generator=g), dbeta0=torch.randn(H, generator=g),
              dbias20=torch.randn(H, generator=g), adds=8)
    if post:
        kw.update(post_keep=_keep(M + 3, H, 5), post_scale=_scale())
    if pre:
        kw.update(pre_keep=_keep(M + 3, H, 6), pre_scale=_scale())
    if maps:
        kw.update(dy_rows=torch.randperm(M, generator=g), drop_rows=torch.randperm(M, generator=g) + 3, dy_row_limit=M - M // 5)
    ref = R.ln_bwd(dy, x, mean, rstd, gamma, **kw)
    emu = R.ln_bwd(dy, x, mean, rstd, gamma, emu=True, mutation=mutation, **kw)
    return emu, ref


@pytest.mark.parametrize("form", list(BWD_FORMS))
@pytest.mark.parametrize("H,eps,dist", [(64, 1e-5, "mixed"), (200, 1e-12, "real"), (256, 1e-5, "mixed"), (768, 1e-12, "mixed"),
                                        (768, 1e-5, "real"), (1024, 1e-12, "real")])
def test_emulation_passes_ln_bwd(form, H, eps, dist):
    emu, ref = bwd_case(140, H, eps, dist, form, maps=form == "TFF")
    _assert_emu(_worst(emu, ref), (form, H, eps, dist))


def test_emulation_passes_ln_bwd_over_several_trips():
    """5000 rows at H = 256: 3 trips per wave of the lean backward, 256 workgroups in 8 reduce slices."""
    emu, ref = bwd_case(5000, 256, 1e-12, "real", "TTT")
    _assert_emu(_worst(emu, ref), "5000 rows")


# ------------------------------------------------------------------------------------------------ cross-entropy
def ce_case(M, V_, ldv, kind, nseg, seed, mutation=None, rows=False, gscale=None):
    lab = R.ce_labels(M, V_, ldv, seed, frac=0.6)
    X = R.ce_logits(M, V_, ldv, seed, kind="scaled" if kind == "peaked" else kind)
    if kind == "peaked":
        X = R.make_peaked(X, lab, V_, torch.arange(0, M, 2))
    bounds = torch.tensor([0] + [M * (s + 1) // nseg for s in range(nseg)], dtype=torch.int32)
    gs = gscale if gscale is not None else torch.tensor([0.5, 2.0, -1.25, 0.75])[:nseg]
    ref = R.ce_fwd(X, lab, V_, bounds, nseg)
    emu = R.ce_fwd(X, lab, V_, bounds, nseg, emu=True, mutation=mutation)
    qs = _worst(emu, ref, ["loss", "row_lse"])
    lse32 = emu["row_lse"].float()
    rl = torch.nonzero((lab >= 0) & (lab < V_)).flatten().int() if rows else None
    if rows:
        rl = torch.cat([rl, torch.tensor([1], dtype=torch.int32)])        # (an unlabelled row in the list: zeros)
    worst = R.Ratios(0.0, 0.0, 0, ())
    emu_chunks = R.ce_bwd(X, lab, V_, bounds, nseg, gs, lse32, rows=rl, emu=True, mutation=mutation)
    for (j, r), (je, e) in zip(R.ce_bwd(X, lab, V_, bounds, nseg, gs, lse32, rows=rl), emu_chunks):
        assert torch.equal(j, je)
        q = R.ratios(e, r, gathered=True)
        worst = R.Ratios(max(worst.elem, q.elem), max(worst.norm, q.norm), worst.exact_bad + q.exact_bad, q.where)
    qs["dlogits"] = worst
    return qs


CE_CASES = [(V, LDV, kind, nseg) for kind in ("scaled", "peaked", "uniform", "mixed") for nseg in (1, 3)] + [(1000, 1024, "scaled", 4)]


@pytest.mark.parametrize("V_,ldv,kind,nseg", CE_CASES)
def test_emulation_passes_ce(V_, ldv, kind, nseg):
    _assert_emu(ce_case(48, V_, ldv, kind, nseg, seed=nseg), (V_, kind, nseg))


def test_emulation_passes_ce_compact_rows():
    _assert_emu(ce_case(48, V, LDV, "scaled", 2, seed=9, rows=True), "compact")


# ------------------------------------------------------------------------------------------------ mutations
def _margin(qs):
    return max((math.inf if q.exact_bad else max(q.elem, q.norm)) for q in qs.values())


def _fwd_margin(mut, cases):
    m = math.inf
    for H, eps, dist, drop in cases:
        M = 140
        x, gamma, beta, _ = R.ln_inputs(M, H, dist, seed=H)
        kw = dict(keep=_keep(M + 5, H, 3), dscale=_scale(), drop_row0=5) if drop else {}
        ref = R.ln_fwd(x, gamma, beta, eps, **kw)
        emu = R.ln_fwd(x, gamma, beta, eps, emu=True, mutation=mut, **kw)
        m = min(m, _margin(_worst(emu, ref)))
    return m


def mutation_margins():
    """name -> the mutated emulation's largest ratio to the bound (the smallest over the cases it is tried on)."""
    out = {}
    base = [(H, eps, dist, False) for H in (128, 768) for eps in (1e-12, 1e-5) for dist in R.LN_DISTS]
    out["unbiased variance"] = _fwd_margin(R.unbiased_variance(), base)
    # eps only matters where var is not >> eps: the mixed rows (constant and tiny-variance rows) at eps = 1e-5
    out["eps outside the square root"] = _fwd_margin(R.eps_outside_sqrt(), [(H, 1e-5, "mixed", False) for H in (128, 768)])
    out["gamma from the neighbouring column"] = _fwd_margin(R.gamma_neighbour(), base)
    out["beta from the neighbouring column"] = _fwd_margin(R.beta_neighbour(), base)
    out["forward dropout row + 1"] = _fwd_margin(R.drop_row_plus_one(), [(H, 1e-12, "real", True) for H in (128, 768)])
    for H in (200, 768):
        out[f"backward dropout row + 1 (H {H})"] = _margin(_worst(*bwd_case(140, H, 1e-12, "real", "TTT", mutation=R.drop_row_plus_one())))
        out[f"xhat * mean(g gamma xhat) dropped (H {H})"] = _margin(_worst(*bwd_case(140, H, 1e-12, "real", "FFF", mutation=R.no_m2_term())))
        out[f"gamma from the neighbouring column, backward (H {H})"] = _margin(_worst(*bwd_case(140, H, 1e-12, "real", "FFF",
                                                                                            mutation=R.gamma_neighbour())))
        out[f"dbias2 from the unmasked gradient (H {H})"] = _margin(_worst(*bwd_case(140, H, 1e-12, "real", "FTT", mutation=R.dbias2_unmasked())))
        out[f"dbias2 pair takes its first element (H {H})"] = _margin(_worst(*bwd_case(140, H, 1e-12, "real", "FTT",
                                                                                     mutation=R.dbias2_pair_first())))
    for M, b in ((140, 0), (5000, 255)):
        out[f"one workgroup's partial missing ({M} rows, workgroup {b})"] = _margin(_worst(*bwd_case(M, 256, 1e-12, "real", "FTT",
                                                                                                     mutation=R.workgroup_partial_missing(b))))
    ce = [("pad columns in the LSE", R.lse_over_pad(), {}), ("label logit from the neighbouring column", R.label_neighbour(1), {}),
          ("label logit from the neighbouring chunk", R.label_neighbour(8), {}),
          ("labels >= V counted in inv_count", R.count_out_of_range_labels(), {}),
          ("ignored labels counted in inv_count", R.count_ignored_labels(), {}),
          ("a boundary row in the previous segment", R.boundary_row_previous_segment(), {}),
          ("no -1 at the label", R.no_minus_one(), {}), ("the neighbouring segment's gscale", R.gscale_neighbour(), {}),
          ("compact backward reads row j's LSE", R.compact_lse_of_j(), {"rows": True})]
    for name, mut, kw in ce:
        out[name] = min(_margin(ce_case(48, V, LDV, kind, 3, seed=3, mutation=mut, **kw)) for kind in ("scaled", "peaked"))
    return out


def test_every_mutation_fails_the_check():
    margins = mutation_margins()
    low = {k: v for k, v in margins.items() if not v > MIN_MARGIN}
    assert not low, low


# ------------------------------------------------------------------------------------------------ the check itself
def test_check_rejects_a_nan_left_in_the_output():
    x, gamma, beta, _ = R.ln_inputs(16, 256, "real", 1)
    ref = R.ln_fwd(x, gamma, beta, 1e-12)
    got = R.ln_fwd(x, gamma, beta, 1e-12, emu=True)["y"].clone()
    got[3, 7] = float("nan")
    assert R.ratios(got, ref["y"], gathered=True).elem == math.inf


def test_still_canary_sees_one_store():
    t = torch.full((4, 8), R.NAN_BF16, dtype=torch.int16).view(torch.bfloat16)
    R.still_canary(t)
    t[2, 5] = 0.0
    with pytest.raises(AssertionError):
        R.still_canary(t)
    R.still_canary(t, torch.tensor([True, True, False, True]))
