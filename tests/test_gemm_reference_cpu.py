"""tests/gemm_ref.py on the CPU: the emulation of the kernels' roundings passes ``check`` with about a factor 2 to spare on every
calibration case, and every value-only mutation of the reference fails it.

Smallest margin (error / bound of the mutated emulation; > 1 fails): 4.8, alpha x (1 + 2^-6) on the plain bf16 product (the
normwise check: a systematic 4 u against TAU_OUT = 0.8 u).  Every other mutation fails by more than 200: a dropped K term of the last
row of a partial tile 555, the last split-K split 260, aux after GELU 226, everything else 1e3 ... 2e6 (elements near zero).

Canary: a store into one padding column, one row after M, or one element beyond a flat W view is seen.
"""
import math

import pytest
import torch

from tests import gemm_ref as G

torch.set_num_threads(min(16, torch.get_num_threads()))

EMU_LIMIT = 0.6            # the emulation's ratios stay below this (about half the bound)

EPILOGUES = ("plain", "bias", "gelu", "bias_resid_drop", "resid", "resid_drop", "gelu_bwd", "f32", "bias_f32")


def _keep(M, N, seed, p=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(M, N, generator=g) >= p).to(torch.uint8)


def nt_kwargs(epi, M, N, seed, alpha=1.0):
    bias, R, U = G.epilogue_inputs(M, N, seed)
    keep = _keep(M, N, seed + 1)
    s = 1.0 / 0.9
    kw = {"plain": {}, "bias": dict(bias=bias), "gelu": dict(bias=bias, gelu=True),
          "bias_resid_drop": dict(bias=bias, resid=R, keep=keep, drop_scale=s), "resid": dict(resid=R),
          "resid_drop": dict(resid=R, keep=keep, drop_scale=s), "gelu_bwd": dict(gelu_u=U), "f32": dict(out_f32=True),
          "bias_f32": dict(bias=bias, out_f32=True)}[epi]
    return dict(kw, alpha=alpha)


def _nt_cases():
    for (M, N, K) in [(130, 136, 64), (200, 264, 192), (257, 256, 768), (96, 128, 3072)]:
        for dist in G.DISTS:
            for epi in EPILOGUES:
                yield f"nt {M}x{N}x{K} {dist} {epi}", (M, N, K, dist, epi)


NT_CASES = list(_nt_cases())


@pytest.mark.parametrize("name,case", NT_CASES, ids=[n for n, _ in NT_CASES])
def test_emulation_passes_nt(name, case):
    M, N, K, dist, epi = case
    A, B = G.operands(M, N, K, dist, seed=M + K)
    kw = nt_kwargs(epi, M, N, seed=7, alpha=0.75 if epi in ("plain", "f32") else 1.0)
    ref = G.nt(A, B, **kw)
    emu = G.nt(A, B, emu=True, **kw)
    for k, r in ref.items():
        q = G.ratios(emu[k], r)
        assert q.exact_bad == 0 and q.elem <= EMU_LIMIT and q.norm <= EMU_LIMIT, (name, k, q)


@pytest.mark.parametrize("M,N,K,resid", [(77, 768, 30592, False), (300, 256, 4096, True), (130, 136, 1024, True)])
def test_emulation_passes_splitk(M, N, K, resid):
    for dist in G.DISTS:
        A, B = G.operands(M, N, K, dist, seed=3)
        R = G.epilogue_inputs(M, N, 4)[1] if resid else None
        q = G.ratios(G.splitk(A, B, resid=R, emu=True)["out"], G.splitk(A, B, resid=R)["out"])
        assert q.exact_bad == 0 and q.elem <= EMU_LIMIT and q.norm <= EMU_LIMIT, (dist, q)


def tn_inputs(M, N, K, dist, seed):
    """Token-major X [M,N], Y [M,K] (the distribution acts on the columns: scaled / zero / offset columns of X against columns of Y
    that sum to ~0 over the tokens), W0 [N,K] and bias0 [N] fp32."""
    A, B = G.operands(N, K, M, dist, seed, wscale=1.0)
    g = torch.Generator().manual_seed(seed + 1)
    return A.t().contiguous(), B.t().contiguous(), torch.randn(N, K, generator=g), torch.randn(N, generator=g)


@pytest.mark.parametrize("M,splits", [(33, 1), (1700, 1), (1700, 3), (4129, 2), (4129, 8)])
@pytest.mark.parametrize("dist", G.DISTS)
def test_emulation_passes_tn(M, splits, dist):
    N, K = 264, 136
    X, Y, W0, b0 = tn_inputs(M, N, K, dist, seed=M)
    for acc in (True, False):
        kw = dict(W0=W0, bias0=b0, with_bias=True, alpha=0.5, alpha_dev=torch.tensor(1.5), accumulate=acc)
        ref = G.tn(X, Y, splits=splits, **kw)
        emu = G.tn(X, Y, splits=splits, emu=True, **kw)
        for k in ("W", "bias"):
            q = G.ratios(emu[k], ref[k])
            assert q.exact_bad == 0 and q.elem <= EMU_LIMIT and q.norm <= EMU_LIMIT, (k, acc, q)


def test_emulation_passes_colsum():
    for dist in G.DISTS:
        X = G.operands(776, 8, 1234, dist, 5)[0].t().contiguous()
        out0 = torch.randn(776)
        adds = (1234 + 31) // 32
        q = G.ratios(G.colsum(X, out0, alpha=2.0, adds=adds, emu=True)["out"], G.colsum(X, out0, alpha=2.0, adds=adds)["out"])
        assert q.exact_bad == 0 and q.elem <= EMU_LIMIT and q.norm <= EMU_LIMIT, (dist, q)


# ------------------------------------------------------------------------------------------------ mutations
def _margin(emu, ref):
    q = G.ratios(emu, ref)
    return math.inf if q.exact_bad else max(q.elem, q.norm)


def _nt_mutation(mut, epi, M=333, N=520, K=768, dist="real", tile=(224, 256)):
    A, B = G.operands(M, N, K, dist, seed=11)
    kw = nt_kwargs(epi, M, N, seed=12)
    ref = G.nt(A, B, tile=tile, **kw)
    emu = G.nt(A, B, emu=True, mutation=mut, **kw)
    return max(_margin(emu[k], ref[k]) for k in ref)


def mutation_margins():
    """name -> the mutated emulation's largest ratio to the bound."""
    out = {}
    for dist in ("real", "cancel"):
        out[f"one K tile dropped for one row tile ({dist})"] = _nt_mutation(G.drop_k_tile(1, 5, 224), "bias", dist=dist)
        out[f"one K term dropped, last row of a partial tile ({dist})"] = _nt_mutation(G.drop_k_term_last_row(700), "plain", dist=dist)
    for epi in ("plain", "bias", "f32"):
        out[f"alpha x (1 + 2^-6), {epi}"] = _nt_mutation(G.alpha_scale(), epi)
    out["bias one column right in one column tile"] = _nt_mutation(G.bias_shift(2, 256), "bias")
    out["dropout keep index off by one row"] = _nt_mutation(G.keep_row_shift(), "bias_resid_drop")
    out["dropout scale applied to the residual"] = _nt_mutation(G.resid_scaled(), "bias_resid_drop")
    out["GELU' reading U from the next row"] = _nt_mutation(G.gelu_u_neighbour(), "gelu_bwd")
    out["aux stored after the activation"] = _nt_mutation(G.aux_after_activation(), "gelu")
    # TN
    M, N, K, splits = 1700, 264, 136, 3
    X, Y, W0, b0 = tn_inputs(M, N, K, "real", seed=21)
    kw = dict(W0=W0, bias0=b0, with_bias=True, alpha=0.5, accumulate=True)
    ref = G.tn(X, Y, splits=splits, **kw)
    rps = G.tn_rows_per_split(M, splits)
    emu = G.tn(X, Y, splits=splits, emu=True, mutation=G.tn_row_lost_at_split(rps), **kw)
    out["TN: one token row lost at a split boundary"] = max(_margin(emu[k], ref[k]) for k in ref)
    emu = G.tn(X, Y, splits=splits, emu=True, mutation=G.tn_bias_without_alpha(), **kw)
    out["TN: bias column sum without alpha"] = _margin(emu["bias"], ref["bias"])
    # grouped TN, few-row problems behind long ones, per-problem flags
    probs = [tn_inputs(m, n, k, "real", seed=30 + i) for i, (m, n, k) in enumerate([(600, 264, 136), (600, 136, 264), (77, 264, 264)])]
    probs = [(X, Y, W0, b0 if i != 1 else None) for i, (X, Y, W0, b0) in enumerate(probs)]
    flags = [True, False, True]
    ref = G.tn_grouped(probs, flags)
    for p in range(3):
        emu = G.tn_grouped(probs, flags, emu=True, mutation=G.grouped_ignores_accumulate(p))
        out[f"grouped TN: problem {p} ignores its accumulate flag"] = max(_margin(e["W"], r["W"]) for e, r in zip(emu, ref))
    # split-K
    M, N, K = 300, 768, 30592
    A, B = G.operands(M, N, K, "real", seed=41)
    R = G.epilogue_inputs(M, N, 42)[1]
    zs, per = G.splitk_plan(M, N, K)
    assert K // 64 < zs * per, "the last split must be the shorter one"
    out["split-K: the last, shorter split dropped"] = _margin(G.splitk(A, B, resid=R, emu=True, mutation=G.splitk_last_split_dropped(M, N, K))["out"],
                                                          G.splitk(A, B, resid=R)["out"])
    return out


MIN_MARGIN = 4.0


def test_every_mutation_fails_the_check():
    margins = mutation_margins()
    low = {k: v for k, v in margins.items() if not v > MIN_MARGIN}
    assert not low, low


# ------------------------------------------------------------------------------------------------ canaries
@pytest.mark.parametrize("where", ["pad", "post", "pre", "flat_before", "flat_after"])
def test_canary_sees_a_store_out_of_range(where):
    M, N = 37, 20
    if where.startswith("flat"):
        c = G.Canary(M, N, torch.float32, "cpu", pre=64, post=64, flat=True)
        c.view.zero_()
        c.intact("in range")
        c.buf[63 if where == "flat_before" else 64 + M * N] = 0.0
    else:
        c = G.Canary(M, N, torch.bfloat16, "cpu", pre=2, post=3, pad=8)
        c.view.zero_()
        c.intact("in range")
        if where == "pad":
            c.buf[2 + 5, N] = 1.0                  # one padding column of one row
        elif where == "post":
            c.buf[2 + M, 0] = 0.0                  # the first row after M
        else:
            c.buf[1, N - 1] = 0.0
    assert c.damaged() == 1
    with pytest.raises(AssertionError):
        c.intact(where)


def test_check_rejects_a_nan_left_in_the_output():
    """An element the kernel never wrote keeps the canary NaN: the check must fail on it."""
    A, B = G.operands(64, 16, 64, "real", 1)
    ref = G.nt(A, B)["out"]
    got = G.nt(A, B, emu=True)["out"].clone()
    got[63, 15] = float("nan")
    assert G.ratios(got, ref).elem == math.inf
