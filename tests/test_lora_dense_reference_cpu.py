"""Calibrates tests/lora_dense_ref.py on the CPU: the emulation (the dense-seam adapter kernels' documented roundings) against the
float64 reference, and the mutations the bounds must catch.

Calibration: M in {1, 63, 65, 129, 257} x (K, N) in {(64, 64), (64, 256), (256, 64), (128, 512)} with the rank rotating through
{4, 8, 16}, on each input family of lora_ref.DISTS; forward in both modes, ADD with and without dropout (p = 0.1); backward with and without
the gelu' factor.  The emulation's error must stay within HALF of the bound (the margin tests/gemm_ref.py keeps).  The largest ratios are
in lora_dense_ref's docstring.

Mutations (M = 257: three slabs, a partial last 16-row block; (K, N) = (128, 512), and (256, 64) where the mutation needs K > N; r = 4 and
16; realistic inputs; p = 0.1): each must push at least one output past its bound.  Ratios error / bound reached by the mutated emulation
(the smallest over the two ranks; 1 fails; inf: an element the dropout dropped lost its bits):

    the delta is not masked                 y (p = 0.1) inf
    mask indexed by m * ldy + n, ldy = 520  y (p = 0.1) inf
    drop_scale left out                     y (p = 0.1) 12.0
    GELU applied before the delta           y (GELU) 1.8e4
    aux stored after GELU                   aux 126
    gelu' missing from the input gradient   dx (gelu') 3.4e3
    gelu' read from the neighbouring row    dx (gelu') 3.8e3
    s x (1 + 2^-6)                          y 1.91      y (p = 0.1) 2.01   aux 1.91   dx 2.03   dB 7.0e3
    last 16-row block skipped               y 77        y (GELU) 4.6e4     dx 95      dA 1.68   dB 3.0e4
    one fold slab skipped                   dA 27       dB 3.3e5
    accumulate ignored                      dB 2.8e3
    contraction stops at min(K, N), K < N   dx 139      dA 33
    contraction stops at min(K, N), K > N   h 7.1e3     y 96               y (GELU) 101

(Outputs a mutation cannot reach are left out, as in tests/test_lora_reference_cpu.py.)  The smallest margin is the skipped last row block
on dA (1.68: one token of 257 inside the bound on the bf16 rounding of g -- the same mutation misses every other output by one to four
orders of magnitude), then s x (1 + 2^-6) on the bf16 outputs (1.91): 2^-6 of the update against 2^-7 of the value plus the rounding of h.
"""
import math

import pytest
import torch

from tests import lora_dense_ref as DR
from tests import rng_ref as RNG

MS, KNS, RS = (1, 63, 65, 129, 257), ((64, 64), (64, 256), (256, 64), (128, 512)), (4, 8, 16)
P_DROP = 0.1
STREAM = RNG.rng_stream(20260, 9)


def _drop():
    t = RNG.thr16(P_DROP)
    return (STREAM, t, RNG.drop_scale(t))


def _all(inp, s, *, emu, mutation=None, h=None, accumulate=True):
    """Every output of both entry points on one input set: {label: Ref}."""
    x, y, A, B = inp["x"], inp["y"], inp["A"], inp["B"]
    out = {}
    f = DR.fwd(x, y, A, B, s, DR.ADD, emu=emu, mutation=mutation)
    out["h"], out["y_add"] = f["h"], f["y"]
    out["y_drop"] = DR.fwd(x, y, A, B, s, DR.ADD, drop=_drop(), emu=emu, mutation=mutation)["y"]
    f = DR.fwd(x, y, A, B, s, DR.GELU, emu=emu, mutation=mutation)
    out["aux"], out["y_gelu"] = f["aux"], f["y"]
    kw = dict(gA0=inp["gA0"], gB0=inp["gB0"], accumulate=accumulate, emu=emu, mutation=mutation)
    b = DR.bwd(inp["dy"], x, h, A, B, s, dx=inp["dx"], **kw)
    out["dx"], out["dA"], out["dB"] = b["dx"], b["dA"], b["dB"]
    out["dx_gelu"] = DR.bwd(inp["dy"], x, h, A, B, s, dx=inp["dx"], gelu_u=inp["u"], **kw)["dx"]
    return out


def _ratios(inp, s, mutation=None):
    h = DR.forward_h(inp)
    ref = _all(inp, s, emu=False, h=h)
    got = _all(inp, s, emu=True, h=h, mutation=mutation)
    return {k: DR.ratio(got[k].val, ref[k]) for k in ref}


@pytest.mark.parametrize("dist", DR.DISTS)
def test_emulation_stays_within_half_of_the_bound(dist):
    worst, n = {}, 0
    for M in MS:
        for K, N in KNS:
            r = RS[n % 3]
            q = _ratios(DR.inputs(M, K, N, r, dist, 3000 + n), 16.0 / r)
            n += 1
            for k, v in q.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(dist, {k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == {"h", "y_add", "y_drop", "aux", "y_gelu", "dx", "dx_gelu", "dA", "dB"}
    for k, v in worst.items():
        assert v <= 0.5 + 1e-9, f"{dist}: {k} reaches {v:.3f} of its bound"
    assert max(worst.values()) >= 0.05                         # the bound is not vacuous


def test_the_reference_mask_has_the_generators_keep_rate():
    """p = 0.1 on the shapes the tests use: the reference's own keep rate is within five binomial standard deviations of 1 - thr16 / 65536
    (tests/rng_ref.py's generator: independent 16-bit halves) and a mask of all ones or all zeros cannot pass; a dropped element of the
    reference keeps the bits of y and any change there fails the check."""
    s, t, c = _drop()
    assert t == 6554 and abs(c - 1.0 / (1.0 - 6554 / 65536.0)) < 1e-12
    for M, N in ((63, 64), (65, 256), (129, 512), (257, 512), (129, 3072), (129, 768)):
        k = DR.keep_mask(M, N, s, t)
        assert DR.keep_rate_ok(k, t), (M, N, float(k.mean()))
        assert not DR.keep_rate_ok(torch.ones_like(k), t)
    # the pitch enters the index: another pitch is another mask
    assert not torch.equal(DR.keep_mask(65, 64, s, t), DR.keep_mask(65, 64, s, t, pitch=72))
    inp = DR.inputs(65, 64, 64, 8, "real", 5)
    ref = DR.fwd(inp["x"], inp["y"], inp["A"], inp["B"], 2.0, DR.ADD, drop=_drop())["y"]
    y0 = inp["y"].to(torch.float64)
    assert bool(ref.exact.any()) and torch.equal(ref.val[ref.exact], y0[ref.exact])
    got = ref.val.clone()
    m, n = [int(v[0]) for v in torch.nonzero(ref.exact, as_tuple=True)]
    got[m, n] += 2.0 ** -12
    assert DR.ratio(got, ref) == math.inf


def test_zero_b_leaves_the_add_seam_bit_identical():
    """B = 0: the ADD update is fma(s c, 0, float(y)) -- the emulated y equals the input bit for bit, with and without dropout."""
    inp = DR.inputs(65, 64, 256, 8, "real", 9)
    B0 = torch.zeros_like(inp["B"])
    for drop in (None, _drop()):
        y = DR.fwd(inp["x"], inp["y"], inp["A"], B0, 2.0, DR.ADD, drop=drop, emu=True)["y"].val
        assert torch.equal(y, inp["y"].to(torch.float64))


def _mutated(mut, r, K=128, N=512):
    inp = DR.inputs(257, K, N, r, "real", 5151 + r)
    return _ratios(inp, 16.0 / r, mut)


MUTATIONS = {
    "the delta is not masked": (lambda: DR.delta_not_masked(), ("y_drop",)),
    "mask indexed by m * ldy + n": (lambda: DR.mask_by_pitch(512 + 8), ("y_drop",)),
    "drop_scale left out": (lambda: DR.no_drop_scale(), ("y_drop",)),
    "GELU before the delta": (lambda: DR.gelu_before_delta(), ("y_gelu",)),
    "aux stored after GELU": (lambda: DR.aux_after_gelu(), ("aux",)),
    "gelu' missing": (lambda: DR.no_gelu_grad(), ("dx_gelu",)),
    "gelu' from the neighbouring row": (lambda: DR.gelu_grad_neighbour_row(), ("dx_gelu",)),
    "s off by 2^-6": (lambda: DR.scale_off(), ("y_add", "y_drop", "aux", "dx", "dB")),
    "last 16-row block skipped": (lambda: DR.skip_last_row_block(), ("y_add", "y_gelu", "dx", "dA", "dB")),
    "one fold slab skipped": (lambda: DR.skip_fold_slab(1), ("dA", "dB")),
    "accumulate ignored": (lambda: DR.ignore_accumulate(), ("dB",)),
    "contraction stops at min(K, N), K < N": (lambda: DR.contraction_stops_at_min(), ("dx", "dA")),              # (g = dy . B is cut short)
    "contraction stops at min(K, N), K > N": (lambda: DR.contraction_stops_at_min(), ("h", "y_add", "y_gelu"), (256, 64)),   # (h = x . A^T is)
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_each_mutation_fails_the_check(name):
    make, outputs, *shape = MUTATIONS[name]
    shape = shape[0] if shape else (128, 512)
    smallest = {}
    for r in (4, 16):
        clean = _mutated(None, r, *shape)
        assert max(clean.values()) <= 0.5 + 1e-9
        q = _mutated(make(), r, *shape)
        for k in outputs:
            smallest[k] = min(smallest.get(k, math.inf), q[k])
    print(name, {k: float(f"{v:.3g}") for k, v in smallest.items()})
    for k, v in smallest.items():
        assert v > 1.0, f"{name}: {k} stays within its bound ({v:.3g})"


@pytest.mark.parametrize("dist", DR.DISTS)
def test_identity_bound_on_the_cpu(dist):
    """The model test's gradient identity (dB = s dW A^T, dA = s B^T dW with dW = the fp32 weight gradient of the same dy and x) for
    K != N under lora_ref.identity's bound: the emulated adapter gradients against the identity evaluated on the EMULATED weight gradient
    stay within half of the bound."""
    from tests import gemm_ref as G
    worst = 0.0
    for n, (M, K, N, r) in enumerate(((33, 64, 256, 4), (257, 128, 512, 8), (65, 256, 64, 16))):
        inp = DR.inputs(M, K, N, r, dist, 88 + n)
        s = 16.0 / r
        h = DR.forward_h(inp)
        emu = DR.bwd(inp["dy"], inp["x"], h, inp["A"], inp["B"], s, emu=True, accumulate=False)
        dW = G.tn(inp["dy"], inp["x"], accumulate=False, emu=True)
        dW = dW[0] if isinstance(dW, (tuple, list)) else (dW["W"] if isinstance(dW, dict) else dW)
        ref = DR.identity(dW, inp["A"], inp["B"], inp["dy"], inp["x"], h, s)
        worst = max(worst, DR.ratio(emu["dA"].val, ref["dA"]), DR.ratio(emu["dB"].val, ref["dB"]))
    print("identity", dist, round(worst, 3))
    assert worst <= 0.5
