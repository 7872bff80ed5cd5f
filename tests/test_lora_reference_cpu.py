"""Calibrates tests/lora_ref.py on the CPU: the emulation (the adapter kernels' documented roundings) against the float64 reference, and
the mutations the bounds must catch.

Calibration: every (M, H, r) of M in {1, 63, 65, 257, 1153}, H in {64, 128, 768}, r in {4, 8, 16} on each input family, the target set
rotating through {q}, {q, v}, {q, k, v}; the emulation's error must stay within HALF of the bound (the margin tests/gemm_ref.py keeps).
The largest ratios are in lora_ref's docstring.

Mutations (M = 257: three slabs, a partial last block; H = 128; r = 4 and 16; q + v; realistic inputs): each must push at least one output
past its bound.  Ratios error / bound reached by the mutated emulation (the smallest over the two ranks; 1 fails):

    rank column dropped            qkv 57      dres 22
    s x (1 + 2^-6)                 qkv 1.83    dres 1.36   dB 7.0e3
    q and v adapters swapped       qkv 2.6e2   dres 1.9e2  dA 66
    last partial row block skipped                         dA 3.2     dB 4.5e4
    partial sum left out of fold                           dA 27      dB 2.9e5
    accumulate ignored                                                dB 2.2e3

(Outputs a mutation cannot reach are left out: dA and dB do not read A, dB reads neither adapter matrix -- h is its input --, and an old
gradient of 0.01 hides inside dA's bound on the rounding of g.)  The smallest margin is s x (1 + 2^-6) on the bf16 outputs (1.36): 2^-6 of
the update against 2^-7 of the value plus the bf16 rounding of h / g -- caught where the rank terms of an element share a sign and the
base value is small; on the fp32 dB (no rounded intermediate) the same mutation misses by almost four orders of magnitude.
"""
import math

import pytest
import torch

from tests import lora_ref as LR

MS, HS, RS = (1, 63, 65, 257, 1153), (64, 128, 768), (4, 8, 16)
TSETS = (("query",), ("query", "value"), ("query", "key", "value"))


def _emu_ratios(M, H, r, targets, dist, seed):
    inp = LR.inputs(M, H, r, targets, dist, seed)
    s = 16.0 / r
    out = {}
    ref = LR.fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], targets, s)
    emu = LR.fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], targets, s, emu=True)
    for (k, rf), (_, em) in zip(LR.walk(ref), LR.walk(emu)):
        out[k] = LR.ratio(em.val, rf)
    h = emu["h"].val.to(torch.bfloat16)
    kw = dict(dres=inp["dres"], gA0=inp["gA0"], gB0=inp["gB0"], accumulate=True)
    ref = LR.bwd(inp["dqkv"], inp["x"], h, inp["A"], inp["B"], targets, s, **kw)
    emu = LR.bwd(inp["dqkv"], inp["x"], h, inp["A"], inp["B"], targets, s, emu=True, **kw)
    for (k, rf), (_, em) in zip(LR.walk(ref), LR.walk(emu)):
        k = k.split("[")[0]
        out[k] = max(out.get(k, 0.0), LR.ratio(em.val, rf))
    return out


@pytest.mark.parametrize("dist", LR.DISTS)
def test_emulation_stays_within_half_of_the_bound(dist):
    worst = {}
    n = 0
    for M in MS:
        for H in HS:
            for r in RS:
                if M == 1153 and H == 768 and r != 8:
                    continue                                   # (the largest shape once per family)
                q = _emu_ratios(M, H, r, TSETS[n % 3], dist, 1000 + n)
                n += 1
                for k, v in q.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(dist, {k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == {"qkv", "h", "dres", "dA", "dB"}
    for k, v in worst.items():
        assert v <= 0.5 + 1e-9, f"{dist}: {k} reaches {v:.3f} of its bound"
    assert max(worst.values()) >= 0.05                         # the bound is not vacuous


def test_untargeted_thirds_and_zero_rows_are_exact():
    inp = LR.inputs(65, 64, 8, ("query",), "zeros", 7)
    ref = LR.fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], ("query",), 2.0)["qkv"]
    q0 = inp["qkv"].to(torch.float64)
    assert torch.equal(ref.val[:, 64:], q0[:, 64:]) and float(ref.acc[:, 64:].abs().max()) == 0.0
    assert torch.equal(ref.val[0, :64], q0[0, :64])            # a zero token row leaves its qkv row alone
    got = q0.clone()
    got[3, 70] += 2.0 ** -12
    assert LR.ratio(got, ref) == math.inf                      # any change of an untargeted element fails


def _mutated(mut, r):
    M, H, targets = 257, 128, ("query", "value")
    inp = LR.inputs(M, H, r, targets, "real", 4242 + r)
    s = 16.0 / r
    h = LR.forward_h(inp, targets)
    ref_f = LR.fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], targets, s)
    ref_b = LR.bwd(inp["dqkv"], inp["x"], h, inp["A"], inp["B"], targets, s, dres=inp["dres"], gA0=inp["gA0"], gB0=inp["gB0"])
    mf = LR.fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], targets, s, emu=True, mutation=mut)
    mb = LR.bwd(inp["dqkv"], inp["x"], h, inp["A"], inp["B"], targets, s, dres=inp["dres"], gA0=inp["gA0"], gB0=inp["gB0"], emu=True, mutation=mut)
    out = {}
    for ref, got in ((ref_f, mf), (ref_b, mb)):
        for (k, rf), (_, em) in zip(LR.walk(ref), LR.walk(got)):
            k = k.split("[")[0]
            out[k] = max(out.get(k, 0.0), LR.ratio(em.val, rf))
    return out


MUTATIONS = {
    "rank column dropped": (lambda: LR.drop_rank_column("value", 1), ("qkv", "dres")),
    "s off by 2^-6": (lambda: LR.scale_off(), ("qkv", "dres", "dB")),
    "q and v swapped": (lambda: LR.swap_q_v(), ("qkv", "dres", "dA")),
    "last partial row block skipped": (lambda: LR.skip_last_row_block(), ("dA", "dB")),
    "partial sum left out of the fold": (lambda: LR.skip_fold_slab(1), ("dA", "dB")),
    "accumulate ignored": (lambda: LR.ignore_accumulate(), ("dB",)),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_each_mutation_fails_the_check(name):
    make, outputs = MUTATIONS[name]
    smallest = {}
    for r in (4, 16):
        clean = _mutated(None, r)
        assert max(clean.values()) <= 0.5 + 1e-9
        q = _mutated(make(), r)
        for k in outputs:
            smallest[k] = min(smallest.get(k, math.inf), q[k])
    print(name, {k: float(f"{v:.3g}") for k, v in smallest.items()})
    for k, v in smallest.items():
        assert v > 1.0, f"{name}: {k} stays within its bound ({v:.3g})"


@pytest.mark.parametrize("dist", LR.DISTS)
def test_identity_bound_on_the_cpu(dist):
    """The model test's gradient identity (dB = s dW A^T, dA = s B^T dW with dW = the fp32 weight gradient of the same dqkv and x) under
    lora_ref.identity's bound, calibrated like the kernels': the emulated adapter gradients against the identity evaluated on the EMULATED
    weight gradient (gemm_ref.tn: 32-token blocks into fp32) stay within half of the bound.  Largest ratios: real 0.18, cancel 0.08,
    scaled 0.43, zeros 0.17 (the bound's ``mid`` term counts every token's bf16 rounding with one sign; where one token's power of two
    dominates a sum -- scaled -- there is little to average)."""
    from tests import gemm_ref as G
    worst = 0.0
    for n, (M, H, r) in enumerate(((33, 64, 4), (257, 128, 8), (65, 128, 16), (1153, 64, 8))):
        targets = ("query", "value")
        inp = LR.inputs(M, H, r, targets, dist, 77 + n)
        s = 16.0 / r
        h = LR.forward_h(inp, targets)
        emu = LR.bwd(inp["dqkv"], inp["x"], h, inp["A"], inp["B"], targets, s, emu=True, accumulate=False)
        for ti, t in enumerate(targets):
            k = LR.TARGETS.index(t)
            dq = inp["dqkv"][:, k * H:(k + 1) * H]
            dW = G.tn(dq, inp["x"], accumulate=False, emu=True)
            dW = dW[0] if isinstance(dW, (tuple, list)) else (dW["W"] if isinstance(dW, dict) else dW)
            ref = LR.identity(dW, inp["A"][t], inp["B"][t], dq, inp["x"], h[:, ti * r:(ti + 1) * r], s)
            worst = max(worst, LR.ratio(emu["dA"][t].val, ref["dA"]), LR.ratio(emu["dB"][t].val, ref["dB"]))
    print("identity", dist, round(worst, 3))
    assert worst <= 0.5
