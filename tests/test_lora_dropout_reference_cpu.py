"""Calibrates tests/lora_dropout_ref.py on the CPU: the emulation (the adapter kernels' documented roundings under the dropout of their
input) against the float64 reference, its equality with the two older references at thr16 = 0, and the mutations the bounds
must catch.

Calibration: M in {1, 65, 257}; q / k / v at H in {64, 768}, the dense seams at (K, N) in {(64, 64), (128, 832), (832, 128)} (832 = 768 + 64
crosses the 768-column staging chunk); every shape at p = 0.1, p = 0.5 and thr16 = 1, the rank rotating through {4, 8, 16} and the target
set through lora_ref's three; each input family of lora_ref.DISTS.  The emulation's error must stay within HALF of the bound; the largest
ratios are in lora_dropout_ref's docstring.

Mutations (M = 257, H = 128 for q / k / v and (K, N) = (128, 832) for the dense seam, r = 4 and 16, realistic inputs, p = 0.5 -- and p = 0.1
for the two mutations on c, where c - 1 is smallest): each must push at least one output past its bound.  Ratios error / bound reached by
the mutated emulation (the smallest over the ranks; inf: an element the mask dropped lost its bits, or a kept one kept them):

    mask indexed by the row pitch            qkv: h 1.7e5   dres inf   dA 69.9        dense: h 2.5e5   dx inf   dA 58.8
    mask of row m + 1                        qkv: h 6.6e4   dres inf   dA 66.9        dense: h 1.4e5   dx inf   dA 55.1
    even / odd halves of a pair swapped      qkv: h 2.0e5   dres inf   dA 64.6        dense: h 2.1e5   dx inf   dA 59.6
    c left out of h (p = 0.1)                qkv: h 13.2    qkv 12.0                  dense: h 13.2    y 12.2   aux 12.2
    c left out of g (p = 0.1)                qkv: dres 7.73 dA 4.90                   dense: dx 12.0   dx (gelu') 12.5   dA 3.91
    no mask in dA                            qkv: dA 70.0                             dense: dA 62.7
    no mask in dx                            qkv: dres inf                            dense: dx inf    dx (gelu') inf
    rows ignored (a 257-row gather)                                                   dense: dx inf    dx (gelu') inf    dA 67.3
    a per-target site for q / k / v          qkv: h 1.4e5   qkv 210    dA 59.3

The smallest margin is c left out of g on the dense dA at p = 0.1 (3.91): c - 1 = 0.111 of g against the bound's 2^-7 on the bf16 rounding
of g, summed over tokens whose roundings do not align.

``dropped dx elements rounded instead of kept`` changes no VALUE on finite inputs (bf16 -> fp32 -> bf16 is exact): it is held on the one
thing it changes, the sign of a dropped -0.
"""
import math

import numpy as np
import pytest
import torch

from tests import lora_dense_ref as DR
from tests import lora_dropout_ref as XR
from tests import lora_ref as LR
from tests import rng_ref as RNG

MS, HS, KNS, RS = (1, 65, 257), (64, 768), ((64, 64), (128, 832), (832, 128)), (4, 8, 16)
TSETS = (("query",), ("query", "value"), ("query", "key", "value"))
SEED = 20261021
DROPS = (XR.in_drop(0.1, SEED, 3), XR.in_drop(0.5, SEED, 11), XR.in_drop_thr(1, SEED, 19))
OUT_DROP = XR.in_drop(0.1, SEED, 1)                          # the GEMM's own output mask on the ADD seam


def _qkv_all(inp, targets, s, drop, *, emu, h, mutation=None):
    f = XR.qkv_fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], targets, s, drop, emu=emu, mutation=mutation)
    b = XR.qkv_bwd(inp["dqkv"], inp["x"], h, inp["A"], inp["B"], targets, s, drop, dres=inp["dres"], gA0=inp["gA0"], gB0=inp["gB0"],
                   emu=emu, mutation=mutation)
    out = {"h": f["h"], "qkv": f["qkv"], "dres": b["dres"]}
    for k in ("dA", "dB"):
        for t, r in b[k].items():
            out[f"{k}[{t}]"] = r
    return out


def _qkv_ratios(inp, targets, s, drop, mutation=None):
    h = XR.qkv_fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], targets, 1.0, drop, emu=True)["h"].val.to(torch.bfloat16)
    ref = _qkv_all(inp, targets, s, drop, emu=False, h=h)
    got = _qkv_all(inp, targets, s, drop, emu=True, h=h, mutation=mutation)
    q = {}
    for k in ref:
        kk = k.split("[")[0]
        q[kk] = max(q.get(kk, 0.0), XR.ratio(got[k].val, ref[k]))
    return q


def _dense_all(inp, s, drop, *, emu, h, rows=None, mutation=None):
    x, y, A, B = inp["x"], inp["y"], inp["A"], inp["B"]
    out = {}
    f = XR.dense_fwd(x, y, A, B, s, XR.ADD, in_drop=drop, emu=emu, mutation=mutation)
    out["h"], out["y_add"] = f["h"], f["y"]
    out["y_drop"] = XR.dense_fwd(x, y, A, B, s, XR.ADD, drop=OUT_DROP, in_drop=drop, emu=emu, mutation=mutation)["y"]
    f = XR.dense_fwd(x, y, A, B, s, XR.GELU, in_drop=drop, emu=emu, mutation=mutation)
    out["aux"], out["y_gelu"] = f["aux"], f["y"]
    kw = dict(in_drop=drop, rows=rows, gA0=inp["gA0"], gB0=inp["gB0"], emu=emu, mutation=mutation)
    b = XR.dense_bwd(inp["dy"], x, h, A, B, s, dx=inp["dx"], **kw)
    out["dx"], out["dA"], out["dB"] = b["dx"], b["dA"], b["dB"]
    out["dx_gelu"] = XR.dense_bwd(inp["dy"], x, h, A, B, s, dx=inp["dx"], gelu_u=inp["u"], **kw)["dx"]
    return out


def _dense_ratios(inp, s, drop, rows=None, mutation=None):
    h = XR._dense_h(inp["x"].to(torch.float64), inp["A"].to(torch.float64), drop, rows, True, None, inp["x"].shape[1])[0].to(torch.bfloat16)
    ref = _dense_all(inp, s, drop, emu=False, h=h, rows=rows)
    got = _dense_all(inp, s, drop, emu=True, h=h, rows=rows, mutation=mutation)
    return {k: XR.ratio(got[k].val, ref[k]) for k in ref}


@pytest.mark.parametrize("dist", LR.DISTS)
def test_qkv_emulation_stays_within_half_of_the_bound(dist):
    worst, n = {}, 0
    for M in MS:
        for H in HS:
            for drop in DROPS:
                r, ts = RS[n % 3], TSETS[(n // 3 + n) % 3]
                q = _qkv_ratios(LR.inputs(M, H, r, ts, dist, 4000 + n), ts, 16.0 / r, drop)
                n += 1
                for k, v in q.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print("qkv", dist, {k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == {"h", "qkv", "dres", "dA", "dB"}
    for k, v in worst.items():
        assert v <= 0.5 + 1e-9, f"{dist}: {k} reaches {v:.3f} of its bound"
    assert max(worst.values()) >= 0.05                         # the bound is not vacuous


@pytest.mark.parametrize("dist", LR.DISTS)
def test_dense_emulation_stays_within_half_of_the_bound(dist):
    worst, n = {}, 0
    for M in MS:
        for K, N in KNS:
            for drop in DROPS:
                r = RS[n % 3]
                q = _dense_ratios(DR.inputs(M, K, N, r, dist, 5000 + n), 16.0 / r, drop)
                n += 1
                for k, v in q.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print("dense", dist, {k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == {"h", "y_add", "y_drop", "aux", "y_gelu", "dx", "dx_gelu", "dA", "dB"}
    for k, v in worst.items():
        assert v <= 0.5 + 1e-9, f"{dist}: {k} reaches {v:.3f} of its bound"
    assert max(worst.values()) >= 0.05


def _same(a, b, what):
    for f in ("val", "acc", "mid"):
        assert torch.equal(getattr(a, f), getattr(b, f)), (what, f)


@pytest.mark.parametrize("emu", (False, True))
def test_without_a_mask_the_reference_is_the_older_ones(emu):
    """thr16 = 0 (a None triple, and a triple with a stream and a scale that must not be read): values, acc and mid equal exactly."""
    ts = ("query", "key", "value")
    inp = LR.inputs(65, 64, 8, ts, "real", 77)
    h = LR.forward_h(inp, ts)
    for drop in (None, (12345, 0, 3.0)):
        a = XR.qkv_fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], ts, 2.0, drop, emu=emu)
        b = LR.fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], ts, 2.0, emu=emu)
        _same(a["qkv"], b["qkv"], "qkv"); _same(a["h"], b["h"], "h")
        a = XR.qkv_bwd(inp["dqkv"], inp["x"], h, inp["A"], inp["B"], ts, 2.0, drop, dres=inp["dres"], gA0=inp["gA0"], gB0=inp["gB0"], emu=emu)
        b = LR.bwd(inp["dqkv"], inp["x"], h, inp["A"], inp["B"], ts, 2.0, dres=inp["dres"], gA0=inp["gA0"], gB0=inp["gB0"], emu=emu)
        _same(a["dres"], b["dres"], "dres")
        for t in ts:
            _same(a["dA"][t], b["dA"][t], t); _same(a["dB"][t], b["dB"][t], t)
        assert not bool(a["dres"].exact.any())
    d = DR.inputs(65, 128, 832, 4, "real", 78)
    hd = DR.forward_h(d)
    for drop in (None, (12345, 0, 3.0)):
        for mode, od in ((XR.ADD, None), (XR.ADD, OUT_DROP), (XR.GELU, None)):
            a = XR.dense_fwd(d["x"], d["y"], d["A"], d["B"], 2.0, mode, drop=od, in_drop=drop, emu=emu)
            b = DR.fwd(d["x"], d["y"], d["A"], d["B"], 2.0, mode, drop=od, emu=emu)
            assert set(a) == set(b)
            for k in a:
                _same(a[k], b[k], k)
        for u in (None, d["u"]):
            a = XR.dense_bwd(d["dy"], d["x"], hd, d["A"], d["B"], 2.0, in_drop=drop, rows=list(range(64, -1, -1)), dx=d["dx"], gelu_u=u,
                             gA0=d["gA0"], gB0=d["gB0"], emu=emu)
            b = DR.bwd(d["dy"], d["x"], hd, d["A"], d["B"], 2.0, dx=d["dx"], gelu_u=u, gA0=d["gA0"], gB0=d["gB0"], emu=emu)
            for k in b:
                _same(a[k], b[k], k)


def test_the_mask_is_the_generators():
    """Kp is rng_ref.keep_at on row(m) * K + k: the keep rate of p = 0.1 / 0.5 within five binomial standard deviations, thr16 = 1 drops
    almost nothing, a row list moves rows of the mask, the 64-bit index of row 2^24 + 5 at K = 832 is past 2^33 and its pair counter wraps
    mod 2^32, and a dropped NaN does not travel."""
    for drop, p in zip(DROPS[:2], (0.1, 0.5)):
        k = XR.keep_matrix(257, 768, drop)
        assert DR.keep_rate_ok(k, drop[1]) and abs(drop[1] / 65536 - p) < 1e-4
    assert float(XR.keep_matrix(257, 768, DROPS[2]).mean()) > 0.999
    drop = DROPS[1]
    full = XR.keep_matrix(300, 832, drop)
    rows = [299, 0, 17, 3, 250]
    assert torch.equal(XR.keep_matrix(5, 832, drop, rows), full[rows])
    big = 2 ** 24 + 5
    assert big * 832 > 2 ** 33
    k = XR.keep_matrix(1, 832, drop, [big])[0]
    idx = np.uint64(big * 832) + np.arange(832, dtype=np.uint64)
    pair = (idx >> np.uint64(1)) & np.uint64(0xFFFFFFFF)                  # the wrapped counter
    want = RNG.keep_at(drop[0], pair * np.uint64(2) + (idx & np.uint64(1)), drop[1])
    assert np.array_equal(k.numpy().astype(np.uint8), want) and 0 < int(want.sum()) < 832
    d = DR.inputs(65, 64, 64, 8, "real", 9)
    Kp = XR.keep_matrix(65, 64, drop)
    x = d["x"].clone()
    x[Kp == 0] = float("nan")
    for emu in (False, True):
        f = XR.dense_fwd(x, d["y"], d["A"], d["B"], 2.0, in_drop=drop, emu=emu)
        assert not bool(torch.isnan(f["h"].val).any()) and not bool(torch.isnan(f["y"].val).any())


# ------------------------------------------------------------------------------------------------ mutations
M_MUT, H_MUT, KN_MUT = 257, 128, (128, 832)
ROWS_MUT = [(7 * i + 3) % 300 for i in range(M_MUT)]          # a non-monotonic gather from a 300-row site


def _qkv_mut(mut, r, drop):
    ts = ("query", "key", "value")
    return _qkv_ratios(LR.inputs(M_MUT, H_MUT, r, ts, "real", 6100 + r), ts, 16.0 / r, drop, mut)


def _dense_mut(mut, r, drop, rows=None):
    return _dense_ratios(DR.inputs(M_MUT, *KN_MUT, r, "real", 6200 + r), 16.0 / r, drop, rows, mut)


P5, P1 = DROPS[1], DROPS[0]
# name -> (mutation, {"qkv": outputs, "dense": outputs}, the triple, with the row list)
MUTATIONS = {
    "mask indexed by the row pitch": (lambda: XR.mask_by_pitch(KN_MUT[0] + 64), {"qkv": ("h", "dres", "dA"), "dense": ("h", "dx", "dA")}, P5, False),
    "mask of row m + 1": (lambda: XR.mask_of_next_row(), {"qkv": ("h", "dres", "dA"), "dense": ("h", "dx", "dA")}, P5, False),
    "halves of a pair swapped": (lambda: XR.halves_swapped(), {"qkv": ("h", "dres", "dA"), "dense": ("h", "dx", "dA")}, P5, False),
    "c left out of h": (lambda: XR.c_left_out_of_h(), {"qkv": ("h", "qkv"), "dense": ("h", "y_add", "aux")}, P1, False),
    "c left out of g": (lambda: XR.c_left_out_of_g(), {"qkv": ("dres", "dA"), "dense": ("dx", "dx_gelu", "dA")}, P1, False),
    "no mask in dA": (lambda: XR.no_mask_in_dA(), {"qkv": ("dA",), "dense": ("dA",)}, P5, False),
    "no mask in dx": (lambda: XR.no_mask_in_dx(), {"qkv": ("dres",), "dense": ("dx", "dx_gelu")}, P5, False),
    "rows ignored": (lambda: XR.rows_ignored(), {"dense": ("dx", "dx_gelu", "dA")}, P5, True),      # (forward takes no row list: h is not reached)
    "a per-target site for q / k / v": (lambda: XR.per_target_site(SEED), {"qkv": ("h", "qkv", "dA")}, P5, False),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_each_mutation_fails_the_check(name):
    make, outputs, drop, with_rows = MUTATIONS[name]
    smallest = {}
    for r in (4, 16):
        for fam, run in (("qkv", lambda m: _qkv_mut(m, r, drop)), ("dense", lambda m: _dense_mut(m, r, drop, ROWS_MUT if with_rows else None))):
            if fam not in outputs:
                continue
            clean = run(None)
            assert max(clean.values()) <= 0.5 + 1e-9
            q = run(make())
            for k in outputs[fam]:
                smallest[f"{fam}: {k}"] = min(smallest.get(f"{fam}: {k}", math.inf), q[k])
    print(name, {k: float(f"{v:.3g}") for k, v in smallest.items()})
    for k, v in smallest.items():
        assert v > 1.0, f"{name}: {k} stays within its bound ({v:.3g})"


def test_a_dropped_dx_element_keeps_its_bits():
    """The dropped elements of dx / dres are ``exact``: any change of value there fails; the rounded form, bf16(fma(s, 0, old)), turns a
    dropped -0 into +0 where the reference keeps the sign."""
    drop = P5
    d = DR.inputs(65, 64, 64, 8, "real", 12)
    Kp = XR.keep_matrix(65, 64, drop)
    dx = d["dx"].clone()
    dx[Kp == 0] = -0.0
    h = XR._dense_h(d["x"].to(torch.float64), d["A"].to(torch.float64), drop, None, True, None, 64)[0].to(torch.bfloat16)
    ref = XR.dense_bwd(d["dy"], d["x"], h, d["A"], d["B"], 2.0, in_drop=drop, dx=dx, emu=True)["dx"]
    mut = XR.dense_bwd(d["dy"], d["x"], h, d["A"], d["B"], 2.0, in_drop=drop, dx=dx, emu=True, mutation=XR.dropped_dx_rounded())["dx"]
    dropped = Kp == 0
    assert bool(dropped.any()) and torch.equal(ref.exact, dropped)
    assert bool(torch.signbit(ref.val[dropped]).all()) and not bool(torch.signbit(mut.val[dropped]).any())
    got = ref.val.clone()
    m, n = [int(v[0]) for v in torch.nonzero(dropped, as_tuple=True)]
    got[m, n] = 2.0 ** -20
    assert XR.ratio(got, ref) == math.inf
    ts = ("query", "value")
    q = LR.inputs(65, 64, 4, ts, "real", 13)
    dres = q["dres"].clone()
    Kq = XR.keep_matrix(65, 64, drop)
    dres[Kq == 0] = -0.0
    hq = XR.qkv_fwd(q["x"], q["qkv"], q["A"], q["B"], ts, 1.0, drop, emu=True)["h"].val.to(torch.bfloat16)
    ref = XR.qkv_bwd(q["dqkv"], q["x"], hq, q["A"], q["B"], ts, 2.0, drop, dres=dres, emu=True)["dres"]
    mut = XR.qkv_bwd(q["dqkv"], q["x"], hq, q["A"], q["B"], ts, 2.0, drop, dres=dres, emu=True, mutation=XR.dropped_dx_rounded())["dres"]
    assert bool(torch.signbit(ref.val[Kq == 0]).all()) and not bool(torch.signbit(mut.val[Kq == 0]).any())
