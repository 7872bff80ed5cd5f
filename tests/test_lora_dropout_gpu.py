"""The four *_drop entry points of csrc/lora.hip (the adapter kernels under the dropout of their input) through the C ABI against
tests/lora_dropout_ref.py: float64 values under a mask rebuilt by tests/rng_ref.py, the calibrated bounds (C_OUT = 2, C_ACC = 0.75,
C_MID = 4 and the GELU terms), NaN canaries around every output and behind the workspace.

Shapes: M in {1, 65, 257} (one lane row; one row past a 64-row workgroup; three 128-token slabs with a one-row tail); q / k / v at H in
{64, 768} with rank, target set, input family and p in {0.1, 0.5} rotating; the dense seams at (K, N) in {(64, 64), (128, 832), (832, 128)}
(832 = 768 + 64 crosses the 768-column staging chunk on either side), both modes, with and without the GEMM's own output mask; thr16 = 1
once per entry point.  x, dy, dx and u are column windows of wider matrices (pitch = width + 64): the mask index must use the logical
width.  The gathered-rows case draws 70 rows in non-monotonic order from a 300-row site plus the row id 2^24 + 5 at K = 832, whose element
index is past 2^33 (the pair counter wraps mod 2^32 as rng_ref.keep_at defines it)."""
import ctypes

import pytest
import torch

from tests import gemm_ref as G
from tests import lora_dense_ref as DR
from tests import lora_dropout_ref as XR
from tests import lora_ref as LR

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 991
MS, HS, KNS, RS = (1, 65, 257), (64, 768), ((64, 64), (128, 832), (832, 128)), (4, 8, 16)
TSETS = (("query",), ("query", "value"), ("query", "key", "value"))
PS = (0.1, 0.5)
QKV_CASES = [(M, H, RS[(i + j) % 3], TSETS[(i + 2 * j) % 3], LR.DISTS[(i + j) % 4], PS[(i + j) % 2]) for i, M in enumerate(MS) for j, H in enumerate(HS)]
DENSE_CASES = [(M, K, N, RS[(i + j) % 3], LR.DISTS[(i + j + 1) % 4], PS[(i + j + 1) % 2]) for i, M in enumerate(MS) for j, (K, N) in enumerate(KNS)]
P3 = ctypes.c_void_p * 3


def _drop(p, site, thr1=False):
    return XR.in_drop_thr(1, SEED, site) if thr1 else XR.in_drop(p, SEED, site)


def _mask(targets):
    return sum(1 << LR.TARGETS.index(t) for t in targets)


def _ptrs(d, targets):
    return P3(*[(d[t].data_ptr() if (d is not None and t in targets and d.get(t) is not None) else None) for t in LR.TARGETS])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _window(t, pad=64, fill=1e30):
    """t [M, N] as a column window of a wider matrix (row pitch N + pad) whose other columns hold ``fill``."""
    M, N = t.shape
    wide = torch.full((max(M, 1), N + pad), fill, dtype=t.dtype, device=DEV)
    wide[:M, 8:8 + N] = t.to(DEV)
    return wide[:M, 8:8 + N]


def _lib():
    from msa_amd import _lib as L
    return L, L.load()


# ------------------------------------------------------------------------------------------------ q / k / v
class _Qkv:
    def __init__(self, M, H, r, targets, dist, seed=0):
        self.M, self.H, self.r, self.targets = M, H, r, targets
        self.names = [t for t in LR.TARGETS if t in targets]
        self.nt, self.s = len(self.names), 16.0 / r
        self.inp = inp = LR.inputs(M, H, r, targets, dist, seed)
        self.x, self.dqkv, self.dres = _window(inp["x"]), _window(inp["dqkv"]), _window(inp["dres"])
        self.A = {t: inp["A"][t].to(DEV) for t in self.names}
        self.B = {t: inp["B"][t].to(DEV) for t in self.names}

    def fwd(self, drop, old=False):
        """(qkv canary, h canary); ``old``: through the entry point without _drop."""
        L, lib = _lib()
        M, H, r = self.M, self.H, self.r
        qkv = G.Canary(M, 3 * H, torch.bfloat16, DEV, pre=2, post=3, pad=8, fill=self.inp["qkv"].to(DEV))
        h = G.Canary(M, self.nt * r, torch.bfloat16, DEV, pre=1, post=2, pad=4)
        args = (_stream(), self.x.data_ptr(), self.x.stride(0), qkv.view.data_ptr(), qkv.view.stride(0), M, H, r, _mask(self.targets),
                _ptrs(self.A, self.names), _ptrs(self.B, self.names), self.s, h.view.data_ptr(), h.view.stride(0))
        if old:
            L.check(lib.mmbert_lora_qkv_fwd(*args), "mmbert_lora_qkv_fwd")
        else:
            L.check(lib.mmbert_lora_qkv_fwd_drop(*args, *drop), "mmbert_lora_qkv_fwd_drop")
        return qkv, h

    def bwd(self, h, drop, *, with_dres=True, accumulate=True, which=None, old=False):
        L, lib = _lib()
        M, H, r = self.M, self.H, self.r
        which = self.names if which is None else which
        out = G.Canary(M, H, torch.bfloat16, DEV, pre=2, post=3, pad=8) if with_dres else None
        gA = {t: G.Canary(r, H, torch.float32, DEV, pre=64, post=64, flat=True, fill=self.inp["gA0"][t].to(DEV)) for t in which}
        gB = {t: G.Canary(H, r, torch.float32, DEV, pre=64, post=64, flat=True, fill=self.inp["gB0"][t].to(DEV)) for t in which}
        need = lib.mmbert_lora_qkv_bwd_workspace(M, H, r, _mask(self.targets))
        ws = torch.full((need // 4 + 64,), G.NAN_F32, dtype=torch.int32, device=DEV)
        args = (_stream(), self.dqkv.data_ptr(), self.dqkv.stride(0), self.x.data_ptr(), self.x.stride(0),
                None if h is None else h.data_ptr(), 0 if h is None else h.stride(0), M, H, r, _mask(self.targets),
                _ptrs(self.A, self.names), _ptrs(self.B, self.names), self.s,
                self.dres.data_ptr() if with_dres else None, self.dres.stride(0) if with_dres else 0,
                out.view.data_ptr() if with_dres else None, out.view.stride(0) if with_dres else 0,
                _ptrs({t: c.view for t, c in gA.items()}, which), _ptrs({t: c.view for t, c in gB.items()}, which),
                1 if accumulate else 0, ws.data_ptr())
        if old:
            L.check(lib.mmbert_lora_qkv_bwd(*args), "mmbert_lora_qkv_bwd")
        else:
            L.check(lib.mmbert_lora_qkv_bwd_drop(*args, *drop), "mmbert_lora_qkv_bwd_drop")
        assert bool((ws[need // 4:] == G.NAN_F32).all()), "the workspace was written past mmbert_lora_qkv_bwd_workspace() bytes"
        return out, gA, gB


def _qkv_case(M, H, r, targets, dist, drop):
    S = _Qkv(M, H, r, targets, dist, seed=M + H + r)
    inp = S.inp
    qkv, h = S.fwd(drop)
    ref = XR.qkv_fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], targets, S.s, drop)
    q = {"qkv": XR.check(qkv.view, ref["qkv"], "qkv"), "h": XR.check(h.view, ref["h"], "h")}
    qkv.intact("qkv"); h.intact("h")
    accumulate = bool((M + r // 4) & 1)
    hg = h.view
    out, gA, gB = S.bwd(hg, drop, accumulate=accumulate)
    rb = XR.qkv_bwd(inp["dqkv"], inp["x"], hg.cpu(), inp["A"], inp["B"], targets, S.s, drop, dres=inp["dres"], gA0=inp["gA0"], gB0=inp["gB0"],
                    accumulate=accumulate)
    q["dres"] = XR.check(out.view, rb["dres"], "dres")
    q["dA"] = max(XR.check(gA[t].view, rb["dA"][t], f"dA[{t}]") for t in S.names)
    q["dB"] = max(XR.check(gB[t].view, rb["dB"][t], f"dB[{t}]") for t in S.names)
    print(f"qkv M={M} H={H} r={r} {targets} {dist} thr16={drop[1]}: " + " ".join(f"{k} {v:.3f}" for k, v in q.items()))
    out.intact("dres")
    for t in S.names:
        gA[t].intact(f"dA[{t}]"); gB[t].intact(f"dB[{t}]")
    # the other forms of the call give the same bits: h recomputed; no input-gradient part; one target's gradients only; accumulate flipped
    out2, gA2, gB2 = S.bwd(None, drop, accumulate=accumulate)
    assert torch.equal(out2.view, out.view)
    out3, gA3, gB3 = S.bwd(hg, drop, with_dres=False, accumulate=accumulate)
    assert out3 is None
    last = S.names[-1:]
    _, gA4, gB4 = S.bwd(hg, drop, with_dres=False, accumulate=accumulate, which=last)
    for t in S.names:
        assert torch.equal(gA2[t].view, gA[t].view) and torch.equal(gB2[t].view, gB[t].view), t
        assert torch.equal(gA3[t].view, gA[t].view) and torch.equal(gB3[t].view, gB[t].view), t
    assert torch.equal(gA4[last[0]].view, gA[last[0]].view) and torch.equal(gB4[last[0]].view, gB[last[0]].view)
    out5, gA5, gB5 = S.bwd(hg, drop, accumulate=not accumulate)
    rb5 = XR.qkv_bwd(inp["dqkv"], inp["x"], hg.cpu(), inp["A"], inp["B"], targets, S.s, drop, gA0=inp["gA0"], gB0=inp["gB0"], accumulate=not accumulate)
    assert torch.equal(out5.view, out.view)
    for t in S.names:
        XR.check(gA5[t].view, rb5["dA"][t], f"dA[{t}] (accumulate flipped)")
        XR.check(gB5[t].view, rb5["dB"][t], f"dB[{t}] (accumulate flipped)")


@pytest.mark.parametrize("M,H,r,targets,dist,p", QKV_CASES, ids=lambda v: "".join(t[0] for t in v) if isinstance(v, tuple) else str(v))
def test_qkv_kernels_against_float64(M, H, r, targets, dist, p):
    _qkv_case(M, H, r, targets, dist, _drop(p, 8 * (M % 5) + 3))


def test_qkv_kernels_at_the_smallest_threshold():
    _qkv_case(65, 64, 8, ("query", "key", "value"), "real", _drop(None, 3, thr1=True))


# ------------------------------------------------------------------------------------------------ the dense seams
class _Dense:
    def __init__(self, M, K, N, r, dist, seed=0, x=None):
        self.M, self.K, self.N, self.r = M, K, N, r
        self.s = 16.0 / r
        self.inp = inp = DR.inputs(M, K, N, r, dist, seed)
        if x is not None:
            inp["x"] = x
        self.x, self.dy, self.u = _window(inp["x"]), _window(inp["dy"]), _window(inp["u"])
        self.A, self.B = inp["A"].to(DEV), inp["B"].to(DEV)

    def fwd(self, mode, in_drop, drop=None, old=False):
        L, lib = _lib()
        M, K, N, r = self.M, self.K, self.N, self.r
        y = G.Canary(M, N, torch.bfloat16, DEV, pre=2, post=3, pad=8, fill=self.inp["y"].to(DEV))
        aux = G.Canary(M, N, torch.bfloat16, DEV, pre=1, post=2, pad=16) if mode == XR.GELU else None
        h = G.Canary(M, r, torch.bfloat16, DEV, pre=1, post=2, pad=4)
        ds, dt, dc = drop if drop is not None else (0, 0, 1.0)
        args = (_stream(), self.x.data_ptr(), self.x.stride(0), y.view.data_ptr(), y.view.stride(0), M, K, N, r, self.A.data_ptr(), self.B.data_ptr(),
                self.s, mode, ds, dt, dc, aux.view.data_ptr() if aux else None, aux.view.stride(0) if aux else 0, h.view.data_ptr(), h.view.stride(0))
        if old:
            L.check(lib.mmbert_lora_dense_fwd(*args), "mmbert_lora_dense_fwd")
        else:
            L.check(lib.mmbert_lora_dense_fwd_drop(*args, *in_drop), "mmbert_lora_dense_fwd_drop")
        return y, aux, h

    def bwd(self, h, in_drop, *, rows=None, with_dx=True, gelu=False, accumulate=True, with_ga=True, with_gb=True, old=False):
        L, lib = _lib()
        M, K, N, r = self.M, self.K, self.N, self.r
        dx = G.Canary(M, K, torch.bfloat16, DEV, pre=2, post=3, pad=8, fill=self.inp["dx"].to(DEV)) if with_dx else None
        gA = G.Canary(r, K, torch.float32, DEV, pre=64, post=64, flat=True, fill=self.inp["gA0"].to(DEV)) if with_ga else None
        gB = G.Canary(N, r, torch.float32, DEV, pre=64, post=64, flat=True, fill=self.inp["gB0"].to(DEV)) if with_gb else None
        need = lib.mmbert_lora_dense_bwd_workspace(M, K, N, r)
        ws = torch.full((need // 4 + 64,), G.NAN_F32, dtype=torch.int32, device=DEV)
        args = (_stream(), self.dy.data_ptr(), self.dy.stride(0), self.x.data_ptr(), self.x.stride(0),
                None if h is None else h.data_ptr(), 0 if h is None else h.stride(0), M, K, N, r, self.A.data_ptr(), self.B.data_ptr(), self.s,
                dx.view.data_ptr() if dx else None, dx.view.stride(0) if dx else 0, self.u.data_ptr() if gelu else None, self.u.stride(0) if gelu else 0,
                gA.view.data_ptr() if gA else None, gB.view.data_ptr() if gB else None, 1 if accumulate else 0, ws.data_ptr())
        if old:
            L.check(lib.mmbert_lora_dense_bwd(*args), "mmbert_lora_dense_bwd")
        else:
            L.check(lib.mmbert_lora_dense_bwd_drop(*args, *in_drop, None if rows is None else rows.data_ptr()), "mmbert_lora_dense_bwd_drop")
        assert bool((ws[need // 4:] == G.NAN_F32).all()), "the workspace was written past mmbert_lora_dense_bwd_workspace() bytes"
        return dx, gA, gB


def _dense_case(M, K, N, r, dist, ind):
    S = _Dense(M, K, N, r, dist, seed=M + K + N + r)
    inp = S.inp
    x, y0, A, B = inp["x"], inp["y"], inp["A"], inp["B"]
    q = {}
    y, _, h = S.fwd(XR.ADD, ind)
    ref = XR.dense_fwd(x, y0, A, B, S.s, XR.ADD, in_drop=ind)
    q["y"] = XR.check(y.view, ref["y"], "y (ADD)")
    q["h"] = XR.check(h.view, ref["h"], "h")
    y.intact("y"); h.intact("h")
    od = XR.in_drop(0.1, SEED + 1, M + N)                         # the GEMM's own output mask on top
    yd, _, hd = S.fwd(XR.ADD, ind, drop=od)
    q["y_drop"] = XR.check(yd.view, XR.dense_fwd(x, y0, A, B, S.s, XR.ADD, drop=od, in_drop=ind)["y"], "y (ADD, output mask)")
    assert torch.equal(hd.view, h.view)
    yd.intact("y (drop)")
    yg, aux, hg = S.fwd(XR.GELU, ind)
    refg = XR.dense_fwd(x, y0, A, B, S.s, XR.GELU, in_drop=ind)
    q["y_gelu"] = XR.check(yg.view, refg["y"], "y (GELU)")
    q["aux"] = XR.check(aux.view, refg["aux"], "aux")
    assert torch.equal(hg.view, h.view)
    yg.intact("y (GELU)"); aux.intact("aux")
    accumulate = bool((M + r // 4) & 1)
    hv = h.view
    kw = dict(in_drop=ind, gA0=inp["gA0"], gB0=inp["gB0"], accumulate=accumulate)
    dx, gA, gB = S.bwd(hv, ind, accumulate=accumulate)
    rb = XR.dense_bwd(inp["dy"], x, hv.cpu(), A, B, S.s, dx=inp["dx"], **kw)
    q["dx"] = XR.check(dx.view, rb["dx"], "dx")
    q["dA"] = XR.check(gA.view, rb["dA"], "dA")
    q["dB"] = XR.check(gB.view, rb["dB"], "dB")
    dx.intact("dx"); gA.intact("dA"); gB.intact("dB")
    dxg, gAg, gBg = S.bwd(hv, ind, gelu=True, accumulate=accumulate)
    q["dx_gelu"] = XR.check(dxg.view, XR.dense_bwd(inp["dy"], x, hv.cpu(), A, B, S.s, dx=inp["dx"], gelu_u=inp["u"], **kw)["dx"], "dx (gelu')")
    dxg.intact("dx (gelu')")
    assert torch.equal(gAg.view, gA.view) and torch.equal(gBg.view, gB.view)
    print(f"dense M={M} K={K} N={N} r={r} {dist} thr16={ind[1]}: " + " ".join(f"{k} {v:.3f}" for k, v in q.items()))
    # the other forms of the call give the same bits: h recomputed; no input-gradient part; one gradient only; accumulate flipped
    dx2, gA2, gB2 = S.bwd(None, ind, accumulate=accumulate)
    assert torch.equal(dx2.view, dx.view) and torch.equal(gA2.view, gA.view) and torch.equal(gB2.view, gB.view)
    dx3, gA3, gB3 = S.bwd(hv, ind, with_dx=False, accumulate=accumulate)
    assert dx3 is None and torch.equal(gA3.view, gA.view) and torch.equal(gB3.view, gB.view)
    _, gA4, gB4 = S.bwd(hv, ind, with_dx=False, accumulate=accumulate, with_gb=False)
    assert gB4 is None and torch.equal(gA4.view, gA.view)
    _, gA5, gB5 = S.bwd(None, ind, with_dx=False, accumulate=accumulate, with_ga=False)
    assert gA5 is None and torch.equal(gB5.view, gB.view)
    dx6, gA6, gB6 = S.bwd(hv, ind, accumulate=not accumulate)
    r6 = XR.dense_bwd(inp["dy"], x, hv.cpu(), A, B, S.s, in_drop=ind, gA0=inp["gA0"], gB0=inp["gB0"], accumulate=not accumulate)
    assert torch.equal(dx6.view, dx.view)
    XR.check(gA6.view, r6["dA"], "dA (accumulate flipped)"); XR.check(gB6.view, r6["dB"], "dB (accumulate flipped)")


@pytest.mark.parametrize("M,K,N,r,dist,p", DENSE_CASES)
def test_dense_kernels_against_float64(M, K, N, r, dist, p):
    _dense_case(M, K, N, r, dist, _drop(p, 8 * (M % 5) + 4 + (K > N) + 2 * (K == N)))


def test_dense_kernels_at_the_smallest_threshold():
    _dense_case(65, 128, 832, 4, "real", _drop(None, 5, thr1=True))


def test_gathered_rows_draw_the_mask_of_their_site_rows():
    """70 rows in non-monotonic order out of a 300-row site: backward on the gathered operands with the row list equals the reference under
    the mask of the ORIGINAL rows, with forward's h gathered and with h recomputed (the same bits); then the same with one more row whose id
    is 2^24 + 5 -- at K = 832 its element index is past 2^33."""
    K, N, r, site_rows = 832, 128, 8, 300
    ind = _drop(0.5, 8 * 11 + 6)
    full = _Dense(site_rows, K, N, r, "real", seed=31)
    _, _, h_full = full.fwd(XR.ADD, ind)
    XR.check(h_full.view, XR.dense_fwd(full.inp["x"], full.inp["y"], full.inp["A"], full.inp["B"], full.s, XR.ADD, in_drop=ind)["h"], "h (site)")
    rows = [(37 * i + 11) % site_rows for i in range(70)]
    assert len(set(rows)) == 70 and rows != sorted(rows)
    for extra in ((), (2 ** 24 + 5,)):
        rl = rows + list(extra)
        M = len(rl)
        xg = torch.cat([full.inp["x"][rows]] + ([full.inp["x"][:1]] if extra else []))
        S = _Dense(M, K, N, r, "real", seed=32, x=xg)
        S.A, S.B, S.inp["A"], S.inp["B"] = full.A, full.B, full.inp["A"], full.inp["B"]
        rt = torch.tensor(rl, dtype=torch.int32, device=DEV)
        inp = S.inp
        dx, gA, gB = S.bwd(None, ind, rows=rt, gelu=True)
        ref = XR.dense_bwd(inp["dy"], xg, None, inp["A"], inp["B"], S.s, in_drop=ind, rows=rl, dx=inp["dx"], gelu_u=inp["u"], gA0=inp["gA0"], gB0=inp["gB0"])
        q = (XR.check(dx.view, ref["dx"], "dx"), XR.check(gA.view, ref["dA"], "dA"), XR.check(gB.view, ref["dB"], "dB"))
        print(f"gathered rows M={M}: dx {q[0]:.3f} dA {q[1]:.3f} dB {q[2]:.3f}")
        dx.intact("dx"); gA.intact("dA"); gB.intact("dB")
        assert bool(ref["dx"].exact[-1].any()) and not bool(ref["dx"].exact[-1].all())
        # the mask of the identity rows is another one: the row list is read
        ref_id = XR.dense_bwd(inp["dy"], xg, None, inp["A"], inp["B"], S.s, in_drop=ind, dx=inp["dx"], gelu_u=inp["u"], gA0=inp["gA0"], gB0=inp["gB0"])
        assert XR.ratio(dx.view, ref_id["dx"]) > 1.0
        if not extra:                                             # forward's h of the site, gathered: the bits of the recomputed one
            hg = h_full.view[torch.tensor(rows, device=DEV)].contiguous()
            dx2, gA2, gB2 = S.bwd(hg, ind, rows=rt, gelu=True)
            assert torch.equal(dx2.view, dx.view) and torch.equal(gA2.view, gA.view) and torch.equal(gB2.view, gB.view)


def test_threshold_zero_is_the_entry_point_without_dropout():
    """in_thr16 = 0 through the new entry points (with a stream, a scale and a row list that must not change anything): every output has the
    bits of the old entry points."""
    nd = (0xDEADBEEF, 0, 1.25)
    Q = _Qkv(257, 768, 16, ("query", "key", "value"), "real", seed=3)
    a, b = Q.fwd(nd), Q.fwd(None, old=True)
    assert torch.equal(a[0].view, b[0].view) and torch.equal(a[1].view, b[1].view)
    for h in (a[1].view, None):
        o1, ga1, gb1 = Q.bwd(h, nd)
        o2, ga2, gb2 = Q.bwd(h, None, old=True)
        assert torch.equal(o1.view, o2.view)
        for t in Q.names:
            assert torch.equal(ga1[t].view, ga2[t].view) and torch.equal(gb1[t].view, gb2[t].view)
    D = _Dense(257, 832, 128, 8, "real", seed=4)
    od = XR.in_drop(0.1, SEED, 2)
    for mode, drop in ((XR.ADD, None), (XR.ADD, od), (XR.GELU, None)):
        a, b = D.fwd(mode, nd, drop=drop), D.fwd(mode, None, drop=drop, old=True)
        assert torch.equal(a[0].view, b[0].view) and torch.equal(a[2].view, b[2].view)
        assert mode != XR.GELU or torch.equal(a[1].view, b[1].view)
    rows = torch.arange(256, -1, -1, dtype=torch.int32, device=DEV)
    for h in (a[2].view, None):
        for gelu in (False, True):
            x1, ga1, gb1 = D.bwd(h, nd, rows=rows, gelu=gelu)
            x2, ga2, gb2 = D.bwd(h, None, gelu=gelu, old=True)
            assert torch.equal(x1.view, x2.view) and torch.equal(ga1.view, ga2.view) and torch.equal(gb1.view, gb2.view)


def test_bits_are_reproducible_and_independent_of_deterministic_mode():
    from msa_amd import ops
    Q = _Qkv(257, 768, 8, ("query", "value"), "real", seed=11)
    D = _Dense(257, 832, 128, 16, "real", seed=12)
    dq, dd = _drop(0.1, 3), _drop(0.1, 6)

    def run():
        qkv, h = Q.fwd(dq)
        out, gA, gB = Q.bwd(h.view, dq)
        y, _, hd = D.fwd(XR.ADD, dd)
        dx, ga, gb = D.bwd(None, dd, gelu=True)
        return ([qkv.view.clone(), h.view.clone(), out.view.clone(), y.view.clone(), hd.view.clone(), dx.view.clone(), ga.view.clone(), gb.view.clone()]
                + [gA[t].view.clone() for t in Q.names] + [gB[t].view.clone() for t in Q.names])

    was = ops.deterministic()
    try:
        ops.set_deterministic(False)
        a, b = run(), run()
        ops.set_deterministic(True)
        c = run()
    finally:
        ops.set_deterministic(was)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_ops_wrappers_take_the_triple():
    """ops.lora_* with ``in_drop`` / ``rows`` make the _drop calls (the bits of the raw ABI); without them, today's."""
    from msa_amd import ops
    ind = _drop(0.5, 4)
    D = _Dense(65, 128, 832, 8, "real", seed=21)
    y, _, h = D.fwd(XR.ADD, ind)
    y2 = D.inp["y"].to(DEV).clone()
    h2 = torch.empty((65, 8), dtype=torch.bfloat16, device=DEV)
    ops.lora_dense_fwd(D.x, y2, D.A, D.B, D.s, h_out=h2, in_drop=ind)
    assert torch.equal(y2, y.view) and torch.equal(h2, h.view)
    rows = torch.arange(64, -1, -1, dtype=torch.int32, device=DEV)
    dx, gA, gB = D.bwd(None, ind, rows=rows)
    dx2, ga2, gb2 = D.inp["dx"].to(DEV).clone(), D.inp["gA0"].to(DEV).clone(), D.inp["gB0"].to(DEV).clone()
    ops.lora_dense_bwd(D.dy, D.x, None, D.A, D.B, ga2, gb2, D.s, dx=dx2, in_drop=ind, rows=rows)
    assert torch.equal(dx2, dx.view) and torch.equal(ga2, gA.view) and torch.equal(gb2, gB.view)
    Q = _Qkv(65, 64, 4, ("query", "value"), "real", seed=22)
    qkv, hq = Q.fwd(ind)
    q2 = Q.inp["qkv"].to(DEV).clone()
    hq2 = torch.empty((65, 8), dtype=torch.bfloat16, device=DEV)
    ops.lora_qkv_fwd(Q.x, q2, Q.A, Q.B, Q.targets, Q.s, h_out=hq2, in_drop=ind)
    assert torch.equal(q2, qkv.view) and torch.equal(hq2, hq.view)
    out, gA, gB = Q.bwd(hq.view, ind)
    ga = {t: Q.inp["gA0"][t].to(DEV).clone() for t in Q.names}
    gb = {t: Q.inp["gB0"][t].to(DEV).clone() for t in Q.names}
    out2 = ops.lora_qkv_bwd(Q.dqkv, Q.x, hq2, Q.A, Q.B, ga, gb, Q.targets, Q.s, dres=Q.dres, in_drop=ind)
    assert torch.equal(out2, out.view) and all(torch.equal(ga[t], gA[t].view) and torch.equal(gb[t], gB[t].view) for t in Q.names)


def test_bad_arguments_are_refused():
    _, lib = _lib()
    H = 64
    x = torch.zeros((4, H), dtype=torch.bfloat16, device=DEV)
    qkv = torch.zeros((4, 3 * H), dtype=torch.bfloat16, device=DEV)
    A = {"query": torch.zeros((4, H), dtype=torch.bfloat16, device=DEV)}
    B = {"query": torch.zeros((H, 4), dtype=torch.bfloat16, device=DEV)}
    pa, pb = _ptrs(A, ["query"]), _ptrs(B, ["query"])
    ws = torch.zeros(1 << 16, device=DEV)
    rows = torch.zeros(8, dtype=torch.int32, device=DEV)
    qf = (_stream(), x.data_ptr(), H, qkv.data_ptr(), 3 * H, 4, H, 4, 1, pa, pb, 1.0, None, 0)
    qb = (_stream(), qkv.data_ptr(), 3 * H, x.data_ptr(), H, None, 0, 4, H, 4, 1, pa, pb, 1.0, None, 0, None, 0, None, None, 1, ws.data_ptr())
    a, b = A["query"], B["query"]
    df = (_stream(), x.data_ptr(), H, qkv.data_ptr(), 3 * H, 4, H, H, 4, a.data_ptr(), b.data_ptr(), 1.0, 0, 0, 0, 1.0, None, 0, None, 0)
    db = (_stream(), qkv.data_ptr(), 3 * H, x.data_ptr(), H, None, 0, 4, H, H, 4, a.data_ptr(), b.data_ptr(), 1.0, None, 0, None, 0, None, None, 1, ws.data_ptr())
    bad = ((5, 65536, 1.0), (5, 100, 0.0), (5, 100, -1.0), (5, 100, float("inf")), (5, 100, float("nan")), (5, 0, 0.0))
    for t in bad:
        assert lib.mmbert_lora_qkv_fwd_drop(*qf, *t) == -1, t
        assert lib.mmbert_lora_qkv_bwd_drop(*qb, *t) == -1, t
        assert lib.mmbert_lora_dense_fwd_drop(*df, *t) == -1, t
        assert lib.mmbert_lora_dense_bwd_drop(*db, *t, None) == -1, t
    ok = (5, 100, 1.0)
    assert lib.mmbert_lora_dense_bwd_drop(*db, *ok, rows.data_ptr() + 2) == -1            # a misaligned row list
    assert lib.mmbert_lora_dense_bwd_drop(*db[:-1], None, *ok, None) == -3                 # the old checks still hold: no workspace
    assert lib.mmbert_lora_qkv_fwd_drop(*qf[:8], 0, *qf[9:], *ok) == -1                    # ... no target
    # nothing asked for / M == 0: 0 without a launch, whatever the triple's stream
    assert lib.mmbert_lora_dense_bwd_drop(*db, *ok, rows.data_ptr()) == 0
    assert lib.mmbert_lora_qkv_fwd_drop(None, None, 0, None, 0, 0, H, 4, 1, None, None, 1.0, None, 0, *ok) == 0
    torch.cuda.synchronize()
    assert not bool(qkv.any())
