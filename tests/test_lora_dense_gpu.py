"""mmbert_lora_dense_fwd / _bwd (csrc/lora.hip) through the C ABI against tests/lora_dense_ref.py: float64 values, the calibrated bounds
(C_OUT = 2, C_ACC = 0.75, C_MID = 4 and the GELU terms), NaN canaries around every output and behind the workspace, bit-reproducibility.

Shapes: M in {1, 63, 64, 65, 129, 257} (one lane row; one row short of / exactly / one past a 64-row workgroup; two and three 128-token
slabs with a one-row tail) x (K, N) in {(64, 64), (64, 256), (256, 64), (128, 512)} with rank and input family rotating; (768, 3072) and
(3072, 768) -- the model's FFN seams: four / one 768-column chunks on either side, three column blocks of the token sums -- at M = 129 for
every rank.  Every case runs the forward in both modes, ADD with and without dropout (p = 0.1, the mask of tests/rng_ref.py: a dropped
element must keep its bits), and the backward with and without the gelu' factor.  x, y, dy, dx and u are column windows of wider matrices
(pitch = width + 64), so the dropout index must use N, not the pitch."""
import pytest
import torch

from tests import gemm_ref as G
from tests import lora_dense_ref as DR
from tests import rng_ref as RNG

pytestmark = pytest.mark.gpu

DEV = "cuda"
MS, KNS, RS = (1, 63, 64, 65, 129, 257), ((64, 64), (64, 256), (256, 64), (128, 512)), (4, 8, 16)
CASES = [(M, K, N, RS[(i + j) % 3], DR.DISTS[(i + j) % 4]) for i, M in enumerate(MS) for j, (K, N) in enumerate(KNS)]
CASES += [(129, K, N, r, "real") for (K, N) in ((768, 3072), (3072, 768)) for r in RS]
P_DROP = 0.1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _drop(site):
    t = RNG.thr16(P_DROP)
    return (RNG.rng_stream(777, site), t, RNG.drop_scale(t))


def _window(t, pad=64, fill=1e30):
    """t [M, N] as a column window of a wider matrix (row pitch N + pad) whose other columns hold ``fill``."""
    M, N = t.shape
    wide = torch.full((max(M, 1), N + pad), fill, dtype=t.dtype, device=DEV)
    wide[:M, 8:8 + N] = t.to(DEV)
    return wide[:M, 8:8 + N]


class _Setup:
    def __init__(self, M, K, N, r, dist, seed=0):
        self.M, self.K, self.N, self.r = M, K, N, r
        self.s = 16.0 / r
        self.inp = inp = DR.inputs(M, K, N, r, dist, seed)
        self.x, self.dy, self.u = _window(inp["x"]), _window(inp["dy"]), _window(inp["u"])
        self.A, self.B = inp["A"].to(DEV), inp["B"].to(DEV)

    def fwd(self, mode, drop=None, with_aux=True, with_h=True):
        """(y canary, aux canary or None, h canary or None) after the forward launch."""
        from msa_amd import _lib
        M, K, N, r = self.M, self.K, self.N, self.r
        y = G.Canary(M, N, torch.bfloat16, DEV, pre=2, post=3, pad=8, fill=self.inp["y"].to(DEV))
        aux = G.Canary(M, N, torch.bfloat16, DEV, pre=1, post=2, pad=16) if (mode == DR.GELU and with_aux) else None
        h = G.Canary(M, r, torch.bfloat16, DEV, pre=1, post=2, pad=4) if with_h else None
        ds, dt, dc = drop if drop is not None else (0, 0, 1.0)
        _lib.check(_lib.load().mmbert_lora_dense_fwd(
            _stream(), self.x.data_ptr(), self.x.stride(0), y.view.data_ptr(), y.view.stride(0), M, K, N, r, self.A.data_ptr(), self.B.data_ptr(),
            self.s, mode, ds, dt, dc, aux.view.data_ptr() if aux else None, aux.view.stride(0) if aux else 0,
            h.view.data_ptr() if h else None, h.view.stride(0) if h else 0), "mmbert_lora_dense_fwd")
        return y, aux, h

    def bwd(self, h, *, with_dx=True, gelu=False, accumulate=True, with_ga=True, with_gb=True):
        """Raw backward call into canary buffers.  Returns (dx canary or None, gA canary or None, gB canary or None, workspace tail ok)."""
        from msa_amd import _lib
        lib = _lib.load()
        M, K, N, r = self.M, self.K, self.N, self.r
        dx = G.Canary(M, K, torch.bfloat16, DEV, pre=2, post=3, pad=8, fill=self.inp["dx"].to(DEV)) if with_dx else None
        gA = G.Canary(r, K, torch.float32, DEV, pre=64, post=64, flat=True, fill=self.inp["gA0"].to(DEV)) if with_ga else None
        gB = G.Canary(N, r, torch.float32, DEV, pre=64, post=64, flat=True, fill=self.inp["gB0"].to(DEV)) if with_gb else None
        need = lib.mmbert_lora_dense_bwd_workspace(M, K, N, r)
        assert need % 16 == 0 and need > 0
        ws = torch.full((need // 4 + 64,), G.NAN_F32, dtype=torch.int32, device=DEV)
        _lib.check(lib.mmbert_lora_dense_bwd(
            _stream(), self.dy.data_ptr(), self.dy.stride(0), self.x.data_ptr(), self.x.stride(0),
            None if h is None else h.data_ptr(), 0 if h is None else h.stride(0), M, K, N, r, self.A.data_ptr(), self.B.data_ptr(), self.s,
            dx.view.data_ptr() if dx else None, dx.view.stride(0) if dx else 0,
            self.u.data_ptr() if gelu else None, self.u.stride(0) if gelu else 0,
            gA.view.data_ptr() if gA else None, gB.view.data_ptr() if gB else None, 1 if accumulate else 0, ws.data_ptr()), "mmbert_lora_dense_bwd")
        tail_ok = bool((ws[need // 4:] == G.NAN_F32).all())
        return dx, gA, gB, tail_ok


@pytest.mark.parametrize("M,K,N,r,dist", CASES)
def test_both_kernels_against_float64(M, K, N, r, dist):
    S = _Setup(M, K, N, r, dist, seed=M + K + N + r)
    inp = S.inp
    x, y0, A, B = inp["x"], inp["y"], inp["A"], inp["B"]
    q = {}
    # ---- forward, ADD without dropout
    y, _, h = S.fwd(DR.ADD)
    ref = DR.fwd(x, y0, A, B, S.s, DR.ADD)
    q["y"] = DR.check(y.view, ref["y"], "y (ADD)")
    q["h"] = DR.check(h.view, ref["h"], "h")
    y.intact("y"); h.intact("h")
    y_b, _, _ = S.fwd(DR.ADD, with_h=False)                     # h_out = NULL: the same y
    assert torch.equal(y_b.view, y.view)
    # ---- ADD behind a dropout of p = 0.1: the reference's mask has the generator's keep rate, dropped elements keep their bits
    drop = _drop(M + N)
    keep = DR.keep_mask(M, N, drop[0], drop[1])
    if M * N >= 4096:
        assert DR.keep_rate_ok(keep, drop[1]), float(keep.mean())
    yd, _, hd = S.fwd(DR.ADD, drop=drop)
    refd = DR.fwd(x, y0, A, B, S.s, DR.ADD, drop=drop)
    q["y_drop"] = DR.check(yd.view, refd["y"], "y (ADD, p = 0.1)")
    assert torch.equal(hd.view, h.view)
    yd.intact("y (drop)")
    # ---- GELU, with and without aux
    yg, aux, hg = S.fwd(DR.GELU)
    refg = DR.fwd(x, y0, A, B, S.s, DR.GELU)
    q["y_gelu"] = DR.check(yg.view, refg["y"], "y (GELU)")
    q["aux"] = DR.check(aux.view, refg["aux"], "aux")
    assert torch.equal(hg.view, h.view)
    yg.intact("y (GELU)"); aux.intact("aux")
    yg2, _, _ = S.fwd(DR.GELU, with_aux=False, with_h=False)
    assert torch.equal(yg2.view, yg.view)
    # ---- backward, reading forward's h; the old gradients are added or overwritten by the parity of M + r / 4
    accumulate = bool((M + r // 4) & 1)
    hv = h.view
    kw = dict(gA0=inp["gA0"], gB0=inp["gB0"], accumulate=accumulate)
    dx, gA, gB, tail_ok = S.bwd(hv, accumulate=accumulate)
    rb = DR.bwd(inp["dy"], x, hv.cpu(), A, B, S.s, dx=inp["dx"], **kw)
    q["dx"] = DR.check(dx.view, rb["dx"], "dx")
    q["dA"] = DR.check(gA.view, rb["dA"], "dA")
    q["dB"] = DR.check(gB.view, rb["dB"], "dB")
    dx.intact("dx"); gA.intact("dA"); gB.intact("dB")
    assert tail_ok, "the workspace was written past mmbert_lora_dense_bwd_workspace() bytes"
    dxg, gAg, gBg, tail_g = S.bwd(hv, gelu=True, accumulate=accumulate)
    rg = DR.bwd(inp["dy"], x, hv.cpu(), A, B, S.s, dx=inp["dx"], gelu_u=inp["u"], **kw)
    q["dx_gelu"] = DR.check(dxg.view, rg["dx"], "dx (gelu')")
    dxg.intact("dx (gelu')")
    assert tail_g and torch.equal(gAg.view, gA.view) and torch.equal(gBg.view, gB.view)
    print(f"M={M} K={K} N={N} r={r} {dist}: " + " ".join(f"{k} {v:.3f}" for k, v in q.items()))
    # ---- the other forms of the call give the same bits: h recomputed; no input-gradient part; one gradient only
    dx2, gA2, gB2, tail2 = S.bwd(None, accumulate=accumulate)
    assert tail2 and torch.equal(dx2.view, dx.view) and torch.equal(gA2.view, gA.view) and torch.equal(gB2.view, gB.view)
    dx3, gA3, gB3, _ = S.bwd(hv, with_dx=False, accumulate=accumulate)
    assert dx3 is None and torch.equal(gA3.view, gA.view) and torch.equal(gB3.view, gB.view)
    _, gA4, none4, _ = S.bwd(hv, with_dx=False, accumulate=accumulate, with_gb=False)
    _, none5, gB5, _ = S.bwd(None, with_dx=False, accumulate=accumulate, with_ga=False)
    assert none4 is None and none5 is None and torch.equal(gA4.view, gA.view) and torch.equal(gB5.view, gB.view)
    dx6, _, _, _ = S.bwd(hv, with_ga=False, with_gb=False)
    assert torch.equal(dx6.view, dx.view)


def test_zero_b_leaves_the_add_seam_bit_identical():
    """B = 0 behind a dropout: y keeps its bits (what makes a model with fresh adapters on the two ADD seams a bit-exact twin)."""
    S = _Setup(129, 128, 512, 8, "real", seed=3)
    S.B = torch.zeros_like(S.B)
    for drop in (None, _drop(1)):
        y, _, _ = S.fwd(DR.ADD, drop=drop)
        assert torch.equal(y.view, S.inp["y"].to(DEV))


def test_row_sliced_call_through_ops():
    """ops.lora_dense_fwd / _bwd on [:ra] of larger buffers: the rows behind ra keep their bits, the rows in front follow the reference."""
    from msa_amd import ops
    M, ra, K, N, r = 200, 131, 128, 512, 8
    S = _Setup(M, K, N, r, "real", seed=5)
    inp = S.inp
    drop = _drop(2)
    y_full = inp["y"].to(DEV).clone()
    h_full = torch.zeros((M, r), dtype=torch.bfloat16, device=DEV)
    assert ops.lora_dense_fwd(S.x[:ra], y_full[:ra], S.A, S.B, S.s, drop=drop, h_out=h_full[:ra]) is not None
    assert torch.equal(y_full[ra:], inp["y"].to(DEV)[ra:]) and not bool(h_full[ra:].any())
    ref = DR.fwd(inp["x"][:ra], inp["y"][:ra], inp["A"], inp["B"], S.s, DR.ADD, drop=drop)
    DR.check(y_full[:ra], ref["y"], "y[:ra]")
    DR.check(h_full[:ra], ref["h"], "h[:ra]")
    g_full, u_full = inp["y"].to(DEV).clone(), torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
    ops.lora_dense_fwd(S.x[:ra], g_full[:ra], S.A, S.B, S.s, mode=ops.LORA_DENSE_GELU, aux=u_full[:ra])
    refg = DR.fwd(inp["x"][:ra], inp["y"][:ra], inp["A"], inp["B"], S.s, DR.GELU)
    DR.check(g_full[:ra], refg["y"], "g[:ra]")
    DR.check(u_full[:ra], refg["aux"], "u[:ra]")
    assert torch.equal(g_full[ra:], inp["y"].to(DEV)[ra:]) and not bool(u_full[ra:].any())
    gA, gB = inp["gA0"].to(DEV).clone(), inp["gB0"].to(DEV).clone()
    dx_full = inp["dx"].to(DEV).clone()
    out = ops.lora_dense_bwd(S.dy[:ra], S.x[:ra], h_full[:ra], S.A, S.B, gA, gB, S.s, dx=dx_full[:ra], gelu_u=S.u[:ra], accumulate=True)
    assert out.data_ptr() == dx_full.data_ptr() and torch.equal(dx_full[ra:], inp["dx"].to(DEV)[ra:])       # in place, the rows behind untouched
    rb = DR.bwd(inp["dy"][:ra], inp["x"][:ra], h_full[:ra].cpu(), inp["A"], inp["B"], S.s, dx=inp["dx"][:ra], gelu_u=inp["u"][:ra],
                gA0=inp["gA0"], gB0=inp["gB0"], accumulate=True)
    DR.check(dx_full[:ra], rb["dx"], "dx[:ra]")
    DR.check(gA, rb["dA"], "dA")
    DR.check(gB, rb["dB"], "dB")
    assert ops.lora_dense_bwd(S.dy[:ra], S.x[:ra], None, S.A, S.B, None, None, S.s) is None


def test_empty_call_launches_nothing():
    from msa_amd import _lib, ops
    K, N, r = 64, 128, 4
    A = torch.zeros((r, K), dtype=torch.bfloat16, device=DEV)
    B = torch.zeros((N, r), dtype=torch.bfloat16, device=DEV)
    x = torch.empty((0, K), dtype=torch.bfloat16, device=DEV)
    y = torch.empty((0, N), dtype=torch.bfloat16, device=DEV)
    ops.lora_dense_fwd(x, y, A, B, 1.0)
    gA, gB = torch.full((r, K), 3.0, device=DEV), torch.full((N, r), 5.0, device=DEV)
    ops.lora_dense_bwd(y, x, None, A, B, gA, gB, 1.0, dx=x, accumulate=False)
    assert bool((gA == 3.0).all()) and bool((gB == 5.0).all())
    lib = _lib.load()
    assert lib.mmbert_lora_dense_bwd_workspace(0, K, N, r) == 0
    # M == 0 returns before any pointer is looked at
    assert lib.mmbert_lora_dense_fwd(None, None, 0, None, 0, 0, K, N, r, None, None, 1.0, 0, 0, 0, 1.0, None, 0, None, 0) == 0
    assert lib.mmbert_lora_dense_bwd(None, None, 0, None, 0, None, 0, 0, K, N, r, None, None, 1.0, None, 0, None, 0, None, None, 1, None) == 0


def test_bits_are_reproducible_and_independent_of_deterministic_mode():
    from msa_amd import ops
    S = _Setup(257, 128, 512, 16, "real", seed=11)
    drop = _drop(3)

    def run():
        y, _, h = S.fwd(DR.ADD, drop=drop)
        g, aux, _ = S.fwd(DR.GELU)
        dx, gA, gB, _ = S.bwd(h.view, gelu=True, accumulate=True)
        return [t.view.clone() for t in (y, h, g, aux, dx, gA, gB)]

    was = ops.deterministic()
    try:
        ops.set_deterministic(False)
        a, b = run(), run()
        ops.set_deterministic(True)
        c = run()
    finally:
        ops.set_deterministic(was)
    for p, q, w in zip(a, b, c):
        assert torch.equal(p, q) and torch.equal(p, w)


def test_bad_arguments_are_refused():
    """-1 and -3 by arguments alone, nothing launched or written.  The -2 of the library's convention (staged operands beyond 160 KiB of
    LDS) cannot be provoked here: A and B are staged in 768-column chunks, 24.8 KB whatever K and N are -- a width whose whole padded tile
    would be 262 KB (K = 8192) runs and matches the reference instead."""
    from msa_amd import _lib, ops
    lib = _lib.load()
    K, N, r, M = 64, 128, 4, 4
    x = torch.zeros((M, K), dtype=torch.bfloat16, device=DEV)
    y = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
    for rr in (2, 5, 32):
        A = torch.zeros((rr, K), dtype=torch.bfloat16, device=DEV)
        B = torch.zeros((N, rr), dtype=torch.bfloat16, device=DEV)
        with pytest.raises(RuntimeError, match="mmbert_lora_dense_fwd failed with code -1"):
            ops.lora_dense_fwd(x, y, A, B, 1.0)
    A = torch.ones((r, K), dtype=torch.bfloat16, device=DEV)
    B = torch.ones((N, r), dtype=torch.bfloat16, device=DEV)
    x.fill_(1.0)
    with pytest.raises(ValueError):
        ops.lora_dense_fwd(x, y, A.t().contiguous(), B, 1.0)

    def fwd(**o):
        a = dict(x=x.data_ptr(), ldx=K, y=y.data_ptr(), ldy=N, M=M, K=K, N=N, r=r, A=A.data_ptr(), B=B.data_ptr(), mode=0, thr=0, aux=None, ldaux=0,
                 h=None, ldh=0)
        a.update(o)
        return lib.mmbert_lora_dense_fwd(_stream(), a["x"], a["ldx"], a["y"], a["ldy"], a["M"], a["K"], a["N"], a["r"], a["A"], a["B"], 1.0, a["mode"],
                                         0, a["thr"], 1.0, a["aux"], a["ldaux"], a["h"], a["ldh"])

    assert fwd() == 0
    torch.cuda.synchronize()
    assert bool((y == 64 * 4).all())                             # (the good call does run: 64 ones times 4 rank entries)
    y.zero_()
    for bad in (dict(K=32, ldx=32), dict(N=96, ldy=96), dict(K=0), dict(M=-1), dict(ldx=K - 8), dict(ldx=K + 4), dict(ldy=N + 4), dict(mode=2), dict(mode=-1),
                dict(x=x.data_ptr() + 2), dict(y=y.data_ptr() + 8), dict(A=None), dict(B=B.data_ptr() + 4), dict(thr=65536),
                dict(aux=y.data_ptr(), ldaux=N), dict(mode=1, aux=y.data_ptr(), ldaux=N - 8), dict(h=x.data_ptr() + 2, ldh=r), dict(h=x.data_ptr(), ldh=2)):
        assert fwd(**bad) == -1, bad
    ws = torch.zeros(1 << 16, device=DEV)
    gA, gB = torch.zeros((r, K), device=DEV), torch.zeros((N, r), device=DEV)
    dxb = torch.zeros((M, K), dtype=torch.bfloat16, device=DEV)

    def bwd(**o):
        a = dict(dy=y.data_ptr(), lddy=N, x=x.data_ptr(), ldx=K, h=None, ldh=0, M=M, K=K, N=N, r=r, dx=dxb.data_ptr(), lddx=K, u=None, ldu=0,
                 gA=gA.data_ptr(), gB=gB.data_ptr(), ws=ws.data_ptr())
        a.update(o)
        return lib.mmbert_lora_dense_bwd(_stream(), a["dy"], a["lddy"], a["x"], a["ldx"], a["h"], a["ldh"], a["M"], a["K"], a["N"], a["r"], A.data_ptr(),
                                         B.data_ptr(), 1.0, a["dx"], a["lddx"], a["u"], a["ldu"], a["gA"], a["gB"], 1, a["ws"])

    for bad in (dict(K=32, ldx=32), dict(N=32, lddy=32), dict(r=3), dict(lddy=N - 8), dict(lddx=K + 4), dict(dx=dxb.data_ptr() + 2),
                dict(u=x.data_ptr(), ldu=K, dx=None), dict(u=x.data_ptr(), ldu=K - 8), dict(gA=gA.data_ptr() + 4), dict(h=x.data_ptr(), ldh=2)):
        assert bwd(**bad) == -1, bad
    assert bwd(ws=None) == -3 and bwd(ws=ws.data_ptr() + 4) == -3
    torch.cuda.synchronize()
    assert not bool(y.any()) and not bool(gA.any()) and not bool(gB.any()) and not bool(dxb.any())
    # a width past what ONE padded tile could hold in 160 KiB: chunked staging runs it
    S = _Setup(65, 8192, 64, 8, "real", seed=2)
    yw, _, hw = S.fwd(DR.ADD)
    ref = DR.fwd(S.inp["x"], S.inp["y"], S.inp["A"], S.inp["B"], S.s, DR.ADD)
    DR.check(yw.view, ref["y"], "y (K = 8192)")
    DR.check(hw.view, ref["h"], "h (K = 8192)")
