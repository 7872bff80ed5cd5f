"""mmbert_lora_qkv_fwd / _bwd (csrc/lora.hip) through the C ABI against tests/lora_ref.py: float64 values, the calibrated bounds
(C_OUT = 2, C_ACC = 0.75, C_MID = 4), NaN canaries around every output, bit-reproducibility.

Shapes: M in {1, 63, 64, 65, 257, 1153} (one lane row; one row short of / exactly / one past a 64-row workgroup; three 128-token slabs
with a one-row tail; ten slabs -- the fold runs over more than one partial sum from M = 129 on), H in {64, 128, 768} (one and two 32-column
steps per lane group; the model's width, whose staged operands pass 64 KiB of LDS with three targets), r in {4, 8, 16}, targets {q},
{q, v}, {q, k, v}; every M x H pair once with rank, target set and input family rotating, and every rank x target set at M = 257, H = 128.
x is always a column window of a wider matrix (ldx = H + 64)."""
import ctypes

import pytest
import torch

from tests import gemm_ref as G
from tests import lora_ref as LR

pytestmark = pytest.mark.gpu

DEV = "cuda"
MS, HS, RS = (1, 63, 64, 65, 257, 1153), (64, 128, 768), (4, 8, 16)
TSETS = (("query",), ("query", "value"), ("query", "key", "value"))
CASES = [(M, H, RS[(i + j) % 3], TSETS[(i + 2 * j) % 3], LR.DISTS[(i + j) % 4]) for i, M in enumerate(MS) for j, H in enumerate(HS)]
CASES += [(257, 128, r, ts, "real") for r in RS for ts in TSETS if (257, 128, r, ts, "real") not in CASES]
P3 = ctypes.c_void_p * 3


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


class _Setup:
    def __init__(self, M, H, r, targets, dist, seed=0):
        self.M, self.H, self.r, self.targets = M, H, r, targets
        self.names = [t for t in LR.TARGETS if t in targets]
        self.nt = len(self.names)
        self.s = 16.0 / r
        self.inp = inp = LR.inputs(M, H, r, targets, dist, seed)
        self.x = _window(inp["x"])
        self.dqkv = _window(inp["dqkv"])
        self.dres = _window(inp["dres"])
        self.A = {t: inp["A"][t].to(DEV) for t in self.names}
        self.B = {t: inp["B"][t].to(DEV) for t in self.names}

    def fwd(self):
        """(qkv canary, h canary) after the forward launch."""
        from msa_amd import _lib
        M, H, r = self.M, self.H, self.r
        qkv = G.Canary(M, 3 * H, torch.bfloat16, DEV, pre=2, post=3, pad=8, fill=self.inp["qkv"].to(DEV))
        h = G.Canary(M, self.nt * r, torch.bfloat16, DEV, pre=1, post=2, pad=4)
        _lib.check(_lib.load().mmbert_lora_qkv_fwd(_stream(), self.x.data_ptr(), self.x.stride(0), qkv.view.data_ptr(), qkv.view.stride(0), M, H, r,
                                                   _mask(self.targets), _ptrs(self.A, self.names), _ptrs(self.B, self.names), self.s,
                                                   h.view.data_ptr(), h.view.stride(0)), "mmbert_lora_qkv_fwd")
        return qkv, h

    def bwd(self, h, *, with_dres=True, accumulate=True, which=None):
        """Raw backward call into canary buffers.  Returns (dres canary or None, {name: gA canary}, {name: gB canary}, workspace tail ok)."""
        from msa_amd import _lib
        lib = _lib.load()
        M, H, r = self.M, self.H, self.r
        which = self.names if which is None else which
        out = G.Canary(M, H, torch.bfloat16, DEV, pre=2, post=3, pad=8) if with_dres else None
        gA = {t: G.Canary(r, H, torch.float32, DEV, pre=64, post=64, flat=True, fill=self.inp["gA0"][t].to(DEV)) for t in which}
        gB = {t: G.Canary(H, r, torch.float32, DEV, pre=64, post=64, flat=True, fill=self.inp["gB0"][t].to(DEV)) for t in which}
        need = lib.mmbert_lora_qkv_bwd_workspace(M, H, r, _mask(self.targets))
        assert need % 16 == 0
        ws = torch.full((need // 4 + 64,), G.NAN_F32, dtype=torch.int32, device=DEV)
        _lib.check(lib.mmbert_lora_qkv_bwd(
            _stream(), self.dqkv.data_ptr(), self.dqkv.stride(0), self.x.data_ptr(), self.x.stride(0),
            None if h is None else h.data_ptr(), 0 if h is None else h.stride(0), M, H, r, _mask(self.targets),
            _ptrs(self.A, self.names), _ptrs(self.B, self.names), self.s,
            self.dres.data_ptr() if with_dres else None, self.dres.stride(0) if with_dres else 0,
            out.view.data_ptr() if with_dres else None, out.view.stride(0) if with_dres else 0,
            _ptrs({t: c.view for t, c in gA.items()}, which), _ptrs({t: c.view for t, c in gB.items()}, which),
            1 if accumulate else 0, ws.data_ptr()), "mmbert_lora_qkv_bwd")
        tail_ok = bool((ws[need // 4:] == G.NAN_F32).all())
        return out, gA, gB, tail_ok


@pytest.mark.parametrize("M,H,r,targets,dist", CASES, ids=lambda v: "".join(t[0] for t in v) if isinstance(v, tuple) else str(v))
def test_both_kernels_against_float64(M, H, r, targets, dist):
    S = _Setup(M, H, r, targets, dist, seed=M + H + r)
    inp = S.inp
    # ---- forward
    qkv, h = S.fwd()
    ref = LR.fwd(inp["x"], inp["qkv"], inp["A"], inp["B"], targets, S.s)
    q1 = LR.check(qkv.view, ref["qkv"], "qkv")
    q2 = LR.check(h.view, ref["h"], "h")
    qkv.intact("qkv"); h.intact("h")
    # ---- backward, reading forward's h; the old gradients are added on odd r * M, overwritten otherwise
    accumulate = bool((M + r // 4) & 1)
    hg = h.view
    out, gA, gB, tail_ok = S.bwd(hg, accumulate=accumulate)
    rb = LR.bwd(inp["dqkv"], inp["x"], hg.cpu(), inp["A"], inp["B"], targets, S.s, dres=inp["dres"], gA0=inp["gA0"], gB0=inp["gB0"],
                accumulate=accumulate)
    q3 = LR.check(out.view, rb["dres"], "dres")
    q4 = max(LR.check(gA[t].view, rb["dA"][t], f"dA[{t}]") for t in S.names)
    q5 = max(LR.check(gB[t].view, rb["dB"][t], f"dB[{t}]") for t in S.names)
    print(f"M={M} H={H} r={r} {targets} {dist}: qkv {q1:.3f} h {q2:.3f} dres {q3:.3f} dA {q4:.3f} dB {q5:.3f}")
    out.intact("dres")
    for t in S.names:
        gA[t].intact(f"dA[{t}]"); gB[t].intact(f"dB[{t}]")
    assert tail_ok, "the workspace was written past mmbert_lora_qkv_bwd_workspace() bytes"
    # ---- the other forms of the call give the same bits: h recomputed; no input-gradient part; one target's gradients only
    out2, gA2, gB2, tail2 = S.bwd(None, accumulate=accumulate)
    assert tail2 and torch.equal(out2.view, out.view)
    out3, gA3, gB3, _ = S.bwd(hg, with_dres=False, accumulate=accumulate)
    assert out3 is None
    last = S.names[-1:]
    _, gA4, gB4, _ = S.bwd(hg, with_dres=False, accumulate=accumulate, which=last)
    for t in S.names:
        assert torch.equal(gA2[t].view, gA[t].view) and torch.equal(gB2[t].view, gB[t].view), t
        assert torch.equal(gA3[t].view, gA[t].view) and torch.equal(gB3[t].view, gB[t].view), t
    assert torch.equal(gA4[last[0]].view, gA[last[0]].view) and torch.equal(gB4[last[0]].view, gB[last[0]].view)


def test_row_sliced_call_through_ops():
    """ops.lora_qkv_fwd / _bwd on [:ra] of larger buffers: the rows behind ra keep their bits, the rows in front equal a call on copies."""
    from msa_amd import ops
    M, ra, H, r, targets = 200, 131, 128, 8, ("query", "value")
    S = _Setup(M, H, r, targets, "real", seed=5)
    inp = S.inp
    qkv_full = inp["qkv"].to(DEV).clone()
    h_full = torch.zeros((M, 2 * r), dtype=torch.bfloat16, device=DEV)
    ops.lora_qkv_fwd(S.x[:ra], qkv_full[:ra], S.A, S.B, targets, S.s, h_out=h_full[:ra])
    assert torch.equal(qkv_full[ra:], inp["qkv"].to(DEV)[ra:]) and not bool(h_full[ra:].any())
    ref = LR.fwd(inp["x"][:ra], inp["qkv"][:ra], inp["A"], inp["B"], targets, S.s)
    LR.check(qkv_full[:ra], ref["qkv"], "qkv[:ra]")
    LR.check(h_full[:ra], ref["h"], "h[:ra]")
    gA = {t: inp["gA0"][t].to(DEV).clone() for t in targets}
    gB = {t: inp["gB0"][t].to(DEV).clone() for t in targets}
    dres = S.dres.clone()
    out = ops.lora_qkv_bwd(S.dqkv[:ra], S.x[:ra], h_full[:ra], S.A, S.B, gA, gB, targets, S.s, dres=S.dres[:ra], accumulate=True)
    assert out.shape == (ra, H) and torch.equal(S.dres, dres)                         # dres itself is not written
    rb = LR.bwd(inp["dqkv"][:ra], inp["x"][:ra], h_full[:ra].cpu(), inp["A"], inp["B"], targets, S.s, dres=inp["dres"][:ra],
                gA0=inp["gA0"], gB0=inp["gB0"], accumulate=True)
    LR.check(out, rb["dres"], "dres[:ra]")
    for t in targets:
        LR.check(gA[t], rb["dA"][t], f"dA[{t}]")
        LR.check(gB[t], rb["dB"][t], f"dB[{t}]")
    assert ops.lora_qkv_bwd(S.dqkv[:ra], S.x[:ra], h_full[:ra], S.A, S.B, None, None, targets, S.s, dres=None) is None


def test_empty_call_launches_nothing():
    from msa_amd import _lib, ops
    H, r = 64, 4
    A = {"query": torch.zeros((r, H), dtype=torch.bfloat16, device=DEV)}
    B = {"query": torch.zeros((H, r), dtype=torch.bfloat16, device=DEV)}
    x = torch.empty((0, H), dtype=torch.bfloat16, device=DEV)
    qkv = torch.empty((0, 3 * H), dtype=torch.bfloat16, device=DEV)
    ops.lora_qkv_fwd(x, qkv, A, B, ("query",), 1.0)
    g = {"query": torch.full((r, H), 3.0, device=DEV)}
    gb = {"query": torch.full((H, r), 5.0, device=DEV)}
    out = ops.lora_qkv_bwd(qkv, x, None, A, B, g, gb, ("query",), 1.0, dres=x, accumulate=False)
    assert out.shape == (0, H) and bool((g["query"] == 3.0).all()) and bool((gb["query"] == 5.0).all())
    assert _lib.load().mmbert_lora_qkv_bwd_workspace(0, H, r, 1) == 0
    # M == 0 returns before any pointer is looked at
    assert _lib.load().mmbert_lora_qkv_fwd(None, None, 0, None, 0, 0, H, r, 1, None, None, 1.0, None, 0) == 0


def test_bits_are_reproducible_and_independent_of_deterministic_mode():
    from msa_amd import ops
    S = _Setup(1153, 128, 16, ("query", "key", "value"), "real", seed=11)

    def run():
        qkv, h = S.fwd()
        out, gA, gB, _ = S.bwd(h.view, accumulate=True)
        return [qkv.view.clone(), h.view.clone(), out.view.clone()] + [gA[t].view.clone() for t in S.names] + [gB[t].view.clone() for t in S.names]

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


def test_bad_arguments_are_refused():
    from msa_amd import _lib, ops
    lib = _lib.load()
    H = 64
    x = torch.zeros((4, H), dtype=torch.bfloat16, device=DEV)
    qkv = torch.zeros((4, 3 * H), dtype=torch.bfloat16, device=DEV)
    for r in (2, 5, 32):
        A = {"query": torch.zeros((r, H), dtype=torch.bfloat16, device=DEV)}
        B = {"query": torch.zeros((H, r), dtype=torch.bfloat16, device=DEV)}
        with pytest.raises(RuntimeError, match="mmbert_lora_qkv_fwd failed with code -1"):
            ops.lora_qkv_fwd(x, qkv, A, B, ("query",), 1.0)
    A = {"query": torch.zeros((4, H), dtype=torch.bfloat16, device=DEV)}
    B = {"query": torch.zeros((H, 4), dtype=torch.bfloat16, device=DEV)}
    with pytest.raises(ValueError):
        ops.lora_qkv_fwd(x, qkv, A, B, (), 1.0)
    with pytest.raises(ValueError):
        ops.lora_qkv_fwd(x, qkv, A, B, ("output",), 1.0)
    pa, pb = _ptrs(A, ["query"]), _ptrs(B, ["query"])
    # targets 0 and 8, H not a multiple of 64, a target without matrices: -1 before any launch
    assert lib.mmbert_lora_qkv_fwd(_stream(), x.data_ptr(), H, qkv.data_ptr(), 3 * H, 4, H, 4, 0, pa, pb, 1.0, None, 0) == -1
    assert lib.mmbert_lora_qkv_fwd(_stream(), x.data_ptr(), H, qkv.data_ptr(), 3 * H, 4, H, 4, 8, pa, pb, 1.0, None, 0) == -1
    assert lib.mmbert_lora_qkv_fwd(_stream(), x.data_ptr(), 32, qkv.data_ptr(), 96, 4, 32, 4, 1, pa, pb, 1.0, None, 0) == -1
    assert lib.mmbert_lora_qkv_fwd(_stream(), x.data_ptr(), H, qkv.data_ptr(), 3 * H, 4, H, 4, 5, pa, pb, 1.0, None, 0) == -1
    # backward: in place on the residual gradient is refused; so is a missing workspace
    ws = torch.zeros(1 << 16, device=DEV)
    args = (_stream(), qkv.data_ptr(), 3 * H, x.data_ptr(), H, None, 0, 4, H, 4, 1, pa, pb, 1.0)
    assert lib.mmbert_lora_qkv_bwd(*args, x.data_ptr(), H, x.data_ptr(), H, None, None, 1, ws.data_ptr()) == -1
    assert lib.mmbert_lora_qkv_bwd(*args, None, 0, None, 0, None, None, 1, None) == -3
    torch.cuda.synchronize()
    assert not bool(qkv.any())
