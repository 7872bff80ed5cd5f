"""The vocabulary cross-entropy with label smoothing (csrc/rowwise.hip, mmbert_ce_fwd_smooth / mmbert_ce_bwd_smooth) through
``ops.ce_fwd`` / ``ops.ce_bwd(smoothing=)`` against the float64 reference of tests/loss_options_ref.py: 40 rows at (V, ldv) =
(30 522, 30 592), (1 000, 1 000) and (13, 16) -- a row that is mostly pad, where a pad column in the row sum or a -eps/V on a pad
column shows --, eps 0.1 and 0.5, bf16 and fp32 logits, 1 and 3 segments and 4 with an empty one, gscale 0 and negative, the
dense, the compact ``rows=`` and the in-place backward, deterministic mode on and off (bit-identical on repeat when on).  Inputs as
tests/test_rowwise_gpu.py's (pads above the row max, uniform and peaked rows, labels V and -1 among the ignored); the backward
writes into a NaN canary.  Unlabelled rows and pad columns must be exactly zero, eps = 0 through the new entry points must give
the old entry points' bits, and every refusal must return -1 with nothing written.  The largest ratios are printed at the end (``-s``)."""
import collections
import ctypes

import pytest
import torch

from tests import loss_options_ref as LR
from tests import rowwise_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
torch.set_num_threads(min(16, torch.get_num_threads()))
WORST = collections.defaultdict(lambda: [0.0, 0.0])
CASES = LR.ce_cases()


@pytest.fixture(scope="module")
def ops():
    from msa_amd import ops as o
    yield o
    if WORST:
        print("\nlargest ratios (elementwise, normwise):")
        for k in sorted(WORST):
            print(f"  {k:16s} {WORST[k][0]:.3f} {WORST[k][1]:.3f}")


def _check(got, ref, op, what):
    r = R.check(got, ref, f"{what} {op}")
    w = WORST[op]
    w[0], w[1] = max(w[0], r.elem), max(w[1], r.norm)


class det_mode:
    def __init__(self, ops, on):
        self.ops, self.on = ops, on

    def __enter__(self):
        self.was = self.ops.deterministic()
        self.ops.set_deterministic(self.on)

    def __exit__(self, *exc):
        self.ops.set_deterministic(self.was)


def _gs(nseg):
    return torch.tensor(LR.CE_GS)[:nseg]


def run_case(ops, V, ldv, eps, dtype, nseg, empty, seed, what):
    """Forward and the three backward forms of one case against the reference; returns (loss, inv, lse, dense dlogits)."""
    Xc, lab, bounds = LR.ce_inputs(V, ldv, nseg, empty, seed, dtype)
    X, labd, bd = Xc.to(DEV), lab.to(DEV), bounds.to(DEV)
    M = lab.numel()
    loss, inv, lse = ops.ce_fwd(X, V, labd, bd, nseg, smoothing=eps)
    torch.cuda.synchronize()
    ref = LR.ce_fwd(Xc, lab, V, bounds, nseg, eps)
    _check(loss, ref["loss"], "ce loss", what)
    _check(lse, ref["row_lse"], "ce row_lse", what)
    cnt = ref["count"].clamp(min=1).double()
    assert bool(((inv[:nseg].cpu().double() * cnt - 1.0).abs() <= 2.0 ** -23).all()), f"{what}: inv_count {inv[:nseg].cpu()} for counts {ref['count']}"
    if empty is not None:
        assert float(loss[empty]) == 0.0 and int(ref["count"][empty]) == 0
    gs = _gs(nseg)
    args = (Xc, lab, V, bounds, nseg, gs, lse.cpu(), eps)
    c = R.Canary(M, ldv, torch.bfloat16, DEV, pre=2, post=3, pad=64)
    ops.ce_bwd(X, V, labd, bd, nseg, inv, gs.to(DEV), lse, c.view, smoothing=eps)
    torch.cuda.synchronize()
    LR.ce_check_bwd(c.view, *args, count=ref["count"], what=what + " dense", worst=WORST)
    c.intact(what + " dense dlogits")
    dense = c.view.clone()
    rows = LR.ce_compact_rows(lab, V)
    k = rows.numel() - 2
    cc = R.Canary(rows.numel(), ldv, torch.bfloat16, DEV, pre=2, post=3, pad=64)
    ops.ce_bwd(X, V, labd, bd, nseg, inv, gs.to(DEV), lse, cc.view, rows=rows.to(DEV), smoothing=eps)
    torch.cuda.synchronize()
    LR.ce_check_bwd(cc.view, *args, rows=rows, count=ref["count"], what=what + " compact", worst=WORST)
    cc.intact(what + " compact dlogits")
    assert torch.equal(cc.view[:k], dense[rows[:k].long().to(DEV)]), f"{what}: compact rows differ from the dense form"
    if dtype == torch.bfloat16:
        out = X.clone()
        ops.ce_bwd(out, V, labd, bd, nseg, inv, gs.to(DEV), lse, out, smoothing=eps)
        torch.cuda.synchronize()
        assert torch.equal(out, dense), f"{what}: the in-place form differs from the dense one"
    return loss, inv[:nseg], lse, dense


@pytest.mark.parametrize("i", range(len(CASES)))
def test_ce_smooth_against_the_reference(ops, i):
    V, ldv, eps, dtype, nseg, empty, seed = CASES[i]
    with det_mode(ops, False):
        run_case(ops, V, ldv, eps, dtype, nseg, empty, seed, f"ce V {V} eps {eps} {dtype} nseg {nseg}")


@pytest.mark.parametrize("shape", LR.CE_SHAPES)
@pytest.mark.parametrize("eps", LR.CE_EPS)
def test_ce_smooth_deterministic_mode(ops, shape, eps):
    """The ordered loss sum (row_loss route) with the smoothed terms: within the same bounds, bit-identical on repeat, and on fp32 logits
    the bits of the bf16 path (the fp32 form rounds as it loads)."""
    V, ldv = shape
    with det_mode(ops, True):
        a = run_case(ops, V, ldv, eps, torch.bfloat16, 3, None, 7, f"ce det V {V} eps {eps}")
        b = run_case(ops, V, ldv, eps, torch.bfloat16, 3, None, 7, f"ce det V {V} eps {eps} again")
        f = run_case(ops, V, ldv, eps, torch.bfloat16, 4, 2, 9, f"ce det V {V} eps {eps} empty segment")
        Xc, lab, bounds = LR.ce_inputs(V, ldv, 3, None, 7, torch.bfloat16)
        X32 = Xc.float().to(DEV)
        loss, inv, lse = ops.ce_fwd(X32, V, lab.to(DEV), bounds.to(DEV), 3, smoothing=eps)
        dl = torch.empty(lab.numel(), ldv, device=DEV, dtype=torch.bfloat16)
        ops.ce_bwd(X32, V, lab.to(DEV), bounds.to(DEV), 3, inv, _gs(3).to(DEV), lse, dl, smoothing=eps)
    for x, y, z, nm in zip(a, b, (loss, inv[:3], lse, dl), ("loss", "inv_count", "row_lse", "dlogits")):
        assert torch.equal(x, y), f"deterministic mode: {nm} not bit-identical on repeat"
        assert torch.equal(x, z), f"deterministic mode: {nm} of the fp32-logits form differs from the bf16 form"
    assert float(f[0][2]) == 0.0


def _raw_args(ops, X, lab, bounds, nseg, V, inv, loss, lse, row_loss):
    from msa_amd.ops import _stream
    return (_stream(), X.data_ptr(), X.stride(0), V, lab.data_ptr(), lab.numel(), bounds.data_ptr(), nseg, inv.data_ptr(), loss.data_ptr(),
            lse.data_ptr(), 1 if X.dtype == torch.float32 else 0, None if row_loss is None else row_loss.data_ptr())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("det", [False, True])
def test_eps_zero_through_the_new_entry_points_is_the_old_code(ops, dtype, det):
    """mmbert_ce_fwd_smooth / mmbert_ce_bwd_smooth with smoothing = 0 run the unsmoothed instantiation: loss, lse and dlogits bit for bit
    those of mmbert_ce_fwd / mmbert_ce_bwd (deterministic mode for the loss: the atomic sum's bits depend on the arrival order)."""
    from msa_amd import _lib
    lib = _lib.load()
    V, ldv = LR.CE_SHAPES[0]
    Xc, lab, bounds = LR.ce_inputs(V, ldv, 3, None, 3, dtype)
    X, labd, bd = Xc.to(DEV), lab.to(DEV), bounds.to(DEV)
    M = lab.numel()
    gs = _gs(3).to(DEV)
    out = []
    with det_mode(ops, det):
        for smooth in (False, True):
            inv = torch.zeros(4, device=DEV)
            loss = torch.zeros(3, device=DEV)
            lse = torch.zeros(M, device=DEV)
            row_loss = torch.zeros(M, device=DEV)
            a = _raw_args(ops, X, labd, bd, 3, V, inv, loss, lse, row_loss)
            rc = lib.mmbert_ce_fwd_smooth(*a, 0.0) if smooth else lib.mmbert_ce_fwd(*a)
            assert rc == 0
            dl = torch.zeros(M, ldv, device=DEV, dtype=torch.bfloat16)
            b = a[:8] + (inv.data_ptr(), gs.data_ptr(), lse.data_ptr(), dl.data_ptr(), dl.stride(0), None, 0, a[11])
            rc = lib.mmbert_ce_bwd_smooth(*b, 0.0) if smooth else lib.mmbert_ce_bwd(*b)
            assert rc == 0
            torch.cuda.synchronize()
            out.append((loss, lse, dl, inv))
    names = ("loss", "row_lse", "dlogits", "inv_count")
    for x, y, nm in zip(out[0], out[1], names):
        if nm == "loss" and not det:
            continue
        assert torch.equal(x, y), f"smoothing = 0: {nm} differs from the old entry point's"
    l0, _, l1 = ops.ce_fwd(X, V, labd, bd, 3), None, ops.ce_fwd(X, V, labd, bd, 3, smoothing=0.0)
    assert torch.equal(l0[2], l1[2]) and torch.equal(l0[1][:3], l1[1][:3])          # (inv_count has 4 slots: nseg are written)


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf"), -1e-30])
def test_refusals_launch_nothing(ops, bad):
    """smoothing outside [0, 1) or not finite: -1 from both entry points, every output buffer still holds its canary; ops raises."""
    from msa_amd import _lib
    lib = _lib.load()
    V, ldv = LR.CE_SHAPES[1]
    Xc, lab, bounds = LR.ce_inputs(V, ldv, 3, None, 3, torch.bfloat16)
    X, labd, bd = Xc.to(DEV), lab.to(DEV), bounds.to(DEV)
    M = lab.numel()
    inv, loss, lse, row_loss = (R.canary_vec(n, torch.float32, DEV) for n in (4, 3, M, M))
    dl = R.Canary(M, ldv, torch.bfloat16, DEV, pre=2, post=3, pad=64)
    for det in (False, True):
        with det_mode(ops, det):
            a = _raw_args(ops, X, labd, bd, 3, V, inv.view, loss.view, lse.view, row_loss.view)
            assert lib.mmbert_ce_fwd_smooth(*a, ctypes.c_float(bad)) == -1
            ok_inv = torch.full((4,), 0.1, device=DEV)
            gs = _gs(3).to(DEV)
            zl = torch.zeros(M, device=DEV)
            b = a[:8] + (ok_inv.data_ptr(), gs.data_ptr(), zl.data_ptr(), dl.view.data_ptr(), dl.view.stride(0), None, 0, 0)
            assert lib.mmbert_ce_bwd_smooth(*b, ctypes.c_float(bad)) == -1
    torch.cuda.synchronize()
    for c, nm in ((inv, "inv_count"), (loss, "loss"), (lse, "row_lse"), (row_loss, "row_loss")):
        R.still_canary(c.buf, what=f"refused forward: {nm}")
    R.still_canary(dl.buf, what="refused backward: dlogits")
    with pytest.raises(ValueError):
        ops.ce_fwd(X, V, labd, bd, 3, smoothing=bad)
    with pytest.raises(ValueError):
        ops.ce_bwd(X, V, labd, bd, 3, ok_inv, gs, zl, dl.view, smoothing=bad)
    R.still_canary(dl.buf, what="refused ops.ce_bwd: dlogits")


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_torch_operator_with_label_smoothing(ops, eps):
    """torch.ops.mmbert.mlm_head_ce(logits, labels, vocab, label_smoothing) and its autograd formula (mlm_head_ce_fwd / _bwd with the
    trailing argument) against F.cross_entropy(label_smoothing=, ignore_index=-100) in float64 on the same bf16 logits: the loss within
    the reference's loss bound, the gradient through rowwise_ref's dlogits check; pad columns and unlabelled rows exactly zero."""
    import msa_amd.torch_ops  # noqa: F401
    V, ldv = LR.CE_SHAPES[1][0], 1008                                  # 8 pad columns
    Xc, lab, bounds = LR.ce_inputs(V, ldv, 1, None, 21, torch.bfloat16)
    X = Xc.to(DEV).requires_grad_(True)
    loss = torch.ops.mmbert.mlm_head_ce(X, lab.to(DEV), V, eps) if eps else torch.ops.mmbert.mlm_head_ce(X, lab.to(DEV), V)
    (loss * -1.5).backward()
    torch.cuda.synchronize()
    ref = LR.ce_fwd(Xc, lab, V, bounds, 1, eps)
    _check(loss.detach().reshape(1), ref["loss"], "ce loss", f"operator eps {eps}")
    X64 = Xc.double()[:, :V].clone().requires_grad_(True)
    labt = torch.where((lab >= 0) & (lab < V), lab, torch.full_like(lab, -100))
    want = torch.nn.functional.cross_entropy(X64, labt, label_smoothing=LR.eps32(eps), ignore_index=-100)
    assert abs(float(want.detach()) - float(ref["loss"].val[0])) <= 1e-12
    lse32 = ops.ce_fwd(X.detach(), V, lab.to(DEV), bounds.to(DEV), 1, smoothing=eps)[2].cpu()
    assert X.grad.dtype == torch.bfloat16 and X.grad.shape == X.shape
    LR.ce_check_bwd(X.grad, Xc, lab, V, bounds, 1, torch.tensor([-1.5]), lse32, eps, what=f"operator eps {eps}", worst=WORST)
    fwd = torch.ops.mmbert.mlm_head_ce_fwd(X.detach(), lab.to(DEV), V, eps)
    assert torch.equal(fwd[2].cpu(), lse32)                          # (row_lse is per row: the same bits; the loss is an atomic sum)
    _check(fwd[0].reshape(1), ref["loss"], "ce loss", f"operator forward eps {eps}")
