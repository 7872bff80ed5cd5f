"""The pretraining heads against the float64 reference of tests/heads_ref.py through ``heads_ref.check``, element by element and per
sample row: the level-launch form (csrc/heads_coop.hip, model._HeadsStepFn) at every batch edge up to 128 and the K-split edges of
the hidden size, and the 19-launch form (csrc/heads.hip, model._HeadsFn) up to its 32 samples in both deterministic modes.  Every
call runs with an upstream gradient d != 1 in most cases, random prior gradients in the whole flat gradient buffer (every word
outside the heads' 22 parameter views must keep its bits), the level-launch workspace filled with NaN before the forward, and the
loss level's counter words checked back at zero.  The skinny products of the 19-launch form (mmbert_skinny_mm, its ordered form
and mmbert_skinny_wgrad) against float64 products at M up to 128, inner sizes 1, 2 and 768 and odd N, inside NaN canaries.  The
largest ratios per output, and the case of each, are printed at the end (``-s``)."""
import ctypes

import pytest
import torch

from tests import heads_ref as HR

pytestmark = pytest.mark.gpu

DEV = "cuda"
torch.set_num_threads(min(16, torch.get_num_threads()))
WORST = {}
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest ratios per output (elementwise, normwise; the case of each):")
        for k in sorted(WORST):
            w = WORST[k]
            print(f"  {k:28s} {w[0]:.3f} {w[1]:.3f}   {w[2]} | {w[3]}")


def _model(H, num_labels):
    key = (H, num_labels)
    if key not in _MODELS:
        from tests.test_model_gpu import build
        cfg = dict(hidden=H, layers=1, heads=1, intermediate=4 * H, vocab=512, dataset="mosei")
        m = build(cfg)
        m.num_labels = num_labels
        m._ensure_ready(torch.device(DEV, 0))
        _MODELS[key] = m
    return _MODELS[key]


def _load(m, c):
    """The case's parameters, alpha / beta, and its prior gradients in a flat gradient buffer otherwise filled with random words.
    Returns (snapshot of the buffer, mask of the words outside the heads' views)."""
    m.set_alpha_beta(c.alpha, c.beta)
    params = dict(m.named_parameters())
    with torch.no_grad():
        for n, t in c.params.items():
            params[n].copy_(t.to(DEV))
    m.parameters_changed()
    g = m._flat.grads
    g.copy_(torch.randn(g.numel(), generator=torch.Generator().manual_seed(c.B * 7 + c.H)).to(DEV))
    outside = torch.ones(g.numel(), dtype=torch.bool, device=DEV)
    for n in HR.PARAMS:
        o = (params[n].grad.data_ptr() - g.data_ptr()) // 4
        k = params[n].numel()
        params[n].grad.copy_(c.prior[n].to(DEV))
        outside[o:o + k] = False
    return g.clone(), outside


class _NanWorkspace:
    """ops.heads_step_workspace hands out NaN-filled buffers: a read of a word no level wrote shows."""

    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        self.orig = self.ops.heads_step_workspace
        self.ops.heads_step_workspace = lambda B, H, dev, _o=self.orig: _o(B, H, dev).fill_(float("nan"))

    def __exit__(self, *exc):
        self.ops.heads_step_workspace = self.orig


def _run(c, form="step", model_form=False, det=False):
    from msa_amd import model as MM, ops
    m = _model(c.H, c.num_labels)
    snap, outside = _load(m, c)
    B, H = c.B, c.H
    ap_v, ap_s, sent = c.ap_v.to(DEV), c.ap_s.to(DEV), c.sent.to(DEV)
    mlm = c.mlm.to(DEV).requires_grad_(True) if c.nmlm else None
    was = ops.deterministic()
    ops.set_deterministic(det)
    try:
        with _NanWorkspace(ops):
            if form == "launches":
                f = c.first.to(DEV).requires_grad_(True)
                loss, aux, logits, t_rel, rel = MM._HeadsFn.apply(f, m, torch.cat((ap_v, ap_s)), sent, mlm)
            elif model_form:
                # the model's form: rows read from a bf16 encoder output (row stride != H) through a non-monotonic row list
                ld = H + 48
                y = torch.randn(5 * B + 7, ld, generator=torch.Generator().manual_seed(B)).to(torch.bfloat16).to(DEV)
                rows = torch.randperm(5 * B + 7, generator=torch.Generator().manual_seed(B + 1))[:3 * B].to(DEV)
                y[rows, :H] = c.first.to(torch.bfloat16).to(DEV)
                y = y[:, :H]
                f = torch.empty(3 * B, H, device=DEV).requires_grad_(True)
                loss, aux, logits, t_rel, rel = MM._HeadsStepFn.apply(f, m, (ap_v, ap_s), sent, mlm, (y, rows))
            else:
                f = c.first.to(DEV).requires_grad_(True)
                loss, aux, logits, t_rel, rel = MM._HeadsStepFn.apply(f, m, torch.cat((ap_v, ap_s)), sent, mlm)
            out5 = loss.grad_fn.keep[-1] if form == "step" else None      # (ctx.keep ends with the out5 record)
            loss.backward(torch.tensor(c.d, device=DEV))
            MM._join_heads(m)
            torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    for t in ops._heads_sync.values():
        assert int(t.abs().sum()) == 0, "the loss level's counter words are not back at zero"
    g = m._flat.grads
    assert torch.equal(g[outside].view(torch.int32), snap[outside].view(torch.int32)), \
        f"{int((g[outside].view(torch.int32) != snap[outside].view(torch.int32)).sum())} words outside the heads' views changed"
    params = dict(m.named_parameters())
    got = dict(loss=loss.detach(), aux=aux, logits=logits, t_rel=t_rel, rel=rel, dfirst=f.grad)
    if out5 is not None:
        got["out5"] = out5
    if mlm is not None:
        got["dmlm"] = mlm.grad
    for n in HR.PARAMS:
        got[n] = params[n].grad.detach().clone()
    return got


def _case_check(c, what, **kw):
    exp = HR.expected(c)
    got = _run(c, **kw)
    HR.check_all(got, exp, what, WORST)


# (B, H): every B meets at least two H; H: the K-split edges (16 waves x 16-deep granules) and the ABI's minimum
STEP = [(1, 16), (1, 768), (2, 64), (2, 1024), (3, 80), (3, 256), (15, 192), (15, 320), (16, 768), (16, 80), (17, 64), (17, 320),
        (31, 256), (31, 16), (32, 1024), (32, 192), (33, 80), (33, 768), (48, 256), (48, 64), (63, 320), (63, 16), (64, 192), (64, 1024),
        (65, 80), (65, 256), (127, 64), (127, 768), (128, 256), (128, 16)]
DS = (1.0, -0.37, 2.0 ** 10)
NMLM = (0, 3, 256)


@pytest.mark.parametrize("i", range(len(STEP)))
def test_level_launch_heads(i):
    B, H = STEP[i]
    c = HR.make_case(B, H, 100 + i, num_labels=(1, 7)[i % 2], alpha=0.6, beta=0.7 if i % 5 else 1.3, nmlm=NMLM[(i // 3) % 3], d=DS[i % 3],
                     ap=("mixed", "zeros", "ones", "mixed")[i % 4])
    _case_check(c, f"step B={B} H={H}")


@pytest.mark.parametrize("B,H", [(1, 64), (17, 768), (32, 1024), (128, 256), (65, 80)])
def test_level_launch_heads_in_the_models_form(B, H):
    """Rows from a bf16 y with row stride != H through a non-monotonic row list, MLM losses set: the backward runs on the heads'
    side stream and is joined as _MLMHeadFn.backward joins it."""
    c = HR.make_case(B, H, 7 + B, num_labels=7, alpha=0.8, beta=0.6, nmlm=3, d=-0.37)
    _case_check(c, f"model form B={B} H={H}", model_form=True)


def test_level_launch_heads_at_beta_zero_have_exactly_zero_cpc_gradients():
    c = HR.make_case(17, 64, 5, beta=0.0, nmlm=0, d=2.0 ** 10)
    got = _run(c)
    for m in range(3):
        for w in ("weight", "bias"):
            n = f"{HR.CPCS[m]}.{w}"
            assert torch.equal(got[n].cpu(), c.prior[n]), n
    HR.check_all(got, HR.expected(c), "beta=0", WORST)


def _step_record(m, B, H, seed):
    """A complete argument record of the level-launch heads for B samples on the H-wide model ``m`` -- forward AND backward
    pointers (dloss, dfirst, every parameter gradient) -- whose buffers are sized for B and for the model's width.  Returns (record,
    the output and dfirst tensors, everything to keep alive)."""
    from msa_amd import model as MM
    g = torch.Generator().manual_seed(seed)
    first = torch.randn(3 * B, m.config.hidden_size, generator=g).to(DEV)
    ap, sent = torch.randint(0, 2, (2 * B,), generator=g).to(DEV), (torch.rand(B, generator=g) * 6 - 3).to(DEV)
    a, outs, keep = MM._HeadsStepFn._setup(m, B, m.config.hidden_size, torch.device(DEV, 0), ap, sent, first=first)
    dloss = torch.ones(1, device=DEV)
    dfirst = torch.full_like(first, float("nan"))
    a.dloss, a.dfirst = dloss.data_ptr(), dfirst.data_ptr()
    pool, al, at, c1, c2 = m.bert.pooler.dense, m.cls.align, m.attn, m.classifier1_1, m.classifier1_2
    a.gWp, a.gbp, a.gWal, a.gbal = (t.grad.data_ptr() for t in (pool.weight, pool.bias, al.weight, al.bias))
    a.gWat, a.gbat, a.gWc1, a.gbc1, a.gWc2, a.gbc2 = (t.grad.data_ptr() for t in (at.weight, at.bias, c1.weight, c1.bias, c2.weight, c2.bias))
    for q, (v, cp) in enumerate(zip((m.vt, m.vv, m.vs), (m.cpc_zt.net, m.cpc_zv.net, m.cpc_za.net))):
        a.gvw[q], a.gvb[q], a.gWq[q], a.gbq[q] = (t.grad.data_ptr() for t in (v.weight, v.bias, cp.weight, cp.bias))
    for t in outs:
        t.fill_(float("nan"))
    return a, list(outs) + [dfirst], (first, ap, sent, keep, dloss)


def test_level_launch_heads_refuse_what_they_cannot_run():
    """B = 129 and H % 16 != 0 (or H < 16) are refused by both C entry points before any launch: -1, the outputs, dfirst and the whole
    flat gradient buffer keep their bits.  Each record is otherwise complete -- the same record at B = 128 / H = 64 is accepted, forward
    and backward -- and its buffers are sized for the refused shape (B = 129 rows; widths below the model's 64), so a check that
    stopped refusing would fail this test without a store out of range."""
    from msa_amd import ops, _lib
    m = _model(64, 7)
    _load(m, HR.make_case(4, 64, 3))
    lib = _lib.load()
    stream = ops._stream()
    for (B, H), ok in (((129, 64), (128, 64)), ((4, 56), (4, 64)), ((4, 8), (4, 64))):
        a, outs, keep = _step_record(m, B, H, seed=B + H)
        a.B, a.H = B, H
        snap = m._flat.grads.clone()
        assert lib.mmbert_heads_step_fwd_levels(stream, ctypes.addressof(a), 1, 7) == -1, (B, H)
        assert lib.mmbert_heads_step_bwd_levels(stream, ctypes.addressof(a), 1, 6) == -1, (B, H)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in outs), (B, H)
        assert torch.equal(m._flat.grads.view(torch.int32), snap.view(torch.int32)), (B, H)
        a.B, a.H = ok
        assert lib.mmbert_heads_step_fwd_levels(stream, ctypes.addressof(a), 1, 7) == 0, ok
        assert lib.mmbert_heads_step_bwd_levels(stream, ctypes.addressof(a), 1, 6) == 0, ok
        torch.cuda.synchronize()
        assert bool(torch.isfinite(outs[0]).all()) and bool(torch.isfinite(outs[-1][:3 * ok[0]]).all()), ok


LAUNCHES = [(B, H) for B in (1, 2, 15, 16, 17, 31, 32) for H in (64, 768, 1024)]


@pytest.mark.parametrize("i", range(len(LAUNCHES)))
@pytest.mark.parametrize("det", [False, True])
def test_multi_launch_heads(i, det):
    B, H = LAUNCHES[i]
    c = HR.make_case(B, H, 300 + i, num_labels=(7, 1)[i % 2], alpha=0.6, beta=0.7, nmlm=NMLM[(i // 3) % 3], d=DS[(i + det) % 3])
    _case_check(c, f"launches B={B} H={H} det={det}", form="launches", det=det)


# ------------------------------------------------------------------------------------------------ the skinny products (csrc/heads.hip)
SK_M = (1, 17, 127, 128)
SK_INNER = (1, 2, 768)
SK_N = (3, 769)


def _sk_operands(M, inner, N, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, inner, generator=g) * torch.exp2(torch.randint(-8, 9, (M, 1), generator=g).float())
    W = torch.randn(N, inner, generator=g) / max(1.0, inner ** 0.5)
    return X, W, torch.randn(N, generator=g), torch.randn(M, N, generator=g)


def _sk_ref(val, S, T, adds):
    """The bound of a skinny product: S = sum|a b| (the 64-deep fma chains, F_SUM S as in heads_ref), T = |start| + |bias| + S bounds
    every intermediate of the ``adds`` roundings that add chunk partials, bias and start value in whatever order the atomics or the
    fold take (each at most half an ulp of T)."""
    return HR.Ref(val, HR.F_SUM * S + adds * T + val.abs(), 0.0, HR.U_F32)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("wim", [0, 1])
@pytest.mark.parametrize("inner", SK_INNER)
@pytest.mark.parametrize("M", SK_M)
def test_skinny_mm_against_float64(M, inner, wim, det):
    """mmbert_skinny_mm (fp32 atomics of 64-deep chunks) and, in deterministic mode, mmbert_skinny_mm_ordered (a slab of chunk partials
    folded in order): Y = Y0 + bias + X op(W) + X2 op(W2) over rows row0 .. M of the second source, W as [N, inner] (wim = 0) or
    [inner, N] (wim = 1), at odd N; Y inside a NaN canary (2 rows before, 3 after, 5 padding columns) that must keep its bits."""
    from msa_amd import ops
    from tests.gemm_ref import Canary
    for N in SK_N:
        X, W, bias, Y0 = _sk_operands(M, inner, N, seed=M * 1000 + inner * 10 + N + wim)
        r0 = M // 3
        X2, W2, _, _ = _sk_operands(M - r0, 2, N, seed=M + N + 7)
        Wk, W2k = (W.t().contiguous(), W2.t().contiguous()) if wim else (W, W2)
        y = Canary(M, N, torch.float32, DEV, pre=2, post=3, pad=5, fill=Y0.to(DEV))
        was = ops.deterministic()
        ops.set_deterministic(det)
        try:
            ops.skinny_mm([(y.view, bias.to(DEV), 0, True, [(X.to(DEV), Wk.to(DEV), wim, 0), (X2.to(DEV), W2k.to(DEV), wim, r0)])])
            torch.cuda.synchronize()
        finally:
            ops.set_deterministic(was)
        y.intact(f"skinny_mm M={M} inner={inner} N={N}")
        f64 = torch.float64
        X, W, X2, W2, bias, Y0 = (t.to(f64) for t in (X, W, X2, W2, bias, Y0))
        lower, lower_abs = torch.zeros(M, N, dtype=f64), torch.zeros(M, N, dtype=f64)
        lower[r0:], lower_abs[r0:] = X2 @ W2.t(), X2.abs() @ W2.abs().t()
        val = Y0 + bias + X @ W.t() + lower
        S = X.abs() @ W.abs().t() + lower_abs
        adds = (inner + 63) // 64 + 1 + 1                      # the chunk partials of both sources, the bias, the start value
        ref = _sk_ref(val, S, Y0.abs() + bias.abs() + S, adds)
        HR.check_all({"skinny_mm": y.view}, {"skinny_mm": ref}, f"M={M} inner={inner} N={N} wim={wim} det={det}", WORST)


@pytest.mark.parametrize("K", SK_INNER)
@pytest.mark.parametrize("M", SK_M)
def test_skinny_wgrad_against_float64(M, K):
    """mmbert_skinny_wgrad: dW += dY^T X and db += column sums of dY onto nonzero prior values, at odd N, the 64-row LDS blocks' edge
    (M = 127, 128), K = 1 and 2 (scalar stores) and K = 768; two ops in one launch, dW / db inside NaN canaries."""
    from msa_amd import ops
    from tests.gemm_ref import Canary
    ops_list, refs, views = [], {}, {}
    for N in SK_N:
        g = torch.Generator().manual_seed(M * 100 + K + N)
        dY = torch.randn(M, N, generator=g)
        X = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-8, 9, (M, 1), generator=g).float())
        W0, b0 = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        cw = Canary(N, K, torch.float32, DEV, pre=1, post=2, pad=3, fill=W0.to(DEV))
        cb = Canary(1, N, torch.float32, DEV, pre=16, post=16, flat=True, fill=b0.reshape(1, N).to(DEV))
        ops_list.append((dY.to(DEV), X.to(DEV), cw.view, cb.view.reshape(N)))
        f64 = torch.float64
        dY, X, W0, b0 = (t.to(f64) for t in (dY, X, W0, b0))
        # one fma chain over the M rows per element (its roundings a random walk: sqrt(M) S), then one add onto the prior value
        chain = 2.0 + M ** 0.5
        Sw, Sb = dY.abs().t() @ X.abs(), dY.abs().sum(0)
        refs[f"dW N={N}"] = HR.Ref(W0 + dY.t() @ X, chain * Sw + 2 * (W0.abs() + Sw), 0.0, HR.U_F32)
        refs[f"db N={N}"] = HR.Ref(b0 + dY.sum(0), chain * Sb + 2 * (b0.abs() + Sb), 0.0, HR.U_F32)
        views[f"dW N={N}"], views[f"db N={N}"] = (cw, cw.view), (cb, cb.view.reshape(N))
    ops.skinny_wgrad(ops_list)
    torch.cuda.synchronize()
    for k, (can, v) in views.items():
        can.intact(f"skinny_wgrad M={M} K={K} {k}")
        HR.check_all({"skinny_wgrad " + k.split()[0]: v}, {"skinny_wgrad " + k.split()[0]: refs[k]}, f"M={M} K={K} {k}", WORST)
