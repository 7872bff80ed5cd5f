"""The level-launch heads with a C-CLASS label head (csrc/heads_coop.hip, ``ncls`` = C) against the float64 reference of
tests/heads_cls_ref.py through ``heads_ref.check``, element by element and per row, in the mould of tests/test_heads_gpu.py: C in
(2, 3, 6, 16) over the batch and hidden-size edges, both input forms (fp32 rows; bf16 encoder rows with a row stride != H through a
non-monotonic row list), an upstream gradient d != 1 in most cases, random prior gradients in the whole flat gradient buffer (every
word outside the heads' 22 parameter views keeps its bits), a NaN-filled workspace, the loss level's counter words back at zero, and
``pred`` equal to the float64 argmax on EVERY sample (the cases keep every sample's two largest logits 64 bounds apart:
tests/test_heads_cls_reference_cpu.py).  ``mmbert_heads_predict`` with ``ncls`` > 0 against forward levels 1 - 5 of the step, bit for
bit, and in chunks; what the ABI refuses; and the regression instantiation untouched by the new fields.  The largest ratios per
output, and the case of each, are printed at the end (``-s``)."""
import ctypes

import pytest
import torch

from tests import heads_cls_ref as HCR
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


def _model(H, C):
    """An H-wide model with a C-class head (C = 0: the regression model, num_labels 7)."""
    key = (H, C)
    if key not in _MODELS:
        from tests.test_model_gpu import build
        m = build(dict(hidden=H, layers=1, heads=1, intermediate=4 * H, vocab=512, dataset="mosei"))
        if C:
            m.set_num_labels(C)
        m._ensure_ready(torch.device(DEV, 0))
        _MODELS[key] = m
    return _MODELS[key]


def _load(m, c):
    """tests/test_heads_gpu.py's: the case's parameters and prior gradients in a flat gradient buffer otherwise filled with random words."""
    m.set_alpha_beta(c.alpha, c.beta)
    params = dict(m.named_parameters())
    with torch.no_grad():
        for n, t in c.params.items():
            assert params[n].shape == t.shape, n
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
    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        self.orig = self.ops.heads_step_workspace
        self.ops.heads_step_workspace = lambda B, H, dev, _o=self.orig: _o(B, H, dev).fill_(float("nan"))

    def __exit__(self, *exc):
        self.ops.heads_step_workspace = self.orig


def _run(c, model_form=False):
    from msa_amd import model as MM, ops
    m = _model(c.H, c.C)
    snap, outside = _load(m, c)
    B, H = c.B, c.H
    ap_v, ap_s, y = c.ap_v.to(DEV), c.ap_s.to(DEV), c.y.to(DEV)
    mlm = c.mlm.to(DEV).requires_grad_(True) if c.nmlm else None
    with _NanWorkspace(ops):
        if model_form:
            ld = H + 48
            yy = torch.randn(5 * B + 7, ld, generator=torch.Generator().manual_seed(B)).to(torch.bfloat16).to(DEV)
            rows = torch.randperm(5 * B + 7, generator=torch.Generator().manual_seed(B + 1))[:3 * B].to(DEV)
            yy[rows, :H] = c.first.to(torch.bfloat16).to(DEV)
            yy = yy[:, :H]
            f = torch.empty(3 * B, H, device=DEV).requires_grad_(True)
            loss, aux, logits, t_rel, rel = MM._HeadsStepFn.apply(f, m, (ap_v, ap_s), y, mlm, (yy, rows))
        else:
            f = c.first.to(DEV).requires_grad_(True)
            loss, aux, logits, t_rel, rel = MM._HeadsStepFn.apply(f, m, torch.cat((ap_v, ap_s)), y, mlm)
        pred = loss.grad_fn.keep[-2]
        out5 = loss.grad_fn.keep[-1]
        loss.backward(torch.tensor(c.d, device=DEV))
        MM._join_heads(m)
        torch.cuda.synchronize()
    for t in ops._heads_sync.values():
        assert int(t.abs().sum()) == 0, "the loss level's counter words are not back at zero"
    g = m._flat.grads
    assert torch.equal(g[outside].view(torch.int32), snap[outside].view(torch.int32)), \
        f"{int((g[outside].view(torch.int32) != snap[outside].view(torch.int32)).sum())} words outside the heads' views changed"
    assert logits.shape == (B, c.C) and pred.shape == (B,) and pred.dtype == torch.int64
    params = dict(m.named_parameters())
    got = dict(loss=loss.detach(), aux=aux, out5=out5, logits=logits, t_rel=t_rel, rel=rel, dfirst=f.grad, pred=pred)
    if mlm is not None:
        got["dmlm"] = mlm.grad
    for n in HR.PARAMS:
        got[n] = params[n].grad.detach().clone()
    return got


@pytest.mark.parametrize("i", range(len(HCR.GPU_STEP)))
def test_level_launch_class_heads(i):
    c = HCR.gpu_step_case(i)
    HCR.check_all(_run(c), HCR.expected(c), f"cls step B={c.B} H={c.H} C={c.C}", WORST)


@pytest.mark.parametrize("i", range(len(HCR.GPU_MODEL_FORM)))
def test_level_launch_class_heads_in_the_models_form(i):
    c = HCR.gpu_model_form_case(i)
    HCR.check_all(_run(c, model_form=True), HCR.expected(c), f"cls model form B={c.B} H={c.H} C={c.C}", WORST)


# ------------------------------------------------------------------------------------------------ records built by hand
def _record(m, B, seed, ncls, labels=True):
    """A complete argument record (forward and backward pointers) for B samples on the model ``m``; returns (record, dict of the
    output tensors, everything to keep alive).  ``ncls`` = 0: the regression record."""
    from msa_amd import model as MM, ops
    H = m.config.hidden_size
    g = torch.Generator().manual_seed(seed)
    first = torch.randn(3 * B, H, generator=g).to(DEV)
    ap = torch.randint(0, 2, (2 * B,), generator=g).to(DEV)
    sent = (torch.rand(B, generator=g) * 6 - 3).to(DEV)
    y = torch.randint(0, max(ncls, 2), (B,), generator=g).to(DEV)
    a = ops.heads_step_struct()
    a.B, a.H, a.alpha, a.beta = B, H, 0.6, 0.7
    a.first, a.ap = first.data_ptr(), ap.data_ptr()
    MM._HeadsStepFn._set_params(m, a)
    a.ncls = ncls
    f32 = dict(device=DEV, dtype=torch.float32)
    o = dict(loss=torch.empty(1, **f32), aux=torch.empty(3, **f32), out5=torch.empty(5, **f32), logits=torch.empty(B, max(ncls, 1), **f32),
             t_rel=torch.empty(B, 2, **f32), rel=torch.empty(2 * B, 2, **f32), dfirst=torch.empty(3 * B, H, **f32))
    for t in o.values():
        t.fill_(float("nan"))
    o["pred"] = torch.full((B,), -7, device=DEV, dtype=torch.int64)
    ws = ops.heads_step_workspace(B, H, torch.device(DEV, 0))
    a.loss, a.aux, a.out5, a.logits, a.t_rel, a.rel, a.ws = (t.data_ptr() for t in (o["loss"], o["aux"], o["out5"], o["logits"], o["t_rel"], o["rel"], ws))
    a.sync = ops.heads_step_sync(torch.device(DEV, 0)).data_ptr()
    if ncls == 0:
        a.sent = sent.data_ptr()
    if labels:
        a.sent_cls, a.pred = y.data_ptr(), o["pred"].data_ptr()
    dloss = torch.ones(1, device=DEV)
    a.dloss, a.dfirst = dloss.data_ptr(), o["dfirst"].data_ptr()
    pool, al, at, c1, c2 = m.bert.pooler.dense, m.cls.align, m.attn, m.classifier1_1, m.classifier1_2
    a.gWp, a.gbp, a.gWal, a.gbal = (t.grad.data_ptr() for t in (pool.weight, pool.bias, al.weight, al.bias))
    a.gWat, a.gbat, a.gWc1, a.gbc1, a.gWc2, a.gbc2 = (t.grad.data_ptr() for t in (at.weight, at.bias, c1.weight, c1.bias, c2.weight, c2.bias))
    for q, (v, cp) in enumerate(zip((m.vt, m.vv, m.vs), (m.cpc_zt.net, m.cpc_zv.net, m.cpc_za.net))):
        a.gvw[q], a.gvb[q], a.gWq[q], a.gbq[q] = (t.grad.data_ptr() for t in (v.weight, v.bias, cp.weight, cp.bias))
    return a, o, (first, ap, sent, y, ws, dloss)


def _scaled_head(m, seed):
    """Head weights at a scale where the logits are spread (the HF initialisation leaves them a few 1e-2 wide)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, q in m.named_parameters():
            if n in HR.PARAMS or n in HR.FWD_ONLY:
                q.copy_((torch.randn(q.shape, generator=g) * ((1.0 if q.dim() > 1 else 0.1) / (q.shape[-1] ** 0.5 if q.dim() > 1 else 1.0))).to(DEV))
    m.parameters_changed()


@pytest.mark.parametrize("C,H", [(2, 64), (6, 256), (16, 80)])
def test_predict_entry_point_equals_forward_levels_1_to_5(C, H):
    """mmbert_heads_predict with ncls > 0: raw logits [B, C], pred, t_rel, rel and the workspace's P / T bit-identical to the step's
    forward at the same inputs (which runs the same level kernels), and a batch of 300 in chunks of 128 equal to its three chunks."""
    from msa_amd import model as MM, ops, _lib
    m = _model(H, C)
    _scaled_head(m, C * 100 + H)
    lib, stream = _lib.load(), ops._stream()
    for B in (1, 17, 128):
        a, o, keep = _record(m, B, seed=B + C, ncls=C)
        assert lib.mmbert_heads_step_fwd_levels(stream, ctypes.addressof(a), 1, 7) == 0
        torch.cuda.synchronize()
        step = {k: v.clone() for k, v in o.items()}
        Ps, Ts = (t.clone() for t in ops.heads_step_outputs(keep[4], B, H))
        assert bool(torch.isfinite(step["logits"]).all()) and int(step["pred"].min()) >= 0 and int(step["pred"].max()) < C
        assert torch.equal(step["pred"], step["logits"].argmax(1))              # (no ties at these inputs)
        b, ob, keepb = _record(m, B, seed=B + C, ncls=C, labels=False)
        b.pred = ob["pred"].data_ptr()
        b.ap = b.sent = b.loss = b.aux = b.out5 = b.sync = b.dloss = b.dfirst = None
        assert lib.mmbert_heads_predict(stream, ctypes.addressof(b)) == 0
        torch.cuda.synchronize()
        for k in ("logits", "t_rel", "rel"):
            assert torch.equal(ob[k].view(torch.int32), step[k].view(torch.int32)), (B, k)
        assert torch.equal(ob["pred"], step["pred"]), B
        Pp, Tp = ops.heads_step_outputs(keepb[4], B, H)
        assert torch.equal(Pp.view(torch.int32), Ps.view(torch.int32)) and torch.equal(Tp.view(torch.int32), Ts.view(torch.int32))
    # B = 300 through _HeadsStepFn.predict (chunks of 128) = its three chunks
    B = 300
    y = torch.randn(3 * B, H, generator=torch.Generator().manual_seed(C)).to(torch.bfloat16).to(DEV)
    whole = MM._HeadsStepFn.predict(m, y, B)
    assert len(whole) == 7 and whole[0].shape == (B, C) and whole[6].shape == (B,) and whole[6].dtype == torch.int64
    for b0 in range(0, B, 128):
        n = min(128, B - b0)
        yc = torch.cat([y[mm * B + b0:mm * B + b0 + n] for mm in range(3)]).contiguous()
        part = MM._HeadsStepFn.predict(m, yc, n)
        for i in range(7):
            w = whole[i][:, b0:b0 + n] if i == 4 else whole[i][b0:b0 + n]
            assert torch.equal(w, part[i]), (b0, i)


def test_class_head_abi_refusals():
    """ncls = 1, 17, -1, and ncls = 2 with a null sent_cls or pred, are refused by every entry point before any launch: -1, the outputs,
    dfirst and the whole flat gradient buffer keep their bits.  The same record with ncls = 2 and both pointers is accepted."""
    from msa_amd import ops, _lib
    m = _model(64, 2)
    lib, stream = _lib.load(), ops._stream()
    B = 4
    for ncls, drop in ((1, None), (17, None), (-1, None), (2, "sent_cls"), (2, "pred")):
        a, o, keep = _record(m, B, seed=11, ncls=2)
        a.ncls = ncls
        if drop:
            setattr(a, drop, None)
        snap = m._flat.grads.clone()
        assert lib.mmbert_heads_step_fwd_levels(stream, ctypes.addressof(a), 1, 7) == -1, (ncls, drop)
        assert lib.mmbert_heads_step_bwd_levels(stream, ctypes.addressof(a), 1, 6) == -1, (ncls, drop)
        if drop != "sent_cls":                                      # (prediction reads no labels)
            assert lib.mmbert_heads_predict(stream, ctypes.addressof(a)) == -1, (ncls, drop)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for k, t in o.items() if k != "pred") and bool((o["pred"] == -7).all()), (ncls, drop)
        assert torch.equal(m._flat.grads.view(torch.int32), snap.view(torch.int32)), (ncls, drop)
    a, o, keep = _record(m, B, seed=11, ncls=2)
    assert lib.mmbert_heads_step_fwd_levels(stream, ctypes.addressof(a), 1, 7) == 0
    assert lib.mmbert_heads_step_bwd_levels(stream, ctypes.addressof(a), 1, 6) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o["loss"]).all()) and bool(torch.isfinite(o["dfirst"]).all()) and int(o["pred"].min()) >= 0


def test_out_of_range_labels_stay_in_bounds():
    """A label outside [0, C) is clamped: nothing is read or written out of range -- the logits, pred and every other sample's seed
    are those of the in-range run, and the clamped sample's loss is that of the nearest class."""
    from msa_amd import ops, _lib
    m = _model(64, 6)
    _scaled_head(m, 3)
    lib, stream = _lib.load(), ops._stream()
    B = 5
    outs = []
    for labels in ((0, 5, 5, 0, 3), (-4, 5, 1 << 40, 0, 3)):
        a, o, keep = _record(m, B, seed=2, ncls=6)
        keep[3].copy_(torch.tensor(labels, dtype=torch.int64))
        assert lib.mmbert_heads_step_fwd_levels(stream, ctypes.addressof(a), 1, 7) == 0
        torch.cuda.synchronize()
        outs.append({k: v.clone() for k, v in o.items() if k != "dfirst"})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_regression_is_untouched_by_the_new_fields():
    """ncls = 0: one call with sent_cls / pred null and one with them pointing at canary-filled buffers give bit-identical outputs and
    gradients, and the canaries keep their bits."""
    from msa_amd import ops, _lib
    m = _model(64, 0)
    lib, stream = _lib.load(), ops._stream()
    B = 17
    g0 = torch.randn(m._flat.grads.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)
    res = []
    for with_ptrs in (False, True):
        m._flat.grads.copy_(g0)
        a, o, keep = _record(m, B, seed=5, ncls=0, labels=False)
        can_y = torch.full((B + 32,), 0x5A5A5A5A5A5A5A5A, device=DEV, dtype=torch.int64)
        can_p = can_y.clone()
        if with_ptrs:
            a.sent_cls, a.pred = can_y[16:].data_ptr(), can_p[16:].data_ptr()
        assert lib.mmbert_heads_step_fwd_levels(stream, ctypes.addressof(a), 1, 7) == 0
        assert lib.mmbert_heads_step_bwd_levels(stream, ctypes.addressof(a), 1, 6) == 0
        torch.cuda.synchronize()
        assert bool((can_y == 0x5A5A5A5A5A5A5A5A).all()) and bool((can_p == 0x5A5A5A5A5A5A5A5A).all())
        assert bool(torch.isfinite(o["loss"]).all()) and bool(torch.isfinite(o["dfirst"]).all())
        res.append(({k: v.clone() for k, v in o.items() if k != "pred"}, m._flat.grads.clone()))
    for k in res[0][0]:
        assert torch.equal(res[0][0][k].view(torch.int32), res[1][0][k].view(torch.int32)), k
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
    assert not torch.equal(res[0][1], g0)
