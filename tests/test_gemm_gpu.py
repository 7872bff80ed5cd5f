"""The GEMM kernels (csrc/gemm.hip) against the float64 reference of tests/gemm_ref.py through ``gemm_ref.check``: every kernel form
forced (and asserted through mmbert_gemm_nt_describe), the static tile walk and the device tile queue, the model's production calls at
its packed row counts, the edge shapes, four input distributions, and canaries around every output, aux and W.  Dropout masks are
replayed from the library (ops.dropout_mask).  The largest ratios per operation are printed at the end of the module (``-s``)."""
import collections

import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
torch.set_num_threads(min(16, torch.get_num_threads()))
WORST = collections.defaultdict(lambda: [0.0, 0.0])


@pytest.fixture(scope="module")
def ops():
    from msa_amd import ops as o
    yield o
    if WORST:
        print("\nlargest ratios (elementwise, normwise):")
        for k in sorted(WORST):
            print(f"  {k:28s} {WORST[k][0]:.3f} {WORST[k][1]:.3f}")


@pytest.fixture(scope="module")
def lib(ops):
    from msa_amd import _lib
    return _lib.load()


def _record(op, r):
    w = WORST[op]
    w[0], w[1] = max(w[0], r.elem), max(w[1], r.norm)


class knobs:
    """Forced NT form, device tile queue, TN splits / one-launch mode and deterministic mode for a block, restored afterwards."""

    def __init__(self, ops, lib, nt=0, queue=False, splits=0, one_launch=False, det=None):
        self.ops, self.lib, self.nt, self.queue, self.splits, self.one, self.det = ops, lib, nt, queue, splits, one_launch, det

    def __enter__(self):
        self.q0, self.d0 = self.ops.dynamic_tile_queue, self.ops.deterministic()
        self.lib.mmbert_gemm_nt_force(self.nt)
        self.ops.dynamic_tile_queue = self.queue
        self.lib.mmbert_gemm_tn_force_splits(self.splits)
        self.lib.mmbert_gemm_tn_force_one_launch(1 if self.one else 0)
        if self.det is not None:
            self.ops.set_deterministic(self.det)

    def __exit__(self, *exc):
        self.lib.mmbert_gemm_nt_force(0)
        self.lib.mmbert_gemm_tn_force_splits(0)
        self.lib.mmbert_gemm_tn_force_one_launch(0)
        self.ops.dynamic_tile_queue = self.q0
        self.ops.set_deterministic(self.d0)


EPI = {"plain": 0, "bias": 1, "gelu": 3, "bias_resid_drop": 5, "resid": 4, "resid_drop": 4, "gelu_bwd": 8, "f32": 16, "bias_f32": 17}


def nt_call(ops, A, B, epi, *, seed=7, alpha=1.0, alpha_dev=None, rows=None, expect=None, a_pad=0, what=""):
    """One mmbert_gemm_nt call on CPU bf16 operands A [M,K], B [N,K] with epilogue ``epi``: output (and aux) inside canaries with
    8 padding columns, 2 rows before and 3 after; A as a view with ``a_pad`` extra columns (lda > K).  Checks the tile geometry the
    kernel ran against ``expect`` (dict of describe() fields), the values against the reference on ``rows`` (None: all rows, or a
    row subset by the tile height when M > 4096), and the canaries.  Returns the describe() dict."""
    M, K = A.shape
    N = B.shape[0]
    bias, R, U = G.epilogue_inputs(M, N, seed, need=("R",) if "resid" in epi else ("U",) if epi == "gelu_bwd" else ())
    drop = ops.make_drop(0.1, seed, 11) if epi in ("bias_resid_drop", "resid_drop") else None
    keep = ops.dropout_mask(M * N, drop, DEV).view(M, N).cpu() if drop else None
    f32 = epi in ("f32", "bias_f32")
    d = ops.gemm_nt_describe(M, N, K, epi=EPI[epi], with_queue=ops.dynamic_tile_queue)
    for k, v in (expect or {}).items():
        assert d[k] == v, (what, k, d)
    tile = tuple(int(x) for x in d["tile"].split("x"))
    if rows is None and M > 4096:
        rows = G.row_subset(M, tile[0], seed=M + N)
    Ab = torch.zeros(M, K + a_pad, dtype=torch.bfloat16)
    Ab[:, :K] = A
    Ad = Ab.to(DEV)[:, :K]
    out = G.Canary(M, N, torch.float32 if f32 else torch.bfloat16, DEV, pre=2, post=3, pad=8)
    aux = G.Canary(M, N, torch.bfloat16, DEV, pre=2, post=3, pad=8) if epi == "gelu" else None
    kw = dict(bias=bias.to(DEV) if epi in ("bias", "gelu", "bias_resid_drop", "bias_f32") else None, gelu=epi == "gelu",
              aux=aux.view if aux else None, resid=R.to(DEV) if "resid" in epi else None, gelu_bwd_u=U.to(DEV) if epi == "gelu_bwd" else None,
              alpha=alpha, alpha_dev=torch.tensor([alpha_dev], device=DEV) if alpha_dev is not None else None, drop=drop, out_f32=f32)
    ops.gemm_nt(Ad, B.to(DEV), out=out.view, **kw)
    torch.cuda.synchronize()
    ref = G.nt(A, B, bias=bias if kw["bias"] is not None else None, gelu=kw["gelu"], resid=R if kw["resid"] is not None else None,
               keep=keep, drop_scale=drop[2] if drop else 1.0, gelu_u=U if epi == "gelu_bwd" else None, alpha=alpha,
               alpha_dev=alpha_dev, out_f32=f32, rows=rows, tile=tile)
    label = f"nt {epi}"
    _record(label, G.check(out.view, ref["out"], f"{what} {epi} out"))
    out.intact(f"{what} {epi} out")
    if aux:
        _record("nt gelu aux", G.check(aux.view, ref["aux"], f"{what} aux"))
        aux.intact(f"{what} aux")
    return d


# ------------------------------------------------------------------------------------------------ every form, every epilogue
_FORMS = [(1, "128x128"), (8, None), (128, "128x256"), (192, "192x256"), (224, "224x256"), (256, "256x256")]


@pytest.mark.parametrize("mode,tile", _FORMS)
@pytest.mark.parametrize("dist", G.DISTS)
def test_every_form_every_epilogue(ops, lib, mode, tile, dist):
    """Each form of the NT kernels forced on a ragged single-round shape (M, N not tile multiples), every epilogue instantiation of
    the C ABI, on each input distribution; alpha and alpha_dev on the plain and fp32 forms."""
    M, N, K = 1150, 776, 768
    A, B = G.operands(M, N, K, dist, seed=mode)
    expect = {"kernel": "128x128" if mode == 1 else "8phase"}
    if tile:
        expect["tile"] = tile
    with knobs(ops, lib, nt=mode):
        for epi in EPI:
            a, ad = (0.75, 1.5) if epi in ("plain", "f32") else (1.0, None)
            nt_call(ops, A, B, epi, seed=len(epi), alpha=a, alpha_dev=ad, expect=expect, what=f"mode {mode} {dist}")


@pytest.mark.parametrize("mode", [192, 224, 256])
@pytest.mark.parametrize("queue", [False, True])
def test_multi_tile_form_static_walk_and_tile_queue(ops, lib, mode, queue):
    """The multi-tile form (more tiles than CUs) at each tile height, on the static walk and on the device tile queue."""
    M, N, K = 8013, 2304, 768
    A, B = G.operands(M, N, K, "real", seed=mode + queue)
    with knobs(ops, lib, nt=mode, queue=queue):
        d = nt_call(ops, A, B, "bias", expect={"kernel": "8phase", "tile": f"{mode}x256"}, what=f"multi {mode} queue {queue}")
        assert d["workgroups"] < d["tiles"], d
        nt_call(ops, A, B, "gelu", what=f"multi {mode} queue {queue}")


# ------------------------------------------------------------------------------------------------ production calls (msa_amd/model.py)
_FWD = [("qkv", 2304, 768, "bias"), ("wo", 768, 768, "bias_resid_drop"), ("w1", 3072, 768, "gelu"), ("w2", 768, 3072, "bias_resid_drop"),
        ("mlm_transform", 768, 768, "gelu")]
_BWD = [("du gelu'", 3072, 768, "gelu_bwd"), ("dy1 resid", 768, 3072, "resid"), ("dy resid", 768, 2304, "resid"), ("dctx", 768, 768, "plain")]


@pytest.mark.parametrize("M,queue", [(18400, False), (13850 - 37, True)])
def test_production_calls(ops, lib, M, queue):
    """The encoder's forward and backward products and the MLM transform at the packed row counts of the headline step, static
    walk at M = 18 400 and device tile queue at 13 813 (activations ~ N(0,1) against weights at BERT's 0.02)."""
    with knobs(ops, lib, queue=queue):
        for i, (name, N, K, epi) in enumerate(_FWD + _BWD):
            A, B = G.operands(M, N, K, "real", seed=100 + i)
            d = nt_call(ops, A, B, epi, seed=200 + i, expect={"kernel": "8phase"}, what=f"{name} M {M}")
            assert N == 768 or d["workgroups"] < d["tiles"], (name, d)         # (N = 768: one round of single tiles)


@pytest.mark.parametrize("M,queue", [(18400, False), (13850 - 37, True)])
def test_vocabulary_projection(ops, lib, M, queue):
    """logits = t . word^T + pred_bias at N = 30 592 (119 * 256 + 128: a half column tile at the end) in bf16 and in fp32, on the
    group_m = 4 walk of the multi-tile form."""
    N, K = 30592, 768
    A, B = G.operands(M, N, K, "real", seed=M)
    with knobs(ops, lib, queue=queue):
        for epi in ("bias", "bias_f32"):
            d = nt_call(ops, A, B, epi, expect={"kernel": "8phase", "group_m": 4}, what=f"vocab M {M}")
            assert d["workgroups"] < d["tiles"], d


def test_mlm_backward_few_row_products(ops, lib):
    """The MLM head's backward on the few hundred rows with a loss: dt = dl . word (split-K over K = 30 592), dpre . Wt^T into the
    first n rows of a larger buffer (rows after n must stay untouched), and the top layer's few-row du_c . W1^T + dz2_c in the
    split-K residual form."""
    n, M, V, H = 360, 1000, 30592, 768
    dl, wordT = G.operands(n, H, V, "real", seed=1)
    ref = G.splitk(dl, wordT)["out"]
    out = G.Canary(n, H, torch.bfloat16, DEV, pre=2, post=3, pad=8)
    ops.gemm_nt_splitk(dl.to(DEV), wordT.to(DEV), out=out.view)
    _record("splitk", G.check(out.view, ref, "dt split-K"))
    out.intact("dt split-K")
    # dpre . Wt^T -> dy_all[:n]
    dpre, WtT = G.operands(n, H, H, "real", seed=2)
    dy_all = G.Canary(M, H, torch.bfloat16, DEV)
    ops.gemm_nt(dpre.to(DEV), WtT.to(DEV), out=dy_all.view[:n])
    torch.cuda.synchronize()
    _record("nt plain", G.check(dy_all.view[:n], G.nt(dpre, WtT)["out"], "dy_all[:n]"))
    assert int((dy_all.view[n:].view(torch.int16) != G.NAN_BF16).sum()) == 0, "rows after n written"
    # du_c . W1T + dz2_c (split-K residual form), R with a row pitch != N
    for m in (391, 7):
        du_c, W1T = G.operands(m, H, 3072, "real", seed=3 + m)
        Rb = G.epilogue_inputs(m, H + 8, 4, need=("R",))[1]
        R = Rb[:, :H]
        out = G.Canary(m, H, torch.bfloat16, DEV, pre=2, post=3, pad=8)
        ops.gemm_nt_splitk(du_c.to(DEV), W1T.to(DEV), out=out.view, resid=Rb.to(DEV)[:, :H])
        _record("splitk resid", G.check(out.view, G.splitk(du_c, W1T, resid=R)["out"], f"du_c split-K resid m {m}"))
        out.intact("du_c split-K resid")


# ------------------------------------------------------------------------------------------------ edges
def _edge_cases():
    out = []
    for bm in (128, 192, 224, 256):
        for M in (3 * bm + 1, 3 * bm - 1):
            out.append((bm, M, 520, 256))
    out += [(256, 1, 520, 256), (0, 1, 520, 256), (0, 1, 4, 64), (1, 129, 4, 64), (1, 255, 8, 192), (0, 300, 132, 768), (0, 700, 132, 192),
            (0, 513, 264, 64), (0, 700, 776, 4096), (256, 600, 264, 4096), (224, 1000, 30592, 256)]
    return out


@pytest.mark.parametrize("mode,M,N,K", _edge_cases())
def test_edges(ops, lib, mode, M, N, K):
    """M = 1 and M = 1 / bm - 1 past a multiple of each tile height; N = 4, 8, 132 (N & 7 != 0: the 128 x 128 kernel) and a column
    tail at 30 592; K = 64 and 192 (K % 128 != 0: the 128 x 128 kernel), 256 (the 8-phase kernel's smallest) and long K; A as a
    view with lda > K."""
    A, B = G.operands(M, N, K, "real", seed=M + N + K)
    small = K % 128 != 0 or K < 256 or N % 8 != 0
    expect = {"kernel": "128x128"} if small or mode == 1 else ({"kernel": "8phase", "tile": f"{mode}x256"} if mode > 8 else {})
    with knobs(ops, lib, nt=mode):
        for epi in ("bias", "gelu", "bias_resid_drop", "gelu_bwd", "f32"):
            nt_call(ops, A, B, epi, a_pad=64, expect=expect, what=f"edge mode {mode} {M}x{N}x{K}")


# ------------------------------------------------------------------------------------------------ weight gradients
def _tn_splits(lib, M, N, K):
    """The token split mmbert_gemm_tn runs (forced or planned)."""
    import ctypes
    sp = ctypes.c_int(0)
    lib.mmbert_gemm_tn_workspace(M, N, K, ctypes.byref(sp))
    return sp.value


def _tn_operands(M, N, K, dist, seed):
    A, B = G.operands(N, K, M, dist, seed, wscale=1.0)
    g = torch.Generator().manual_seed(seed + 1)
    return A.t().contiguous(), B.t().contiguous(), torch.randn(N, K, generator=g), torch.randn(N, generator=g)


@pytest.mark.parametrize("splits,det", [(0, False), (3, False), (3, True), (8, True)])
@pytest.mark.parametrize("dist", ["real", "cancel", "scaled", "zeros"])
def test_gemm_tn(ops, lib, splits, det, dist):
    """W (+)= alpha * alpha_dev * A^T . B with the bias column sum, accumulate and overwrite, forced token splits (fp32 slabs reduced in
    split order), deterministic mode on and off, W inside a flat buffer of NaN canaries (the flat gradient buffer's views)."""
    M, N, K = 4129, 776, 520
    X, Y, W0, b0 = _tn_operands(M, N, K, dist, seed=splits + 10 * det)
    with knobs(ops, lib, splits=splits, det=det):
        for acc in (True, False):
            W = G.Canary(N, K, torch.float32, DEV, pre=40, post=72, flat=True, fill=W0 if acc else torch.full((N, K), float("nan")))
            bias = G.Canary(1, N, torch.float32, DEV, pre=1, post=1, pad=4, fill=b0[None])
            ops.gemm_tn(X.to(DEV), Y.to(DEV), W.view, accumulate=acc, alpha=0.5, alpha_dev=torch.tensor([1.5], device=DEV), bias_out=bias.view[0])
            torch.cuda.synchronize()
            ref = G.tn(X, Y, W0=W0, bias0=b0, with_bias=True, alpha=0.5, alpha_dev=1.5, accumulate=acc, splits=_tn_splits(lib, M, N, K))
            _record("tn W", G.check(W.view, ref["W"], f"W acc {acc}"))
            _record("tn bias", G.check(bias.view[0], ref["bias"], f"bias acc {acc}"))
            W.intact("W")
            bias.intact("bias")


def test_gemm_tn_at_the_headline_token_count(ops, lib):
    """A dense layer's weight gradient over 18 400 tokens (the cost model's own split count), W rows on a subset."""
    M, N, K = 18400, 768, 3072
    X, Y, W0, b0 = _tn_operands(M, N, K, "real", seed=5)
    W = G.Canary(N, K, torch.float32, DEV, pre=16, post=16, flat=True, fill=W0)
    bias = b0.clone().to(DEV)
    ops.gemm_tn(X.to(DEV), Y.to(DEV), W.view, accumulate=True, bias_out=bias)
    torch.cuda.synchronize()
    cols = G.row_subset(N, 256, seed=1)
    ref = G.tn(X, Y, W0=W0, bias0=b0, with_bias=True, cols=cols, splits=_tn_splits(lib, M, N, K))
    _record("tn W", G.check(W.view, ref["W"], "W"))
    _record("tn bias", G.check(bias, ref["bias"], "bias"))
    W.intact("W")


@pytest.mark.parametrize("one_launch", [False, True])
def test_gemm_tn_grouped_twelve_layers_then_few_rows(ops, lib, one_launch):
    """The deferred weight-gradient call: twelve layers' four dense problems over the same tokens, then the few-row problems (tied
    decoder, MLM transform, the top layer's FFN) riding in the last launch; per-problem accumulate flags, some W overwritten from NaN;
    every W inside its own NaN canary."""
    M = 2085
    shapes = [(2304, 768, M), (768, 768, M), (3072, 768, M), (768, 3072, M)] * 12 + [(30592, 768, 368), (768, 768, 368), (3072, 768, 391),
                                                                                    (768, 3072, 391)]
    assert len(shapes) <= ops.TN_MAX_PROBLEMS
    probs, cpu, flags, canaries, cols = [], [], [], [], []
    for i, (N, K, m) in enumerate(shapes):
        X, Y, W0, b0 = _tn_operands(m, N, K, "real", seed=300 + i)
        acc = i % 5 != 3
        b0 = b0 if i % 2 == 0 else None
        W = G.Canary(N, K, torch.float32, DEV, pre=8, post=8, flat=True, fill=W0 if acc else torch.full((N, K), float("nan")))
        probs.append((X.to(DEV), Y.to(DEV), W.view, b0.clone().to(DEV) if b0 is not None else None))
        cpu.append((X, Y, W0, b0))
        flags.append(acc)
        canaries.append(W)
        cols.append(G.row_subset(N, 256, seed=i, seeded=4))
    with knobs(ops, lib, one_launch=one_launch):
        ops.gemm_tn_grouped(probs, accumulate=flags)
        torch.cuda.synchronize()
    refs = G.tn_grouped(cpu, flags, cols=cols)
    for i, (p, r, W) in enumerate(zip(probs, refs, canaries)):
        _record("tn grouped W", G.check(p[2], r["W"], f"problem {i} {shapes[i]}"))
        if p[3] is not None:
            _record("tn grouped bias", G.check(p[3], r["bias"], f"problem {i} bias"))
        W.intact(f"problem {i}")


@pytest.mark.parametrize("det", [False, True])
def test_colsum(ops, lib, det):
    M, N = 18400, 776
    for dist in G.DISTS:
        X = G.operands(N, 8, M, dist, seed=9)[0].t().contiguous()
        out0 = torch.randn(N)
        out = out0.clone().to(DEV)
        with knobs(ops, lib, det=det):
            ops.colsum(X.to(DEV), out, alpha=0.5, alpha_dev=torch.tensor([3.0], device=DEV))
            torch.cuda.synchronize()
        ref = G.colsum(X, out0, alpha=0.5, alpha_dev=3.0, adds=G.colsum_adds(M, N, det))["out"]
        _record("colsum", G.check(out, ref, f"colsum {dist}"))
