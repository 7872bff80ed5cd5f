"""The LayerNorm and cross-entropy kernels (csrc/layernorm.hip, csrc/rowwise.hip) against the float64 reference of tests/rowwise_ref.py through
``rowwise_ref.check``, run through the C ABI (msa_amd.ops): every LayerNorm width and both eps at the trip edges of the lean and
generic kernels, every reachable lean backward template, row maps and drop_row0 over several trips, the immediate, deferred and
ordered gamma / beta reduces; the cross-entropy at the model's vocabulary (V = 30 522, ldv = 30 592) with bf16 and fp32 logits,
labels at the chunk edges and in the pad, up to 4 segments (one empty), more than 8192 rows, the dense, compact and in-place
backward and deterministic mode.  NaN canaries surround every output; rows a map leaves out and mean / rstd past M must keep them
bit for bit.  Dropout masks are replayed from the library (ops.dropout_mask).  The largest ratios per output are printed at the end
of the module (``-s``)."""
import collections

import pytest
import torch

from tests import rowwise_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
torch.set_num_threads(min(16, torch.get_num_threads()))
WORST = collections.defaultdict(lambda: [0.0, 0.0])
V, LDV = 30522, 30592


@pytest.fixture(scope="module")
def ops():
    from msa_amd import ops as o
    yield o
    if WORST:
        print("\nlargest ratios (elementwise, normwise):")
        for k in sorted(WORST):
            print(f"  {k:16s} {WORST[k][0]:.3f} {WORST[k][1]:.3f}")


def _check(got, ref, op, what, gathered=False):
    r = R.check(got, ref, f"{what} {op}", gathered=gathered)
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


def _keep(ops, drop, rows, H):
    return ops.dropout_mask(rows * H, drop, DEV).view(rows, H).cpu() if drop else None


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd_call(ops, x, gamma, beta, eps, *, in_rows=None, out_rows=None, ny=None, drop=None, drop_row0=0, what=""):
    """One mmbert_ln_fwd call: y inside a canary (2 rows before, 3 after, 8 padding columns; ``ny`` rows when out_rows maps into a
    larger matrix), mean / rstd inside canaries.  Checks values, the canaries, and that rows out_rows leaves out are untouched.
    Returns (mean, rstd) on the device and the reference."""
    H = x.shape[1]
    M = in_rows.numel() if in_rows is not None else x.shape[0]
    ny = ny or M
    y = R.Canary(ny, H, torch.bfloat16, DEV, pre=2, post=3, pad=8)
    mean, rstd = R.canary_vec(M, torch.float32, DEV), R.canary_vec(M, torch.float32, DEV)
    ops.ln_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV), eps, M=M, out=y.view, in_rows=None if in_rows is None else in_rows.int().to(DEV),
               out_rows=None if out_rows is None else out_rows.int().to(DEV), drop=drop, stats=(mean.view[0], rstd.view[0]), drop_row0=drop_row0)
    torch.cuda.synchronize()
    keep = _keep(ops, drop, M + drop_row0, H)
    ref = R.ln_fwd(x, gamma, beta, eps, in_rows=in_rows, out_rows=out_rows, keep=keep, dscale=drop[2] if drop else 1.0, drop_row0=drop_row0)
    _check(y.view, ref["y"], "ln y", what)
    _check(mean.view[0], ref["mean"], "ln mean", what)
    _check(rstd.view[0], ref["rstd"], "ln rstd", what)
    for c, nm in ((y, "y"), (mean, "mean"), (rstd, "rstd")):
        c.intact(f"{what} {nm}")
    if out_rows is not None:
        left = torch.ones(ny, dtype=torch.bool)
        left[out_rows.long()] = False
        R.still_canary(y.view, left, f"{what} y rows out_rows leaves out")
    return mean.view[0].clone(), rstd.view[0].clone(), ref


def ln_bwd_call(ops, dy, x, mean, rstd, gamma, *, form=(False, False, False, False), post=None, pre=None, dy_rows=None, x_rows=None,
                dx_rows=None, ndx=None, drop_rows=None, drop_site_rows=None, dy_row_limit=0, deferred=None, grads=None, what=""):
    """One mmbert_ln_bwd call of the form (POST, DX2, PRE, dbias2): dx (``ndx`` rows when dx_rows maps into a larger matrix), dx2 and
    the gradient vectors (random start values) inside canaries.  Returns (grads, reference kwargs, dx canary, dx2 canary) -- the
    values are checked here unless ``deferred`` (the caller checks after the flush)."""
    po, d2, pr, b2 = form
    H = x.shape[1]
    M = mean.numel()
    ndx = ndx or M
    site = drop_site_rows or M
    g = torch.Generator().manual_seed(M + H)
    if grads is None:
        grads = [R.canary_vec(H, torch.float32, DEV, fill=torch.randn(H, generator=g)) for _ in range(3)]
    start = [c.view[0].cpu().clone() for c in grads]
    dx = R.Canary(ndx, H, torch.bfloat16, DEV, pre=2, post=3, pad=8)
    dx2 = R.Canary(M, H, torch.bfloat16, DEV, pre=2, post=3, pad=8) if d2 else None
    dev = lambda t: None if t is None else t.int().to(DEV)      # noqa: E731
    ops.ln_bwd(dy.to(DEV), x.to(DEV), mean, rstd, gamma.to(DEV), grads[0].view[0], grads[1].view[0], M=M, dx=dx.view,
               dx2=dx2.view if dx2 else None, dy_rows=dev(dy_rows), x_rows=dev(x_rows), dx_rows=dev(dx_rows),
               post_drop=post if po else None, pre_drop=pre if pr else None, dbias2=grads[2].view[0] if b2 else None,
               drop_rows=dev(drop_rows), deferred=deferred, dy_row_limit=dy_row_limit)
    torch.cuda.synchronize()
    kw = dict(dy_rows=dy_rows, x_rows=x_rows, dx_rows=dx_rows, drop_rows=drop_rows, dy_row_limit=dy_row_limit, dx2=d2, dbias2=b2,
              post_keep=_keep(ops, post, site, H) if po else None, post_scale=post[2] if po else 1.0,
              pre_keep=_keep(ops, pre, site, H) if pr else None, pre_scale=pre[2] if pr else 1.0,
              dgamma0=start[0], dbeta0=start[1], dbias20=start[2], adds=8)
    ref = R.ln_bwd(dy, x, mean.cpu(), rstd.cpu(), gamma, **kw)
    _check(dx.view, ref["dx"], "ln dx", what)
    dx.intact(f"{what} dx")
    if dx_rows is not None:
        left = torch.ones(ndx, dtype=torch.bool)
        left[dx_rows.long()] = False
        R.still_canary(dx.view, left, f"{what} dx rows not in dx_rows")
    if dx2:
        _check(dx2.view, ref["dx2"], "ln dx2", what)
        dx2.intact(f"{what} dx2")
    if not b2:
        assert torch.equal(grads[2].view[0].cpu().view(torch.int32), start[2].view(torch.int32)), f"{what}: dbias2 written"
    if deferred is None:
        check_grads(grads, ref, b2, what)
    return grads, ref


def check_grads(grads, ref, b2, what):
    for c, k in zip(grads, ("dgamma", "dbeta", "dbias2")):
        c.intact(f"{what} {k}")
        if k != "dbias2" or b2:
            _check(c.view[0], ref[k], "ln " + k, what)


ENC = (False, True, True, True)          # the encoder's form: dx2 with branch dropout, bias gradient, no post-LN dropout


@pytest.mark.parametrize("H", [64, 128, 200, 256, 512, 768, 1024])
@pytest.mark.parametrize("eps", [1e-12, 1e-5])
def test_ln_every_width(ops, H, eps):
    """Every width (lean NV = 1 .. 4, generic at 64, 128, 200), both eps, on the mixed rows (mean of 64 sigma, constant, tiny
    variance, 2^+-20, one outlier) and a realistic residual stream; forward, then the plain and the encoder's backward."""
    pre = ops.make_drop(0.1, 7, 3)
    for M, dist in ((3, "mixed"), (700, "mixed"), (1000, "real")):
        x, gamma, beta, dy = R.ln_inputs(M, H, dist, seed=H + M)
        what = f"H {H} eps {eps} M {M} {dist}"
        mean, rstd, _ = ln_fwd_call(ops, x, gamma, beta, eps, what=what)
        ln_bwd_call(ops, dy, x, mean, rstd, gamma, what=what)
        ln_bwd_call(ops, dy, x, mean, rstd, gamma, form=ENC, pre=pre, what=what + " encoder form")


TRIP_M = [1, 3, 4, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 13813, 18400]


@pytest.mark.parametrize("M", TRIP_M)
@pytest.mark.parametrize("H", [768, 200])
def test_ln_trip_edges(ops, M, H):
    """Row counts at the trip edges: the lean forward runs 4096 rows per trip (1024 workgroups x 4 waves), its backward 2048 (256 x 8),
    the generic kernels switch to two rows per wave at 8192 (H = 200); 13 813 and 18 400 are the model's packed row counts."""
    x, gamma, beta, dy = R.ln_inputs(M, H, "real", seed=M)
    pre = ops.make_drop(0.1, 11, 4)
    mean, rstd, _ = ln_fwd_call(ops, x, gamma, beta, 1e-12, what=f"M {M} H {H}")
    ln_bwd_call(ops, dy, x, mean, rstd, gamma, form=ENC, pre=pre, what=f"M {M} H {H}")


FORMS = {"FFF": (False, False, False, False), "TFF": (True, False, False, False), "FTT": (False, True, True, True),
         "FTF": (False, True, False, True), "TTT": (True, True, True, True), "dbias2 without dx2": (False, False, False, True)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("H", [768, 512, 128])
def test_ln_every_backward_template(ops, form, H):
    """Every lean backward template the C ABI reaches -- (POST, DX2, PRE) = FFF, TFF, FTT (the encoder's), FTF, TTT -- and a bias
    gradient without dx2, on 3000 mixed rows (two trips); H = 128: the generic kernel's same forms."""
    M = 3000
    x, gamma, beta, dy = R.ln_inputs(M, H, "mixed", seed=5)
    post, pre = ops.make_drop(0.1, 21, 5), ops.make_drop(0.1, 21, 6)
    mean, rstd, _ = ln_fwd_call(ops, x, gamma, beta, 1e-5, what=f"{form} H {H}")
    ln_bwd_call(ops, dy, x, mean, rstd, gamma, form=FORMS[form], post=post, pre=pre, what=f"{form} H {H}")


@pytest.mark.parametrize("H", [768, 256, 128])
def test_ln_row_maps_and_drop_row0_over_several_trips(ops, H):
    """The joint-embedding form at B*S = 8 800 rows: in_rows gathers, out_rows scatters into a larger matrix (the rows it leaves out keep
    their canary), the post-LN dropout drawn from row i + drop_row0 of its site; backward with dy_rows = out_rows, x_rows = in_rows,
    dx_rows into a larger matrix, drop_rows = i + drop_row0, dy_row_limit, and both dropouts, dx2 and dbias2."""
    M, n, r0 = 8800, 9500, 1000
    g = torch.Generator().manual_seed(H)
    x, gamma, beta, dy = R.ln_inputs(n, H, "real", seed=H)
    in_rows = torch.randperm(n, generator=g)[:M]
    out_rows = torch.randperm(n, generator=g)[:M]
    post, pre = ops.make_drop(0.1, 31, 7), ops.make_drop(0.1, 31, 8)
    what = f"maps H {H}"
    mean, rstd, _ = ln_fwd_call(ops, x, gamma, beta, 1e-12, in_rows=in_rows, out_rows=out_rows, ny=n, drop=post, drop_row0=r0, what=what)
    dx_rows = torch.randperm(n, generator=g)[:M]
    for form in (FORMS["TTT"], FORMS["TFF"]):
        ln_bwd_call(ops, dy, x, mean, rstd, gamma, form=form, post=post, pre=pre, dy_rows=out_rows, x_rows=in_rows, dx_rows=dx_rows,
                    ndx=n, drop_rows=torch.arange(M) + r0, drop_site_rows=M + r0, dy_row_limit=n - 700, what=f"{what} {form}")


@pytest.mark.parametrize("det", [False, True])
def test_ln_deferred_and_ordered_reduce_against_the_true_sums(ops, det):
    """LnDeferred over calls of different M (MLM head, the packed layers, a single row) folded by ONE reduce, two of them into one
    shared gradient (the joint LayerNorm's per-modality calls), against out0 + the float64 sums; deterministic mode: the ordered reduce,
    bit-identical on repeat."""
    H = 768
    Ms = [360, 8800, 37, 1, 4097]
    share = {1: 4}                                   # call 4 adds into call 1's gradients
    pre = ops.make_drop(0.1, 41, 9)
    calls = []
    for q, M in enumerate(Ms):
        x, gamma, beta, dy = R.ln_inputs(M, H, "real", seed=50 + q)
        calls.append((x, gamma, dy) + ln_fwd_call(ops, x, gamma, beta, 1e-12, what=f"deferred fwd {q}")[:2])
    results = []
    with det_mode(ops, det):
        for rep in range(2 if det else 1):
            ops._lnd_cache.clear()
            lnd = ops.LnDeferred(32)
            grads, starts, refs = {}, {}, []
            for q, (x, gamma, dy, mean, rstd) in enumerate(calls):
                owner = next((a for a, b in share.items() if b == q), q)
                gr, ref = ln_bwd_call(ops, dy, x, mean, rstd, gamma, form=ENC, pre=pre, deferred=lnd, grads=grads.get(owner),
                                      what=f"deferred {q} det {det}")
                if owner not in grads:
                    grads[owner], starts[owner] = gr, [c.view[0].cpu().double() for c in gr]
                refs.append((owner, ref))
            lnd.flush()
            torch.cuda.synchronize()
            for owner in sorted(grads):
                mine = [ref for o, ref in refs if o == owner]
                total = {}
                for j, k in enumerate(("dgamma", "dbeta", "dbias2")):
                    # every call's reference starts from the owner's values (nothing is folded before the flush): add their own sums
                    val = mine[0][k].val + sum(r[k].val - starts[owner][j] for r in mine[1:])
                    total[k] = R.Ref(val, sum(r[k].acc for r in mine), 0.0, R.U_F32)
                check_grads(grads[owner], total, True, f"deferred owner {owner} det {det}")
            results.append([c.view[0].clone() for o in sorted(grads) for c in grads[o]])
    if det:
        for a, b in zip(*results):
            assert torch.equal(a, b), "ordered reduce: not bit-identical on repeat"


# ------------------------------------------------------------------------------------------------ cross-entropy
def _bounds(M, nseg, empty=None):
    b = [0] + [M * (s + 1) // nseg for s in range(nseg)]
    if empty is not None:
        b[empty + 1] = b[empty]                       # segment ``empty`` holds no rows
    return torch.tensor(b, dtype=torch.int32)


def ce_inputs(M, nseg, seed, dtype=torch.bfloat16, frac=0.3, empty=None):
    """Logits on the device (pads above the row max, every third row uniform, every fifth labelled row peaked), labels with the edge
    columns, the pad and -1 first, segment bounds (optionally one empty segment)."""
    lab = R.ce_labels(M, V, LDV, seed, frac=frac)
    X = R.ce_logits(M, V, LDV, seed, kind="mixed", device=DEV, dtype=torch.float32)
    X = R.make_peaked(X, lab, V, torch.arange(0, M, 5))
    X[:, V:] = X[:, :V].max(1, keepdim=True).values + 4.0
    return X.to(dtype), lab, _bounds(M, nseg, empty)


def ce_check_fwd(ops, X, lab, bounds, nseg, what):
    M = lab.numel()
    loss, inv, lse = ops.ce_fwd(X, V, lab.to(DEV), bounds.to(DEV), nseg)
    torch.cuda.synchronize()
    ref = R.ce_fwd(lambda r: X[r.to(DEV)].cpu(), lab, V, bounds, nseg)
    _check(loss, ref["loss"], "ce loss", what)
    _check(lse, ref["row_lse"], "ce row_lse", what)
    # inv_count = 1 / max(1, count) within an fp32 ulp (the kernel's division is the fast-math reciprocal): one label more or less
    # moves it by 1 / count, thousands of ulps
    cnt = ref["count"].clamp(min=1).double()
    off = (inv[:nseg].cpu().double() * cnt - 1.0).abs()
    assert bool((off <= 2.0 ** -23).all()), f"{what}: inv_count {inv[:nseg].cpu()} for counts {ref['count']}"
    assert lse.numel() == M
    return loss, inv, lse, ref


def ce_check_bwd(ops, X, lab, bounds, nseg, inv, gs, lse, what, rows=None, count=None, inplace=False):
    """Dense (or compact ``rows``) backward inside a canary (2 rows before, 3 after, 64 columns past ldv); labelled rows against the
    reference, every other row and every pad column exactly zero.  Returns the output."""
    n = rows.numel() if rows is not None else lab.numel()
    if inplace:
        out = X.clone()
        ops.ce_bwd(out, V, lab.to(DEV), bounds.to(DEV), nseg, inv, gs.to(DEV), lse, out)
        dl = out
    else:
        c = R.Canary(n, LDV, torch.bfloat16, DEV, pre=2, post=3, pad=64)
        ops.ce_bwd(X, V, lab.to(DEV), bounds.to(DEV), nseg, inv, gs.to(DEV), lse, c.view, rows=None if rows is None else rows.to(DEV))
        dl = c.view
    torch.cuda.synchronize()
    src = torch.arange(n) if rows is None else rows.long()
    labelled = (lab[src] >= 0) & (lab[src] < V)
    for j, ref in R.ce_bwd(lambda r: X[r.to(DEV)].cpu(), lab, V, bounds, nseg, gs, lse.cpu(), rows=rows, count=count):
        _check(dl[j.to(DEV)], ref, "ce dlogits", what, gathered=True)
    zero_rows = dl[(~labelled).to(DEV)]
    assert int((zero_rows.view(torch.int16) != 0).sum()) == 0, f"{what}: unlabelled rows of dlogits not exactly zero"
    if not inplace:
        c.intact(f"{what} dlogits")
    return dl


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("nseg,empty", [(1, None), (2, None), (3, None), (4, 2)])
def test_ce_at_the_vocabulary(ops, dtype, nseg, empty):
    """V = 30 522 in rows of 30 592 (15 chunks of 8 per thread column, the last valid chunk 2 real + 6 pad columns): loss, row_lse and
    inv_count, then the dense backward with gscale 0 and negative, the compact rows= backward (the labelled rows plus two unlabelled
    ones) and, for bf16, the in-place form.  An empty segment's loss is the kernel's documented 0 (torch's mean over no rows is NaN)."""
    M = 600
    X, lab, bounds = ce_inputs(M, nseg, seed=nseg, dtype=dtype, empty=empty)
    what = f"ce {dtype} nseg {nseg}"
    loss, inv, lse, ref = ce_check_fwd(ops, X, lab, bounds, nseg, what)
    if empty is not None:
        assert float(loss[empty]) == 0.0 and int(ref["count"][empty]) == 0
        nan = torch.nn.functional.cross_entropy(torch.zeros(0, 4), torch.zeros(0, dtype=torch.long))
        assert torch.isnan(nan), "torch's mean over no rows"
    gs = torch.tensor([0.5, -2.0, 0.0, 1.25])[:nseg]
    dense = ce_check_bwd(ops, X, lab, bounds, nseg, inv, gs, lse, what + " dense", count=ref["count"])
    act, cnt = ops.active_rows(lab.to(DEV), V)
    k = int(cnt)
    rows = torch.cat([act[:k].cpu(), torch.tensor([0, 2], dtype=torch.int32)]).int()     # (rows 0 and 2 carry ignored labels: V and -1)
    assert int(lab[0]) == V and int(lab[2]) == -1
    comp = ce_check_bwd(ops, X, lab, bounds, nseg, inv, gs, lse, what + " compact", rows=rows, count=ref["count"])
    assert torch.equal(comp[:k], dense[act[:k].long()]), f"{what}: compact rows differ from the dense form"
    if dtype == torch.bfloat16:
        inplace = ce_check_bwd(ops, X, lab, bounds, nseg, inv, gs, lse, what + " in place", count=ref["count"], inplace=True)
        assert torch.equal(inplace, dense), f"{what}: in-place form differs"


@pytest.mark.parametrize("det", [False, True])
def test_ce_more_than_8192_rows(ops, det):
    """18 400 rows (the model's dense MLM path; three trips of ce_count_kernel's and ce_loss_sum_ordered_kernel's 8192-row loops), 15 %
    labelled, three segments; deterministic mode: the ordered loss sum, bit-identical on repeat."""
    M, nseg = 18400, 3
    X, lab, bounds = ce_inputs(M, nseg, seed=77, frac=0.15)
    with det_mode(ops, det):
        loss, inv, lse, ref = ce_check_fwd(ops, X, lab, bounds, nseg, f"ce 18400 det {det}")
        gs = torch.tensor([1.0, -0.5, 2.0])
        dl = ce_check_bwd(ops, X, lab, bounds, nseg, inv, gs, lse, f"ce 18400 det {det}", count=ref["count"])
        if det:
            loss2, inv2, lse2 = ops.ce_fwd(X, V, lab.to(DEV), bounds.to(DEV), nseg)
            assert torch.equal(loss, loss2) and torch.equal(lse, lse2) and torch.equal(inv[:nseg], inv2[:nseg])
            dl2 = torch.empty_like(dl)
            ops.ce_bwd(X, V, lab.to(DEV), bounds.to(DEV), nseg, inv, gs.to(DEV), lse, dl2)
            assert torch.equal(dl2, dl)


def test_ce_fp32_logits_halfway_between_bf16_neighbours(ops):
    """fp32 logits placed exactly halfway between two bf16 neighbours (and a tenth of them left as they are): the fp32 path rounds them
    to bf16 as it loads them, so it must give the bits of the bf16 path on logits.to(bfloat16) (round to nearest, ties to even).  In
    deterministic mode: the atomic loss sum's bits depend on the arrival order."""
    M, nseg = 300, 2
    X, lab, bounds = ce_inputs(M, nseg, seed=5, dtype=torch.float32)
    b = X.to(torch.bfloat16)
    up = (b.view(torch.int16) + 1).view(torch.bfloat16)                  # the next bf16 away from zero (finite: |X| << max)
    half = ((b.float().double() + up.float().double()) / 2).float()      # exact in fp32
    X = torch.where(torch.rand(X.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6)) < 0.9, half, X)
    X[:, V:] = X[:, :V].max(1, keepdim=True).values + 4.0
    Xb = X.to(torch.bfloat16)
    assert bool(((Xb.view(torch.int16) & 1) == 0)[half == X].all()), "ties must round to even"
    gs = torch.tensor([1.5, -1.0])
    out = {}
    with det_mode(ops, True):
        for name, L in (("f32", X), ("bf16", Xb)):
            loss, inv, lse, _ = ce_check_fwd(ops, L, lab, bounds, nseg, f"halfway {name}")
            dl = torch.empty(M, LDV, device=DEV, dtype=torch.bfloat16)
            ops.ce_bwd(L, V, lab.to(DEV), bounds.to(DEV), nseg, inv, gs.to(DEV), lse, dl)
            out[name] = (loss, inv[:nseg], lse, dl)
    for a, b_, nm in zip(out["f32"], out["bf16"], ("loss", "inv_count", "row_lse", "dlogits")):
        assert torch.equal(a, b_), f"fp32 logits: {nm} differs from the bf16 path"
