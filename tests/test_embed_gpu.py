"""The embedding-stage kernels (csrc/rowwise.hip: embed_gather, embed_scatter with its type fold, id_runs_sum_rows, rows_to_block,
pair_proj_fwd, pair_wgrad + its reduce) against the float64 reference of tests/embed_ref.py through ``rowwise_ref.check``, run
through the C ABI (msa_amd.ops) in both deterministic modes, onto nonzero prior gradients (a second micro-batch): the headline's
2400 text rows with realistic ids ([CLS] at every position 0, [SEP], ~12 % [MASK], padding tails, id V - 1, ids out of range),
bert-large, the golden configurations, no token types, deferred word rows exchanged through rows_to_block, run sums over more than
one 8192-row launch; the pair projections at the headline (about 21 row ranges), in the fused 1050-row sequence, at every product
width the step runs and the tile edges around them, with fp32 and float64 features, zero rows and rows scaled by 2^+-10.  NaN
canaries surround every output; what a kernel must leave alone is checked bit for bit.  The largest ratios per output are printed
at the end of the module (``-s``)."""
import collections

import pytest
import torch

from tests import embed_ref as E
from tests.test_rowwise_gpu import det_mode

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
            print(f"  {k:12s} {WORST[k][0]:.3f} {WORST[k][1]:.3f}")


def _check(got, ref, op, what, gathered=False):
    r = E.check(got, ref, f"{what} {op}", gathered=gathered)
    w = WORST[op]
    w[0], w[1] = max(w[0], r.elem), max(w[1], r.norm)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _flat(t):
    """A fp32 prior inside a flat canary (16 elements before and after)."""
    return E.Canary(t.shape[0], t.shape[1], torch.float32, DEV, pre=16, post=16, flat=True, fill=t.to(DEV))


# ------------------------------------------------------------------------------------------------ gather and scatter
EMB = {
    "headline": dict(B=48, T=50, V=30522, H=768, Tpos=512),
    "bert-large": dict(B=32, T=40, V=30522, H=1024, Tpos=512),
    "golden H=128": dict(B=6, T=50, V=4096, H=128, Tpos=512),
    "golden H=64": dict(B=9, T=16, V=2048, H=64, Tpos=512),
    "no token types": dict(B=13, T=10, V=500, H=64, Tpos=64, tts=False),
    "long run": dict(B=192, T=50, V=30522, H=128, Tpos=512),
}


def emb_case(B, T, V, H, Tpos, tts=True, seed=5):
    ids, tt = E.make_ids(B, T, V, seed)
    word, typ, pos = E.make_tables(V, H, Tpos, seed + 1)
    d = E.make_d(B * T, H, seed + 2)
    g = torch.Generator().manual_seed(seed + 3)
    return dict(ids=ids, tts=tt if tts else None, word=word, typ=typ, pos=pos, T=T, d=d, V=V,
                gword0=0.5 * torch.randn(V, H, generator=g), gtype0=4.0 * torch.randn(2, H, generator=g),
                gpos0=2.0 * torch.randn(Tpos, H, generator=g))


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("name", list(EMB))
def test_gather_scatter(ops, name):
    c = emb_case(**EMB[name])
    ids, tts, T, V = c["ids"], c["tts"], c["T"], c["V"]
    n, H = c["d"].shape
    out = E.Canary(n, H, torch.bfloat16, DEV, pre=2, post=3, pad=8)
    ops.embed_gather(ids.to(DEV), _dev(tts), c["word"].to(DEV), c["typ"].to(DEV), c["pos"].to(DEV), T, out=out.view)
    torch.cuda.synchronize()
    _check(out.view, E.gather(ids, tts, c["word"], c["typ"], c["pos"], T), "gather", name)
    out.intact(f"{name} gather")
    valid = (ids > 0) & (ids < V)
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[ids[valid]] = False
    gpos = {}
    for det in (False, True):
        what = f"{name} det {det}"
        gw, gt, gp = _flat(c["gword0"]), _flat(c["gtype0"]), _flat(c["gpos0"])
        with det_mode(ops, det):
            ops.embed_scatter(ids.to(DEV), _dev(tts), c["d"].to(DEV), T, gw.view, gt.view, gp.view)
        torch.cuda.synchronize()
        ref = E.scatter(ids, tts, c["d"], T, c["gword0"], c["gtype0"], c["gpos0"], det=det)
        _check(gw.view, ref["gword"], "gword", what)
        _check(gt.view, ref["gtype"], "gtype", what)
        _check(gp.view, ref["gpos"], "gpos", what)
        assert torch.equal(gw.view[untouched.to(DEV)], c["gword0"][untouched].to(DEV)), f"{what}: a word row no id references changed"
        assert untouched[0]
        assert torch.equal(gp.view[T:], c["gpos0"][T:].to(DEV)), f"{what}: position rows >= T changed"
        for cn, nm in ((gw, "gword"), (gt, "gtype"), (gp, "gpos")):
            cn.intact(f"{what} {nm}")
        gpos[det] = gp.view.clone()
    assert torch.equal(gpos[False], gpos[True]), f"{name}: position sums differ between the modes (one adder per address in both)"


@pytest.mark.parametrize("det", [False, True])
def test_deferred_word_rows_through_rows_to_block(ops, det):
    """gword None: positions and token types only; the word rows leave through rows_to_block into a block over a union that also
    holds ids this batch never touches (other ranks')."""
    c = emb_case(**EMB["headline"])
    ids, tts, T, V = c["ids"], c["tts"], c["T"], c["V"]
    n, H = c["d"].shape
    valid = ids[(ids > 0) & (ids < V)]
    other = torch.randint(1, V, (300,), generator=torch.Generator().manual_seed(9))
    union = torch.unique(torch.cat([valid, other]))
    blk0 = torch.randn(union.numel(), H, generator=torch.Generator().manual_seed(10))
    gt, gp, blk = _flat(c["gtype0"]), _flat(c["gpos0"]), _flat(blk0)
    with det_mode(ops, det):
        ops.embed_scatter(ids.to(DEV), tts.to(DEV), c["d"].to(DEV), T, None, gt.view, gp.view, vocab=V)
        ops.rows_to_block(ids.to(DEV), c["d"].to(DEV), union.to(DEV), V, blk.view)
    torch.cuda.synchronize()
    what = f"deferred det {det}"
    ref = E.scatter(ids, tts, c["d"], T, None, c["gtype0"], c["gpos0"], V=V, det=det)
    _check(gt.view, ref["gtype"], "gtype", what)
    _check(gp.view, ref["gpos"], "gpos", what)
    _check(blk.view, E.rows_sum(ids, c["d"], blk0, V, union=union, det=det), "run sums", what)
    for cn, nm in ((gt, "gtype"), (gp, "gpos"), (blk, "block")):
        cn.intact(f"{what} {nm}")


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16])
def test_run_sums_across_launches(ops, src_dtype):
    """9600 rows: two launches of the ordered kernel, runs ([CLS], [MASK], repeated words) split across them; into the table
    (ops.scatter_add_rows_ordered) and into a union block (rows_to_block, both modes).  Ordered: the same bits twice."""
    B, T, V, H = 192, 50, 3000, 128
    ids, _ = E.make_ids(B, T, V, 31)
    g = torch.Generator().manual_seed(32)
    src = torch.randn(B * T, H, generator=g).to(src_dtype)
    dst0 = torch.randn(V, H, generator=g)
    union = torch.unique(ids[::3][(ids[::3] > 0) & (ids[::3] < V)])
    blk0 = torch.randn(union.numel(), H, generator=g)
    outs = []
    for rep in range(2):
        dst = _flat(dst0)
        ops.scatter_add_rows_ordered(ids.to(DEV), src.to(DEV), dst.view, V)
        torch.cuda.synchronize()
        _check(dst.view, E.rows_sum(ids, src, dst0, V, det=True), "run sums", f"table {src_dtype}")
        dst.intact("run sums table")
        outs.append(dst.view.clone())
    assert torch.equal(outs[0], outs[1])
    for det in (False, True):
        blk = _flat(blk0)
        with det_mode(ops, det):
            ops.rows_to_block(ids.to(DEV), src.to(DEV), union.to(DEV), V, blk.view)
        torch.cuda.synchronize()
        _check(blk.view, E.rows_sum(ids, src, blk0, V, union=union, det=det), "run sums", f"block det {det} {src_dtype}")
        blk.intact("run sums block")


# ------------------------------------------------------------------------------------------------ pair projections
def _pair_call(ops, f, W, b, *, B, P, T, H, pad=8, seq_len=None, offset=None, J=None, what=""):
    """Forward into a canary sequence matrix (or into ``J``, a Canary already holding other blocks); check the block, then that every
    other row kept what it held.  Returns the Canary and the reference."""
    rows_total = B * (seq_len if seq_len is not None else T + P)
    out = J or E.Canary(rows_total, H, torch.bfloat16, DEV, pre=2, post=2, pad=pad)
    before = out.view.clone()
    ops.pair_proj_fwd(f.to(DEV), W.to(DEV), b.to(DEV), out.view, T, seq_len=seq_len, offset=offset)
    torch.cuda.synchronize()
    rows = E.pair_rows(B, P, T, seq_len, offset)
    ref = E.pair_fwd(f, W, b, rows=rows)
    _check(out.view, ref, "pair out", what)
    zero = ~torch.isnan(ref.exact)
    assert not torch.signbit(out.view[rows.to(DEV)].float().cpu()[zero]).any(), f"{what}: a relu zero is -0"
    left = torch.ones(rows_total, dtype=torch.bool)
    left[rows] = False
    assert torch.equal(out.view[left.to(DEV)].view(torch.int16), before[left.to(DEV)].view(torch.int16)), f"{what}: rows outside the block changed"
    out.intact(what)
    return out, ref


def _pair_bwd(ops, f, Jv, dJv, dW0, db0, *, T, seq_len=None, offset=None):
    dW, db = _flat(dW0), _flat(db0[None, :])
    ops.pair_proj_bwd(f.to(DEV), Jv, dJv, T, dW.view, db.view[0], seq_len=seq_len, offset=offset)
    torch.cuda.synchronize()
    return dW, db


def _pair_case(ops, B, P, D, H, T, *, pad=8, dtype=torch.float32, seed=0, bwd=True, what=""):
    f, W, b = E.make_pair(B, P, D, H, 40 + seed, dtype=dtype)
    J, _ = _pair_call(ops, f, W, b, B=B, P=P, T=T, H=H, pad=pad, what=what)
    if not bwd:
        return
    g = torch.Generator().manual_seed(50 + seed)
    rows = E.pair_rows(B, P, T)
    dJ = E.Canary(J.view.shape[0], H, torch.bfloat16, DEV, pre=2, post=2, pad=pad)
    dJ.view[rows.to(DEV)] = torch.randn(rows.numel(), H, generator=g).to(torch.bfloat16).to(DEV)     # NaN outside the block
    dW0, db0 = 0.3 * torch.randn(H, D, generator=g), 0.3 * torch.randn(H, generator=g)
    res = {}
    for det in (False, True):
        with det_mode(ops, det):
            res[det] = _pair_bwd(ops, f, J.view, dJ.view, dW0, db0, T=T)
    ref = E.pair_bwd(f, J.view[rows.to(DEV)].cpu(), dJ.view[rows.to(DEV)].cpu(), dW0, db0, cus=_cus())
    dW, db = res[False]
    _check(dW.view, ref["dW"], "dW", what)
    _check(db.view[0], ref["db"], "db", what)
    for det, (a, c) in res.items():
        a.intact(f"{what} dW det {det}")
        c.intact(f"{what} db det {det}")
    again = _pair_bwd(ops, f, J.view, dJ.view, dW0, db0, T=T)
    for x in (res[True], again):
        assert torch.equal(x[0].view, dW.view) and torch.equal(x[1].view, db.view), f"{what}: backward not bit-identical"


@pytest.mark.parametrize("D", [35, 74])
def test_pair_headline(ops, D):
    B, P, T, H = 16, 500, 50, 768
    rp, S = E.pair_bwd_split(B * P, D, H, _cus())
    assert S > 1
    _pair_case(ops, B, P, D, H, T, seed=D, what=f"headline D={D} ({S} ranges)")


def test_pair_fused_sequence(ops):
    """S = 1050: text, visual at offset T (a negative base shift), speech at T + Pv.  Each forward leaves the text rows and the other
    modality's rows alone; each backward gives the same bits when every row outside its own block holds NaN."""
    B, T, Pv, Ps, H, Dv, Ds = 16, 50, 500, 500, 768, 35, 74
    S = T + Pv + Ps
    fv, Wv, bv = E.make_pair(B, Pv, Dv, H, 61, dtype=torch.float64)
    fs, Ws, bs = E.make_pair(B, Ps, Ds, H, 62, dtype=torch.float64)
    J = E.Canary(B * S, H, torch.bfloat16, DEV, pre=2, post=2)
    text = torch.arange(B * S) % S < T
    J.view[text.to(DEV)] = torch.randn(int(text.sum()), H, generator=torch.Generator().manual_seed(63)).to(torch.bfloat16).to(DEV)
    _pair_call(ops, fv, Wv, bv, B=B, P=Pv, T=T, H=H, seq_len=S, offset=T, J=J, what="fused visual")
    _pair_call(ops, fs, Ws, bs, B=B, P=Ps, T=T, H=H, seq_len=S, offset=T + Pv, J=J, what="fused speech")
    g = torch.Generator().manual_seed(64)
    dJ = torch.randn(B * S, H, generator=g).to(torch.bfloat16).to(DEV)
    for f, P, off, D, nm in ((fv, Pv, T, Dv, "visual"), (fs, Ps, T + Pv, Ds, "speech")):
        rows = E.pair_rows(B, P, T, S, off)
        dW0, db0 = 0.3 * torch.randn(H, D, generator=g), 0.3 * torch.randn(H, generator=g)
        full = _pair_bwd(ops, f, J.view, dJ, dW0, db0, T=T, seq_len=S, offset=off)
        ref = E.pair_bwd(f, J.view[rows.to(DEV)].cpu(), dJ[rows.to(DEV)].cpu(), dW0, db0, cus=_cus())
        _check(full[0].view, ref["dW"], "dW", f"fused {nm}")
        _check(full[1].view[0], ref["db"], "db", f"fused {nm}")
        own = torch.zeros(B * S, dtype=torch.bool)
        own[rows] = True
        Jn = torch.full_like(J.view, float("nan"))
        dJn = torch.full_like(dJ, float("nan"))
        Jn[own.to(DEV)], dJn[own.to(DEV)] = J.view[own.to(DEV)], dJ[own.to(DEV)]
        nan = _pair_bwd(ops, f, Jn, dJn, dW0, db0, T=T, seq_len=S, offset=off)
        assert torch.equal(nan[0].view, full[0].view) and torch.equal(nan[1].view, full[1].view), f"fused {nm}: rows outside the block read"


PAIR_SHAPES = ([dict(B=4, P=65, D=D, H=128) for D in (35, 47, 74, 81, 371, 1, 4, 5, 16, 17, 63, 64, 65, 79, 80, 127, 128, 129, 257)]
               + [dict(B=3, P=63, D=74, H=64), dict(B=3, P=63, D=35, H=200), dict(B=3, P=63, D=81, H=1024),
                  dict(B=32, P=40, D=74, H=1024, T=40), dict(B=32, P=40, D=35, H=1024, T=40)]
               + [dict(B=5, P=P, D=35, H=128) for P in (1, 63, 64, 65)]
               + [dict(B=4, P=65, D=74, H=128, pad=16), dict(B=4, P=65, D=74, H=128, pad=4, bwd=False),
                  dict(B=4, P=65, D=74, H=200, pad=2, bwd=False)]
               + [dict(B=4, P=65, D=D, H=128, dtype=torch.float64) for D in (35, 74, 371)])


def _pid(s):
    return "-".join(f"{k}{v if k != 'dtype' else str(v)[6:]}" for k, v in s.items())


@pytest.mark.parametrize("i", range(len(PAIR_SHAPES)), ids=[_pid(s) for s in PAIR_SHAPES])
def test_pair_shapes(ops, i):
    s = dict(PAIR_SHAPES[i])
    T = s.pop("T", 7)
    _pair_case(ops, s.pop("B"), s.pop("P"), s.pop("D"), s.pop("H"), T, seed=i, what=_pid(PAIR_SHAPES[i]), **s)
