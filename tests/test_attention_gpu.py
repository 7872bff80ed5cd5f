"""The attention kernels (csrc/attention.hip) against the float64 reference of tests/attention_ref.py, every (sequence, head)
block of every output through ``attention_ref.check``: at the edge lengths packed together, at the model's head counts and
production shapes (full tensor, guide rule 26), on every packed layout the model uses, with the top layer's query limit, with a
forced rescale of the running maximum, plus the exact zeros of masked keys and the dropout index scheme.  Dropout masks are
replayed from the library (mmbert_attn_dropout_mask)."""
import math

import pytest
import torch

from tests import attention_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from msa_amd import ops as o
    return o


def _masks(ops, layout, lens, heads, drop, perm_pos=None):
    """Per sequence the kernels' [heads, S, S] keep mask (CPU uint8); ``perm_pos`` (per sequence: kernel position of every
    original position) maps a row-set packing's masks back to the original order."""
    if drop[1] == 0:
        return None
    out = []
    for s, S in enumerate(lens):
        m = torch.stack([ops.attn_dropout_mask(S, layout.elem_base_host[s], h, drop, DEV) for h in range(heads)])
        if perm_pos is not None:
            r = perm_pos[s].to(DEV)
            m = m[:, r][:, :, r]
        out.append(m.cpu())
    return out


def _kernel(ops, qkv, kb, layout, H, drop, dctx=None, kv_len=None, q_limit=None, dqkv=None):
    ctx, lse = ops.attn_fwd(qkv, kb, layout, H, drop=drop, kv_len=kv_len)
    d = None
    if dctx is not None:
        d = ops.attn_bwd(qkv, ctx, dctx, lse, kb, layout, H, drop=drop, kv_len=kv_len, q_limit=q_limit, dqkv=dqkv)
    torch.cuda.synchronize()
    return ctx, lse, d


def _masked_key_zeros(d, bias, lens, H):
    """dK and dV of every key masked with -10000 are bitwise 0 when its sequence has an unmasked key."""
    s0 = 0
    d = d.cpu()
    for S in lens:
        b = bias[s0:s0 + S]
        if bool((b > A.MASKED).any()) and bool((b <= A.MASKED).any()):
            rows = s0 + (b <= A.MASKED).nonzero().reshape(-1)
            assert float(d[rows, H:].float().abs().max()) == 0.0, f"sequence at row {s0}: masked keys with non-zero dK / dV"
        s0 += S
    return d


# ---------------------------------------------------------------------------------------------- edge lengths
@pytest.mark.parametrize("use_kv", [False, True], ids=["dense", "kv_len"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("heads", [1, 3, 12, 16])
def test_edge_lengths_packed_together(ops, heads, p, use_kv):
    """S in {1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257} in one launch; every key-bias pattern (none, 20 %
    random, masked tail ending inside a tile / on a tile boundary, only key 0 unmasked, fully masked) lands on different lengths
    for every head count."""
    lens, H = A.EDGE_LENS, heads * 64
    pats = [A.PATTERNS[(i + heads) % len(A.PATTERNS)] for i in range(len(lens))]
    qkv, bias, dctx = A.make_inputs(lens, heads, pats, seed=100 + heads)
    layout = ops.SeqLayout(lens, heads, DEV)
    drop = ops.make_drop(p, 1234 + heads, 3)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    kv = ops.attn_kv_len(kb, layout) if use_kv else None
    ctx, lse, d = _kernel(ops, qkv.to(DEV), kb, layout, H, drop, dctx.to(DEV), kv_len=kv)
    ref = A.reference(qkv, bias, lens, heads, _masks(ops, layout, lens, heads, drop), drop[2], dctx)
    A.check(A.outputs(ctx, lse, d), ref, lens, heads, f"edge heads {heads} p {p} kv {use_kv}")
    _masked_key_zeros(d, bias, lens, H)


# ---------------------------------------------------------------------------------------------- production shapes
def _padded_set(ops, B, pass_lens, heads, seed, text_valid=(30, 50)):
    """B x pass_lens sequences, pass-major like the model's packing; padding like the data pipeline's: text passes (the first,
    when it is short) valid 30-50, pair passes half to full.  The output gradient of every padded row is zero (the model's
    guarantee for the rows the valid-first packing leaves out of backward)."""
    g = torch.Generator().manual_seed(seed)
    lens = [S for S in pass_lens for _ in range(B)]
    valid = []
    for S in lens:
        lo, hi = (text_valid if S <= 50 else (S // 2, S))
        valid.append(int(torch.randint(min(lo, S), min(hi, S) + 1, (1,), generator=g)))
    M, H = sum(lens), heads * 64
    qkv = torch.randn(M, 3 * H, generator=g).to(torch.bfloat16)
    dctx = torch.randn(M, H, generator=g)
    bias = torch.zeros(M)
    s0 = 0
    for S, v in zip(lens, valid):
        bias[s0 + v:s0 + S] = A.MASKED
        dctx[s0 + v:s0 + S] = 0.0
        s0 += S
    return lens, valid, qkv, bias, dctx.to(torch.bfloat16)


class _Set:
    pass


@pytest.fixture(scope="module")
def headline(ops):
    """The headline pass set B = 16 x {50, 550, 550}, 12 heads, p = 0.1: inputs, dropout and ONE float64 reference, shared by
    every layout."""
    t = _Set()
    t.heads, t.H = 12, 768
    t.lens, t.valid, t.qkv, t.bias, t.dctx = _padded_set(ops, 16, [50, 550, 550], 12, seed=7)
    t.base = ops.SeqLayout(t.lens, t.heads, DEV)
    t.drop = ops.make_drop(0.1, 2024, 3)
    t.masks = _masks(ops, t.base, t.lens, t.heads, t.drop)
    t.ref = A.reference(t.qkv, t.bias, t.lens, t.heads, t.masks, t.drop[2], t.dctx)
    t.kb = ops.pad_key_bias(t.bias.to(DEV), t.base)
    return t


def test_headline_set_full_tensor(ops, headline):
    """SeqLayout + kv_len at the headline shape: every sequence and head of ctx, LSE, dQ, dK, dV; masked keys' exact zeros."""
    t = headline
    kv = ops.attn_kv_len(t.kb, t.base)
    assert kv.cpu().tolist() == t.valid
    ctx, lse, d = _kernel(ops, t.qkv.to(DEV), t.kb, t.base, t.H, t.drop, t.dctx.to(DEV), kv_len=kv)
    worst = A.check(A.outputs(ctx, lse, d), t.ref, t.lens, t.heads, "headline")
    print("headline largest ratios:", {k: round(v, 4) for k, v in worst.items()})
    _masked_key_zeros(d, t.bias, t.lens, t.H)


@pytest.mark.parametrize("shape", ["fused_4x1050_h12", "bert_large_8x40_80_80_h16"])
def test_production_shapes_full_tensor(ops, shape):
    B, pass_lens, heads = (4, [1050], 12) if shape.startswith("fused") else (8, [40, 80, 80], 16)
    lens, valid, qkv, bias, dctx = _padded_set(ops, B, pass_lens, heads, seed=len(shape), text_valid=(20, 40))
    H = heads * 64
    layout = ops.SeqLayout(lens, heads, DEV)
    drop = ops.make_drop(0.1, 99, 3)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    kv = ops.attn_kv_len(kb, layout)
    ctx, lse, d = _kernel(ops, qkv.to(DEV), kb, layout, H, drop, dctx.to(DEV), kv_len=kv)
    ref = A.reference(qkv, bias, lens, heads, _masks(ops, layout, lens, heads, drop), drop[2], dctx)
    A.check(A.outputs(ctx, lse, d), ref, lens, heads, shape)
    _masked_key_zeros(d, bias, lens, H)


# ---------------------------------------------------------------------------------------------- packed layouts
SENTINEL = 7.0


def _split_run(ops, t, lay, kb, backward=True):
    """Forward (and backward) on a valid-first layout: inputs gathered through ``perm``, outputs mapped back through ``inv``.
    Backward covers region A only (ops.SplitLayout): the dqkv rows of region B are never written -- checked on a sentinel."""
    perm = lay.perm.to(DEV)
    qkv_p = t.qkv.to(DEV)[perm].contiguous()
    ctx, lse = ops.attn_fwd(qkv_p, kb, lay, t.H, drop=t.drop)
    d = None
    if backward:
        dctx_p = t.dctx.to(DEV)[perm].contiguous()
        d = torch.full_like(qkv_p, SENTINEL)
        ops.attn_bwd(qkv_p, ctx, dctx_p, lse, kb, lay, t.H, drop=t.drop, dqkv=d)
        ra = lay.rows_a
        assert bool((d[ra:] == SENTINEL).all()), "backward wrote a region-B row"
        d = d.clone()
        d[ra:] = 0.0                                       # what those rows' gradients are (the model never reads them)
    torch.cuda.synchronize()
    return ctx, lse, d


@pytest.mark.parametrize("mode", ["split", "drop", "device"])
def test_headline_set_on_the_valid_first_layouts(ops, headline, mode):
    """SplitLayout in split and drop mode, DeviceSplitLayout from device-side counts: same reference as the plain layout.  In
    drop mode the region-B rows are left out altogether and only region A is compared."""
    t = headline
    if mode == "device":
        lay = ops.DeviceSplitLayout(t.base, torch.tensor(t.valid, dtype=torch.int32, device=DEV), DEV)
    else:
        lay = ops.SplitLayout(t.base, t.valid, DEV, drop=(mode == "drop"))
    ctx, lse, d = _split_run(ops, t, lay, t.kb)
    rows = None
    if mode == "drop":
        rows = torch.cat([torch.arange(S) < v for S, v in zip(t.lens, t.valid)])
    A.check(A.outputs(ctx, lse, d, lay), t.ref, t.lens, t.heads, f"headline {mode}", rows=rows)


def test_headline_set_dedupe_forward(ops, headline):
    """SplitLayout(dedupe=True) (inference, p = 0): a sequence's masked-out rows have identical inputs and keep one
    representative; every original row is compared through ``inv``."""
    t = headline
    qkv = t.qkv.clone()
    s0 = 0
    for S, v in zip(t.lens, t.valid):
        if v < S:
            qkv[s0 + v:s0 + S] = qkv[s0 + v]
        s0 += S
    lay = ops.SplitLayout(t.base, t.valid, DEV, dedupe=True)
    assert lay.rows_packed < sum(t.lens)
    ctx, lse = ops.attn_fwd(qkv.to(DEV)[lay.perm.to(DEV)].contiguous(), t.kb, lay, t.H)
    ref = A.reference(qkv, t.bias, t.lens, t.heads)
    A.check(A.outputs(ctx, lse, None, lay), ref, t.lens, t.heads, "headline dedupe")


def test_row_set_layout_from_the_prologue(ops):
    """Row-set mode (ops.prologue(rowset=True) + SplitLayout(rank=...)): masked-out rows in the MIDDLE of a sequence.  The kernels
    see every sequence in its active-first order (key bias, dropout positions); mapped back, ctx / LSE / dQ / dK / dV equal the
    reference on the original order, whose dropout mask is the kernel's at the ranks."""
    B, pass_lens, heads, V = 4, [50, 550, 550], 12, 500
    H = heads * 64
    g = torch.Generator().manual_seed(21)
    masks = []
    for S in pass_lens:
        m = torch.ones(B, S)
        for b in range(B):
            a = int(torch.randint(1, S // 2, (1,), generator=g))
            w = int(torch.randint(1, S // 3, (1,), generator=g))
            m[b, a:a + w] = 0                                      # a hole in the middle
            if b % 2:
                m[b, S - S // 5:] = 0                              # and a masked tail
        masks.append(m)
    segs = [(masks[k].to(DEV), k, 0) for k in range(len(pass_lens))]
    pro = ops.prologue(segs, pass_lens, B, None, V, DEV, rowset=True)
    torch.cuda.synchronize()
    lens = [S for S in pass_lens for _ in range(B)]
    M = sum(lens)
    bias = torch.cat([(1.0 - masks[k][b]) * A.MASKED for k in range(len(pass_lens)) for b in range(B)])
    base = ops.SeqLayout(lens, heads, DEV)
    lay = ops.SplitLayout(base, pro.valid.cpu().numpy(), DEV, rank=pro.rank)
    rank = pro.rank.cpu().long()
    starts = [sum(lens[:i]) for i in range(len(lens))]
    perm_pos = [rank[s0:s0 + S] for s0, S in zip(starts, lens)]
    drop = ops.make_drop(0.1, 55, 3)
    qkv = torch.randn(M, 3 * H, generator=g).to(torch.bfloat16)
    dctx = torch.randn(M, H, generator=g)
    active = torch.zeros(M, dtype=torch.bool)
    active[lay.perm[:lay.rows_a].cpu()] = True
    dctx[~active] = 0.0
    dctx = dctx.to(torch.bfloat16)
    t = _Set()
    t.qkv, t.dctx, t.H, t.drop = qkv, dctx, H, drop
    ctx, lse, d = _split_run(ops, t, lay, pro.key_bias)
    ref = A.reference(qkv, bias, lens, heads, _masks(ops, base, lens, heads, drop, perm_pos), drop[2], dctx)
    A.check(A.outputs(ctx, lse, d, lay), ref, lens, heads, "row set")


# ---------------------------------------------------------------------------------------------- top layer: q_limit
def test_top_layer_backward_with_query_limit(ops):
    """dctx non-zero only on a row list (a few rows per sequence, none in one sequence), q_limit from mmbert_attn_q_limit: both
    backward kernels stop their query range there; against the reference with the same dctx."""
    lens, heads = [550, 300, 50, 200, 130, 64, 1050], 12
    H, M = heads * 64, sum(lens)
    pats = ["tail_inside", "random", "none", "tail_boundary", "random", "none", "random"]
    qkv, bias, dctx = A.make_inputs(lens, heads, pats, seed=77)
    g = torch.Generator().manual_seed(78)
    starts = [sum(lens[:i]) for i in range(len(lens))]
    rows = []
    for i, (s0, S) in enumerate(zip(starts, lens)):
        if i == 3:
            continue                                               # a sequence without any gradient row
        rows.append(torch.randperm(min(S, 60), generator=g)[:5] + s0)
        rows.append(torch.tensor([s0]))
    rows = torch.cat(rows)
    keep = torch.zeros(M, dtype=torch.bool)
    keep[rows] = True
    dctx = (dctx.float() * keep[:, None]).to(torch.bfloat16)
    layout = ops.SeqLayout(lens, heads, DEV)
    drop = ops.make_drop(0.1, 4321, 3)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    kv = ops.attn_kv_len(kb, layout)
    qlim = ops.attn_q_limit(rows.int().to(DEV), layout)
    assert qlim.cpu().tolist()[3] == 0
    ctx, lse, d = _kernel(ops, qkv.to(DEV), kb, layout, H, drop, dctx.to(DEV), kv_len=kv, q_limit=qlim)
    ref = A.reference(qkv, bias, lens, heads, _masks(ops, layout, lens, heads, drop), drop[2], dctx)
    A.check(A.outputs(ctx, lse, d), ref, lens, heads, "q_limit")
    assert float(d[starts[3]:starts[3] + lens[3]].float().abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- forced rescale
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_forced_rescale_forward_and_backward(ops, p):
    """Guide rule 26: score std ~ 8, and one key spiked against chosen query rows so that their running maximum jumps at key
    tile 0, at an interior tile and at the last, partial tile -- for some rows of a 16-row block and not for the others."""
    lens, heads = [200, 129, 70], 12
    H = heads * 64
    qkv, bias, dctx = A.make_inputs(lens, heads, ["none", "random", "tail_inside"], seed=31, qk_scale=2 ** 1.5)
    plan = [(0, 3, [0, 2, 5]), (0, 100, [17, 20]), (0, 195, [40, 41, 45]), (1, 128, [1, 7, 100]), (2, 40, [64, 66])]
    qkv = A.spike_rescale(qkv, lens, heads, plan)
    starts = [sum(lens[:i]) for i in range(len(lens))]
    for seq, key, _ in plan:
        bias[starts[seq] + key] = 0.0
    layout = ops.SeqLayout(lens, heads, DEV)
    drop = ops.make_drop(p, 8, 3)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    ctx, lse, d = _kernel(ops, qkv.to(DEV), kb, layout, H, drop, dctx.to(DEV))
    ref = A.reference(qkv, bias, lens, heads, _masks(ops, layout, lens, heads, drop), drop[2], dctx)
    # the spiked keys dominate their rows (score ~ 32 against a maximum of ~ 22 elsewhere)
    assert float(ref["lse"][starts[0] + 0, 0]) > 25.0
    A.check(A.outputs(ctx, lse, d), ref, lens, heads, f"rescale p {p}")


# ---------------------------------------------------------------------------------------------- dropout index scheme
def test_dropout_index_scheme(ops):
    """Independently of the attention kernels: (a) attn_dropout_mask(S, elem_base[s], h) is the slice
    [elem_base + h*S*Spad, ...) of the flat dropout stream (mmbert_dropout_mask), reshaped (S, Spad)[:, :S]; (b) the index ranges
    of all (sequence, head) pairs of every layout are disjoint; (c) every head's keep fraction is within binomial bounds."""
    drop = ops.make_drop(0.1, 2024, 3)
    pk = 1.0 - drop[1] / 65536.0
    for lens, heads in (([50] * 16 + [550] * 32, 12), ([1050] * 4, 12), ([40] * 8 + [80] * 16, 16), (A.EDGE_LENS, 3)):
        lay = ops.SeqLayout(lens, heads, DEV)
        eb = lay.elem_base_host
        spans = []
        for s, S in enumerate(lens):
            Spad = (S + 3) // 4 * 4
            assert eb[s] % 4 == 0
            spans += [(eb[s] + h * S * Spad, eb[s] + (h + 1) * S * Spad) for h in range(heads)]
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "overlapping dropout index ranges"
        pick = sorted({0, 1, len(lens) // 2, len(lens) - 1})
        flat = ops.dropout_mask(spans[-1][1], drop, DEV)
        for s in pick:
            S = lens[s]
            Spad = (S + 3) // 4 * 4
            for h in sorted({0, 1, heads - 1}):
                m = ops.attn_dropout_mask(S, eb[s], h, drop, DEV)
                want = flat[eb[s] + h * S * Spad:eb[s] + (h + 1) * S * Spad]
                assert torch.equal(m, want.view(S, Spad)[:, :S]), (lens[s], h)
        del flat
        for s, S in enumerate(lens):
            if S < 40:
                continue
            frac = torch.stack([ops.attn_dropout_mask(S, eb[s], h, drop, DEV).float().mean() for h in range(heads)]).cpu()
            sd = math.sqrt(pk * (1 - pk) / (S * S))
            assert float((frac - pk).abs().max()) <= 5 * sd, (S, frac.tolist())
