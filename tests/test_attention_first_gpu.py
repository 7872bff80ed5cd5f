"""``ops.attn_fwd_first`` (csrc/attention.hip: attention forward for ONE query row per sequence, the top layer of a label-free
prediction) against the float64 reference of tests/attention_ref.py through ``check(rows=first rows)`` at the module's existing ctx
bounds: the case list of tests/attention_first_ref.py (edge lengths x key-bias patterns at 1 / 3 / 12 / 16 heads, score scale 1 and
2.83, the headline set), with and without ``kv_len``, with the queries away from ``seq_start``, on the inference packing; masked keys
carry exactly zero weight; two runs give the same bits; and the context agrees with row 0 of ``ops.attn_fwd`` in the sense that both
sit within ``check``'s bounds of the float64 reference."""
import pytest
import torch

from tests import attention_first_ref as F
from tests import attention_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from msa_amd import ops as o
    return o


def _q_rows(layout):
    return layout.seq_start.to(torch.int32).contiguous()


@pytest.mark.parametrize("use_kv", [False, True], ids=["dense", "kv_len"])
@pytest.mark.parametrize("case", F.CASES, ids=[c[0] for c in F.CASES])
def test_case_list_against_the_reference(ops, case, use_kv):
    name, lens, heads = case[:3]
    H = heads * 64
    qkv, bias = F.inputs(*case)
    layout = ops.SeqLayout(lens, heads, DEV)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    kv = ops.attn_kv_len(kb, layout) if use_kv else None
    qd = qkv.to(DEV)
    ctx = ops.attn_fwd_first(qd, kb, layout, H, _q_rows(layout), kv_len=kv)
    again = ops.attn_fwd_first(qd, kb, layout, H, _q_rows(layout), kv_len=kv)
    full, _ = ops.attn_fwd(qd, kb, layout, H, kv_len=kv)
    torch.cuda.synchronize()
    assert ctx.shape == (len(lens), H) and ctx.dtype == torch.bfloat16
    assert torch.equal(ctx, again), "two runs differ"
    ref = A.reference(qkv, bias, lens, heads)
    rows = F.first_rows(lens)
    worst = A.check(F.expand_first(ctx, lens), ref, lens, heads, f"{name} kv {use_kv}", rows=rows)
    print(name, "kv_len" if use_kv else "dense", "largest ratio", round(worst["ctx"], 4))
    # the other kernel's row 0: within the same bounds of the same reference (not compared with each other: their roundings differ)
    A.check({"ctx": full.double().cpu()}, ref, lens, heads, f"{name} attn_fwd row 0", rows=rows)


def test_queries_away_from_seq_start(ops):
    """The query of sequence s is read at q_rows[s] and nowhere else: the queries sit in extra rows behind the packed matrix, and
    the Q part of every sequence's own row 0 holds something else."""
    name, lens, heads, pats, qs = F.CASES[4]                 # edge lengths, 12 heads
    H = heads * 64
    qkv, bias = F.inputs(name, lens, heads, pats, qs)
    starts = torch.tensor(A._starts(lens))
    M, ns = sum(lens), len(lens)
    moved = torch.cat((qkv, torch.zeros(ns, 3 * H, dtype=qkv.dtype)))
    order = torch.randperm(ns, generator=torch.Generator().manual_seed(5))
    moved[M + order, :H] = qkv[starts, :H]                     # sequence s's query -> extra row M + order[s]
    moved[starts, :H] = 3.0                                    # ... and its own row 0 no longer holds it (K and V stay)
    layout = ops.SeqLayout(lens, heads, DEV)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    q_rows = (M + order).to(torch.int32).to(DEV)
    ctx = ops.attn_fwd_first(moved.to(DEV), kb, layout, H, q_rows)
    torch.cuda.synchronize()
    base = ops.attn_fwd_first(qkv.to(DEV), kb, layout, H, _q_rows(layout))
    assert torch.equal(ctx, base)
    A.check(F.expand_first(ctx, lens), A.reference(qkv, bias, lens, heads), lens, heads, "moved queries", rows=F.first_rows(lens))


def test_headline_set_on_the_inference_packing(ops):
    """SplitLayout(dedupe=True), the packing ``predict`` runs on: K / V of a sequence are its kept rows, the query row is found through
    ``inv32``; compared after mapping back (the compact output is in sequence order whatever the packing)."""
    name, lens, heads, pats, qs = F.CASES[-1]
    H = heads * 64
    qkv, bias = F.inputs(name, lens, heads, pats, qs)
    starts = A._starts(lens)
    valid = []
    for s0, S in zip(starts, lens):                            # leading rows that keep a row of their own: up to the last unmasked key
        un = (bias[s0:s0 + S] > A.MASKED).nonzero()
        v = int(un.max()) + 1 if un.numel() else S
        valid.append(v)
        if v < S:
            qkv[s0 + v:s0 + S] = qkv[s0 + v]                   # the masked-out tail rows share one input
    base = ops.SeqLayout(lens, heads, DEV)
    lay = ops.SplitLayout(base, valid, DEV, dedupe=True)
    assert lay.rows_packed < sum(lens)
    kb = ops.pad_key_bias(bias.to(DEV), base)
    q_rows = lay.inv32.index_select(0, torch.tensor(starts, device=DEV))
    ctx = ops.attn_fwd_first(qkv.to(DEV)[lay.perm.to(DEV)].contiguous(), kb, lay, H, q_rows)
    torch.cuda.synchronize()
    A.check(F.expand_first(ctx, lens), A.reference(qkv, bias, lens, heads), lens, heads, "headline dedupe", rows=F.first_rows(lens))


@pytest.mark.parametrize("heads", [3, 12])
def test_masked_keys_carry_exactly_zero_weight(ops, heads):
    """K / V of every masked key (in a sequence that has an unmasked one) replaced by huge finite values: the context keeps its bits,
    with ``kv_len`` (trailing masked keys skipped) and without it (their probability is an exact 0) -- and both agree bit for bit."""
    lens, H = list(A.EDGE_LENS) + [550, 550], heads * 64
    pats = [A.PATTERNS[(i + heads) % len(A.PATTERNS)] for i in range(len(A.EDGE_LENS))] + ["tail_inside", "random"]
    qkv, bias, _ = A.make_inputs(lens, heads, pats, seed=900 + heads)
    big = qkv.clone()
    touched = 0
    for s0, S in zip(A._starts(lens), lens):
        b = bias[s0:s0 + S]
        if bool((b > A.MASKED).any()):
            rows = s0 + (b <= A.MASKED).nonzero().reshape(-1)
            big[rows, H:2 * H] = 64.0
            big[rows, 2 * H:] = 1.0e30
            touched += rows.numel()
    assert touched > 100
    layout = ops.SeqLayout(lens, heads, DEV)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    kv = ops.attn_kv_len(kb, layout)
    out = {}
    for tag, x in (("plain", qkv), ("huge", big)):
        for use_kv in (False, True):
            out[(tag, use_kv)] = ops.attn_fwd_first(x.to(DEV), kb, layout, H, _q_rows(layout), kv_len=kv if use_kv else None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[("huge", False)].float()).all())
    for key, v in out.items():
        assert torch.equal(v, out[("plain", False)]), key
