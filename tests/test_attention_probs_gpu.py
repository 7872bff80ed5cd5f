"""``ops.attn_probs_first`` (csrc/attention.hip, ``attn_probs_first_kernel``: the fp32 attention probabilities of ONE query row per
sequence, every head) against the float64 ``reference_probs`` of tests/attention_probs_ref.py through ``check_probs`` (PHI = 4,
calibrated on the CPU): the case list of tests/attention_first_ref.py plus a 2-head case of 1425 / 129 / 1 keys (several 128- and
256-key strides, ``ld`` far beyond the short sequences), each with and without ``kv_len`` -- bit-equal to each other and between two
runs, into a NaN-filled buffer (every element is written); the queries away from ``seq_start``; the inference packing; masked keys
carry exactly zero weight; and sum_k p_k V_k sits within ``attention_ref.check``'s context bounds of the float64 context at row 0."""
import pytest
import torch

from tests import attention_probs_ref as P
from tests import attention_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
_REF = {}


@pytest.fixture(scope="module")
def ops():
    from msa_amd import ops as o
    return o


def _ref(case):
    """(qkv, bias, reference probabilities, reference scores): computed once per case, shared, never written to."""
    if case[0] not in _REF:
        qkv, bias = P.inputs(case)
        _REF[case[0]] = (qkv, bias) + P.reference_probs(qkv, bias, case[1], case[2])
    return _REF[case[0]]


def _q_rows(layout):
    return layout.seq_start.to(torch.int32).contiguous()


@pytest.mark.parametrize("case", P.CASES, ids=[c[0] for c in P.CASES])
def test_case_list_against_the_reference(ops, case):
    name, lens, heads = case[:3]
    H = heads * 64
    qkv, bias, rp, rs = _ref(case)
    layout = ops.SeqLayout(lens, heads, DEV)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    kv = ops.attn_kv_len(kb, layout)
    qd = qkv.to(DEV)
    outs = []
    for use_kv in (False, True, False, True):
        buf = torch.full((len(lens), heads, max(lens)), float("nan"), device=DEV, dtype=torch.float32)
        got = ops.attn_probs_first(qd, kb, layout, H, _q_rows(layout), kv_len=kv if use_kv else None, out=buf)
        assert got is buf
        outs.append(buf)
    fresh = ops.attn_probs_first(qd, kb, layout, H, _q_rows(layout))
    torch.cuda.synchronize()
    assert fresh.shape == (len(lens), heads, max(lens)) and fresh.dtype == torch.float32
    for use_kv, got in zip((False, True), outs[:2]):
        assert bool(torch.isfinite(got).all()), "an element was not written"
        l1, el = P.check_probs(got, rp, rs, f"{name} kv {use_kv}")
        print(name, "kv_len" if use_kv else "dense", "largest ratio: L1 %.3f u, elementwise %.3f u max p (PHI = %g)" % (l1, el, P.PHI))
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]), "two runs differ"
    assert torch.equal(outs[0], outs[1]), "kv_len on and off differ"
    assert torch.equal(outs[0], fresh)


def test_queries_away_from_seq_start(ops):
    """The query of sequence s is read at q_rows[s] and nowhere else (the construction of tests/test_attention_first_gpu.py)."""
    case = P.CASES[4]                                        # edge lengths, 12 heads
    name, lens, heads = case[:3]
    H = heads * 64
    qkv, bias, rp, rs = _ref(case)
    starts = torch.tensor(A._starts(lens))
    M, ns = sum(lens), len(lens)
    moved = torch.cat((qkv, torch.zeros(ns, 3 * H, dtype=qkv.dtype)))
    order = torch.randperm(ns, generator=torch.Generator().manual_seed(5))
    moved[M + order, :H] = qkv[starts, :H]                     # sequence s's query -> extra row M + order[s]
    moved[starts, :H] = 3.0                                    # ... and its own row 0 no longer holds it (K stays)
    layout = ops.SeqLayout(lens, heads, DEV)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    q_rows = (M + order).to(torch.int32).to(DEV)
    got = ops.attn_probs_first(moved.to(DEV), kb, layout, H, q_rows)
    base = ops.attn_probs_first(qkv.to(DEV), kb, layout, H, _q_rows(layout))
    torch.cuda.synchronize()
    assert torch.equal(got, base)
    P.check_probs(got, rp, rs, "moved queries")


def test_headline_set_on_the_inference_packing(ops):
    """SplitLayout(dedupe=True), the packing ``predict`` runs on: the keys of a sequence are its kept rows, the query row is found
    through ``inv32``; entry k is still the key at position k of the caller's sequence, and everything behind the kept rows is 0."""
    case = P.CASES[-2]
    name, lens, heads = case[:3]
    assert name == "headline-h12"
    H = heads * 64
    qkv, bias = P.inputs(case)
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
    got = ops.attn_probs_first(qkv.to(DEV)[lay.perm.to(DEV)].contiguous(), kb, lay, H, q_rows)
    torch.cuda.synchronize()
    assert got.shape == (len(lens), heads, max(lens))
    rp, rs = P.reference_probs(qkv, bias, lens, heads)
    P.check_probs(got, rp, rs, "headline dedupe")
    for s, v in enumerate(valid):
        assert bool((got[s, :, v:] == 0).all()), s


@pytest.mark.parametrize("heads", [3, 12])
def test_masked_keys_carry_exactly_zero_weight(ops, heads):
    """K of every masked key (in a sequence that has an unmasked one) replaced by 64.0: the probabilities keep their bits, with
    ``kv_len`` and without it, and those keys' entries are exact zeros."""
    lens, H = list(A.EDGE_LENS) + [550, 550], heads * 64
    pats = [A.PATTERNS[(i + heads) % len(A.PATTERNS)] for i in range(len(A.EDGE_LENS))] + ["tail_inside", "random"]
    qkv, bias, _ = A.make_inputs(lens, heads, pats, seed=900 + heads)
    big = qkv.clone()
    zero = torch.zeros(len(lens), max(lens), dtype=torch.bool)
    touched = 0
    for s, (s0, S) in enumerate(zip(A._starts(lens), lens)):
        b = bias[s0:s0 + S]
        zero[s, S:] = True
        if bool((b > A.MASKED).any()):
            pos = (b <= A.MASKED).nonzero().reshape(-1)
            big[s0 + pos, H:2 * H] = 64.0
            zero[s, pos] = True
            touched += pos.numel()
    assert touched > 100
    layout = ops.SeqLayout(lens, heads, DEV)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    kv = ops.attn_kv_len(kb, layout)
    out = {}
    for tag, x in (("plain", qkv), ("huge", big)):
        for use_kv in (False, True):
            out[(tag, use_kv)] = ops.attn_probs_first(x.to(DEV), kb, layout, H, _q_rows(layout), kv_len=kv if use_kv else None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[("huge", False)]).all())
    for key, v in out.items():
        assert torch.equal(v, out[("plain", False)]), key
    assert bool((out[("plain", False)].cpu()[zero[:, None, :].expand(-1, heads, -1)] == 0).all())


@pytest.mark.parametrize("case", [P.CASES[4], P.CASES[-2]], ids=[P.CASES[4][0], P.CASES[-2][0]])
def test_probabilities_reproduce_the_context(ops, case):
    """sum_k p_k V_k, taken in float64 from the kernel's probabilities, within ``attention_ref.check``'s existing ctx bounds of the
    float64 context at row 0: the map handed out is the one the context kernel attends with."""
    from tests import attention_first_ref as F
    name, lens, heads = case[:3]
    H = heads * 64
    qkv, bias, _, _ = _ref(case)
    layout = ops.SeqLayout(lens, heads, DEV)
    kb = ops.pad_key_bias(bias.to(DEV), layout)
    p = ops.attn_probs_first(qkv.to(DEV), kb, layout, H, _q_rows(layout)).double().cpu()
    v = qkv.double()[:, 2 * H:].view(-1, heads, 64)
    ctx = torch.zeros(len(lens), H, dtype=torch.float64)
    for s, (s0, S) in enumerate(zip(A._starts(lens), lens)):
        ctx[s] = torch.einsum("hk,khd->hd", p[s, :, :S], v[s0:s0 + S]).reshape(H)
    worst = A.check(F.expand_first(ctx, lens), A.reference(qkv, bias, lens, heads), lens, heads, name, rows=F.first_rows(lens))
    print(name, "context from the probabilities: largest ratio", round(worst["ctx"], 5))
