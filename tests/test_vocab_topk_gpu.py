"""mmbert_vocab_topk (csrc/rowwise.hip) against the float64 reference of tests/vocab_topk_ref.py, through the C ABI: ids and label
ranks exactly equal to the stable-sort order, row_lse and the log-probabilities within the cross-entropy reference's lse model.

Shapes: (V, ldv) at 8 = k, one partial chunk, the one-chunk-per-lane boundary (2047 / 2048 / 2049 columns over 256 lanes x 8), the
model's own row (30 522 in 30 528) and the register limit (32 768); M = 1, 5, 300 rows; k = 1, 5, 8; bf16 and fp32 logits (equal
bits).  Rows (tests/vocab_topk_ref.make_case): gaussian, four-valued (ties dominate), all-equal, the maximum at column V - 1 under
larger pad values, rows with -inf; labels at column 0, V - 1, a tied value, -100 and V.  Every output buffer is pre-filled with a
sentinel and must be fully overwritten; two calls give equal bits; on rows mmbert_ce_fwd scores, row_lse has its bits; the ABI's
refusals return -1 and write nothing.  The largest ratios are printed at the end of the module (``-s``)."""
import collections

import pytest
import torch

from tests import rowwise_ref as R
from tests import vocab_topk_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
torch.set_num_threads(min(16, torch.get_num_threads()))
WORST = collections.defaultdict(lambda: [0.0, 0.0])
SHAPES = [(8, 8), (9, 16), (2047, 2048), (2048, 2048), (2049, 2056), (30522, 30528), (32768, 32768)]
ROWS = [1, 5, 300]
KS = [1, 5, 8]
ID_SENTINEL = -7
_cases = {}


@pytest.fixture(scope="module")
def ops():
    from msa_amd import ops as o
    yield o
    if WORST:
        print("\nlargest ratios (elementwise, normwise):")
        for k in sorted(WORST):
            print(f"  {k:16s} {WORST[k][0]:.3f} {WORST[k][1]:.3f}")


def case(V, ldv, M):
    """(X bf16 CPU, labels, reference at k = min(8, V)) -- built once per shape and shared; a smaller k is a prefix of the ids."""
    key = (V, ldv, M)
    if key not in _cases:
        X, labels, _, _ = T.make_case(V, ldv, M, seed=(V + M) % 11)
        _cases[key] = (X, labels, T.reference(X, V, min(8, V), labels))
    return _cases[key]


def ref_at(ref, k):
    out = dict(ref)
    out["top_ids"] = ref["top_ids"][:, :k]
    lp = ref["top_logprob"]
    out["top_logprob"] = R.Ref(lp.val[:, :k], lp.acc[:, :k], lp.extra, lp.u_out)
    return out


def f32_canary(shape):
    return torch.full(shape, R.NAN_F32, dtype=torch.int32, device=DEV).view(torch.float32)


def raw_call(ops, X, V, k, labels, *, ldv=None, M=None, label_outputs=None):
    """One mmbert_vocab_topk call on sentinel-filled outputs.  Returns (code, outputs dict)."""
    from msa_amd import _lib
    lib = _lib.load()
    M = X.shape[0] if M is None else M
    rows = max(X.shape[0], 1)
    out = {"top_ids": torch.full((rows, max(k, 1)), ID_SENTINEL, dtype=torch.int32, device=DEV), "top_logprob": f32_canary((rows, max(k, 1))),
           "row_lse": f32_canary((rows,))}
    if (labels is not None) if label_outputs is None else label_outputs:
        out["label_logprob"] = f32_canary((rows,))
        out["label_rank"] = torch.full((rows,), ID_SENTINEL, dtype=torch.int32, device=DEV)
    code = lib.mmbert_vocab_topk(ops._stream(), X.data_ptr(), X.stride(0) if ldv is None else ldv, V, M, 1 if X.dtype == torch.float32 else 0, k,
                                 ops._ptr(labels), out["top_ids"].data_ptr(), out["top_logprob"].data_ptr(), out["row_lse"].data_ptr(),
                                 ops._ptr(out.get("label_logprob")), ops._ptr(out.get("label_rank")))
    torch.cuda.synchronize()
    return code, out


def untouched(out):
    return all(bool((t.view(torch.int32) == (ID_SENTINEL if t.dtype == torch.int32 else R.NAN_F32)).all()) for t in out.values())


def fully_written(out, V):
    assert bool(((out["top_ids"] >= 0) & (out["top_ids"] < V)).all()), "top_ids: a sentinel or a pad column is left"
    for n in ("top_logprob", "row_lse", "label_logprob"):
        if n in out:
            assert not bool((out[n].view(torch.int32) == R.NAN_F32).any()), f"{n}: sentinel elements are left"
    if "label_rank" in out:
        assert bool((out["label_rank"] != ID_SENTINEL).all()), "label_rank: sentinel elements are left"


def _note(r):
    for n, q in r.items():
        w = WORST[n]
        w[0], w[1] = max(w[0], q.elem), max(w[1], q.norm)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("V,ldv", SHAPES)
def test_matches_reference(ops, V, ldv, M):
    X, labels, ref = case(V, ldv, M)
    Xd, X32, lab = X.to(DEV), X.float().to(DEV), labels.to(DEV)
    for k in KS:
        code, got = raw_call(ops, Xd, V, k, lab)
        assert code == 0
        fully_written(got, V)
        _note(T.check(got, ref_at(ref, k), f"V={V} ldv={ldv} M={M} k={k}"))
        code, got32 = raw_call(ops, X32, V, k, lab)                                       # fp32 logits: rounded as loaded, equal bits
        assert code == 0
        code, again = raw_call(ops, Xd, V, k, lab)                                        # a second call: equal bits
        assert code == 0
        for n in got:
            assert torch.equal(got[n].view(torch.int32), got32[n].view(torch.int32)), f"{n}: fp32 logits give other bits (k={k})"
            assert torch.equal(got[n].view(torch.int32), again[n].view(torch.int32)), f"{n}: two calls differ (k={k})"
    # without labels: the same ids, log-probabilities and lse; no label outputs asked for
    k = min(5, V)
    code, nolab = raw_call(ops, Xd, V, k, None)
    assert code == 0
    fully_written(nolab, V)
    code, withlab = raw_call(ops, Xd, V, k, lab)
    for n in nolab:
        assert torch.equal(nolab[n].view(torch.int32), withlab[n].view(torch.int32)), n


@pytest.mark.parametrize("V,ldv", [(9, 16), (2049, 2056), (30522, 30528)])
def test_row_lse_has_the_cross_entropy_kernels_bits(ops, V, ldv):
    X, labels, _ = case(V, ldv, 300)
    Xd, lab = X.to(DEV), labels.to(DEV)
    bounds = torch.tensor([0, 300], dtype=torch.int32, device=DEV)
    _, _, lse_ce = ops.ce_fwd(Xd, V, lab, bounds, 1)
    _, _, lse_ce32 = ops.ce_fwd(Xd.float(), V, lab, bounds, 1)
    got = ops.vocab_topk(Xd, V, 5, lab)
    scored = ((labels >= 0) & (labels < V)).to(DEV)
    assert int(scored.sum()) > 100
    assert torch.equal(got[2][scored].view(torch.int32), lse_ce[scored].view(torch.int32))
    assert torch.equal(got[2][scored].view(torch.int32), lse_ce32[scored].view(torch.int32))
    assert bool((lse_ce[~scored] == 0).all())                       # (mmbert_ce_fwd leaves 0 there; this call scores every row)


def test_python_wrappers(ops):
    import msa_amd.torch_ops  # noqa: F401
    V, ldv, M = 2049, 2056, 5
    X, labels, ref = case(V, ldv, M)
    Xd, lab = X.to(DEV), labels.to(DEV)
    ids, lp, lse, llp, rank = ops.vocab_topk(Xd, V, 5, lab)
    assert ids.dtype == torch.int32 and rank.dtype == torch.int32 and ids.shape == (M, 5) and lp.shape == (M, 5)
    T.check(dict(top_ids=ids, top_logprob=lp, row_lse=lse, label_logprob=llp, label_rank=rank), ref_at(ref, 5), "ops.vocab_topk")
    assert len(ops.vocab_topk(Xd, V, 5)) == 3
    t = torch.ops.mmbert.vocab_topk(Xd, V, 5, lab)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(t, (ids, lp, lse, llp, rank)))
    t0 = torch.ops.mmbert.vocab_topk(Xd, V, 5)
    assert torch.equal(t0[0], ids) and t0[3].numel() == 0 and t0[4].numel() == 0
    # a row view with a stride (the rows of a wider matrix) and a one-row call
    wide = torch.full((M, ldv + 64), 99.0, dtype=torch.bfloat16, device=DEV)
    wide[:, :ldv] = Xd
    assert torch.equal(ops.vocab_topk(wide[:, :ldv], V, 5, lab)[0], ids)
    assert torch.equal(ops.vocab_topk(Xd[2:3], V, 5, lab[2:3])[0], ids[2:3])
    with pytest.raises(RuntimeError):
        ops.vocab_topk(Xd, V, 9)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.mmbert.vocab_topk(X, V, 5, None)                     # a CPU tensor: no CPU implementation


def test_abi_refusals_write_nothing(ops):
    V, ldv, M = 9, 16, 5
    X, labels, _ = case(V, ldv, M)
    Xd, lab = X.to(DEV), labels.to(DEV)
    big = torch.zeros((1, 32776), dtype=torch.bfloat16, device=DEV)
    bad = [dict(X=Xd, V=V, k=0, labels=lab), dict(X=Xd, V=V, k=9, labels=lab),
           dict(X=Xd[:, :8].contiguous(), V=8, k=8, labels=lab, ok=True),            # (k = V = 8 is legal)
           dict(X=Xd, V=4, k=5, labels=lab),                                           # k > V
           dict(X=big, V=32769, k=1, labels=None),                                     # V > 32768
           dict(X=Xd, V=V, k=5, labels=lab, ldv=12),                                   # ldv % 8 != 0
           dict(X=Xd, V=V, k=5, labels=lab, ldv=8),                                    # ldv < V
           dict(X=Xd, V=V, k=5, labels=lab, label_outputs=False),                      # labels without rank buffers
           dict(X=Xd, V=V, k=5, labels=None, label_outputs=True),                      # rank buffers without labels
           dict(X=Xd, V=0, k=1, labels=None), dict(X=Xd, V=V, k=5, labels=lab, M=-1)]
    for a in bad:
        a = dict(a)
        ok = a.pop("ok", False)
        code, out = raw_call(ops, a.pop("X"), a.pop("V"), a.pop("k"), a.pop("labels"), **a)
        if ok:
            assert code == 0
            continue
        assert code == -1, a
        assert untouched(out), a
    code, out = raw_call(ops, Xd, V, 5, lab, M=0)                                      # no rows: a no-op success
    assert code == 0 and untouched(out)
    empty = torch.empty((0, ldv), dtype=torch.bfloat16, device=DEV)
    ids, lp, lse = ops.vocab_topk(empty, V, 5)
    assert ids.shape == (0, 5) and lp.shape == (0, 5) and lse.shape == (0,)
