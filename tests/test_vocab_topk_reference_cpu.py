"""CPU: the float64 reference of the vocabulary top-k kernel (tests/vocab_topk_ref.py) is what it says, its check accepts the
emulation of the kernel's arithmetic and rejects every mutation.

Largest ratios the emulation reaches over the cases below (elementwise / normwise, bound = 1): row_lse 0.13 / 0.13, top_logprob
0.26 / 0.31, label_logprob 0.15 / 0.12 -- the lse model is mmbert_ce_fwd's (tests/rowwise_ref.py), whose constants carry the
hardware's v_exp_f32 / v_log_f32, not the emulation's correctly rounded exp2 / log2.  The value mutation (pad columns in the lse:
pads of 30 and 60 above rows of a few units) moves the lse by whole units; the order mutations are exact mismatches of ids or ranks.
"""
import pytest
import torch

from tests import rowwise_ref as R
from tests import vocab_topk_ref as T

SHAPES = [(8, 8), (9, 16), (2049, 2056), (30522, 30528)]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for V, ldv in SHAPES:
        M = 25 if V < 30000 else 10
        X, labels, fam, kind = T.make_case(V, ldv, M, seed=V % 7)
        k = min(8, V)
        out[(V, ldv)] = (X, labels, fam, kind, k, T.reference(X, V, k, labels))
    return out


def test_case_builder_covers_every_family_and_label_kind():
    X, labels, fam, kind = T.make_case(9, 16, 300, seed=3)
    assert {(int(f), int(k)) for f, k in zip(fam, kind)} == {(f, k) for f in range(5) for k in range(5)}
    assert (X[:, 9:].float().min(1).values > X[:, :9].float().max(1).values).all()          # pads above every row's maximum
    tied = torch.nonzero(kind == 2).flatten()
    assert all(bool((X[i, :int(labels[i])] == X[i, int(labels[i])]).any()) for i in tied.tolist())
    assert bool((labels[kind == 3] == -100).all()) and bool((labels[kind == 4] == 9).all())


def test_reference_agrees_with_torch_topk_on_tie_free_rows():
    g = torch.Generator().manual_seed(5)
    V, ldv, M = 300, 304, 40
    X = torch.rand(M, ldv, generator=g).mul(4).sub(2)
    perm = torch.stack([torch.randperm(V, generator=g) for _ in range(M)])
    X[:, :V] = (torch.arange(V, dtype=torch.float32) / 8.0 - 10.0)[perm]                     # V distinct bf16-exact values per row
    X[:, V:] = 100.0
    X = X.to(torch.bfloat16)
    labels = torch.randint(0, V, (M,), generator=g)
    ref = T.reference(X, V, 8, labels)
    tk = torch.topk(X[:, :V].double(), 8, dim=1)
    assert torch.equal(ref["top_ids"], tk.indices)
    lsm = torch.log_softmax(X[:, :V].double(), 1)
    assert torch.allclose(ref["top_logprob"].val, lsm.gather(1, tk.indices), rtol=0, atol=1e-12)
    assert torch.allclose(ref["label_logprob"].val, lsm.gather(1, labels[:, None])[:, 0], rtol=0, atol=1e-12)
    assert torch.equal(ref["label_rank"], (X[:, :V].double() > X[:, :V].double().gather(1, labels[:, None])).sum(1))
    assert bool(((ref["label_rank"] < 8) == (tk.indices == labels[:, None]).any(1)).all())


def test_reference_order_on_ties_and_special_rows(cases):
    X, labels, fam, kind, k, ref = cases[(9, 16)]
    ids = ref["top_ids"]
    assert all(ids[i].tolist() == list(range(k)) for i in torch.nonzero(fam == 2).flatten().tolist())       # an all-equal row: 0 .. k-1
    assert bool((ids < 9).all())
    assert all(int(ids[i, 0]) == 8 for i in torch.nonzero(fam == 3).flatten().tolist())                      # the maximum at column V - 1
    ok = (labels >= 0) & (labels < 9)
    assert bool((ref["label_rank"][~ok] == -1).all()) and bool((ref["label_logprob"].val[~ok] == 0).all())
    # rank 0 <=> first id; rank < k <=> among the ids
    assert bool(((ref["label_rank"] == 0) == ((ids[:, 0] == labels) & ok)).all())
    assert bool((((ref["label_rank"] >= 0) & (ref["label_rank"] < k)) == ((ids == labels[:, None]).any(1) & ok)).all())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"V{s[0]}")
def test_check_accepts_the_emulation(cases, shape):
    X, labels, fam, kind, k, ref = cases[shape]
    V = shape[0]
    emu = T.emulate(X, V, k, labels)
    r = T.check(emu, ref, "emulation")
    print({n: (round(q.elem, 3), round(q.norm, 3)) for n, q in r.items()})
    # fp32 logits carrying the same values: the same outputs
    emu32 = T.emulate(X.float(), V, k, labels)
    assert all(torch.equal(emu[n], emu32[n]) for n in emu)
    # without labels: the same ids and log-probabilities
    emu0 = T.emulate(X, V, k)
    T.check(emu0, T.reference(X, V, k), "emulation, no labels")
    assert torch.equal(emu0["top_ids"], emu["top_ids"]) and torch.equal(emu0["top_logprob"], emu["top_logprob"])
    # a smaller k is a prefix
    assert torch.equal(T.reference(X, V, 1, labels)["top_ids"], ref["top_ids"][:, :1])


@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_check_rejects_the_mutation(cases, mutation):
    rejected = 0
    for (V, ldv), (X, labels, fam, kind, k, ref) in cases.items():
        emu = T.emulate(X, V, k, labels, mutation=mutation)
        try:
            T.check(emu, ref, mutation)
        except AssertionError:
            rejected += 1
    # (V = ldv = 8 has no pad columns, so the two pad mutations change nothing there)
    assert rejected >= (len(cases) - 1 if mutation.startswith("pad_") else len(cases)), f"{mutation}: rejected in {rejected} of {len(cases)} cases"


def test_lse_model_is_the_cross_entropy_reference_s():
    """The lse and its bound are R.ce_fwd's own: the same Ref on rows that carry a label there."""
    X, labels, _, _ = T.make_case(1000, 1008, 12, seed=1)
    X[torch.isinf(X)] = -5.0
    ref = T.reference(X, 1000, 5)
    ce = R.ce_fwd(X, torch.full((12,), 3), 1000, torch.tensor([0, 12]), 1)["row_lse"]
    assert torch.equal(ref["row_lse"].val, ce.val) and torch.equal(ref["row_lse"].acc, ce.acc)
