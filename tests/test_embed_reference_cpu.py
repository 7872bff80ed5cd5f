"""tests/embed_ref.py on the CPU: the reference equals float64 autograd through the oracle's lookup and projection expressions, the
emulation of the kernels' fp32 roundings passes ``check`` in both modes and every emulated arrival order, and every value-only
mutation of the emulation fails it.

Largest emulation ratio over every case: 0.50 (elementwise, the bf16 gather and pair outputs: their final rounding); of the
fp32 sums 0.44 (normwise, dW over the 96-row chains of the headline-like pair backward).

Smallest margin of a mutation (error / bound of the mutated emulation; > 1 fails): 1.5e3, dW's prior overwritten (its 0.3-sized
prior against a sum over 1600 rows).  Next: db's prior overwritten 2.4e3, one wave's rows of the last range lost 3.1e4, gtype's
prior overwritten 3.4e4, one [MASK] row dropped 4.4e4, then 5e4 ... 5e9 and inf (the padding row written, word and position
priors overwritten, the lost k = 127 of D = 371, the neighbouring bias column and the bf16 features all break an exact value).
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import mmbert_oracle as O
from tests import embed_ref as E

torch.set_num_threads(min(16, torch.get_num_threads()))

EMU_LIMIT = 0.6            # the emulation's ratios stay below this
MIN_MARGIN = 4.0
ORDERS = ("asc", "desc", 1, 2)


# ------------------------------------------------------------------------------------------------ cases
def emb_case(B, T, V, H, seed, tts=True, Tpos=None):
    ids, tt = E.make_ids(B, T, V, seed)
    word, typ, pos = E.make_tables(V, H, Tpos or max(T, 64), seed + 1)
    n = B * T
    d = E.make_d(n, H, seed + 2)
    g = torch.Generator().manual_seed(seed + 3)
    gword0 = 0.5 * torch.randn(V, H, generator=g)
    gtype0 = 4.0 * torch.randn(2, H, generator=g)
    gpos0 = 2.0 * torch.randn(pos.shape[0], H, generator=g)
    return dict(ids=ids, tts=tt if tts else None, word=word, typ=typ, pos=pos, T=T, d=d, gword0=gword0, gtype0=gtype0, gpos0=gpos0, V=V)


EMB = {
    "headline": dict(B=48, T=50, V=30522, H=768, seed=1),
    "partial batches, no types": dict(B=13, T=10, V=500, H=64, seed=2, tts=False),
    "bert-large": dict(B=32, T=40, V=4000, H=1024, seed=3),
}


def pair_case(B, P, D, H, seed, dtype=torch.float32):
    f, W, b = E.make_pair(B, P, D, H, seed, dtype=dtype)
    ref = E.pair_fwd(f, W, b)
    J = ref.val.to(torch.bfloat16)
    g = torch.Generator().manual_seed(seed + 5)
    dJ = torch.randn(B * P, H, generator=g).to(torch.bfloat16)
    dW0, db0 = 0.3 * torch.randn(H, D, generator=g), 0.3 * torch.randn(H, generator=g)
    return dict(f=f, W=W, b=b, J=J, dJ=dJ, dW0=dW0, db0=db0)


PAIR = {
    "headline-like D=74": dict(B=16, P=100, D=74, H=768, seed=11),
    "D=371": dict(B=4, P=65, D=371, H=128, seed=12),
    "D=81": dict(B=3, P=63, D=81, H=64, seed=13),
    "D=80": dict(B=5, P=64, D=80, H=200, seed=14),
    "D=1": dict(B=2, P=64, D=1, H=128, seed=15),
    "D=47 float64": dict(B=3, P=65, D=47, H=1024, seed=16, dtype=torch.float64),
}


def _worst(em, ref):
    w = 0.0
    for k, r in ref.items():
        e = em[k]
        q = E.ratios(e[1], r, gathered=True) if isinstance(e, tuple) else E.ratios(e, r)
        w = max(w, q.worst)
    return w


def _scatter(c, det, order="asc", emu=False, mutation=None):
    return E.scatter(c["ids"], c["tts"], c["d"], c["T"], c["gword0"], c["gtype0"], c["gpos0"], det=det, order=order, emu=emu,
                     mutation=mutation)


def _pair(c, emu=False, mutation=None):
    out = {"out": E.pair_fwd(c["f"], c["W"], c["b"], emu=emu, mutation=mutation)}
    out.update(E.pair_bwd(c["f"], c["J"], c["dJ"], c["dW0"], c["db0"], emu=emu, mutation=mutation))
    return out


# ------------------------------------------------------------------------------------------------ the reference against the oracle
@pytest.mark.parametrize("shape", [dict(B=3, T=10, V=500, H=64, P=7, Dv=35, Ds=74), dict(B=48, T=50, V=30522, H=768, P=500, Dv=35, Ds=74)],
                         ids=["small", "headline"])
def test_reference_equals_float64_autograd_through_the_oracle(shape):
    B, T, V, H, P = shape["B"], shape["T"], shape["V"], shape["H"], shape["P"]
    c = emb_case(B, T, V, H, 21)
    ids, tts = c["ids"], c["tts"]
    idp = torch.where((ids >= 0) & (ids < V), ids, torch.zeros_like(ids)).view(B, T)
    p = {"bert.embeddings.word_embeddings.weight": c["word"], "bert.embeddings.token_type_embeddings.weight": c["typ"],
         "bert.embeddings.position_embeddings.weight": c["pos"]}
    p = {k: v.to(torch.float64).requires_grad_(True) for k, v in p.items()}
    # oracle.bert_embeddings' lookup (before its LayerNorm and dropout)
    e = F.embedding(idp, p["bert.embeddings.word_embeddings.weight"], padding_idx=0)
    e = e + p["bert.embeddings.token_type_embeddings.weight"][(tts != 0).long().view(B, T)]
    e = e + p["bert.embeddings.position_embeddings.weight"][:T][None]
    e.backward(c["d"].to(torch.float64).view(B, T, H))
    out = E.gather(ids, tts, c["word"], c["typ"], c["pos"], T)
    _close(out.val, e.detach().reshape(B * T, H), "gather")
    gw, gt, gp = (p[k].grad for k in p)
    for det in (False, True):
        ref = _scatter(c, det)
        _close(ref["gword"].val, (c["gword0"].double() + gw)[ref["gword"].rows], f"gword det {det}")
        _close(ref["gtype"].val, c["gtype0"].double() + gt, f"gtype det {det}")
        _close(ref["gpos"].val, c["gpos0"].double() + gp, f"gpos det {det}")
        rows = ref["gword"].rows
        assert float(gw[rows][~torch.isnan(ref["gword"].exact[:, 0])].abs().max()) == 0.0       # exact rows: no gradient at all
    assert float(gw[0].abs().max()) == 0.0 and torch.isnan(ref["gword"].exact[ref["gword"].rows == 0]).sum() == 0
    # oracle.joint_embeddings' projection: relu(Linear(pair.float()))
    Bp = min(B, 16)
    for which, D in (("Wv", shape["Dv"]), ("Ws", shape["Ds"])):
        f, W, b = E.make_pair(Bp, P, D, H, 22, dtype=torch.float64)
        nm = f"bert.jointEmbeddings.{which}"
        q = {nm + ".weight": W.double().requires_grad_(True), nm + ".bias": b.double().requires_grad_(True)}
        pe = F.relu(O._linear(f.float().double(), q, nm))
        ref = E.pair_fwd(f, W, b)
        _close(ref.val, pe.detach().reshape(-1, H), f"pair fwd {which}")
        J = ref.val.to(torch.bfloat16)
        g = torch.Generator().manual_seed(23)
        dJ = torch.randn(Bp * P, H, generator=g).to(torch.bfloat16)
        dW0, db0 = torch.randn(H, D, generator=g), torch.randn(H, generator=g)
        pe.backward(dJ.double().view(Bp, P, H))
        rb = E.pair_bwd(f, J, dJ, dW0, db0)
        _close(rb["dW"].val, dW0.double() + q[nm + ".weight"].grad, f"d{which}")
        _close(rb["db"].val, db0.double() + q[nm + ".bias"].grad, f"db {which}")


def _close(a, b, what):
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(float(b.abs().max()), 1e-300), (what, err)


# ------------------------------------------------------------------------------------------------ the emulation against the bounds
@pytest.mark.parametrize("name", list(EMB))
def test_embedding_emulation_passes(name):
    c = emb_case(**EMB[name])
    worst = 0.0
    g_ref = E.gather(c["ids"], c["tts"], c["word"], c["typ"], c["pos"], c["T"])
    g_em = E.gather(c["ids"], c["tts"], c["word"], c["typ"], c["pos"], c["T"], emu=True)
    worst = max(worst, E.ratios(g_em, g_ref).worst)
    for det in (False, True):
        ref = _scatter(c, det)
        for order in (ORDERS if not det else ("asc",)):
            w = _worst(_scatter(c, det, order, emu=True), ref)
            assert w <= EMU_LIMIT, (det, order, w)
            worst = max(worst, w)
    assert worst <= EMU_LIMIT
    print(f"\n{name}: emulation ratio {worst:.3f}")


@pytest.mark.parametrize("det", [False, True])
def test_run_sums_emulation_passes_across_launches(det):
    """ops.scatter_add_rows_ordered / rows_to_block at 9600 rows (two launches of the ordered kernel), into the word table and into
    a union block."""
    B, T, V, H = 192, 50, 3000, 128
    ids, _ = E.make_ids(B, T, V, 31)
    src = E.make_d(B * T, H, 32)
    g = torch.Generator().manual_seed(33)
    dst0 = torch.randn(V, H, generator=g)
    union = torch.unique(ids[::3][(ids[::3] > 0) & (ids[::3] < V)])
    blk0 = torch.randn(union.numel(), H, generator=g)
    worst = 0.0
    for kw, d0 in ((dict(), dst0), (dict(union=union), blk0)):
        ref = E.rows_sum(ids, src, d0, V, det=det, **kw)
        for order in (ORDERS if not det else ("asc",)):
            rows, em = E.rows_sum(ids, src, d0, V, det=det, order=order, emu=True, **kw)
            q = E.ratios(em, ref, gathered=True).worst
            assert q <= EMU_LIMIT, (kw.keys(), order, q)
            worst = max(worst, q)
    print(f"\nrun sums det {det}: emulation ratio {worst:.3f}")


@pytest.mark.parametrize("name", list(PAIR))
def test_pair_emulation_passes(name):
    c = pair_case(**PAIR[name])
    w = _worst(_pair(c, emu=True), _pair(c))
    assert w <= EMU_LIMIT, w
    print(f"\n{name}: emulation ratio {w:.3f}")


# ------------------------------------------------------------------------------------------------ mutations
MUTATIONS = [
    (E.padding_row_written(), "emb", "headline", False),
    (E.padding_row_written(), "emb", "headline", True),
    (E.out_of_range_from_last_row(), "gather", "headline", None),
    (E.position_shifted_on_one_sequence(), "gather", "headline", None),
    (E.position_shifted_on_one_sequence(), "emb", "headline", True),
    (E.token_types_swapped_at(), "gather", "headline", None),
    (E.token_types_swapped_at(), "emb", "headline", False),
    (E.prior_overwritten("gword"), "emb", "headline", False),
    (E.prior_overwritten("gword"), "emb", "headline", True),
    (E.prior_overwritten("gtype"), "emb", "headline", True),
    (E.prior_overwritten("gpos"), "emb", "headline", False),
    (E.prior_overwritten("rows"), "runs", "union", True),
    (E.prior_overwritten("rows"), "runs", "union", False),
    (E.prior_overwritten("dW"), "pair", "headline-like D=74", None),
    (E.prior_overwritten("db"), "pair", "headline-like D=74", None),
    (E.word_run_row_dropped(E.CLS), "emb", "headline", False),
    (E.word_run_row_dropped(E.CLS), "emb", "headline", True),
    (E.word_run_row_dropped(E.MASK), "emb", "headline", True),
    (E.last_partial_batch_dropped(), "emb", "partial batches, no types", False),
    (E.split_run_counted_once(), "runs", "table", True),
    (E.chunk_last_k_lost(127), "pair", "D=371", None),
    (E.bias_neighbour(), "pair", "headline-like D=74", None),
    (E.features_bf16(), "pair", "headline-like D=74", None),
    (E.last_range_dropped(), "pair", "headline-like D=74", None),
    (E.second_zslice_lost(), "pair", "D=80", None),
    (E.second_zslice_lost(), "pair", "D=81", None),
    (E.last_range_wave_lost(), "pair", "D=371", None),
    (E.last_range_wave_lost(), "pair", "headline-like D=74", None),
]


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _runs_case(which):
    B, T, V, H = 192, 50, 3000, 128
    ids, _ = E.make_ids(B, T, V, 31)
    src = E.make_d(B * T, H, 32)
    g = torch.Generator().manual_seed(33)
    if which == "table":
        return ids, src, torch.randn(V, H, generator=g), V, None
    union = torch.unique(ids[::3][(ids[::3] > 0) & (ids[::3] < V)])
    return ids, src, torch.randn(union.numel(), H, generator=g), V, union


@pytest.mark.parametrize("j", range(len(MUTATIONS)), ids=[f"{m.name} ({c}, det {d})" for m, _, c, d in MUTATIONS])
def test_mutation_fails_the_check(j):
    mut, kind, case, det = MUTATIONS[j]
    if kind in ("emb", "gather"):
        c = _cached(("emb", case), lambda: emb_case(**EMB[case]))
        if kind == "gather":
            ref = _cached(("gather", case), lambda: E.gather(c["ids"], c["tts"], c["word"], c["typ"], c["pos"], c["T"]))
            margin = E.ratios(E.gather(c["ids"], c["tts"], c["word"], c["typ"], c["pos"], c["T"], emu=True, mutation=mut), ref).worst
        else:
            ref = _cached(("scatter", case, det), lambda: _scatter(c, det))
            margin = _worst(_scatter(c, det, emu=True, mutation=mut), ref)
    elif kind == "runs":
        ids, src, d0, V, union = _cached(("runs", case), lambda: _runs_case(case))
        ref = E.rows_sum(ids, src, d0, V, union=union, det=det)
        _, em = E.rows_sum(ids, src, d0, V, union=union, det=det, emu=True, mutation=mut)
        margin = E.ratios(em, ref, gathered=True).worst
    else:
        c = _cached(("pair", case), lambda: pair_case(**PAIR[case]))
        ref = _cached(("pairref", case), lambda: _pair(c))
        margin = _worst(_pair(c, emu=True, mutation=mut), ref)
    print(f"\n{mut.name}: margin {margin:.3g}")
    assert margin >= MIN_MARGIN, (mut.name, margin)
