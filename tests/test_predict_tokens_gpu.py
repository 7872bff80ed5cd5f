"""``MMBertForPretraining.predict_tokens`` / ``trainer.mlm_eval_epoch``: masked-token prediction without the [tokens, vocab] scores.

* in situ: ``ops.vocab_topk`` is wrapped and every launch recorded -- its ids and label ranks must equal the float64 reference
  (tests/vocab_topk_ref.py) on the launch's OWN logits exactly, its log-probabilities must be within that reference's model;
* the recorded logits and the per-pass ``loss`` against the fp32 CPU oracle's prediction scores at the same rows, at the bounds
  tests/test_model_gpu.py states for the MLM head at two layers: scores 3e-2 absolute, losses 3e-3 relative; the measured deviations go
  to the suite's report directory as predict_tokens_parity.json (test_model_gpu._report).  Predicted ids are NOT compared with the
  oracle's (near-ties would need a leave-out rule): the in-situ check carries id exactness;
* ``index`` = the label positions of each pass in order; ``positions`` mode = the same rows and ids; no rows (per pass and overall);
  ``token_chunk_rows = 4``; the argument errors; a call between deterministic train steps changes nothing; ``mlm_eval_epoch`` end to end."""
import inspect
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmbert_oracle as O
from msa_amd.data import synthetic_batch, batch_to

import tests.test_model_gpu as TM
from tests import vocab_topk_ref as VT

DEV = "cuda"
CFG1 = TM.CFG1
NAMES = ("text", "visual", "speech")
# tests/test_model_gpu.py: check_against_oracle's own score_tol / loss_tol at L = 2 (3e-2 absolute, 3e-3 relative), read from its signature
_TOLS = inspect.signature(TM.check_against_oracle).parameters
SCORE_TOL, LOSS_TOL = _TOLS["score_tol"].default, _TOLS["loss_tol"].default
# (configuration, (B, T, Pv, Pa), full_length = no text padding, seed); P == T in the second: the pair positions carry labels too
CASES = {"padded_B2": (CFG1, (2, 50, 64, 64), False, 1), "full_B3": (dict(CFG1, vocab=4096), (3, 24, 24, 24), True, 6)}
_PARITY = {}
_runs = {}


def _args3(batch):
    return batch["input_ids"], batch["token_type_ids"], batch["attention_mask"]


class Recorder:
    """Wraps ops.vocab_topk (and counts the vocabulary-sized gemm_nt launches) for the duration of a ``with`` block."""

    def __init__(self, vpad=None):
        self.launches, self.vocab_gemms, self.vpad = [], 0, vpad

    def __enter__(self):
        from msa_amd import ops
        self.ops, self.orig, self.orig_gemm = ops, ops.vocab_topk, ops.gemm_nt

        def topk(logits, V, k, labels=None):
            out = self.orig(logits, V, k, labels)
            self.launches.append(dict(logits=logits.detach().cpu(), V=V, k=k, labels=None if labels is None else labels.cpu(),
                                      out=[o.cpu() for o in out]))
            return out

        def gemm(A, B, **kw):
            if self.vpad is not None and B.shape[0] == self.vpad:
                self.vocab_gemms += 1
            return self.orig_gemm(A, B, **kw)
        ops.vocab_topk, ops.gemm_nt = topk, gemm
        return self

    def __exit__(self, *exc):
        self.ops.vocab_topk, self.ops.gemm_nt = self.orig, self.orig_gemm
        return False


def check_launches(launches, what):
    """Every recorded launch against the reference on its own logits: ids and ranks exact, log-probabilities within the model."""
    worst = {}
    for j, l in enumerate(launches):
        ref = VT.reference(l["logits"], l["V"], l["k"], l["labels"])
        got = dict(zip(("top_ids", "top_logprob", "row_lse", "label_logprob", "label_rank"), l["out"]))
        for n, q in VT.check(got, ref, f"{what} launch {j}").items():
            worst[n] = max(worst.get(n, 0.0), q.elem, q.norm)
    return worst


def run_case(name):
    """Model, batch, predict_tokens result, recorded launches -- once per case, shared by the tests (nothing here is modified later)."""
    if name not in _runs:
        cfg, shape, full, seed = CASES[name]
        batch = synthetic_batch(*shape, dataset=cfg["dataset"], vocab=cfg["vocab"], seed=seed, full_length=full)
        m = TM.build(cfg)
        dbatch = batch_to(batch, DEV)
        with Recorder() as rec:
            res = m.predict_tokens(*_args3(dbatch), masked_labels=dbatch["masked_labels"], top_k=5)
        torch.cuda.synchronize()
        _runs[name] = dict(cfg=cfg, shape=shape, batch=batch, dbatch=dbatch, m=m, res=res, launches=rec.launches)
    return _runs[name]


def label_positions(labels, V):
    return torch.nonzero((labels >= 0) & (labels < V))           # row-major: ascending by sample, then position


@pytest.mark.parametrize("name", list(CASES))
def test_every_launch_matches_the_reference_on_its_own_logits(name):
    r = run_case(name)
    V = r["cfg"]["vocab"]
    n = sum(int(((l >= 0) & (l < V)).sum()) for l in r["batch"]["masked_labels"])
    assert n > 0 and len(r["launches"]) == 1 and r["launches"][0]["logits"].shape == (n, r["m"]._flat.vpad)
    assert r["launches"][0]["logits"].dtype == torch.bfloat16
    worst = check_launches(r["launches"], name)
    _PARITY.setdefault(name, {})["in_situ_worst_ratio"] = worst
    print(name, "in situ, largest ratios:", worst)


@pytest.mark.parametrize("name", list(CASES))
def test_result_layout_and_index(name):
    r = run_case(name)
    res, V = r["res"], r["cfg"]["vocab"]
    assert set(res) == set(NAMES) | {"loss"} and res["loss"].shape == (3,) and res["loss"].dtype == torch.float32
    out = [o for o in r["launches"][0]["out"]]
    lo = 0
    for p, nme in enumerate(NAMES):
        e, lab = res[nme], r["batch"]["masked_labels"][p]
        pos = label_positions(lab, V)
        n = pos.shape[0]
        assert e["index"].dtype == torch.int64 and torch.equal(e["index"].cpu(), pos), nme
        assert e["top_ids"].dtype == torch.int64 and e["top_ids"].shape == (n, 5) and e["top_logprob"].shape == (n, 5)
        assert e["top_logprob"].dtype == torch.float32 and e["label_logprob"].dtype == torch.float32 and e["label_rank"].dtype == torch.int64
        assert torch.equal(e["label"].cpu(), lab[pos[:, 0], pos[:, 1]])
        # the launch's rows, pass by pass, in order
        assert torch.equal(e["top_ids"].cpu(), out[0][lo:lo + n].long()) and torch.equal(e["top_logprob"].cpu(), out[1][lo:lo + n])
        assert torch.equal(e["label_logprob"].cpu(), out[3][lo:lo + n]) and torch.equal(e["label_rank"].cpu(), out[4][lo:lo + n].long())
        assert bool(((e["label_rank"] == 0) == (e["top_ids"][:, 0] == e["label"])).all())
        assert bool(((e["label_rank"] < 5) == (e["top_ids"] == e["label"][:, None]).any(1)).all())
        want = float(-e["label_logprob"].double().mean()) if n else 0.0
        assert abs(float(res["loss"][p]) - want) <= 1e-5 * max(1.0, abs(want)), (nme, float(res["loss"][p]), want)
        lo += n
    assert lo == out[0].shape[0]
    if name == "full_B3":
        assert bool((res["visual"]["index"][:, 1] >= 24).any())     # P == T: labelled pair positions


@pytest.mark.parametrize("name", list(CASES))
def test_logits_and_losses_against_the_oracle(name):
    r = run_case(name)
    cfg, res = r["cfg"], r["res"]
    V = cfg["vocab"]
    p = O.seeded_params(cfg)
    ocfg = dict(cfg, hidden_dropout=0.0, attn_dropout=0.0, joint_dropout=0.0)
    with torch.no_grad():
        oout, _ = O.pretraining_forward(p, ocfg, **r["batch"])
    logits = r["launches"][0]["logits"].float()[:, :V]
    rep, lo = {}, 0
    for q, nme in enumerate(NAMES):
        idx = res[nme]["index"].cpu()
        n = idx.shape[0]
        scores = oout[7 + 2 * q].detach()[idx[:, 0], idx[:, 1]]                      # [n, V] fp32
        lab = res[nme]["label"].cpu()
        d = (logits[lo:lo + n] - scores).abs()
        oloss = float(torch.nn.functional.cross_entropy(scores.double(), lab)) if n else 0.0
        ours = float(res["loss"][q])
        rep[nme] = dict(rows=n, score_max_abs=float(d.max()) if n else 0.0, score_mean_abs=float(d.mean()) if n else 0.0, score_bound=SCORE_TOL,
                        loss=ours, oracle_loss=oloss, loss_rel=abs(ours - oloss) / max(abs(oloss), 1e-6), loss_bound=LOSS_TOL)
        lo += n
    _PARITY.setdefault(name, {}).update(shape=list(r["shape"]), vocab=V, layers=cfg["layers"], hidden=cfg["hidden"], passes=rep)
    TM._report("predict_tokens_parity", _PARITY)
    print(name, json.dumps(rep))
    for nme, v in rep.items():
        assert v["rows"] > 0
        assert v["score_max_abs"] < SCORE_TOL, (nme, v)
        assert v["loss_rel"] < LOSS_TOL, (nme, v)


@pytest.mark.parametrize("name", list(CASES))
def test_positions_mode_returns_the_same_rows_and_ids(name):
    r = run_case(name)
    V, m, db = r["cfg"]["vocab"], r["m"], r["dbatch"]
    positions = tuple((l >= 0) & (l < V) for l in db["masked_labels"])
    with Recorder() as rec:
        res = m.predict_tokens(*_args3(db), positions=positions, top_k=5)
    torch.cuda.synchronize()
    assert len(rec.launches) == 1 and rec.launches[0]["labels"] is None and len(rec.launches[0]["out"]) == 3
    check_launches(rec.launches, name + " positions")
    assert bool((res["loss"] == 0).all())
    for nme in NAMES:
        assert set(res[nme]) == {"index", "top_ids", "top_logprob"}
        for key in ("index", "top_ids", "top_logprob"):
            assert torch.equal(res[nme][key], r["res"][nme][key]), (nme, key)


def test_small_chunks_keep_the_order():
    r = run_case("full_B3")
    m, db = r["m"], r["dbatch"]
    n = sum(r["res"][nme]["index"].shape[0] for nme in NAMES)
    was = m.token_chunk_rows
    try:
        m.token_chunk_rows = 4
        with Recorder() as rec:
            res = m.predict_tokens(*_args3(db), masked_labels=db["masked_labels"], top_k=5)
    finally:
        m.token_chunk_rows = was
    torch.cuda.synchronize()
    assert [l["logits"].shape[0] for l in rec.launches] == [4] * (n // 4) + ([n % 4] if n % 4 else [])
    check_launches(rec.launches, "chunks of 4")
    for nme in NAMES:
        assert torch.equal(res[nme]["index"], r["res"][nme]["index"]) and torch.equal(res[nme]["label"], r["res"][nme]["label"])
        assert res[nme]["top_ids"].shape == r["res"][nme]["top_ids"].shape
    # top_k = 1 and 8 run through the same path
    for k in (1, 8):
        with Recorder() as rec:
            res = m.predict_tokens(*_args3(db), masked_labels=db["masked_labels"], top_k=k)
        check_launches(rec.launches, f"top_k={k}")
        assert res["text"]["top_ids"].shape[1] == k


def test_no_rows_per_pass_and_overall():
    r = run_case("padded_B2")
    m, db = r["m"], r["dbatch"]
    lab = db["masked_labels"]
    none = tuple(torch.full_like(l, -100) for l in lab)

    def empty_ok(e, with_labels):
        assert e["index"].shape == (0, 2) and e["index"].dtype == torch.int64
        assert e["top_ids"].shape == (0, 3) and e["top_ids"].dtype == torch.int64
        assert e["top_logprob"].shape == (0, 3) and e["top_logprob"].dtype == torch.float32
        if with_labels:
            assert e["label"].shape == (0,) and e["label"].dtype == torch.int64 and e["label_rank"].dtype == torch.int64
            assert e["label_logprob"].shape == (0,) and e["label_logprob"].dtype == torch.float32
    with Recorder(vpad=m._flat.vpad) as rec:
        res = m.predict_tokens(*_args3(db), masked_labels=none, top_k=3)
        res_p = m.predict_tokens(*_args3(db), positions=tuple(torch.zeros_like(l, dtype=torch.bool) for l in lab), top_k=3)
    assert not rec.launches and rec.vocab_gemms == 0                     # no rows: none of the head's launches
    for nme in NAMES:
        empty_ok(res[nme], True)
        empty_ok(res_p[nme], False)
    assert bool((res["loss"] == 0).all()) and res["loss"].shape == (3,)
    with Recorder(vpad=m._flat.vpad) as rec:                              # the text pass alone carries labels
        res = m.predict_tokens(*_args3(db), masked_labels=(lab[0], none[1], none[2]), top_k=3)
    assert len(rec.launches) == 1 and rec.vocab_gemms == 1
    check_launches(rec.launches, "text only")
    empty_ok(res["visual"], True)
    empty_ok(res["speech"], True)
    assert res["text"]["index"].shape[0] == rec.launches[0]["logits"].shape[0] > 0
    assert float(res["loss"][0]) > 0 and float(res["loss"][1]) == 0 and float(res["loss"][2]) == 0


def test_argument_errors():
    r = run_case("padded_B2")
    m, db, V = r["m"], r["dbatch"], r["cfg"]["vocab"]
    lab = db["masked_labels"]
    pos = tuple(l >= 0 for l in lab)
    with pytest.raises(ValueError):
        m.predict_tokens(*_args3(db))
    with pytest.raises(ValueError):
        m.predict_tokens(*_args3(db), masked_labels=lab, positions=pos)
    for k in (0, 9):
        with pytest.raises(ValueError):
            m.predict_tokens(*_args3(db), masked_labels=lab, top_k=k)
    with pytest.raises(ValueError):
        m.predict_tokens(*_args3(db), masked_labels=(lab[0], lab[1][:, :-1], lab[2]))
    bad = lab[0].clone()
    bad[0, 3] = V
    with pytest.raises(IndexError):
        m.predict_tokens(*_args3(db), masked_labels=(bad, lab[1], lab[2]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.predict_tokens(*_args3(r["batch"]), masked_labels=r["batch"]["masked_labels"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("async_prologue", [False, True])
def test_call_between_two_train_steps_changes_nothing(async_prologue):
    """Deterministic mode, train mode with dropout: step, predict_tokens, step == step, step -- losses, gradients and parameters bit for
    bit; ``model.training`` and ``model.outputs`` are left alone."""
    from msa_amd import ops
    from msa_amd import trainer as T
    import tests.test_train_gpu as TT
    cfg = dict(hidden=128, layers=2, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)
    shape = (4, 24, 60, 40)
    pool = [batch_to(synthetic_batch(*shape, dataset="mosei", vocab=cfg["vocab"], seed=90 + i), DEV) for i in range(3)]
    torch.cuda.synchronize()

    def run(with_call):
        m = TT.build(cfg, dropout=0.1)
        m.train()
        m.manual_seed(17)
        m.async_prologue = async_prologue
        opt, sched = T.build_optimizer(m, T.default_args(train_batch_size=shape[0], learning_rate=1e-3), 10, mode="hf")
        sched.step()
        losses, grads = [], []
        for i in range(3):
            out, _ = m(**pool[i])
            out[0].mean().backward()
            losses.append(out[0].detach().clone())
            grads.append(m._flat.grads.clone())
            opt.step(); sched.step(); opt.zero_grad()
            if with_call:
                held = m.outputs
                nb = pool[(i + 1) % 3]
                res = m.predict_tokens(*_args3(nb), masked_labels=nb["masked_labels"])
                assert m.training and m.outputs is held and bool(torch.isfinite(res["loss"]).all())
                assert not res["text"]["top_logprob"].requires_grad
                assert not m.__dict__.get("_late_wgrads")
        torch.cuda.synchronize()
        return losses, grads, m._flat.params.clone()
    was = ops.deterministic()
    try:
        ops.set_deterministic(True)
        a, b = run(False), run(True)
    finally:
        ops.set_deterministic(was)
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), (i, float(x), float(y))
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), f"gradients of step {i} differ"
    assert torch.equal(a[2], b[2])


def test_mlm_eval_epoch_end_to_end():
    from torch.utils.data import DataLoader, Dataset
    from tests.golden.dataset_features import synthetic_features
    from msa_amd import trainer as T
    from msa_amd.dataset import MMBertDataset
    import random
    random.seed(5)
    ds0 = MMBertDataset(None, synthetic_features(n_items=10, L=10, seed=3), "mosei", "sentiment", 1)
    items = [ds0[i] for i in range(len(ds0))]                   # (the dataset draws its negative pairs from `random` at every access)

    class Frozen(Dataset):
        def __len__(self):
            return len(items)

        def __getitem__(self, i):
            return items[i]
    ds = Frozen()
    V = 30522
    m = TM.build(dict(CFG1, vocab=V), train=True)
    for mlm in (True, False):
        args = T.default_args(val_batch_size=4, mlm=mlm)
        torch.manual_seed(123)
        got = T.mlm_eval_epoch(args, m, ds, device=DEV, top_k=5)
        assert m.training
        torch.manual_seed(123)                                   # the same loader and the same mask draws, replayed
        want = [0, 0, 0]
        for b in DataLoader(ds, batch_size=4, collate_fn=T.collate):
            kw = T.pack_step_inputs(b, args, DEV)
            for p in range(3):
                want[p] += int(((kw["masked_labels"][p] >= 0) & (kw["masked_labels"][p] < V)).sum())
        print("mlm =", mlm, got)
        for p, nme in enumerate(NAMES):
            g = got[nme]
            assert g["count"] == want[p] > 0, (nme, g, want)
            assert 0.0 <= g["top1"] <= g["topk"] <= 1.0 and g["top1"] <= g["mrr"] <= 1.0
            if g["count"]:
                assert g["loss"] > 0 and abs(g["perplexity"] - torch.tensor(g["loss"]).exp().item()) <= 1e-3 * g["perplexity"]
    empty = T.mlm_eval_epoch(T.default_args(val_batch_size=4), m, None, device=DEV, batches=[])
    assert all(empty[nme] == dict(count=0, loss=0.0, perplexity=0.0, top1=0.0, topk=0.0, mrr=0.0) for nme in NAMES)
