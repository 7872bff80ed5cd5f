"""GPU tests of the weight EMA on the model: AdamW.ema() moves no bit of a training trajectory on any of the three step routes, the
average follows float64, the step still syncs nothing, swap_ema() / ema_weights() put the averages under every path of the model and
take them out again bit for bit, the refusals while swapped, the state-dict round trip, and trainer.train evaluating and saving under
the averaged weights.  Deterministic mode throughout: two freshly built models then take bit-identical steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ema_ref as E
from tests.test_adamw_groups_gpu import CFG, _batch, _fb, build

DEV = "cuda"
LR = 1e-3
ROUTES = ["reference", "clip", "layerwise"]


@pytest.fixture(autouse=True)
def deterministic_mode():
    from msa_amd import ops
    was = ops.deterministic()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(was)


def _opt(route, m):
    from msa_amd.optim import AdamW, layerwise_param_groups
    if route == "layerwise":
        return AdamW(layerwise_param_groups(m, LR, layer_decay=0.8, head_lr=5 * LR), lr=LR)
    opt = AdamW(layerwise_param_groups(m, LR), lr=LR)                       # the reference's two groups
    assert len(opt.param_groups) == 2
    return opt


def _step(route, opt):
    if route == "clip":
        opt.clip_grad_norm_(1.0)
    opt.step()
    opt.zero_grad()


def _args3(b):
    return b["input_ids"], b["token_type_ids"], b["attention_mask"]


def _same_state(m1, o1, m2, o2, tag):
    for name, a, b in (("params", m1._flat.params, m2._flat.params), ("m", o1._m, o2._m), ("v", o1._v, o2._v),
                       ("half", m1._flat.half, m2._flat.half)):
        assert torch.equal(a, b), (tag, name)


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("route", ROUTES)
def test_ema_moves_no_bit_of_training_and_swaps_exactly(route, warmup, monkeypatch):
    from msa_amd import ops
    from msa_amd.optim import ema_decay_at
    calls = {"ema": 0, "other": 0}
    for name in ("adamw", "adamw_devscale", "adamw_grouped", "adamw_ema"):
        def spy(*a, _f=getattr(ops, name), _k="ema" if name == "adamw_ema" else "other", **k):
            calls[_k] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    m1, m2 = build(), build()
    o1, o2 = _opt(route, m1).ema(0.9, warmup=warmup), _opt(route, m2)
    for k in range(4):
        for m in (m1, m2):
            _fb(m, _batch(30 + k))
        flat = m1._flat
        e_prev = (flat.params if o1._ema is None else o1._ema).clone()     # (not bound yet: the average starts as a copy of the parameters)
        torch.cuda.synchronize()
        if k == 2:
            torch.cuda.set_sync_debug_mode("error")                       # the step with the average syncs nothing
        try:
            _step(route, o1)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert calls == {"ema": k + 1, "other": 0}
        _step(route, o2)
        assert calls == {"ema": k + 1, "other": 1}
        calls["other"] = 0
        _same_state(m1, o1, m2, o2, k)
        omd = E.omd_f32(ema_decay_at(0.9, k, warmup))
        ref, tol = E.ema_step(e_prev, flat.params, omd), E.ema_bound(e_prev, flat.params, omd)
        live = ((o1._flags & 3) != 2).repeat_interleave(256)
        err = (o1._ema.double() - ref).abs()
        assert bool((err <= tol)[live].all()), (k, float((err / tol)[live].max()))
        assert torch.equal(o1._ema[~live], e_prev[~live]) and bool(live.any()) and not bool(live.all())
        assert not torch.equal(o1._ema[live], flat.params[live]) and not torch.equal(o1._ema[live], e_prev[live])
    assert o1.ema_updates == 4 and o2.ema_updates == 0 and o2._ema is None
    if warmup:
        return                                                              # (the swap below does not depend on the decays)

    # ---- the averages under every path of the model ----
    flat = m1._flat
    b = _batch(77)
    esd = o1.ema_state_dict()
    torch.cuda.synchronize()
    before = [x.clone() for x in (flat.params, flat.half, flat.halfT, o1._ema)]
    versions = flat._param_versions()
    with torch.no_grad():
        trained_pred = m1.predict(*_args3(b))
    with o1.ema_weights():
        assert torch.equal(flat.params, before[3]) and torch.equal(o1._ema, before[0])
        assert torch.equal(flat.half, flat.params.bfloat16())
        torch.cuda.synchronize()
        hT = flat.halfT.clone()
        flat.refresh()
        torch.cuda.synchronize()
        assert torch.equal(flat.halfT, hT) and torch.equal(flat.half, flat.params.bfloat16())
        sd = m1.state_dict()
        assert set(sd) == set(esd) and all(torch.equal(sd[k], esd[k]) for k in sd)
        assert all(torch.equal(v, sd[k]) for k, v in o1.ema_state_dict().items())
        fresh = build()
        fresh.load_state_dict(esd)
        with torch.no_grad():
            got, want = m1.predict(*_args3(b)), fresh.predict(*_args3(b))
            assert torch.equal(got, want) and not torch.equal(got, trained_pred)
            (lo1, _), (lo2, _) = m1(**b), fresh(**b)
            assert torch.equal(lo1[0], lo2[0])
            t1 = m1.predict_tokens(*_args3(b), masked_labels=b["masked_labels"])
            t2 = fresh.predict_tokens(*_args3(b), masked_labels=b["masked_labels"])
            assert torch.equal(t1["text"]["top_logprob"], t2["text"]["top_logprob"])
        for call in (o1.step, lambda: o1.clip_grad_norm_(1.0), o1.state_dict, o1.ema_weights().__enter__):
            with pytest.raises(RuntimeError, match="swapped"):
                call()
    torch.cuda.synchronize()
    for name, x, y in zip(("params", "half", "halfT", "ema"), (flat.params, flat.half, flat.halfT, o1._ema), before):
        assert torch.equal(x, y), name
    assert flat._param_versions() == versions and calls == {"ema": 4, "other": 0}
    with torch.no_grad():
        assert torch.equal(m1.predict(*_args3(b)), trained_pred)
    for m in (m1, m2):
        _fb(m, _batch(40))
    _step(route, o1)
    _step(route, o2)
    _same_state(m1, o1, m2, o2, "after the swap")


def test_state_dict_round_trip_and_dicts_without_the_ema():
    from msa_amd.optim import AdamW
    m = build()
    o1 = _opt("layerwise", m).ema(0.9, warmup=True)
    o1.lazy_zero = False
    _fb(m, _batch(20))
    o1.step()
    o1.zero_grad()
    sd = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in o1.state_dict().items()}
    assert sd["ema_decay"] == 0.9 and sd["ema_warmup"] is True and sd["ema_updates"] == 1 and torch.equal(sd["ema"], o1._ema)
    _fb(m, _batch(21))
    flat = m._flat
    p0, g0 = flat.params.clone(), flat.grads.clone()
    o1.step()
    want = [x.clone() for x in (flat.params, o1._ema, o1._m, o1._v)]
    o2 = _opt("layerwise", m)
    o2.lazy_zero = False
    o2.load_state_dict(sd)
    assert o2.ema_updates == 1 and o2._ema_warmup is True
    flat.params.copy_(p0)
    flat.grads.copy_(g0)
    o2.step()
    for name, a, b in zip(("p", "ema", "m", "v"), want, (flat.params, o2._ema, o2._m, o2._v)):
        assert torch.equal(a, b), name
    # a dict without the four keys (an earlier version's) loads and leaves the EMA as it is: on, with its values, or off
    old = {k: v for k, v in sd.items() if not k.startswith("ema")}
    assert len(old) == len(sd) - 4
    kept = o2._ema.clone()
    o2.load_state_dict(old)
    assert o2._ema_decay == 0.9 and o2.ema_updates == 2 and torch.equal(o2._ema, kept)
    o3 = _opt("layerwise", m)
    o3.load_state_dict(old)
    assert o3._ema is None and o3._ema_decay is None
    with pytest.raises(RuntimeError, match="no EMA"):
        o3.swap_ema()


def test_enabling_late_changing_the_decay_and_reset():
    from msa_amd.optim import AdamW
    m = build()
    opt = _opt("reference", m)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            opt.ema(bad)
    assert opt._ema_decay is None
    _fb(m, _batch(5))
    _step("reference", opt)
    flat = m._flat
    assert opt.ema(0.5) is opt and torch.equal(opt._ema, flat.params)       # bound already: the copy is made at once
    _fb(m, _batch(6))
    p_prev = flat.params.clone()
    _step("reference", opt)
    ref = E.ema_step(p_prev, flat.params, 0.5)
    live = ((opt._flags & 3) != 2).repeat_interleave(256)
    assert bool(((opt._ema.double() - ref).abs() <= E.ema_bound(p_prev, flat.params, 0.5))[live].all())
    e = opt._ema.clone()
    opt.ema(0.75, warmup=True)                                              # a new decay keeps the average and its count
    assert torch.equal(opt._ema, e) and opt.ema_updates == 1 and opt._ema_decay == 0.75
    opt.ema_reset()
    assert torch.equal(opt._ema, flat.params) and opt.ema_updates == 0


@pytest.mark.parametrize("route", ROUTES)
def test_without_ema_the_fused_kernel_is_never_launched(route, monkeypatch):
    from msa_amd import ops

    def refuse(*a, **k):
        raise AssertionError("a step without an EMA launched mmbert_adamw_ema")
    monkeypatch.setattr(ops, "adamw_ema", refuse)
    m = build()
    opt = _opt(route, m)
    _fb(m, _batch(8))
    before = m._flat.params.clone()
    _step(route, opt)
    assert not torch.equal(before, m._flat.params)
    assert set(opt.state_dict()) >= {"steps", "m", "v", "lrs"} and opt.state_dict()["ema"] is None


def test_trainer_evaluates_and_saves_under_the_averaged_weights(tmp_path, monkeypatch):
    from msa_amd import trainer as T
    seen = []

    def rising(preds, y, use_zero=False):                                   # every epoch improves: every epoch saves
        seen.append(1)
        return 0.1 * len(seen), 0.0, 0.0
    monkeypatch.setattr(T, "test_MSE_score_model", rising)

    def run(tag, **extra):
        m = build()
        args = T.default_args(train_batch_size=2, val_batch_size=2, learning_rate=LR, n_epochs=2, num_labels=7, **extra)
        opt, sched = T.build_optimizer(m, args, 4)
        sched.step()                                                        # (lr > 0 from the first step on)
        snaps = {}

        def batches(split, epoch):
            if split == "val" and opt._ema_decay is not None:               # the epoch's training is over: its averages
                snaps[epoch] = opt.ema_state_dict()
            if split == "val":
                snaps[("live", epoch)] = {k: v.clone() for k, v in m.state_dict().items()}
            base = {"train": 100, "val": 200, "test": 300}[split]
            return [_batch(base + 10 * epoch + i) for i in range(2)]
        best = T.train(args, m, None, None, None, opt, sched, epoch_batches=batches, save_root=str(tmp_path / tag / "model_save"),
                       numpy_root=str(tmp_path / tag / "numpy_save"), patience_limit=5)
        files = {e: torch.load(f"{best['save_dir']}/model_{e + 1}.pt", map_location=DEV) for e in range(2)}
        return m, opt, snaps, files

    m1, o1, snaps, files = run("ema", ema_decay=0.9, gradient_accumulation_step=1)
    assert o1._ema is not None and o1.ema_updates == 2 and not o1._swapped   # (one optimizer step per epoch of two micro-batches)
    for e in range(2):
        assert set(files[e]) == set(snaps[e]) and all(torch.equal(files[e][k], snaps[e][k]) for k in files[e]), e
    final = o1.ema_state_dict()
    assert all(torch.equal(files[1][k], final[k]) for k in final)
    assert not all(torch.equal(files[1][k], v) for k, v in m1.state_dict().items())
    m2, o2, snaps2, files2 = run("plain")
    assert o2._ema is None
    assert torch.equal(m1._flat.params, m2._flat.params)                    # the live parameters are the trained ones
    for e in range(2):                                                      # without the argument: the file is the live parameters
        assert all(torch.equal(files2[e][k], snaps2[("live", e)][k]) for k in files2[e]), e
    assert all(torch.equal(files2[1][k], v) for k, v in m2.state_dict().items())
