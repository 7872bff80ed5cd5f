"""GPU tests of per-parameter-group AdamW: the grouped kernel (mmbert_adamw_grouped) against float64 with every flag, mode and scale
form, bit-identity with the single-set kernel when every group shares one combination, the model-level step against the per-group
oracle (layer-wise lr decay, own betas / eps, two weight decays, a warm-up schedule, clipping), no host sync, the reference's grouping
staying on the single-set kernel, and the refusals."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmbert_oracle as O
from msa_amd.data import synthetic_batch, batch_to

DEV = "cuda"
CFG = dict(hidden=128, layers=2, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)


def build(cfg=CFG):
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    c = MMBertConfig(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                     intermediate_size=cfg["intermediate"], hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = MMBertForPretraining(c)
    m.bert.set_joint_embeddings(cfg["dataset"])
    m.bert.jointEmbeddings.dropout_prob = 0.0
    m.load_state_dict(O.seeded_params(cfg), strict=False)
    m = m.to(DEV)
    m.eval()
    return m


def _batch(seed, cfg=CFG):
    return batch_to(synthetic_batch(2, 16, 40, 24, vocab=cfg["vocab"], seed=seed), DEV)


def _fb(m, b):
    out, _ = m(**b)
    out[0].mean().backward()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against float64
# ---------------------------------------------------------------------------------------------------------------------------------
HYPER7 = [(1e-3, 0.9, 0.999, 1e-6, 0.01), (3e-4, 0.85, 0.99, 1e-8, 0.0), (2e-3, 0.95, 0.9995, 1e-7, 0.1), (5e-5, 0.8, 0.98, 1e-5, 0.05),
          (1e-2, 0.9, 0.999, 1e-6, 0.2), (7e-4, 0.5, 0.9, 3e-6, 0.001), (1e-3, 0.9, 0.999, 1e-6, 0.3)]


def _slot_coefs(h, step, mode):
    """mmbert_adamw_grouped's coefficients of one (lr, beta1, beta2, eps, wd): formed in double, rounded to fp32 once (as float64 values)"""
    lr, b1, b2, eps, wd = h
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    ss = lr * math.sqrt(bc2) / bc1 if mode == 0 else lr / bc1
    return [float(np.float32(x)) for x in (b1, b2, 1.0 - b1, 1.0 - b2, eps, ss, 1.0 / math.sqrt(bc2), lr * wd)]


def _random_state(nblk, seed):
    gen = torch.Generator(DEV).manual_seed(seed)
    n = nblk * 256
    p = torch.randn(n, device=DEV, generator=gen)
    g = torch.randn(n, device=DEV, generator=gen) * 0.05
    m = torch.randn(n, device=DEV, generator=gen) * 0.01
    v = torch.rand(n, device=DEV, generator=gen) * 1e-3
    rng = np.random.default_rng(seed)
    flags = torch.from_numpy((rng.integers(0, 3, nblk) + 4 * rng.integers(0, 2, nblk)).astype(np.uint8)).to(DEV)
    return p, g, m, v, flags, rng


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("dev_scale", [False, True])
def test_grouped_kernel_against_float64(mode, step, dev_scale):
    from msa_amd import ops
    nblk = 4099
    p, g, m, v, flags, rng = _random_state(nblk, 1000 + 10 * step + mode + 2 * dev_scale)
    gmap = torch.from_numpy(rng.integers(0, len(HYPER7), nblk).astype(np.uint8)).to(DEV)
    gscale = 0.37
    coef = torch.tensor([gscale], device=DEV) if dev_scale else None
    pd, gd, md, vd = p.clone(), g.clone(), m.clone(), v.clone()
    pb = torch.empty_like(p, dtype=torch.bfloat16)
    ops.adamw_grouped(pd, gd, md, vd, pb, flags, gmap, HYPER7, step=step, gscale=1.0 if dev_scale else gscale, coef=coef, mode=mode)
    torch.cuda.synchronize()
    # float64 evaluation of the rule with the fp32 slot coefficients
    C = torch.tensor([_slot_coefs(h, step, mode) for h in HYPER7], dtype=torch.float64)
    c = C[gmap.long().cpu()].repeat_interleave(256, dim=0)                   # [n, 8]
    b1, b2, omb1, omb2, eps, ss, rsbc2, lrwd = c.unbind(1)
    fl = flags.cpu().long().repeat_interleave(256)
    f = fl & 3
    decay = torch.where(f == 1, lrwd, torch.zeros_like(lrwd))
    P0, G0, M0, V0 = (x.double().cpu() for x in (p, g, m, v))
    gr = G0 * float(np.float32(gscale))
    P = P0 * (1.0 - decay) if mode == 1 else P0.clone()
    M = b1 * M0 + omb1 * gr
    V = b2 * V0 + omb2 * gr * gr
    if mode == 0:
        upd = ss * M / (V.sqrt() + eps)
        P = P - upd
        P = P - decay * P
    else:
        upd = ss * M / (V.sqrt() * rsbc2 + eps)
        P = P - upd
    live = f != 2
    got_p, got_m, got_v = pd.double().cpu(), md.double().cpu(), vd.double().cpu()
    # (bounds of the G11 test, relative to the magnitude of the terms: fp32 roundings only)
    mscale = (b1 * M0).abs() + (omb1 * gr).abs()
    assert bool(((got_m - M).abs() <= 5e-7 * mscale + 1e-30)[live].all()), float(((got_m - M).abs() / (mscale + 1e-30))[live].max())
    assert bool(((got_v - V).abs() <= 5e-7 * V + 1e-30)[live].all()), float(((got_v - V).abs() / (V + 1e-30))[live].max())
    pscale = P0.abs() + upd.abs()
    assert bool(((got_p - P).abs() <= 2e-6 * pscale)[live].all()), float(((got_p - P).abs() / pscale)[live].max())
    # frozen blocks bit-unchanged; zero_grad except the lazy (+4) blocks; bf16 copy = the new p rounded
    frozen = ~live
    assert torch.equal(pd.cpu()[frozen], p.cpu()[frozen]) and torch.equal(md.cpu()[frozen], m.cpu()[frozen])
    assert torch.equal(vd.cpu()[frozen], v.cpu()[frozen])
    lazy = (fl & 4) != 0
    assert torch.equal(gd.cpu()[lazy], g.cpu()[lazy]) and float(gd.cpu()[~lazy].abs().max()) == 0.0
    assert torch.equal(pb, pd.bfloat16())
    # zero_grad off: the gradient is read only; no bf16 copy: nothing else changes
    g2 = g.clone()
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    ops.adamw_grouped(p2, g2, m2, v2, None, flags, gmap, HYPER7, step=step, gscale=1.0 if dev_scale else gscale, coef=coef, mode=mode,
                      zero_grad=False)
    assert torch.equal(g2, g) and torch.equal(p2, pd) and torch.equal(m2, md) and torch.equal(v2, vd)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. one combination: bit-identical to the single-set kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dev_scale", [False, True])
def test_one_combination_is_bit_identical_to_the_single_set_kernel(mode, dev_scale):
    from msa_amd import ops
    nblk = 1031
    p, g, m, v, flags, rng = _random_state(nblk, 77 + mode + 2 * dev_scale)
    h = (2e-3, 0.9, 0.999, 1e-6, 0.01)
    gmap = torch.from_numpy(rng.integers(0, 3, nblk).astype(np.uint8)).to(DEV)
    coef = torch.tensor([0.61], device=DEV)
    outs = []
    for grouped in (False, True):
        pd, gd, md, vd = p.clone(), g.clone(), m.clone(), v.clone()
        pb = torch.empty_like(p, dtype=torch.bfloat16)
        for step in (1, 2, 5):
            if grouped:
                ops.adamw_grouped(pd, gd, md, vd, pb, flags, gmap, [h, h, h], step=step, gscale=0.5, coef=coef if dev_scale else None,
                                  mode=mode)
            elif dev_scale:
                ops.adamw_devscale(pd, gd, md, vd, pb, flags, coef, lr=h[0], beta1=h[1], beta2=h[2], eps=h[3], wd=h[4], step=step, mode=mode)
            else:
                ops.adamw(pd, gd, md, vd, pb, flags, lr=h[0], beta1=h[1], beta2=h[2], eps=h[3], wd=h[4], step=step, gscale=0.5, mode=mode)
            gd.copy_(torch.where(gd == 0, g, gd))                                # (a fresh gradient where the step zeroed it)
        outs.append((pd, gd, md, vd, pb))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_entry_point_limits():
    from msa_amd import ops
    n = 512
    p, g, m, v = (torch.zeros(n, device=DEV) for _ in range(4))
    flags, gmap = torch.zeros(2, dtype=torch.uint8, device=DEV), torch.zeros(2, dtype=torch.uint8, device=DEV)
    ok = [(1e-3 * (1 + k), 0.9, 0.999, 1e-6, 0.0) for k in range(64)]
    ops.adamw_grouped(p, g, m, v, None, flags, gmap, ok + ok[:10] * 19)                    # 64 distinct in 254 groups
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.adamw_grouped(p, g, m, v, None, flags, gmap, ok + [(5.0, 0.9, 0.999, 1e-6, 0.0)])  # 65 distinct
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.adamw_grouped(p, g, m, v, None, flags, gmap, [ok[0]] * 256)                   # 256 groups
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. - 5. the optimizer on the model against the per-group oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def _snapshot(m, opt):
    """{name: (group index, p, g, m, v) as float64 CPU tensors} of every parameter the optimizer steps"""
    from msa_amd.flat import FROZEN
    gi = {id(p): i for i, grp in enumerate(opt.param_groups) for p in grp["params"]}
    out = {}
    for n, p in m.named_parameters():
        if id(p) not in gi:
            continue
        o, k = p._mmb_flat[1], p.numel()
        frozen = n.startswith(FROZEN)
        out[n] = (gi[id(p)], frozen, p.detach().double().cpu().reshape(-1).clone(),
                  None if p.grad is None else p.grad.detach().double().cpu().reshape(-1).clone(),
                  opt._m[o:o + k].double().cpu() if opt._flat is not None else torch.zeros(k, dtype=torch.float64),
                  opt._v[o:o + k].double().cpu() if opt._flat is not None else torch.zeros(k, dtype=torch.float64))
    return out


def _check_against_oracle(m, opt, snap, step, gscale=1.0, grads=None, mode="hf"):
    named = dict(m.named_parameters())
    checked = 0
    for n, (gi, frozen, p0, g0, m0, v0) in snap.items():
        p = named[n]
        got = p.detach().double().cpu().reshape(-1)
        if frozen:
            assert torch.equal(got, p0), n
            continue
        grp = opt.param_groups[gi]
        g = (grads[n] if grads is not None else g0) * gscale
        want, mm, vv = p0.clone(), m0.clone(), v0.clone()
        O.adamw_step(want, g, mm, vv, step, grp["lr"], grp["weight_decay"], beta1=grp["betas"][0], beta2=grp["betas"][1], eps=grp["eps"],
                     mode=mode)
        err = (got - want).abs()
        assert bool((err <= 1e-5 * want.abs() + 1e-7).all()), (n, gi, float(err.max()), grp["lr"])
        o, k = p._mmb_flat[1], p.numel()
        mscale = grp["betas"][0] * m0.abs() + (1.0 - grp["betas"][0]) * g.abs()          # (the terms: fp32 beta1 is 2e-8 off 0.9)
        assert bool(((opt._m[o:o + k].double().cpu() - mm).abs() <= 1e-6 * mscale + 1e-12).all()), n
        checked += 1
    assert checked > 40


def _layerwise_groups(m, lr=1e-3):
    """layerwise_param_groups(layer_decay=0.8, head_lr=5 lr) with the pooler taken out into groups of their own betas and eps"""
    from msa_amd.optim import layerwise_param_groups
    pool = {id(p) for n, p in m.named_parameters() if n.startswith("bert.pooler.")}
    groups = layerwise_param_groups(m, lr, layer_decay=0.8, head_lr=5 * lr)
    for grp in groups:
        grp["params"] = [p for p in grp["params"] if id(p) not in pool]
    groups.append({"params": [m.bert.pooler.dense.weight], "lr": 2 * lr, "betas": (0.8, 0.99), "eps": 1e-8, "weight_decay": 0.05})
    groups.append({"params": [m.bert.pooler.dense.bias], "lr": 3 * lr, "betas": (0.7, 0.95), "eps": 1e-7, "weight_decay": 0.0})
    return groups


@pytest.mark.parametrize("mode", ["hf", "torch"])
def test_model_step_applies_every_groups_own_hyperparameters(mode):
    from msa_amd.optim import AdamW, LinearWarmupSchedule
    m = build()
    opt = AdamW(_layerwise_groups(m), lr=1e-3, mode=mode)
    assert len({g["lr"] for g in opt.param_groups}) >= 5
    _fb(m, _batch(1))
    snap = _snapshot(m, opt)
    opt.step()
    _check_against_oracle(m, opt, snap, 1, mode=mode)
    opt.zero_grad()
    sched = LinearWarmupSchedule(opt, 4, 8)
    sched.step()
    for k in range(3):
        _fb(m, _batch(2 + k))
        snap = _snapshot(m, opt)
        opt.step()
        _check_against_oracle(m, opt, snap, 2 + k, mode=mode)
        opt.zero_grad()
        sched.step()
    assert [g["lr"] for g in opt.param_groups] == [g["initial_lr"] * 1.0 for g in opt.param_groups]      # (lambda(4): warm-up done)


def test_two_nonzero_weight_decays_are_applied_per_group():
    from msa_amd.optim import AdamW
    no_decay = ("bias", "LayerNorm.bias", "LayerNorm.weight")
    m = build()
    named = list(m.named_parameters())
    enc = lambda n: n.startswith("bert.encoder.")
    groups = [{"params": [p for n, p in named if not any(d in n for d in no_decay) and enc(n)], "weight_decay": 0.1},
              {"params": [p for n, p in named if not any(d in n for d in no_decay) and not enc(n)], "weight_decay": 0.01},
              {"params": [p for n, p in named if any(d in n for d in no_decay)], "weight_decay": 0.0}]
    opt = AdamW(groups, lr=1e-2)
    _fb(m, _batch(5))
    snap = _snapshot(m, opt)
    opt.step()
    _check_against_oracle(m, opt, snap, 1)


@pytest.mark.parametrize("frac", [0.2, 5.0])
def test_clip_then_grouped_step_equals_torch_clip_then_oracle(frac):
    from msa_amd.flat import FROZEN
    from msa_amd.optim import AdamW
    m = build()
    opt = AdamW(_layerwise_groups(m))
    _fb(m, _batch(9))
    snap = _snapshot(m, opt)
    live = [(n, s) for n, s in snap.items() if not s[1]]
    clones = {n: torch.nn.Parameter(s[2].clone()) for n, s in live}
    for n, s in live:
        clones[n].grad = s[3].clone()
    norm = float(torch.cat([s[3] for _, s in live]).norm())
    torch.nn.utils.clip_grad_norm_(list(clones.values()), norm * frac)
    got_norm = opt.clip_grad_norm_(norm * frac)
    assert abs(float(got_norm) - norm) <= 1e-5 * norm
    opt.step()
    _check_against_oracle(m, opt, snap, 1, grads={n: c.grad for n, c in clones.items()})
    assert all(not n.startswith(FROZEN) for n, _ in live)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. no host sync
# ---------------------------------------------------------------------------------------------------------------------------------
def test_grouped_clip_and_step_do_not_sync_with_the_host():
    from msa_amd.optim import AdamW
    m = build()
    opt = AdamW(_layerwise_groups(m))
    _fb(m, _batch(70))
    opt.clip_grad_norm_(1.0); opt.step(); opt.zero_grad()
    _fb(m, _batch(71))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        n = opt.clip_grad_norm_(0.5)
        opt.step()
        opt.zero_grad()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    _fb(m, _batch(72))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.param_groups[0]["lr"] *= 0.5                                         # (a schedule's change: read afresh, still no sync)
        opt.step()
        opt.zero_grad()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert math.isfinite(float(n)) and float(n) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the reference's grouping stays on the single-set kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True])
def test_reference_grouping_never_takes_the_grouped_kernel(monkeypatch, clip):
    from msa_amd import ops, trainer as T
    from msa_amd.optim import AdamW, layerwise_param_groups

    def refuse(*a, **k):
        raise AssertionError("the reference's grouping launched the grouped kernel")
    monkeypatch.setattr(ops, "adamw_grouped", refuse)
    m1, m2 = build(), build()
    o1, _ = T.build_optimizer(m1, T.default_args(learning_rate=1e-3), 10)
    for g in o1.param_groups:
        g["lr"] = 1e-3
    o2 = AdamW(layerwise_param_groups(m2, 1e-3), lr=1e-3)
    assert len(o2.param_groups) == 2
    for m in (m1, m2):
        _fb(m, _batch(11))
    m2._flat.grads.copy_(m1._flat.grads)
    for o in (o1, o2):
        if clip:
            o.clip_grad_norm_(0.5)
        o.step()
    for a, b in ((m1._flat.params, m2._flat.params), (o1._m, o2._m), (o1._v, o2._v), (m1._flat.half, m2._flat.half)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. refusals and the state_dict round trip
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split,neighbour", [("attention.self.query.bias", "attention.self.key.bias"),
                                              ("output.LayerNorm.bias", "output.LayerNorm.weight")])
def test_packed_neighbours_in_different_groups_are_refused(split, neighbour):
    """q / k / v biases and a LayerNorm's weight and bias share 256-element blocks (H = 128): one group per block.  (The q / k / v WEIGHTS
    are H * H elements each, whole blocks whenever H % 16 == 0: they may sit in different groups.)"""
    from msa_amd.optim import AdamW
    m = build()
    named = dict(m.named_parameters())
    x = named["bert.encoder.layer.0." + split]
    rest = [p for p in m.parameters() if p is not x]
    opt = AdamW([{"params": rest, "lr": 1e-3}, {"params": [x], "lr": 1e-4}])
    _fb(m, _batch(3))
    before = m._flat.params.clone()
    with pytest.raises(NotImplementedError) as e:
        opt.step()
    msg = str(e.value)
    assert "bert.encoder.layer.0." + split in msg and "bert.encoder.layer.0." + neighbour in msg, msg
    assert torch.equal(before, m._flat.params)
    q = named["bert.encoder.layer.0.attention.self.query.weight"]
    opt = AdamW([{"params": [p for p in m.parameters() if p is not q], "lr": 1e-3}, {"params": [q], "lr": 1e-4}])
    opt.step()                                                                    # (whole blocks of its own: allowed)


def test_limits_and_unimplemented_keys_are_refused_before_any_launch():
    from msa_amd.optim import AdamW
    m = build()
    _fb(m, _batch(4))
    before = m._flat.params.clone()
    with pytest.raises(NotImplementedError, match="merge"):
        AdamW([{"params": list(m.parameters())}] + [{"params": []} for _ in range(255)]).step()       # 256 groups
    dec = [p for n, p in m.named_parameters() if not n.endswith("bias") and "LayerNorm" not in n]
    nod = [p for n, p in m.named_parameters() if n.endswith("bias") or "LayerNorm" in n]
    opt = AdamW([{"params": dec, "lr": 1e-3}, {"params": nod, "lr": 2e-3}] + [{"params": [], "lr": 1e-5 * (k + 1)} for k in range(63)])
    with pytest.raises(NotImplementedError, match="merge"):                                          # 65 distinct combinations
        opt.step()
    assert opt._steps == 0
    opt = AdamW([{"params": dec, "lr": 1e-3}, {"params": nod, "lr": 2e-3, "amsgrad": True}])
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.step()
    opt = AdamW([{"params": dec}, {"params": nod}])
    opt.step()                                                                                       # (allowed)
    opt.param_groups[1]["maximize"] = True
    with pytest.raises(NotImplementedError, match="maximize"):
        opt.step()
    assert opt._steps == 1
    torch.cuda.synchronize()
    assert not torch.equal(before, m._flat.params)


def test_state_dict_round_trip_gives_a_bit_identical_next_step():
    from msa_amd.optim import AdamW
    m = build()
    o1 = AdamW(_layerwise_groups(m))
    o1.lazy_zero = False
    _fb(m, _batch(20))
    o1.step()
    o1.zero_grad()
    o1.param_groups[0]["lr"] *= 0.5
    sd = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in o1.state_dict().items()}
    _fb(m, _batch(21))
    flat = m._flat
    p0, g0 = flat.params.clone(), flat.grads.clone()
    o1.step()
    want = (flat.params.clone(), o1._m.clone(), o1._v.clone(), flat.half.clone())
    o2 = AdamW(_layerwise_groups(m))
    o2.lazy_zero = False
    o2.load_state_dict(sd)
    assert [g["lr"] for g in o2.param_groups] == [g["lr"] for g in o1.param_groups]
    flat.params.copy_(p0)
    flat.grads.copy_(g0)
    o2.step()
    for a, b in zip(want, (flat.params, o2._m, o2._v, flat.half)):
        assert torch.equal(a, b)
