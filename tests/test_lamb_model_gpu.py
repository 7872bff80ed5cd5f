"""GPU tests of msa_amd.optim.LAMB on the model: three clipped, scheduled train steps with layer-wise groups against the
float64 reference (tests/lamb_ref.py) at H = 128 and at H = 64 (where LayerNorm pairs and the q / k / v biases share blocks), and what LAMB
inherits from AdamW's binding: the EMA, freezing, the lazy zero, label-only steps, adapters, the state_dict, no host sync.  An AdamW step
makes no LAMB call."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lamb_ref as L
from tests.test_adamw_groups_gpu import CFG, _batch, _fb, _snapshot, build

DEV = "cuda"
# the h64_L1 shape of the golden fixtures with ONE head: the attention kernels take 64-wide heads
CFG64 = dict(hidden=64, layers=1, heads=1, intermediate=128, vocab=2048, dataset="mosei", alpha=0.7, beta=0.3)


def _groups(m, lr=1e-3):
    from msa_amd.optim import layerwise_param_groups
    return layerwise_param_groups(m, lr, layer_decay=0.8, head_lr=5 * lr)


def _lamb(m, **kw):
    from msa_amd.optim import LAMB
    return LAMB(_groups(m), lr=1e-3, **kw)


def _reference(opt, snap, step, gscale):
    """lamb_ref over the parameters the step updates (a gradient, not one of the never-differentiated names), packed end to end:
    ({name: index}, the reference's dict, {name: slice})"""
    names = [n for n, s in snap.items() if not s[1] and s[3] is not None]
    off, tensors, where = 0, [], {}
    for n in names:
        k = snap[n][2].numel()
        tensors.append((off, k, snap[n][0]))
        where[n] = slice(off, off + k)
        off += k
    cat = lambda j: np.concatenate([snap[n][j].numpy() for n in names])
    hyper = [(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]) for g in opt.param_groups]
    ref = L.lamb_step(cat(2), cat(3), cat(4), cat(5), tensors, hyper, step, gscale=gscale, always_adapt=opt.always_adapt,
                      max_trust=opt.max_trust, f32_coefs=True)
    return {n: i for i, n in enumerate(names)}, ref, where


def _check_step(m, opt, snap, step, gscale):
    index, ref, where = _reference(opt, snap, step, gscale)
    named = dict(m.named_parameters())
    for n, s in snap.items():
        got = named[n].detach().double().cpu().reshape(-1)
        if n not in index:
            assert torch.equal(got, s[2]), n
            continue
        want = torch.from_numpy(ref["P"][where[n]])
        err = (got - want).abs()
        assert bool((err <= 1e-5 * want.abs() + 1e-7).all()), (n, float(err.max()))
    tr = opt.trust_ratios()
    assert set(tr) == set(index)
    worst = 0.0
    for n, i in index.items():
        r, npn, nun = tr[n]
        R, bound = ref["R"][i], L.ratio_bound(ref["R"][i], ref["CANCEL"][i])
        worst = max(worst, abs(r - R) / bound)
        assert abs(r - R) <= bound, (n, r, R, ref["CANCEL"][i])
        assert abs(npn - ref["NP"][i]) <= 2e-6 * ref["NP"][i], n
        grp = opt.param_groups[snap[n][0]]
        if grp["weight_decay"] == 0 and not opt.always_adapt:
            assert r == 1.0, n
    print(f"step {step}: {len(index)} tensors, worst |r - R| / bound = {worst:.3f}")
    return tr


@pytest.mark.parametrize("cfg", [CFG, CFG64], ids=["h128_L2", "h64_L1"])
def test_three_clipped_scheduled_steps_against_float64(cfg):
    from msa_amd.optim import LinearWarmupSchedule
    m = build(cfg)
    opt = _lamb(m)
    assert len({g["lr"] for g in opt.param_groups}) >= 3
    sched = LinearWarmupSchedule(opt, 4, 8)
    sched.step()
    seen = []
    for k in range(3):
        _fb(m, _batch(30 + k, cfg))
        opt.clip_grad_norm_(1.0)
        gscale = float(opt._clip[2])
        assert 0.0 < gscale <= 1.0
        snap = _snapshot(m, opt)
        opt.step()
        tr = _check_step(m, opt, snap, k + 1, gscale)
        seen.append(tr)
        opt.zero_grad()
        sched.step()
    adapted = [r for n, (r, _, _) in seen[-1].items() if r != 1.0]
    assert len(adapted) >= 10 and len(seen[-1]) > len(adapted)              # the weights adapt, biases and LayerNorms take the Adam step
    if cfg is CFG64:                                                        # the packed neighbours are units of their own
        flat, pre = m._flat, "bert.encoder.layer.0."
        for a, b in ((pre + "output.LayerNorm.weight", pre + "output.LayerNorm.bias"),
                     (pre + "attention.self.query.bias", pre + "attention.self.key.bias")):
            assert flat.offset[a] // 256 == flat.offset[b] // 256 and seen[-1][a][1] != seen[-1][b][1]
        assert opt._mixed.shape[0] > 3


def test_always_adapt_and_max_trust_reach_the_kernel():
    m = build(CFG64)
    opt = _lamb(m, always_adapt=True, max_trust=0.5)
    _fb(m, _batch(40, CFG64))
    snap = _snapshot(m, opt)
    opt.step()
    tr = _check_step(m, opt, snap, 1, 1.0)
    rs = [r for r, _, _ in tr.values()]
    assert max(rs) == 0.5 and min(rs) < 0.5 and rs.count(0.5) >= 3         # (a LayerNorm weight: ||p|| = 8, ||u|| about 8 at step 1)
    assert tr["bert.encoder.layer.0.output.LayerNorm.weight"][0] != 1.0     # (wd = 0, adapted all the same)


def test_ema_follows_the_new_weights_and_swaps_back_bit_for_bit():
    m = build()
    opt = _lamb(m).ema(0.9)
    _fb(m, _batch(50))
    opt.step()
    flat = m._flat
    p0, e0 = flat.params.clone(), opt._ema.clone()
    opt.zero_grad()
    _fb(m, _batch(51))
    opt.step()
    live = torch.from_numpy(np.repeat(opt._base_flags.numpy() != 2, 256)).to(DEV)
    want = e0.double() + float(np.float32(1.0 - 0.9)) * (flat.params.double() - e0.double())
    assert bool(((opt._ema.double() - want).abs() <= 5e-7 * (e0.abs() + 0.1 * flat.params.abs()).double() + 1e-30)[live].all())
    assert torch.equal(opt._ema[~live], e0[~live]) and not torch.equal(flat.params, p0) and opt.ema_updates == 2
    p1, e1, h1 = flat.params.clone(), opt._ema.clone(), flat.half.clone()
    opt.swap_ema()
    assert torch.equal(flat.params, e1) and torch.equal(opt._ema, p1)
    with pytest.raises(RuntimeError, match="swapped"):
        opt.step()
    opt.swap_ema()
    assert torch.equal(flat.params, p1) and torch.equal(opt._ema, e1) and torch.equal(flat.half, h1)
    assert set(opt.ema_state_dict()) == set(m.state_dict())


def test_frozen_parameters_keep_their_bits_and_have_no_ratio():
    m = build()
    opt = _lamb(m)
    _fb(m, _batch(60))
    opt.step()
    opt.zero_grad()
    frozen = set(m.freeze(embeddings=True, layers=1))
    assert frozen
    flat = m._flat
    p0, m0, v0 = flat.params.clone(), opt._m.clone(), opt._v.clone()
    _fb(m, _batch(61))
    opt.step()
    tr = opt.trust_ratios()
    assert tr and not (set(tr) & frozen)
    moved = 0
    for n, q in m.named_parameters():
        o, k = q._mmb_flat[1], q.numel()
        same = torch.equal(flat.params[o:o + k], p0[o:o + k])
        if n in frozen:
            assert same and torch.equal(opt._m[o:o + k], m0[o:o + k]) and torch.equal(opt._v[o:o + k], v0[o:o + k]), n
        elif n in tr:
            moved += not same
    assert moved > 10


def test_lazy_zero_on_and_off_give_the_same_parameters():
    from msa_amd import ops
    outs = []
    try:
        for lazy in (True, False):
            m = build()
            m.deterministic = True               # (ordered sums: the two models' gradients are the same bits)
            opt = _lamb(m)
            opt.lazy_zero = lazy
            for k in range(2):
                _fb(m, _batch(70 + k))
                opt.step()
                opt.zero_grad()
            outs.append((m._flat.params.clone(), opt._m.clone(), opt._v.clone(), opt._ratios.clone()))
    finally:
        ops.set_deterministic(False)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_a_label_only_step_leaves_the_mlm_head_alone_and_lets_it_back():
    from msa_amd.model import _MLM_ONLY
    m = build()
    m.set_alpha_beta(0.0, 1.0)
    opt = _lamb(m)
    _fb(m, _batch(80))
    opt.step()
    opt.zero_grad()
    assert set(_MLM_ONLY) <= set(opt.trust_ratios())
    flat = m._flat
    span = lambda x, n: x[flat.offset[n]:flat.offset[n] + flat.numel[n]].clone()
    before = {n: (span(flat.params, n), span(opt._m, n), span(opt._v, n)) for n in _MLM_ONLY}
    out, _ = m(**dict(_batch(81), masked_labels=None))
    out[0].mean().backward()
    opt.step()
    opt.zero_grad()
    tr = opt.trust_ratios()
    assert tr and not (set(tr) & set(_MLM_ONLY))
    for n in _MLM_ONLY:
        for a, b in zip(before[n], (span(flat.params, n), span(opt._m, n), span(opt._v, n))):
            assert torch.equal(a, b), n
    _fb(m, _batch(82))
    opt.step()                                                              # back in, without raising
    assert set(_MLM_ONLY) <= set(opt.trust_ratios())
    assert not torch.equal(before["cls.predictions.transform.dense.weight"][0], span(flat.params, "cls.predictions.transform.dense.weight"))


def test_every_adapter_matrix_is_a_unit_of_its_own():
    m = build()
    m.add_lora(r=8, seed=2)
    opt = _lamb(m)
    _fb(m, _batch(90))
    adapters = {n: float(q.detach().double().norm()) for n, q in m.named_parameters() if ".lora_" in n}
    assert len(adapters) >= 8
    opt.step()
    tr = opt.trust_ratios()
    assert set(adapters) <= set(tr)
    for n, norm in adapters.items():
        r, npn, nun = tr[n]
        assert abs(npn - norm) <= 2e-6 * norm, n
        if n.endswith("lora_B"):
            assert norm == 0.0 and r == 1.0 and nun > 0.0, n                # B starts at zero: nothing to scale by
        else:
            assert norm > 0.0 and r != 1.0 and abs(r - npn / nun) <= 1e-6 * r, n


def test_state_dict_round_trip_continues_bit_identically_and_adamw_state_is_refused():
    from msa_amd.optim import AdamW
    m = build()
    o1 = _lamb(m)
    o1.lazy_zero = False
    _fb(m, _batch(20))
    o1.step()
    o1.zero_grad()
    sd = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in o1.state_dict().items()}
    assert sd["optimizer"] == "lamb" and sd["steps"] == 1
    _fb(m, _batch(21))
    flat = m._flat
    p0, g0 = flat.params.clone(), flat.grads.clone()
    o1.step()
    want = (flat.params.clone(), o1._m.clone(), o1._v.clone(), flat.half.clone(), o1._ratios.clone())
    o2 = _lamb(m)
    o2.lazy_zero = False
    o2.load_state_dict(sd)
    flat.params.copy_(p0)
    flat.grads.copy_(g0)
    o2.step()
    for a, b in zip(want, (flat.params, o2._m, o2._v, flat.half, o2._ratios)):
        assert torch.equal(a, b)
    adamw = AdamW(_groups(m))
    with pytest.raises(ValueError, match="lamb"):
        adamw.load_state_dict(sd)
    with pytest.raises(ValueError, match="adamw"):
        o2.load_state_dict(dict(sd, optimizer="adamw"))
    o2.load_state_dict({k: v for k, v in sd.items() if k != "optimizer"})    # no key: accepted
    assert o2._steps == 1


def test_clip_and_step_do_not_sync_with_the_host():
    m = build()
    opt = _lamb(m).ema(0.99)
    _fb(m, _batch(70))
    opt.clip_grad_norm_(1.0); opt.step(); opt.zero_grad()
    for clip in (True, False):
        _fb(m, _batch(71 + clip))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            if clip:
                n = opt.clip_grad_norm_(0.5)
            else:
                opt.param_groups[0]["lr"] *= 0.5                            # (a schedule's change: read afresh, still no sync)
            opt.step()
            opt.zero_grad()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    assert np.isfinite(float(n)) and float(n) > 0.0 and len(opt.trust_ratios()) > 40


class _Spy:
    """The loaded library with every entry point's name noted as it is called."""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mmbert_"):
            return fn

        def call(*a):
            self._names.append(name)
            return fn(*a)
        return call


def test_an_adamw_step_makes_no_lamb_call(monkeypatch):
    from msa_amd import _lib, trainer as T
    from msa_amd.optim import AdamW
    names = []
    m1, m2, m3 = build(), build(), build()
    opts = (T.build_optimizer(m1, T.default_args(learning_rate=1e-3), 10)[0], AdamW(_groups(m2)), _lamb(m3))
    assert type(opts[0]) is AdamW
    for m in (m1, m2, m3):
        _fb(m, _batch(11))
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "_lib", _Spy(_lib.load(), names))
    made = []
    for o in opts:
        del names[:]
        o.step()
        made.append([n for n in names if n.startswith(("mmbert_adamw", "mmbert_lamb", "mmbert_grad_norm"))])
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert made == [["mmbert_adamw"], ["mmbert_adamw_grouped"], ["mmbert_lamb"]]
