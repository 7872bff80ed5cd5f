"""GPU tests of the AdamW kernel with the weight EMA fused in (mmbert_adamw_ema) and of the swap (mmbert_ema_swap), through ops:
p, m, v, g and the bf16 copy bit-identical to the kernel that runs without the average (single-set, device-scale, grouped), the
average against float64 (tests/ema_ref.py) fed with that kernel's p, frozen blocks untouched, the swap exact both ways, the refusals.
Sizes: one wave, a few waves, a grid whose last workgroup is ragged (4099 blocks of 256 = 1024 workgroups of 4 waves + 3 waves)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ema_ref as E
from tests.test_adamw_groups_gpu import HYPER7, _random_state

DEV = "cuda"
NBLK = [1, 5, 4099]
DECAYS = [0.9, 0.999, 0.9999]
H1 = (2e-3, 0.9, 0.999, 1e-6, 0.01)
GSCALE = 0.37


def _existing(route, state, gmap, coef, pb, *, step, mode, zero_grad):
    """The kernel that runs without the average, in place on ``state`` = (p, g, m, v)."""
    from msa_amd import ops
    p, g, m, v, flags = state
    if route == "single":
        ops.adamw(p, g, m, v, pb, flags, lr=H1[0], beta1=H1[1], beta2=H1[2], eps=H1[3], wd=H1[4], step=step, gscale=GSCALE, mode=mode,
                  zero_grad=zero_grad)
    elif route == "devscale":
        ops.adamw_devscale(p, g, m, v, pb, flags, coef, lr=H1[0], beta1=H1[1], beta2=H1[2], eps=H1[3], wd=H1[4], step=step, mode=mode,
                           zero_grad=zero_grad)
    else:
        ops.adamw_grouped(p, g, m, v, pb, flags, gmap, HYPER7, step=step, gscale=GSCALE, mode=mode, zero_grad=zero_grad)


def _with_ema(route, state, gmap, coef, pb, ema, d, *, step, mode, zero_grad):
    from msa_amd import ops
    p, g, m, v, flags = state
    if route == "grouped":
        ops.adamw_ema(p, g, m, v, pb, flags, gmap, HYPER7, ema, ema_decay=d, step=step, gscale=GSCALE, mode=mode, zero_grad=zero_grad)
    else:
        ops.adamw_ema(p, g, m, v, pb, flags, None, [H1], ema, ema_decay=d, step=step, gscale=GSCALE,
                      coef=coef if route == "devscale" else None, mode=mode, zero_grad=zero_grad)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("route", ["single", "devscale", "grouped"])
@pytest.mark.parametrize("nblk", NBLK)
def test_update_is_bit_identical_and_the_average_follows_float64(nblk, route, mode):
    p, g, m, v, flags, rng = _random_state(nblk, 4000 + 7 * nblk + mode + 2 * len(route))
    gmap = torch.from_numpy(rng.integers(0, len(HYPER7), nblk).astype(np.uint8)).to(DEV)
    coef = torch.tensor([GSCALE], device=DEV)
    e0 = torch.randn(nblk * 256, device=DEV, generator=torch.Generator(DEV).manual_seed(nblk))
    e0[::3] = p[::3] * (1 + 1e-5)                                            # (averages close to the weights, as late in a run)
    live = ((flags & 3) != 2).repeat_interleave(256)
    assert nblk < 5 or (bool(live.any()) and not bool(live.all()))
    worst = 0.0
    for step in (1, 7):
        for zero_grad in (True, False):
            want = [x.clone() for x in (p, g, m, v)]
            want_pb = torch.zeros_like(p, dtype=torch.bfloat16)
            _existing(route, want + [flags], gmap, coef, want_pb, step=step, mode=mode, zero_grad=zero_grad)
            for d in DECAYS:
                got = [x.clone() for x in (p, g, m, v)]
                got_pb, ema = torch.zeros_like(want_pb), e0.clone()
                _with_ema(route, got + [flags], gmap, coef, got_pb, ema, d, step=step, mode=mode, zero_grad=zero_grad)
                for name, a, b in zip("pgmv", got, want):
                    assert torch.equal(a, b), (name, step, zero_grad, d)
                assert torch.equal(got_pb, want_pb), (step, zero_grad, d)
                omd = E.omd_f32(d)
                ref, tol = E.ema_step(e0, want[0], omd), E.ema_bound(e0, want[0], omd)
                err = (ema.double() - ref).abs()
                ratio = float((err / tol)[live].max()) if bool(live.any()) else 0.0
                worst = max(worst, ratio)
                assert ratio <= 1.0, (step, zero_grad, d, ratio)
                assert torch.equal(ema[~live], e0[~live]), (step, zero_grad, d)
                if bool(live.any()):
                    assert not torch.equal(ema[live], e0[live])
            # no bf16 copy: accepted, everything else the same
            got, ema = [x.clone() for x in (p, g, m, v)], e0.clone()
            _with_ema(route, got + [flags], gmap, coef, None, ema, 0.999, step=step, mode=mode, zero_grad=zero_grad)
            for a, b in zip(got, want):
                assert torch.equal(a, b)
    print(f"nblk {nblk} {route} mode {mode}: largest |ema - float64| / bound = {worst:.3f}")


@pytest.mark.parametrize("nblk", NBLK)
def test_swap_exchanges_exactly_and_twice_restores(nblk):
    from msa_amd import ops
    gen = torch.Generator(DEV).manual_seed(50 + nblk)
    p0 = torch.randn(nblk * 256, device=DEV, generator=gen)
    e0 = torch.randn(nblk * 256, device=DEV, generator=gen) * 3
    p, e = p0.clone(), e0.clone()
    pb = torch.zeros_like(p, dtype=torch.bfloat16)
    ops.ema_swap(p, e, pb)
    assert torch.equal(p, e0) and torch.equal(e, p0) and torch.equal(pb, p.bfloat16())
    ops.ema_swap(p, e, pb)
    assert torch.equal(p, p0) and torch.equal(e, e0) and torch.equal(pb, p0.bfloat16())
    ops.ema_swap(p, e, None)
    assert torch.equal(p, e0) and torch.equal(e, p0) and torch.equal(pb, p0.bfloat16())


def test_refusals():
    from msa_amd import ops
    n = 512
    p, g, m, v, ema = (torch.zeros(n, device=DEV) for _ in range(5))
    flags = torch.zeros(2, dtype=torch.uint8, device=DEV)
    ops.adamw_ema(p, g, m, v, None, flags, None, [H1], ema, ema_decay=0.0)
    for bad_ema, d in ((None, 0.9), (ema, 1.0), (ema, -0.1), (ema, float("nan"))):
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.adamw_ema(p, g, m, v, None, flags, None, [H1], bad_ema, ema_decay=d)
    with pytest.raises(RuntimeError, match="invalid argument"):               # mmbert_adamw_grouped's own conditions
        ops.adamw_ema(p, g, m, v, None, flags, None, [H1] * 256, ema, ema_decay=0.9)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.adamw_ema(p[:300], g[:300], m[:300], v[:300], None, flags, None, [H1], ema[:300], ema_decay=0.9)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.ema_swap(p[:300], ema[:300])
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0 and float(ema.abs().max()) == 0.0
