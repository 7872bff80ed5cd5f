"""CPU: the float64 EMA reference (tests/ema_ref.py) and optim.ema_decay_at are what they say -- the recursion is
torch.optim.swa_utils.AveragedModel's with get_ema_multi_avg_fn, the copy at enabling being its first update_parameters."""
import pytest
import torch

from tests import ema_ref as E


def test_ema_decay_at_hand_values():
    from msa_amd.optim import ema_decay_at
    assert ema_decay_at(0.999, 0, True) == 1.0 / 10.0
    assert ema_decay_at(0.999, 9, True) == 10.0 / 19.0
    assert ema_decay_at(0.999, 10 ** 6, True) == 0.999                     # (1000001 / 1000010 = 0.999991 > 0.999)
    assert ema_decay_at(0.3, 0, True) == 0.1 and ema_decay_at(0.3, 3, True) == 0.3      # 4 / 13 = 0.3077 > 0.3
    for u in (0, 9, 10 ** 6):
        assert ema_decay_at(0.999, u, False) == 0.999 and ema_decay_at(0.999, u) == 0.999
    assert ema_decay_at(0.0, 5) == 0.0


def test_ema_step_hand_values():
    got = E.ema_step(torch.tensor([1.0, -2.0, 0.0]), torch.tensor([3.0, -2.0, 8.0]), 0.25)
    assert got.dtype == torch.float64 and torch.equal(got, torch.tensor([1.5, -2.0, 2.0], dtype=torch.float64))
    assert E.omd_f32(0.5) == 0.5 and abs(E.omd_f32(0.9999) - 1e-4) < 1e-11 and E.omd_f32(0.9999) != 1.0 - 0.9999


@pytest.mark.parametrize("d", [0.9, 0.9999])
def test_recursion_is_averaged_models(d):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    torch.manual_seed(3)
    m = torch.nn.Linear(7, 5).double()
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(d))
    avg.update_parameters(m)                                               # the first update copies: AdamW.ema()'s copy at enabling
    mine = {n: p.detach().clone() for n, p in m.named_parameters()}
    worst = 0.0
    for _ in range(5):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn_like(p) * 0.1)
        avg.update_parameters(m)
        for n, p in m.named_parameters():
            mine[n] = E.ema_step(mine[n], p.detach(), 1.0 - d)
            want = dict(avg.module.named_parameters())[n].detach()
            rel = float(((mine[n] - want).abs() / want.abs()).max())
            worst = max(worst, rel)
    print(f"d = {d}: largest relative difference to AveragedModel {worst:.3g}")
    assert worst <= 1e-15, worst


def test_bound_covers_both_forms_of_the_lerp_in_fp32():
    """The kernel's bound admits an fp32 evaluation of either algebraic form (and rejects an update with the wrong coefficient)."""
    g = torch.Generator().manual_seed(0)
    e0, p = torch.randn(1 << 16, generator=g), torch.randn(1 << 16, generator=g)
    p = torch.where(torch.rand(1 << 16, generator=g) < 0.5, e0 + 1e-4 * p, p)            # (updates small against e as well)
    for d in (0.9, 0.999, 0.9999):
        omd = E.omd_f32(d)
        w = torch.tensor(omd, dtype=torch.float32)
        ref, tol = E.ema_step(e0, p, omd), E.ema_bound(e0, p, omd)
        for got in (e0 + w * (p - e0), (1 - w) * e0 + w * p):
            assert bool(((got.double() - ref).abs() <= tol).all()), d
        wrong = e0 + torch.tensor(1.0 - omd, dtype=torch.float32) * (p - e0)
        assert not bool(((wrong.double() - ref).abs() <= tol).all())
