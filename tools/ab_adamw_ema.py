#!/usr/bin/env python3
"""What the weight EMA costs at the headline size: on the bound flat buffer of the headline model, alternating event-timed legs of
  (a) the single-set kernel (mmbert_adamw, adamw_kernel): a step without an average, 28 B/parameter,
  (b) the fused kernel (mmbert_adamw_ema, adamw_ema_kernel<false>): 36 B/parameter,
  (c) mmbert_adamw followed by ``ema.lerp_(params, 1 - d)``, the route open to a user without it: 28 + 12 B/parameter, two launches,
and of the swap (mmbert_ema_swap: 18 B/parameter) alone and with the transposed-copy refresh that swap_ema() runs behind it.
Reports each leg's median, its spread over the rounds, its rate against the 8 TB/s HBM peak, and (b) - (a), (c) - (b).

    python tools/ab_adamw_ema.py [--reps 20] [--rounds 9] [--decay 0.999]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from msa_amd import ops  # noqa: E402
from msa_amd.data import synthetic_batch, batch_to  # noqa: E402
from msa_amd.model import MMBertConfig, MMBertForPretraining  # noqa: E402
from msa_amd.trainer import build_optimizer, default_args  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--lr", type=float, default=5e-5)
ap.add_argument("--decay", type=float, default=0.999)
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = MMBertForPretraining(MMBertConfig())
model.bert.set_joint_embeddings("mosei")
model.to(dev).train()
model.manual_seed(1234)
opt, _ = build_optimizer(model, default_args(train_batch_size=16, learning_rate=a.lr), 1000)
out, _ = model(**batch_to(synthetic_batch(16, 50, 500, 500, seed=1), dev))
out[0].mean().backward()                       # gradients of a real step in the buffer
opt._bind()
flat = model._flat
ema = flat.params.clone()
h = (a.lr, 0.9, 0.999, 1e-6, 0.01)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


# (the fused zero_grad on, as a training step runs it: from the second launch on the gradient reads zeros, the traffic is the same)
kw = dict(step=3, mode=0, zero_grad=True)


def plain():
    ops.adamw(flat.params, flat.grads, opt._m, opt._v, flat.half, opt._flags, lr=h[0], beta1=h[1], beta2=h[2], eps=h[3], wd=h[4], gscale=1.0, **kw)


def fused():
    ops.adamw_ema(flat.params, flat.grads, opt._m, opt._v, flat.half, opt._flags, None, [h], ema, ema_decay=a.decay, gscale=1.0, **kw)


def outside():
    plain()
    ema.lerp_(flat.params, 1.0 - a.decay)


def swap():
    ops.ema_swap(flat.params, ema, flat.half)


def swap_refresh():
    swap()
    flat.refresh_transposes()


legs = [("(a) adamw_kernel", plain, 28), ("(b) adamw_ema_kernel", fused, 36), ("(c) adamw_kernel + lerp_", outside, 40),
        ("ema_swap_kernel", swap, 18), ("ema_swap + transposed copies", swap_refresh, None)]
ts = {n: [] for n, _, _ in legs}
for r in range(a.rounds):
    for n, fn, _ in legs:
        ts[n].append(timed(fn, a.reps))
torch.cuda.synchronize()
med = lambda x: sorted(x)[len(x) // 2]
print(f"parameters {flat.total} in the flat buffer; decay {a.decay}; {a.rounds} rounds of {a.reps} launches per leg, alternating; times in us")
for n, _, bpp in legs:
    t, lo, hi = med(ts[n]), min(ts[n]), max(ts[n])
    rate = "" if bpp is None else f"  {bpp} B/parameter = {bpp * flat.total / 1e6:7.1f} MB  {bpp * flat.total / t / 1e6:5.2f} TB/s = {bpp * flat.total / t / 8e6:.3f} of the 8 TB/s HBM peak"
    print(f"{n:30s} median {t:8.1f}  min {lo:8.1f}  max {hi:8.1f}  spread {hi - lo:6.1f}{rate}  all {[round(x, 1) for x in ts[n]]}", flush=True)
A, B, C = (med(ts[legs[i][0]]) for i in range(3))
spread = max(max(ts[legs[i][0]]) - min(ts[legs[i][0]]) for i in range(3))
print(f"(b) - (a) = {B - A:+.1f} us: what the fused average adds to a step")
print(f"(c) - (b) = {C - B:+.1f} us: what fusing saves over the lerp_ outside; largest spread of one leg over the rounds {spread:.1f} us "
      f"-> (b) {'is' if C - B > spread else 'is NOT'} faster than (c) by more than the spread")
