#!/usr/bin/env python3
"""What per-parameter-group AdamW costs at the headline size: on the bound flat buffer of the headline model, alternating event-timed
launches of the single-set kernel (mmbert_adamw, adamw_kernel) and the grouped one (mmbert_adamw_grouped, adamw_grouped_kernel<false>)
  (a) with the reference's two groups forced through the grouped path, and
  (b) with layerwise_param_groups(layer_decay=0.9, head_lr=10 lr).
Reports each kernel's median time, its rate at 28 B/parameter as a fraction of the 8 TB/s HBM peak, and its time
against adamw_kernel's.

    python tools/ab_adamw_groups.py [--reps 20] [--rounds 7]
    python tools/ab_adamw_groups.py --only-grouped     # the grouped launches only (the run to put under rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from msa_amd import ops  # noqa: E402
from msa_amd.data import synthetic_batch, batch_to  # noqa: E402
from msa_amd.model import MMBertConfig, MMBertForPretraining  # noqa: E402
from msa_amd.optim import AdamW, layerwise_param_groups  # noqa: E402
from msa_amd.trainer import build_optimizer, default_args  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--lr", type=float, default=5e-5)
ap.add_argument("--only-grouped", action="store_true")
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = MMBertForPretraining(MMBertConfig())
model.bert.set_joint_embeddings("mosei")
model.to(dev).train()
model.manual_seed(1234)
ref, _ = build_optimizer(model, default_args(train_batch_size=16, learning_rate=a.lr), 1000)
lw = AdamW(layerwise_param_groups(model, a.lr, layer_decay=0.9, head_lr=10 * a.lr), lr=a.lr)
out, _ = model(**batch_to(synthetic_batch(16, 50, 500, 500, seed=1), dev))
out[0].mean().backward()                       # gradients of a real step in the buffer
ref._bind()
lw._bind()
flat = model._flat
for g in ref.param_groups:
    g["lr"] = a.lr


def hyper(opt):
    return [(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]) for g in opt.param_groups]


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
single = lambda: ops.adamw(flat.params, flat.grads, ref._m, ref._v, flat.half, ref._flags, lr=a.lr, beta1=0.9, beta2=0.999, eps=1e-6,
                           wd=0.01, gscale=1.0, **kw)
grouped_ref = lambda: ops.adamw_grouped(flat.params, flat.grads, ref._m, ref._v, flat.half, ref._flags, ref._group_of_block, hyper(ref),
                                        gscale=1.0, **kw)
grouped_lw = lambda: ops.adamw_grouped(flat.params, flat.grads, lw._m, lw._v, flat.half, lw._flags, lw._group_of_block, hyper(lw),
                                       gscale=1.0, **kw)
variants = [("adamw_grouped (a) 2 groups", grouped_ref), ("adamw_grouped (b) layerwise", grouped_lw)]
if not a.only_grouped:
    variants.insert(0, ("adamw_kernel", single))
ts = {n: [] for n, _ in variants}
for r in range(a.rounds):
    for n, fn in variants:
        ts[n].append(timed(fn, a.reps))
med = lambda x: sorted(x)[len(x) // 2]
nbytes = 28 * flat.total
print(f"parameters {flat.total} in the flat buffer ({nbytes / 1e6:.1f} MB per launch at 28 B/parameter); "
      f"groups: (a) {len(ref.param_groups)}, (b) {len(lw.param_groups)} with {len(set(hyper(lw)))} distinct combinations")
base = med(ts[variants[0][0]])
for n, _ in variants:
    t = med(ts[n])
    print(f"{n:30s} median {t:8.1f} us  {nbytes / t / 1e6:5.2f} TB/s = {nbytes / t / 8e6:.3f} of the 8 TB/s HBM peak  x{t / base:.4f}  "
          f"all {[round(x, 1) for x in ts[n]]}", flush=True)
