#!/usr/bin/env python3
"""What global gradient-norm clipping costs at the headline size: a same-process, interleaved A/B of the train step without and with
``AdamW.clip_grad_norm_`` (fused into the step), then the launches on their own -- the norm (mmbert_grad_norm, two launches) and the
AdamW kernel with the host scale against the one that reads the device coefficient (mmbert_adamw_devscale), alternating, event-timed.

    python tools/ab_clip.py [--steps 40] [--rounds 4] [--max-norm 1.0]
    python tools/ab_clip.py --only-clip --steps 20 --rounds 1      # clipping steps only (the run to put under rocprofv3 --kernel-trace)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from msa_amd import ops  # noqa: E402
from msa_amd.data import synthetic_batch, batch_to  # noqa: E402
from msa_amd.flat import FROZEN  # noqa: E402
from msa_amd.model import MMBertConfig, MMBertForPretraining  # noqa: E402
from msa_amd.trainer import build_optimizer, default_args  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--max-norm", type=float, default=1.0)
ap.add_argument("--only-clip", action="store_true")
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = MMBertForPretraining(MMBertConfig())
model.bert.set_joint_embeddings("mosei")
model.to(dev).train()
model.manual_seed(1234)
opt, sched = build_optimizer(model, default_args(train_batch_size=16, learning_rate=5e-5), 1000)
pool = [batch_to(synthetic_batch(16, 50, 500, 500, seed=1 + i), dev) for i in range(4)]


def step(i, clip):
    out, _ = model(**pool[i % 4])
    out[0].mean().backward()
    if clip:
        opt.clip_grad_norm_(a.max_norm)
    opt.step(); sched.step(); opt.zero_grad()


variants = [("clip", True)] if a.only_clip else [("plain", False), ("clip", True)]
for _, c in variants:
    for i in range(3):
        step(i, c)
torch.cuda.synchronize()
ts = {n: [] for n, _ in variants}
for r in range(a.rounds):
    for n, c in variants:
        step(0, c)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(i, c)
        torch.cuda.synchronize()
        ts[n].append((time.perf_counter() - t0) / a.steps * 1e3)
base = sorted(ts[variants[0][0]])[a.rounds // 2]
for n, _ in variants:
    t = sorted(ts[n])
    print(f"step {n:6s} median {t[a.rounds // 2]:7.3f} ms  (min {t[0]:.3f} max {t[-1]:.3f})  x{t[a.rounds // 2] / base:.4f}", flush=True)
if a.only_clip:
    sys.exit(0)

# ---- the launches on their own, on the bound storage (gradients of a real step in the buffer) ----
flat = model._flat
out, _ = model(**pool[0])
out[0].mean().backward()
segs, nseg = flat.segments(opt._names, FROZEN)
nel = int(sum(int(k) for _, k in segs[:nseg].tolist()))
ws = flat.norm_workspace()
res = ops.grad_norm(flat.grads, segs, nseg, max_norm=a.max_norm)
coef = res[2:3].clone()


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


kw = dict(lr=0.0, beta1=0.9, beta2=0.999, eps=1e-6, wd=0.01, step=1, mode=0, zero_grad=False)
t_norm, t_host, t_dev = [], [], []
for r in range(5):
    t_norm.append(timed(lambda: ops.grad_norm(flat.grads, segs, nseg, max_norm=a.max_norm, workspace=ws)))
    t_host.append(timed(lambda: ops.adamw(flat.params, flat.grads, opt._m, opt._v, flat.half, opt._flags, gscale=1.0, **kw)))
    t_dev.append(timed(lambda: ops.adamw_devscale(flat.params, flat.grads, opt._m, opt._v, flat.half, opt._flags, coef, **kw)))
med = lambda x: sorted(x)[len(x) // 2]
print(f"parameters {flat.total} in the flat buffer, {nel} in the norm's {nseg} segments ({nel * 4 / 1e6:.1f} MB read)")
print(f"grad_norm (2 launches)   median {med(t_norm):8.1f} us   {nel * 4 / med(t_norm) / 1e6:.2f} TB/s of gradient read   all {[round(x, 1) for x in t_norm]}")
print(f"adamw_kernel             median {med(t_host):8.1f} us   all {[round(x, 1) for x in t_host]}")
print(f"adamw_devscale_kernel    median {med(t_dev):8.1f} us   x{med(t_dev) / med(t_host):.4f}   all {[round(x, 1) for x in t_dev]}")
