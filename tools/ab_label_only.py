#!/usr/bin/env python3
"""What the label-only step (``forward(masked_labels=None)``) is worth against the standard train step at the headline shape.

Same-process A/B of the whole train step (forward, backward, optimizer): per configuration one model per route, the routes alternating
in every round.  Routes: the standard step as ``forward`` runs it by default (MLM labels, the prediction scores returned: the whole MLM
head on every row), the standard step with ``return_scores = False`` (the MLM head on the labelled rows only, rows nothing reads left out
of the forward pass) and the label-only step on the same batches without their labels.  Configurations: nothing frozen;
``freeze(embeddings=True, layers=6)``; ``add_lora(r=8)`` on query + value (frozen base).  Per configuration and route: the median step time over the rounds (device events around ``--steps`` steps, after
``--warmup``), min / max / spread, the peak of allocated memory during one step ABOVE what is allocated when the step starts (all models
of the configuration warmed up and resident), and the native calls per step.

    python tools/ab_label_only.py [--steps 12] [--warmup 4] [--rounds 5] [--only add_lora]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from msa_amd import _lib  # noqa: E402
from msa_amd.data import synthetic_batch, batch_to  # noqa: E402
from msa_amd.model import MMBertConfig, MMBertForPretraining  # noqa: E402
from msa_amd.trainer import build_optimizer, default_args  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--only", default=None, help="only the configurations whose name contains this (e.g. add_lora)")
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.manual_seed(0)
med = statistics.median
pool = [batch_to(synthetic_batch(16, 50, 500, 500, seed=1 + i), dev) for i in range(4)]
ROUTES = ("standard, scores", "standard, no scores", "label-only")
pools = {ROUTES[0]: pool, ROUTES[1]: pool, ROUTES[2]: [dict(b, masked_labels=None) for b in pool]}

configs = [("nothing frozen", lambda m: None),
           ("freeze(embeddings=True, layers=6)", lambda m: m.freeze(embeddings=True, layers=6)),
           ("add_lora(r=8), q + v", lambda m: m.add_lora(r=8, seed=0))]


def make(prepare, route):
    m = MMBertForPretraining(MMBertConfig())
    m.bert.set_joint_embeddings("mosei")
    m.to(dev).train()
    m.manual_seed(1234)
    m.return_scores = route == ROUTES[0]
    prepare(m)
    opt, sched = build_optimizer(m, default_args(train_batch_size=16, learning_rate=5e-5), 1000)
    return m, opt, sched


def leg(built, batches, steps, warmup, count=False):
    model, opt, sched = built

    def step(i):
        out, _ = model(**batches[i % 4])
        out[0].mean().backward()
        opt.step()
        sched.step()
        opt.zero_grad()
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    calls = peak = None
    if count:
        k, orig = [0], _lib.check
        _lib.check = lambda code, what: (k.__setitem__(0, k[0] + 1), orig(code, what))[1]
        torch.cuda.reset_peak_memory_stats()
        resident = torch.cuda.memory_allocated()
        try:
            step(0)
        finally:
            _lib.check = orig
        torch.cuda.synchronize()
        calls, peak = k[0], torch.cuda.max_memory_allocated() - resident
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        step(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, calls, peak


print(f"train step at the headline shape (batch 16, text 50, pair 500, 12 layers, H 768); {a.rounds} rounds of {a.steps} steps per "
      "route, alternating; ms per step")
for cname, prepare in configs:
    if a.only and a.only not in cname:
        continue
    built = {r: make(prepare, r) for r in pools}
    for r in pools:                                          # every model's storage and optimizer state exist before anything is measured
        leg(built[r], pools[r], 1, 1)
    ts, info = {r: [] for r in pools}, {}
    for rd in range(a.rounds):
        for r in (list(pools) if rd % 2 == 0 else list(pools)[::-1]):
            t, calls, peak = leg(built[r], pools[r], a.steps, a.warmup, count=(rd == 0))
            ts[r].append(t)
            if calls is not None:
                info[r] = (calls, peak)
    base = med(ts[ROUTES[1]])
    print(f"\n{cname}")
    for r in pools:
        lo, hi = min(ts[r]), max(ts[r])
        print(f"  {r:19s} median {med(ts[r]):7.3f}  min {lo:7.3f}  max {hi:7.3f}  spread {hi - lo:6.3f}  vs standard, no scores {med(ts[r]) - base:+7.3f} ms "
              f"({100 * (med(ts[r]) / base - 1):+5.1f} %)  native calls/step {info[r][0]}  peak memory of a step above the resident state {info[r][1] / 2 ** 30:6.2f} GiB", flush=True)
    del built
    torch.cuda.empty_cache()
