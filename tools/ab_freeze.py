#!/usr/bin/env python3
"""What freezing parameters saves at the headline shape, and what the grouped column sum costs.

Part 1 -- same-process A/B of the whole train step (forward, backward, optimizer) of ONE headline model, the cases alternating in every
round: nothing frozen; embeddings + 6 / 9 / 11 layers; ``layer_weights=True`` alone.  Per case: the median step time over the rounds
(device events around ``--steps`` steps, after ``--warmup``), the spread over the rounds, the native calls per step (each C entry point
makes one or more kernel launches; counted on the host in a step of its own) and the peak allocated memory of the timed window.  Each
leg builds its optimizer over the trainable parameters (trainer.build_optimizer), as a user would.

Part 2 -- mmbert_colsum_grouped on one layer's four bias-gradient matrices (du [rows, I], dz2d [rows, H], dqkv [rows, 3H], dz1d [rows, H])
against four mmbert_colsum calls, in both deterministic settings, alternating; time and achieved bytes/s of the rows x 8H bf16 read.

    python tools/ab_freeze.py [--steps 12] [--warmup 4] [--rounds 5] [--rows 18400]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from msa_amd import _lib, ops  # noqa: E402
from msa_amd.data import synthetic_batch, batch_to  # noqa: E402
from msa_amd.model import MMBertConfig, MMBertForPretraining  # noqa: E402
from msa_amd.trainer import build_optimizer, default_args  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--rows", type=int, default=18400)
ap.add_argument("--skip-step", action="store_true")
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.manual_seed(0)
med = statistics.median

if not a.skip_step:
    model = MMBertForPretraining(MMBertConfig())
    model.bert.set_joint_embeddings("mosei")
    model.to(dev).train()
    model.manual_seed(1234)
    model.return_scores = False
    L = model.config.num_hidden_layers
    pool = [batch_to(synthetic_batch(16, 50, 500, 500, seed=1 + i), dev) for i in range(4)]
    cases = [("nothing frozen", {}), ("embeddings + 6 layers", dict(embeddings=True, layers=6)), ("embeddings + 9 layers", dict(embeddings=True, layers=9)),
             ("embeddings + 11 layers", dict(embeddings=True, layers=11)), ("layer_weights=True", dict(layer_weights=True))]

    def leg(kw, steps, warmup, count=False):
        model.unfreeze()
        if kw:
            model.freeze(**kw)
        opt, sched = build_optimizer(model, default_args(train_batch_size=16, learning_rate=5e-5), 1000)

        def step(i):
            out, _ = model(**pool[i % 4])
            out[0].mean().backward()
            opt.step()
            sched.step()
            opt.zero_grad()
        for i in range(warmup):
            step(i)
        torch.cuda.synchronize()
        calls = None
        if count:
            n, orig = [0], _lib.check
            _lib.check = lambda code, what: (n.__setitem__(0, n[0] + 1), orig(code, what))[1]
            try:
                step(0)
            finally:
                _lib.check = orig
            torch.cuda.synchronize()
            calls = n[0]
        torch.cuda.reset_peak_memory_stats(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(steps):
            step(i)
        e1.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev)
        del opt
        return e0.elapsed_time(e1) / steps, calls, peak

    ts, info = {n: [] for n, _ in cases}, {}
    for r in range(a.rounds):
        for n, kw in cases:
            t, calls, peak = leg(kw, a.steps, a.warmup, count=(r == 0))
            ts[n].append(t)
            if calls is not None:
                info[n] = (calls, peak)
    print(f"train step at the headline shape (batch 16, text 50, pair 500, {L} layers, H {model.config.hidden_size}); {a.rounds} rounds of {a.steps} steps per case, "
          "alternating; ms per step")
    base = med(ts[cases[0][0]])
    for n, kw in cases:
        lo, hi = min(ts[n]), max(ts[n])
        k = kw.get("layers", 0)
        print(f"{n:24s} median {med(ts[n]):7.3f}  min {lo:7.3f}  max {hi:7.3f}  spread {hi - lo:6.3f}  vs nothing frozen {med(ts[n]) - base:+7.3f} ms "
              f"({100 * (med(ts[n]) / base - 1):+5.1f} %)  native calls/step {info[n][0]}  peak {info[n][1] / 2 ** 30:6.2f} GiB  k/L {k / L:.2f}", flush=True)
    print("rough expectation, not asserted: the saving grows with k/L times backward's share of the trunk (backward is about two thirds of a "
          "layer's forward + backward work), less what the heads, the MLM head, the embeddings and the optimizer keep costing")
    del model, pool
    torch.cuda.empty_cache()

# ---- part 2: the grouped column sum against four mmbert_colsum calls ----
H, I, rows = 768, 3072, a.rows
g = torch.Generator(device="cpu").manual_seed(3)
mats = [torch.randn((rows, n), generator=g).to(torch.bfloat16).to(dev) for n in (I, H, 3 * H, H)]
outs = [torch.zeros(m.shape[1], device=dev) for m in mats]
nbytes = rows * 8 * H * 2


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def grouped():
    ops.colsum_grouped(list(zip(mats, outs)), accumulate=True)


def four():
    for m, o in zip(mats, outs):
        ops.colsum(m, o)


was = ops.deterministic()
res = {}
for r in range(a.rounds):
    for det in (False, True):
        ops.set_deterministic(det)
        for n, fn in (("mmbert_colsum_grouped (1 call)", grouped), ("mmbert_colsum x 4", four)):
            res.setdefault((n, det), []).append(timed(fn))
ops.set_deterministic(was)
print(f"\nbias gradients of one layer: {rows} rows x 8H = {8 * H} columns bf16 = {nbytes / 1e6:.1f} MB read; {a.rounds} rounds of 20 calls, alternating; us")
for (n, det), t in res.items():
    print(f"{n:32s} deterministic={int(det)}  median {med(t):8.1f}  min {min(t):8.1f}  max {max(t):8.1f}  {nbytes / med(t) / 1e6:5.2f} TB/s "
          f"= {nbytes / med(t) / 8e6:.3f} of the 8 TB/s HBM peak (the matrices may sit in the 256 MB Infinity Cache between calls)", flush=True)
for det in (False, True):
    gq, fq = med(res[("mmbert_colsum_grouped (1 call)", det)]), med(res[("mmbert_colsum x 4", det)])
    print(f"deterministic={int(det)}: grouped / four calls = {gq / fq:.3f} ({'grouped is faster' if gq < fq else 'GROUPED IS SLOWER'})")
