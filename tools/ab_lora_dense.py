#!/usr/bin/env python3
"""What low-rank adapters on the attention-output and FFN projections cost at the headline shape, and the rate of their kernels.

Part 1 -- same-process A/B of the whole train step (forward, backward, optimizer), one model per case, the cases alternating in every
round: nothing frozen; ``freeze(embeddings=True, layer_weights=True)`` (bias-only); and, for r = 8 and r = 16 with a frozen base on all
layers, ``add_lora`` on query + value, on query + value + attention_output, and on all six projections ("all-linear").  Per case: the median
step time over the rounds (device events around ``--steps`` steps, after ``--warmup``), the spread, the native calls per step and the
trainable parameter count.

Part 2 -- mmbert_lora_dense_fwd and mmbert_lora_dense_bwd alone per target on [rows, K] -> [rows, N] matrices, r = 8 and 16: time and
achieved bytes/s of the streams each call has to move at least once (forward: x read, y read and written, aux written in the GELU mode, h
written; backward: dy read twice -- for g and for dB --, x read for dA, the input gradient read and written, u read where gelu' applies,
the fp32 partial sums written and read), next to the AdamW launch's rate over the flat buffers measured in the same run.

    python tools/ab_lora_dense.py [--steps 12] [--warmup 4] [--rounds 5] [--rows 18400]
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


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


adamw_rate = None
if not a.skip_step:
    pool = [batch_to(synthetic_batch(16, 50, 500, 500, seed=1 + i), dev) for i in range(4)]

    def make(prepare):
        m = MMBertForPretraining(MMBertConfig())
        m.bert.set_joint_embeddings("mosei")
        m.to(dev).train()
        m.manual_seed(1234)
        m.return_scores = False
        prepare(m)
        opt, sched = build_optimizer(m, default_args(train_batch_size=16, learning_rate=5e-5), 1000)
        return m, opt, sched

    QV, QVO = ("query", "value"), ("query", "value", "attention_output")
    cases = [("nothing frozen", lambda m: None),
             ("bias-only (embeddings + layer weights frozen)", lambda m: m.freeze(embeddings=True, layer_weights=True))]
    for r in (8, 16):
        for label, tg in (("q + v", QV), ("q + v + attention_output", QVO), ("all six", "all-linear")):
            cases.append((f"add_lora(r={r}), {label}", lambda m, r=r, tg=tg: m.add_lora(r=r, alpha=2.0 * r, targets=tg, seed=0)))
    built = {n: make(p) for n, p in cases}

    def leg(n, steps, warmup, count=False):
        model, opt, sched = built[n]

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
            k, orig = [0], _lib.check
            _lib.check = lambda code, what: (k.__setitem__(0, k[0] + 1), orig(code, what))[1]
            try:
                step(0)
            finally:
                _lib.check = orig
            torch.cuda.synchronize()
            calls = k[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(steps):
            step(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps, calls

    ts, info = {n: [] for n, _ in cases}, {}
    for r in range(a.rounds):
        for n, _ in cases:
            t, calls = leg(n, a.steps, a.warmup, count=(r == 0))
            ts[n].append(t)
            if calls is not None:
                info[n] = calls
    cfg = built[cases[0][0]][0].config
    print(f"train step at the headline shape (batch 16, text 50, pair 500, {cfg.num_hidden_layers} layers, H {cfg.hidden_size}, I {cfg.intermediate_size}); "
          f"{a.rounds} rounds of {a.steps} steps per case, alternating; ms per step")
    base = med(ts[cases[0][0]])
    for n, _ in cases:
        lo, hi = min(ts[n]), max(ts[n])
        trainable = sum(p.numel() for p in built[n][0].parameters() if p.requires_grad)
        print(f"{n:46s} median {med(ts[n]):7.3f}  min {lo:7.3f}  max {hi:7.3f}  spread {hi - lo:6.3f}  vs nothing frozen {med(ts[n]) - base:+7.3f} ms "
              f"({100 * (med(ts[n]) / base - 1):+5.1f} %)  native calls/step {info[n]}  trainable parameters {trainable / 1e6:8.3f} M", flush=True)
    # the AdamW launch over the whole flat buffer of the unfrozen model: params, grads, m, v read, params, m, v, bf16 copy, grads written
    model, opt, _ = built[cases[0][0]]
    out, _ = model(**pool[0])
    out[0].mean().backward()
    n_el = model._flat.total
    adamw_bytes = n_el * (4 * 4 + 3 * 4 + 2 + 4)
    try:
        t_opt = timed(lambda: opt.step(), reps=10)
        adamw_rate = adamw_bytes / t_opt / 1e6
    except Exception as e:                                           # (the kernel numbers below do not depend on it)
        print("AdamW timing failed:", repr(e))
        t_opt = float("nan")
    print(f"\nAdamW.step() over {n_el / 1e6:.1f} M elements (about {adamw_bytes / 1e6:.0f} MB moved, the transposed-copy launch beside it): {t_opt:8.1f} us = "
          f"{adamw_rate or float('nan'):5.2f} TB/s", flush=True)
    del built, pool, model, opt
    torch.cuda.empty_cache()

# ---- part 2: the two kernels alone, per target ----
H, I, rows = 768, 3072, a.rows
g = torch.Generator(device="cpu").manual_seed(3)
rn = lambda *s: torch.randn(*s, generator=g)
drop = ops.make_drop(0.1, 1234, 1)
for r in (8, 16):
    print(f"\ndense adapter kernels alone, {rows} rows, r {r}; {a.rounds} rounds of 20 calls; us")
    for t in ops.LORA_DENSE_TARGETS:
        K, N = ops.lora_dense_dims(t, H, I)
        gelu = t == "intermediate"
        x = rn(rows, K).to(torch.bfloat16).to(dev)
        y = rn(rows, N).to(torch.bfloat16).to(dev)
        dy = (rn(rows, N) * 0.05).to(torch.bfloat16).to(dev)
        dx = (rn(rows, K) * 0.05).to(torch.bfloat16).to(dev)
        u = rn(rows, K).to(torch.bfloat16).to(dev) if t == "ffn_output" else None
        aux = torch.empty((rows, N), dtype=torch.bfloat16, device=dev) if gelu else None
        A = (rn(r, K) / K ** 0.5).to(torch.bfloat16).to(dev)
        B = (rn(N, r) * 0.02).to(torch.bfloat16).to(dev)
        gA, gB = torch.zeros((r, K), device=dev), torch.zeros((N, r), device=dev)
        h = torch.empty((rows, r), dtype=torch.bfloat16, device=dev)
        ws_bytes = ops.lora_dense_bwd_workspace(rows, K, N, r)
        part = ws_bytes - 2 * ((rows * r * 2 + 15) // 16 * 16)
        fwd_bytes = rows * (K * 2 + N * 4 + (N * 2 if gelu else 0) + r * 2)
        bwd_bytes = rows * (N * 4 + K * 2 + K * 4 + (K * 2 if u is not None else 0)) + 2 * part
        mode = ops.LORA_DENSE_GELU if gelu else ops.LORA_DENSE_ADD
        res = {}
        for rd in range(a.rounds):
            res.setdefault("fwd", []).append(timed(lambda: ops.lora_dense_fwd(x, y, A, B, 16.0 / r, mode=mode, drop=None if gelu else drop, aux=aux, h_out=h)))
            res.setdefault("bwd", []).append(timed(lambda: ops.lora_dense_bwd(dy, x, h, A, B, gA, gB, 16.0 / r, dx=dx, gelu_u=u)))
            res.setdefault("bwd, h recomputed", []).append(timed(lambda: ops.lora_dense_bwd(dy, x, None, A, B, gA, gB, 16.0 / r, dx=dx, gelu_u=u)))
        for what, nb in (("fwd", fwd_bytes), ("bwd", bwd_bytes), ("bwd, h recomputed", bwd_bytes + rows * K * 2)):
            tt = res[what]
            line = (f"r={r:2d} {t:17s} {K:4d} -> {N:4d} {what:18s} median {med(tt):8.1f}  min {min(tt):8.1f}  max {max(tt):8.1f}  {nb / 1e6:7.1f} MB  "
                    f"{nb / med(tt) / 1e6:5.2f} TB/s")
            if adamw_rate:
                line += f"  = {nb / med(tt) / 1e6 / adamw_rate:.2f} of the AdamW launch's rate"
            print(line, flush=True)
        del x, y, dy, dx, u, aux
