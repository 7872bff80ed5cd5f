#!/usr/bin/env python3
"""What the adapters' input dropout costs: the train step at the headline shape and the adapter kernels alone.

    python tools/ab_lora_dropout.py step [--tree DIR] [--p 0.1] [--steps 12] [--warmup 4] [--rounds 5]
        One process, one model per case, the cases alternating in every round: add_lora(r=8) over a frozen base on query + value and on
        all six projections, each at dropout 0 and at --p.  ``--tree DIR`` imports msa_amd from another checkout (its own built library)
        and runs the dropout-0 cases only, as ``--p 0`` does for this tree: the two legs of the no-regression comparison -- the same two
        models per process, this tree and the parent's in alternating processes; compare their medians and spreads.
    python tools/ab_lora_dropout.py kernels [--rows 18400] [--p 0.1] [--rounds 5]
        The four entry points per target at r = 8, dropout 0 against --p, in the forms that isolate their kernels: fwd (the forward
        kernel); bwd with the input gradient only (the g kernel with its dx / dres part); bwd complete, h saved (g + the token sums + the
        fold); bwd complete, h recomputed.  Beside each surcharge stands the yardstick: ONE extra elementwise pass that reads and writes
        the [rows, K] bf16 input, 4 * rows * K bytes, at the bandwidth the dropout-0 call itself achieves over its minimal traffic.
"""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=("step", "kernels"))
ap.add_argument("--tree", default=None)
ap.add_argument("--p", type=float, default=0.1)
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--rows", type=int, default=18400)
a = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(a.tree) if a.tree else HERE)
import torch  # noqa: E402
from msa_amd import ops  # noqa: E402
from msa_amd.data import synthetic_batch, batch_to  # noqa: E402
from msa_amd.model import MMBertConfig, MMBertForPretraining  # noqa: E402
from msa_amd.trainer import build_optimizer, default_args  # noqa: E402

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


if a.what == "step":
    pool = [batch_to(synthetic_batch(16, 50, 500, 500, seed=1 + i), dev) for i in range(4)]
    cases = []
    for label, tg in (("q + v", ("query", "value")), ("all six", "all-linear")):
        for p in ((0.0,) if (a.tree or a.p <= 0.0) else (0.0, a.p)):
            cases.append((f"add_lora(r=8), {label}, dropout {p:g}", tg, p))
    built = {}
    for n, tg, p in cases:
        m = MMBertForPretraining(MMBertConfig())
        m.bert.set_joint_embeddings("mosei")
        m.to(dev).train()
        m.manual_seed(1234)
        m.return_scores = False
        m.add_lora(r=8, alpha=16.0, targets=tg, seed=0)
        if p > 0.0:
            m.set_lora_dropout(p)
        built[n] = (m,) + tuple(build_optimizer(m, default_args(train_batch_size=16, learning_rate=5e-5), 1000))

    def leg(n):
        model, opt, sched = built[n]

        def step(i):
            out, _ = model(**pool[i % 4])
            out[0].mean().backward()
            opt.step()
            sched.step()
            opt.zero_grad()
        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.steps):
            step(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    ts = {n: [] for n, _, _ in cases}
    for _ in range(a.rounds):
        for n, _, _ in cases:
            ts[n].append(leg(n))
    print(f"train step at the headline shape (batch 16, text 50, pair 500), tree {a.tree or '.'}; {a.rounds} rounds of {a.steps} steps per case, "
          "alternating; ms per step")
    for n, _, _ in cases:
        lo, hi = min(ts[n]), max(ts[n])
        print(f"{n:40s} median {med(ts[n]):7.3f}  min {lo:7.3f}  max {hi:7.3f}  spread {hi - lo:6.3f}", flush=True)
    if not a.tree and a.p > 0.0:
        for label in ("q + v", "all six"):
            t0, t1 = med(ts[f"add_lora(r=8), {label}, dropout 0"]), med(ts[f"add_lora(r=8), {label}, dropout {a.p:g}"])
            print(f"{label:8s} dropout {a.p:g} against 0: {t1 - t0:+7.3f} ms ({100 * (t1 / t0 - 1):+5.2f} %)")
    sys.exit(0)

# ---- the kernels alone ----
H, I, rows, r = 768, 3072, a.rows, 8
s = 16.0 / r
g = torch.Generator(device="cpu").manual_seed(3)
rn = lambda *sh: torch.randn(*sh, generator=g)
bf = lambda t: t.to(torch.bfloat16).to(dev)
ind = ops.make_drop(a.p, 1234, 3)
out_drop = ops.make_drop(0.1, 1234, 1)
print(f"adapter kernels alone, {rows} rows, r {r}, input dropout {a.p:g} (thr16 {ind[1]}) against 0; {a.rounds} rounds of 20 calls; us")
print(f"{'seam':28s} {'form':22s} {'p = 0':>9s} {'p > 0':>9s} {'surcharge':>10s} {'unfused pass':>13s}  min traffic, rate at p = 0")


def report(name, form, t0, t1, nbytes, K):
    m0, m1 = med(t0), med(t1)
    rate = nbytes / m0                                   # bytes per us
    yard = 4.0 * rows * K / rate
    print(f"{name:28s} {form:22s} {m0:9.1f} {m1:9.1f} {m1 - m0:+10.1f} {yard:13.1f}  {nbytes / 1e6:7.1f} MB {rate / 1e6:5.2f} TB/s"
          f"{'   ABOVE the unfused pass' if m1 - m0 > yard else ''}", flush=True)


def both(fn):
    t0, t1 = [], []
    for _ in range(a.rounds):
        t0.append(timed(lambda: fn(None)))
        t1.append(timed(lambda: fn(ind)))
    return t0, t1


kw = lambda d: {} if d is None else {"in_drop": d}
# q / k / v: per target set (one target; q + v; all three)
for names in (("query",), ("query", "value"), ("query", "key", "value")):
    nt = len(names)
    x, qkv, dqkv, dres = bf(rn(rows, H)), bf(rn(rows, 3 * H)), bf(rn(rows, 3 * H) * 0.05), bf(rn(rows, H) * 0.05)
    A = {t: bf(rn(r, H) / H ** 0.5) for t in names}
    B = {t: bf(rn(H, r) * 0.02) for t in names}
    gA = {t: torch.zeros((r, H), device=dev) for t in names}
    gB = {t: torch.zeros((H, r), device=dev) for t in names}
    h = torch.empty((rows, nt * r), dtype=torch.bfloat16, device=dev)
    part = ops.lora_qkv_bwd_workspace(rows, H, r, names) - 2 * ((rows * nt * r * 2 + 15) // 16 * 16)
    name = "qkv " + "+".join(t[0] for t in names)
    report(name, "fwd", *both(lambda d: ops.lora_qkv_fwd(x, qkv, A, B, names, s, h_out=h, **kw(d))), rows * (H * 2 + nt * H * 4 + nt * r * 2), H)
    report(name, "bwd, dres only", *both(lambda d: ops.lora_qkv_bwd(dqkv, x, h, A, B, None, None, names, s, dres=dres, **kw(d))),
           rows * (nt * H * 2 + H * 4), H)
    report(name, "bwd", *both(lambda d: ops.lora_qkv_bwd(dqkv, x, h, A, B, gA, gB, names, s, dres=dres, **kw(d))),
           rows * (nt * H * 4 + H * 4 + nt * H * 2) + 2 * part, H)
    report(name, "bwd, h recomputed", *both(lambda d: ops.lora_qkv_bwd(dqkv, x, None, A, B, gA, gB, names, s, dres=dres, **kw(d))),
           rows * (nt * H * 4 + H * 4 + nt * H * 2 + H * 2) + 2 * part, H)
    del x, qkv, dqkv, dres
# the dense seams
for t in ops.LORA_DENSE_TARGETS:
    K, N = ops.lora_dense_dims(t, H, I)
    gelu = t == "intermediate"
    x, y, dy, dx = bf(rn(rows, K)), bf(rn(rows, N)), bf(rn(rows, N) * 0.05), bf(rn(rows, K) * 0.05)
    u = bf(rn(rows, K)) if t == "ffn_output" else None
    aux = torch.empty((rows, N), dtype=torch.bfloat16, device=dev) if gelu else None
    A, B = bf(rn(r, K) / K ** 0.5), bf(rn(N, r) * 0.02)
    gA, gB = torch.zeros((r, K), device=dev), torch.zeros((N, r), device=dev)
    h = torch.empty((rows, r), dtype=torch.bfloat16, device=dev)
    part = ops.lora_dense_bwd_workspace(rows, K, N, r) - 2 * ((rows * r * 2 + 15) // 16 * 16)
    mode = ops.LORA_DENSE_GELU if gelu else ops.LORA_DENSE_ADD
    name = f"{t} {K}->{N}"
    report(name, "fwd", *both(lambda d: ops.lora_dense_fwd(x, y, A, B, s, mode=mode, drop=None if gelu else out_drop, aux=aux, h_out=h, **kw(d))),
           rows * (K * 2 + N * 4 + (N * 2 if gelu else 0) + r * 2), K)
    report(name, "bwd, dx only", *both(lambda d: ops.lora_dense_bwd(dy, x, h, A, B, None, None, s, dx=dx, gelu_u=u, **kw(d))),
           rows * (N * 2 + K * 4 + (K * 2 if u is not None else 0)), K)
    report(name, "bwd", *both(lambda d: ops.lora_dense_bwd(dy, x, h, A, B, gA, gB, s, dx=dx, gelu_u=u, **kw(d))),
           rows * (N * 4 + K * 2 + K * 4 + (K * 2 if u is not None else 0)) + 2 * part, K)
    report(name, "bwd, h recomputed", *both(lambda d: ops.lora_dense_bwd(dy, x, None, A, B, gA, gB, s, dx=dx, gelu_u=u, **kw(d))),
           rows * (N * 4 + K * 2 + K * 4 + (K * 2 if u is not None else 0) + K * 2) + 2 * part, K)
    del x, y, dy, dx, u, aux
