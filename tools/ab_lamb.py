#!/usr/bin/env python3
"""What a LAMB step costs at the headline size, and that the AdamW step is the parent's.  On the bound flat buffer of the
headline model (12 layers, d = 768, batch 16), gradients of a real step in it:

  default        alternating event-timed legs in ONE process of (a) mmbert_adamw (adamw_kernel, 28 B/parameter), (b) mmbert_adamw_grouped
                 with the reference's two groups, (c) mmbert_lamb (three launches, 24 + 22 B/parameter) and (d) mmbert_lamb with the
                 weight EMA (+8).  Each leg's median, spread over the rounds and rate; (c) / (a) against the paper 46 / 28.
  --kernels      only the launches of (a) and (c), --reps times each after a warm-up: the run to put under
                 ``rocprofv3 --kernel-trace --stats --output-format csv``
  --stats CSV    reads that run's kernel_stats file: the three LAMB launches' mean times and achieved bytes/s beside adamw_kernel's
  --adamw-only   one process's median of leg (a) alone, from the tree --tree (default: this one): run alternately in a checkout of the
                 parent commit and in this one, it is the parent-against-this comparison of the AdamW step (--alternate PARENT_TREE does
                 that: --procs processes per tree, one after the other)

    python tools/ab_lamb.py [--reps 20] [--rounds 9]
"""
import argparse
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--lr", type=float, default=5e-5)
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--stats", default=None)
ap.add_argument("--adamw-only", action="store_true")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--alternate", default=None, metavar="PARENT_TREE")
ap.add_argument("--procs", type=int, default=4)
ap.add_argument("--total", type=int, default=None, help="--stats: elements of the flat buffer")
a = ap.parse_args()
med = lambda x: sorted(x)[len(x) // 2]

if a.alternate:
    res = {"parent": [], "this": []}
    for k in range(a.procs):
        for name, tree in (("parent", a.alternate), ("this", a.tree)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--adamw-only", "--tree", tree, "--reps", str(a.reps), "--rounds", str(a.rounds)],
                                 capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.exit(f"{name} tree failed:\n{out.stdout}\n{out.stderr}")
            line = [x for x in out.stdout.splitlines() if x.startswith("adamw-only")][-1]
            res[name].append(float(line.split()[2]))
            print(f"process {k} {name:6s} {line}", flush=True)
    for name, v in res.items():
        print(f"{name:6s} mmbert_adamw, median of each of {len(v)} processes: {[round(x, 1) for x in v]}  median {med(v):.1f} us  "
              f"spread {max(v) - min(v):.1f} us")
    d, s = med(res["this"]) - med(res["parent"]), max(max(v) - min(v) for v in res.values())
    print(f"this - parent = {d:+.1f} us; the larger run-to-run spread of one tree {s:.1f} us -> {'inside' if abs(d) <= s else 'OUTSIDE'} the spread")
    sys.exit(0)

sys.path.insert(0, os.path.abspath(a.tree))
import torch  # noqa: E402
from msa_amd import ops  # noqa: E402
from msa_amd.data import synthetic_batch, batch_to  # noqa: E402
from msa_amd.model import MMBertConfig, MMBertForPretraining  # noqa: E402
from msa_amd.trainer import build_optimizer, default_args  # noqa: E402

# bytes per parameter that each launch must move at least once
BYTES = {"adamw_kernel": 28, "lamb_moments_kernel": 24, "lamb_apply_kernel": 22}

if a.stats:
    import csv
    rows = {}
    for r in csv.DictReader(open(a.stats)):
        for name in ("adamw_kernel", "lamb_moments_kernel", "lamb_fold_kernel", "lamb_apply_kernel"):      # (demangled or not)
            if name in r["Name"]:
                c, t = rows.get(name, (0, 0.0))
                rows[name] = (c + int(r["Calls"]), t + float(r["TotalDurationNs"]))
    total = a.total
    if total is None:
        sys.exit("--stats needs --total: the flat buffer's element count (the --kernels run prints it)")
    print(f"kernel times (rocprofv3 --kernel-trace --stats), {total} elements in the flat buffer")
    for name, (c, t) in sorted(rows.items()):
        us = t / c / 1e3
        bpp = BYTES.get(name)
        rate = "" if bpp is None else f"  {bpp} B/parameter  {bpp * total / us / 1e6:5.2f} TB/s = {bpp * total / us / 8e6:.3f} of the 8 TB/s HBM peak"
        print(f"{name:24s} {c:5d} launches  mean {us:8.1f} us{rate}")
    if "adamw_kernel" in rows and all(k in rows for k in ("lamb_moments_kernel", "lamb_fold_kernel", "lamb_apply_kernel")):
        per = {k: rows[k][1] / rows[k][0] / 1e3 for k in rows}
        lamb = per["lamb_moments_kernel"] + per["lamb_fold_kernel"] + per["lamb_apply_kernel"]
        print(f"three LAMB launches {lamb:.1f} us = {lamb / per['adamw_kernel']:.3f} x adamw_kernel ({per['adamw_kernel']:.1f} us); paper 46 / 28 = {46 / 28:.3f} "
              f"+ the fold ({per['lamb_fold_kernel']:.1f} us)")
    sys.exit(0)

dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = MMBertForPretraining(MMBertConfig())
model.bert.set_joint_embeddings("mosei")
model.to(dev).train()
model.manual_seed(1234)
args = default_args(train_batch_size=16, learning_rate=a.lr)
opt, _ = build_optimizer(model, args, 1000)
out, _ = model(**batch_to(synthetic_batch(16, 50, 500, 500, seed=1), dev))
out[0].mean().backward()                       # gradients of a real step in the buffer
opt._bind()
flat = model._flat
h = (a.lr, 0.9, 0.999, 1e-6, 0.01)
kw = dict(step=3, zero_grad=True)              # (the fused zero_grad on, as a training step runs it)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def plain():
    ops.adamw(flat.params, flat.grads, opt._m, opt._v, flat.half, opt._flags, lr=h[0], beta1=h[1], beta2=h[2], eps=h[3], wd=h[4], gscale=1.0, mode=0, **kw)


if a.adamw_only:
    ts = [timed(plain, a.reps) for _ in range(a.rounds)]
    print(f"adamw-only median {med(ts):.1f} us  min {min(ts):.1f}  max {max(ts):.1f}  ({a.rounds} rounds of {a.reps} launches, {flat.total} elements)")
    sys.exit(0)

args.optimizer = "lamb"
lamb, _ = build_optimizer(model, args, 1000)
lamb._bind()
ema = flat.params.clone()
hyper = lamb._hyper()


def grouped():
    ops.adamw_grouped(flat.params, flat.grads, opt._m, opt._v, flat.half, opt._flags, opt._group_of_block, hyper, gscale=1.0, mode=0, **kw)


def lamb_step(ema=None):
    ops.lamb(flat.params, flat.grads, lamb._m, lamb._v, flat.half, lamb._flags, lamb._group_of_block, hyper, lamb._unit_of_block, lamb._mixed,
             lamb._units, gscale=1.0, ratios=lamb._ratios, workspace=lamb._lamb_ws, ema=ema, ema_decay=0.999, **kw)


if a.kernels:
    for fn in (plain, lamb_step):
        timed(fn, a.reps)
    print(f"total {flat.total}")
    sys.exit(0)

legs = [("(a) mmbert_adamw", plain, 28), ("(b) mmbert_adamw_grouped", grouped, 28), ("(c) mmbert_lamb", lamb_step, 46),
        ("(d) mmbert_lamb + ema", lambda: lamb_step(ema), 54)]
ts = {n: [] for n, _, _ in legs}
for r in range(a.rounds):
    for n, fn, _ in legs:
        ts[n].append(timed(fn, a.reps))
torch.cuda.synchronize()
nunits, nmixed = lamb._units.shape[0], lamb._mixed.shape[0]
print(f"parameters {flat.total} in the flat buffer, {nunits} trust units, {nmixed} mixed-block records; {a.rounds} rounds of {a.reps} calls per leg, "
      f"alternating; times in us")
for n, _, bpp in legs:
    t, lo, hi = med(ts[n]), min(ts[n]), max(ts[n])
    print(f"{n:26s} median {t:8.1f}  min {lo:8.1f}  max {hi:8.1f}  spread {hi - lo:6.1f}  {bpp} B/parameter = {bpp * flat.total / 1e6:7.1f} MB  "
          f"{bpp * flat.total / t / 1e6:5.2f} TB/s = {bpp * flat.total / t / 8e6:.3f} of the 8 TB/s HBM peak  all {[round(x, 1) for x in ts[n]]}", flush=True)
A, C = med(ts[legs[0][0]]), med(ts[legs[2][0]])
print(f"(c) / (a) = {C / A:.3f} (paper: 46 / 28 = {46 / 28:.3f} plus the fold); (c) - (a) = {C - A:+.1f} us per optimizer step")
