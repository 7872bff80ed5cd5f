#!/usr/bin/env python3
"""What the multi-label head costs where it runs: the heads' forward + backward (7 + 6 launches of csrc/heads_coop.hip, one C call each
way) at the headline (B, H) = (16, 768) with C = 6, event-timed, for
  * the class head of THIS tree,
  * the multi-label head of this tree (pos_weight, thresholds, smoothing 0.1, a quarter of the entries not annotated),
  * the class head of ANOTHER tree (``--parent DIR``: a built checkout of the parent commit, e.g. under tools/_ab/) -- the runtime branch
    the multi-label head adds to forward levels 5 and 7 sits in the class head's instantiation, so this is the pair that shows its cost.
One fresh process per leg and round, the legs alternating (a process's clocks and allocator state are its own: a difference between two
trees is only readable against the spread of one tree's repeated processes).  Each process also counts the kernels of one forward +
backward (torch.profiler): a multi-label step must make exactly the launches of a class-head step.

    python tools/ab_multilabel.py --parent tools/_ab/parent_tree [--rounds 5] [--reps 200]
    python tools/ab_multilabel.py --leg multilabel            # one leg in this process: a JSON line
"""
import argparse
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("class", "multilabel"))
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--parent")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
B, H, C = 16, 768, 6


def leg():
    sys.path.insert(0, a.root)
    import torch
    from msa_amd import model as MM, ops
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    dev = torch.device("cuda", 0)
    multi = a.leg == "multilabel"
    torch.manual_seed(0)
    cfg = MMBertConfig(hidden_size=H, num_hidden_layers=1, num_attention_heads=H // 64, intermediate_size=4 * H, vocab_size=512)
    m = MMBertForPretraining(cfg, num_labels=C, **({"multi_label": True} if multi else {}))
    m.bert.set_joint_embeddings("mosei")
    m.to(dev)
    m._ensure_ready(dev)
    g = torch.Generator(device=dev).manual_seed(B)
    first = torch.randn(3 * B, H, device=dev, generator=g)
    apl = torch.randint(0, 2, (2 * B,), device=dev, generator=g)
    if multi:
        m.set_loss_options(pos_weight=[0.5, 1.0, 2.0, 4.0, 0.25, 1.5], thresholds=[0.5, 0.4, 0.6, 0.5, 0.3, 0.7], multilabel_smoothing=0.1)
        sent = torch.randint(0, 2, (B, C), device=dev, generator=g).float()
        sent[torch.rand(B, C, device=dev, generator=g) < 0.25] = -1.0
    else:
        sent = torch.randint(0, C, (B,), device=dev, generator=g)
    rec, outs, keep = MM._HeadsStepFn._setup(m, B, H, dev, apl, sent, first=first)
    # the backward's pointers (what _HeadsStepFn.backward sets)
    d1 = torch.ones(1, device=dev)
    dfirst = torch.empty(3 * B, H, device=dev)
    pool, al, at, c1, c2 = m.bert.pooler.dense, m.cls.align, m.attn, m.classifier1_1, m.classifier1_2
    rec.dloss, rec.dfirst = d1.data_ptr(), dfirst.data_ptr()
    rec.gWp, rec.gbp, rec.gWal, rec.gbal = (t.grad.data_ptr() for t in (pool.weight, pool.bias, al.weight, al.bias))
    rec.gWat, rec.gbat, rec.gWc1, rec.gbc1, rec.gWc2, rec.gbc2 = (t.grad.data_ptr() for t in (at.weight, at.bias, c1.weight, c1.bias, c2.weight, c2.bias))
    for q, (v, cp) in enumerate(zip((m.vt, m.vv, m.vs), (m.cpc_zt.net, m.cpc_zv.net, m.cpc_za.net))):
        rec.gvw[q], rec.gvb[q], rec.gWq[q], rec.gbq[q] = (t.grad.data_ptr() for t in (v.weight, v.bias, cp.weight, cp.bias))

    def step():
        ops.heads_step_fwd(rec)
        ops.heads_step_bwd(rec)
    for _ in range(20):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / a.reps * 1e3)
    kernels = None
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        kernels = dict(total=len(names), heads_fwd=sum("heads_fwd_level_kernel" in n for n in names),
                       heads_bwd=sum("heads_bwd_level_kernel" in n for n in names))
    except Exception as e:                                         # (no profiler in this build: the timing stands without the count)
        kernels = dict(error=repr(e))
    assert bool(torch.isfinite(outs[0]).all())
    print(json.dumps(dict(leg=a.leg, root=a.root, us=sorted(ts)[len(ts) // 2], us_min=min(ts), us_max=max(ts), kernels=kernels)), flush=True)


def drive():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    legs = [("new tree, class head", here, "class"), ("new tree, multi-label head", here, "multilabel")]
    if a.parent:
        legs.insert(0, ("parent tree, class head", os.path.abspath(a.parent), "class"))
    res = {n: [] for n, _, _ in legs}
    for r in range(a.rounds):
        for n, root, which in legs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--root", root, "--reps", str(a.reps)],
                                 capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                print(out.stderr[-2000:])
                raise SystemExit(f"{n}: the leg's process ended with {out.returncode}")
            res[n].append(json.loads(out.stdout.strip().splitlines()[-1]))
    med = lambda x: sorted(x)[len(x) // 2]
    print(f"heads forward + backward, (B, H) = ({B}, {H}), C = {C}: {a.rounds} alternating processes per leg, {a.reps} steps x 5 per process (us per step)")
    for n, _, _ in legs:
        us = [q["us"] for q in res[n]]
        print(f"  {n:28s} median {med(us):7.1f}  min {min(us):7.1f}  max {max(us):7.1f}   per process: {' '.join(f'{u:.1f}' for u in us)}")
        print(f"  {'':28s} kernels of one forward + backward: {res[n][0]['kernels']}")
    k = [res[n][0]["kernels"] for n, _, _ in legs]
    same = all(q == k[0] for q in k) and "error" not in k[0]
    print(f"  launches equal on every leg: {same}")
    if a.parent:
        p = [q["us"] for q in res[legs[0][0]]]
        c = [q["us"] for q in res[legs[1][0]]]
        print(f"  class head, new - parent: {med(c) - med(p):+.1f} us; spread of the parent's own processes (max - min) {max(p) - min(p):.1f} us")
    c = [q["us"] for q in res["new tree, class head"]]
    ml = [q["us"] for q in res["new tree, multi-label head"]]
    print(f"  multi-label - class, new tree: {med(ml) - med(c):+.1f} us; spread of the class leg's processes {max(c) - min(c):.1f} us")
    if not same:
        raise SystemExit("the legs' launch counts differ")


if a.leg:
    leg()
else:
    drive()
