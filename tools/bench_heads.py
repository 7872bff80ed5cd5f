#!/usr/bin/env python3
"""Stand-alone GPU time of the pretraining heads, forward and backward: the level-launch form (csrc/heads_coop.hip, model._HeadsStepFn: 7 + 6 launches) against the
multi-launch form (csrc/heads.hip, model._HeadsFn) at the headline shape (B = 16, H = 768) and at the reference's default (B = 32, H = 1024).

    python tools/bench_heads.py                                   # the two shapes, both forms, regression head: medians of 20
    python tools/bench_heads.py --classes 7,2,6,16 --shape 128,768 # the level-launch form per label head: 7 (or 1) = regression, C = a C-class head
                                                                  # (min / median / max of --reps; the multi-launch form is regression-only)"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from msa_amd import model as MM
from msa_amd.model import MMBertConfig, MMBertForPretraining

ap_ = argparse.ArgumentParser()
ap_.add_argument("--classes", default=None, help="comma-separated num_labels values, e.g. 7,2,6,16")
ap_.add_argument("--shape", default=None, help="B,H (with --classes; default 128,768)")
ap_.add_argument("--reps", type=int, default=20)
opt = ap_.parse_args()
dev = torch.device("cuda", 0)


def build(H, num_labels=None):
    torch.manual_seed(0)
    cfg = MMBertConfig(hidden_size=H, num_hidden_layers=1, num_attention_heads=H // 64, intermediate_size=4 * H, vocab_size=512)
    m = MMBertForPretraining(cfg) if num_labels is None else MMBertForPretraining(cfg, num_labels=num_labels)
    m.bert.set_joint_embeddings("mosei"); m.to(dev)
    m._ensure_ready(dev)
    return m


def time_heads(fn, m, first, ap, sent, mlm, reps):
    for _ in range(3):
        f = first.clone().requires_grad_(True)
        fn.apply(f, m, ap, sent, mlm)[0].backward()
    torch.cuda.synchronize()
    tf, tb, tt = [], [], []
    for _ in range(reps):
        f = first.clone().requires_grad_(True)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record(); loss = fn.apply(f, m, ap, sent, mlm)[0]; e1.record(); loss.backward(); e2.record()
        torch.cuda.synchronize()
        tf.append(e0.elapsed_time(e1) * 1e3); tb.append(e1.elapsed_time(e2) * 1e3); tt.append(e0.elapsed_time(e2) * 1e3)
    tf.sort(); tb.sort(); tt.sort()
    return tf, tb, tt


if opt.classes is None:
    for B, H in ((16, 768), (32, 1024)):
        m = build(H)
        first = torch.randn(3 * B, H, device=dev)
        ap = torch.randint(0, 2, (2 * B,), device=dev); sent = torch.rand(B, device=dev) * 6 - 3
        mlm = torch.tensor([7.0, 7.1, 6.9], device=dev)
        for name, fn in (("level launches", MM._HeadsStepFn), ("multi-launch", MM._HeadsFn)):
            tf, tb, _ = time_heads(fn, m, first, ap, sent, mlm, opt.reps)
            print(f"B={B:3d} H={H:5d} {name:14s}: forward {tf[opt.reps // 2]:7.1f} us  backward {tb[opt.reps // 2]:7.1f} us", flush=True)
else:
    B, H = (int(x) for x in (opt.shape or "128,768").split(","))
    first = torch.randn(3 * B, H, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    ap = torch.randint(0, 2, (2 * B,), device=dev)
    mlm = torch.tensor([7.0, 7.1, 6.9], device=dev)
    for C in (int(x) for x in opt.classes.split(",")):
        m = build(H, C)
        sent = torch.rand(B, device=dev) * 6 - 3 if C in (1, 7) else torch.randint(0, C, (B,), device=dev)
        tf, tb, tot = time_heads(MM._HeadsStepFn, m, first, ap, sent, mlm, opt.reps)
        md = opt.reps // 2
        print(f"B={B:3d} H={H:5d} num_labels={C:2d} ({'regression' if C in (1, 7) else f'{C}-class'}): forward {tf[0]:6.1f} / {tf[md]:6.1f} / {tf[-1]:6.1f} us  "
              f"backward {tb[0]:6.1f} / {tb[md]:6.1f} / {tb[-1]:6.1f} us  forward + backward {tot[0]:6.1f} / {tot[md]:6.1f} / {tot[-1]:6.1f} us  (min / median / max of {opt.reps})", flush=True)
