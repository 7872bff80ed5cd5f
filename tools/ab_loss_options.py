#!/usr/bin/env python3
"""What the loss options cost where they run, in one process, alternating event-timed legs:
  * the vocabulary cross-entropy (ops.ce_fwd / ops.ce_bwd: ce_count_kernel + ce_row_kernel) at the headline vocabulary (V = 30 522,
    ldv = 30 592) with label smoothing 0.1 against 0 -- the dense form over the step's 18 400 packed rows (15 % labelled) and the
    compact form over the ~400 labelled rows a training step really runs it on;
  * the heads' loss level (forward level 7 of csrc/heads_coop.hip alone, behind one run of levels 1 - 6) for a 6-class head with class
    weights + smoothing against without, and the regression head with Huber against MSE, at B = 16 and 128, H = 768.
Reports each leg's median, min and max over the rounds and the difference of the medians against the larger spread of the two legs.

    python tools/ab_loss_options.py [--reps 20] [--rounds 9]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from msa_amd import model as MM, ops  # noqa: E402
from msa_amd.model import MMBertConfig, MMBertForPretraining  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=9)
a = ap.parse_args()
dev = torch.device("cuda", 0)
V, LDV = 30522, 30592


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def ab(title, legs):
    ts = {n: [] for n, _ in legs}
    for _ in range(a.rounds):
        for n, fn in legs:
            ts[n].append(timed(fn, a.reps))
    med = lambda x: sorted(x)[len(x) // 2]
    print(title)
    for n, _ in legs:
        print(f"  {n:34s} median {med(ts[n]):8.1f}  min {min(ts[n]):8.1f}  max {max(ts[n]):8.1f} us", flush=True)
    (n0, _), (n1, _) = legs
    spread = max(max(ts[n]) - min(ts[n]) for n in (n0, n1))
    print(f"  difference of the medians {med(ts[n1]) - med(ts[n0]):+.1f} us; larger spread of a leg over the rounds {spread:.1f} us")


# ---- vocabulary cross-entropy
g = torch.Generator(device=dev).manual_seed(1)
for M, frac, name in ((18400, 0.15, "dense, 18 400 rows, 15 % labelled"), (400, 1.0, "compact, 400 labelled rows")):
    X = (torch.randn(M, LDV, device=dev, generator=g) * 3).to(torch.bfloat16)
    lab = torch.randint(0, V, (M,), device=dev, generator=g)
    lab[torch.rand(M, device=dev, generator=g) >= frac] = -100
    bounds = torch.tensor([0, M // 3, 2 * M // 3, M], dtype=torch.int32, device=dev)
    gs = torch.tensor([0.3, 0.3, 0.3], device=dev)
    dl = torch.empty_like(X)
    state = {e: ops.ce_fwd(X, V, lab, bounds, 3, smoothing=e) for e in (0.0, 0.1)}
    ab(f"ce forward ({name}): ce_count_kernel + ce_row_kernel<0>",
       [(f"eps = {e}", (lambda e=e: ops.ce_fwd(X, V, lab, bounds, 3, smoothing=e))) for e in (0.0, 0.1)])
    ab(f"ce backward ({name}): ce_row_kernel<1>",
       [(f"eps = {e}", (lambda e=e: ops.ce_bwd(X, V, lab, bounds, 3, state[e][1], gs, state[e][2], dl, smoothing=e))) for e in (0.0, 0.1)])
    del X, dl

# ---- the heads' loss level
H = 768


def head_model(C):
    torch.manual_seed(0)
    cfg = MMBertConfig(hidden_size=H, num_hidden_layers=1, num_attention_heads=H // 64, intermediate_size=4 * H, vocab_size=512)
    m = MMBertForPretraining(cfg, num_labels=C)
    m.bert.set_joint_embeddings("mosei")
    m.to(dev)
    m._ensure_ready(dev)
    return m


def level7(m, B, C, options):
    m.set_loss_options(**options)
    first = torch.randn(3 * B, H, device=dev, generator=torch.Generator(device=dev).manual_seed(B))
    apl = torch.randint(0, 2, (2 * B,), device=dev)
    sent = torch.randint(0, C, (B,), device=dev) if C not in (1, 7) else torch.rand(B, device=dev) * 6 - 3
    rec, outs, keep = MM._HeadsStepFn._setup(m, B, H, dev, apl, sent, first=first)
    ops.heads_step_fwd(rec, 1, 6)
    # (level 7 normalises the CPC score matrices in place: repeated launches rescale them again -- the work per launch is the same)
    return (lambda: ops.heads_step_fwd(rec, 7, 7)), (rec, outs, keep, first, apl, sent, m.class_weights)


for B in (16, 128):
    m6, m7 = head_model(6), head_model(7)
    plain, k0 = level7(m6, B, 6, {})
    full, k1 = level7(m6, B, 6, dict(class_weights=[0.5, 1.0, 2.0, 4.0, 0.25, 1.5], label_smoothing=0.1))
    ab(f"heads forward level 7, B = {B}, H = {H}, 6-class head", [("plain cross-entropy", plain), ("class weights + smoothing 0.1", full)])
    mse, k2 = level7(m7, B, 7, {})
    hub, k3 = level7(m7, B, 7, dict(regression="huber", huber_delta=0.5))
    ab(f"heads forward level 7, B = {B}, H = {H}, regression head", [("MSE", mse), ("Huber(0.5)", hub)])
