#!/usr/bin/env python3
"""What a prediction costs: ``model.predict`` against what had to be called before it existed, same process, alternating order.

    python tools/bench_predict.py [--calls 50] [--rounds 3] [--shapes headline,refdef32,refdef256] [--kernel]

Shapes: ``headline`` (12 layers, d = 768, T = 50, A = V = 500, B = 16) and the reference's default model (bert-large, T = P = 40:
REF:train.py:28,32,38) at B = 32 and B = 256.  Legs, ms per call (device events around ``--calls`` calls, every shape and leg warmed
up first, ``--rounds`` alternating rounds: median, and the spread max - min over the rounds of the SAME leg):
  (a) model.eval() + no_grad + forward with dummy labels          -- the only way to predictions without predict()
  (b) the same with return_scores = False                         -- expected equal to (a): the dense MLM head runs under no_grad anyway
  (c) model.predict                                               -- no labels, [CLS]-only top layer, no MLM head
  (d) model.predict(return_attention="top")                       -- (c) + one ops.attn_probs_first launch and the slicing of its result
  (e) model.predict(return_attention="all")                       -- (c) + one such launch per layer
plus the peak allocation of each above the level before the call (torch.cuda.max_memory_allocated).
``--kernel``: the stand-alone time of ops.attn_fwd_first at the headline layout (16 x 50 + 32 x 550 rows, 12 heads; device events
around 200 launches) and the bytes it reads (K and V of every row once, one query row and the key bias per (sequence, head)) over
that time, as a share of the 6.3 TB/s a long copy reaches (a bandwidth share: the kernel has no MFMA work); and the same for
ops.attn_probs_first, whose counted bytes are the K read, the fp32 [sequences, heads, 550] store, the query rows and the key bias.
``--tokens``: masked-token prediction at ``headline`` and ``refdef32`` (15 % masking, the batch's own labels), same timing rules:
  (ta) the route without predict_tokens: (a) with return_scores = True, then log_softmax + torch.topk(5) + the labels' log-probabilities on
       the labelled rows of the three score tensors
  (tb) model.predict_tokens on the same labels
``--topk-kernel``: ops.vocab_topk (k = 1, 5, 8, with labels) against ops.ce_fwd on the same [n, Vpad] bf16 logits (V = 30 522), n = the
headline batch's labelled rows and n = 4096 (one full chunk of predict_tokens); device events around 200 launches, median of 3.
The last line of the output is one JSON object with every number."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msa_amd.data import synthetic_batch, batch_to
from msa_amd.model import MMBertConfig, MMBertForPretraining

SHAPES = {
    "headline": dict(L=12, H=768, heads=12, I=3072, V=30522, T=50, Pv=500, Pa=500, B=16),
    "refdef32": dict(L=24, H=1024, heads=16, I=4096, V=30522, T=40, Pv=40, Pa=40, B=32),
    "refdef256": dict(L=24, H=1024, heads=16, I=4096, V=30522, T=40, Pv=40, Pa=40, B=256),
}
COPY_BW = 6.3e12          # bytes/s of a long device copy on this part


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def bench_shape(name, s, calls, rounds, dev):
    torch.manual_seed(0)
    model = MMBertForPretraining(MMBertConfig(vocab_size=s["V"], hidden_size=s["H"], num_hidden_layers=s["L"], num_attention_heads=s["heads"],
                                              intermediate_size=s["I"]))
    model.bert.set_joint_embeddings("mosei")
    model.set_alpha_beta(1.0, 1.0)
    model.to(dev).eval()
    batch = batch_to(synthetic_batch(s["B"], s["T"], s["Pv"], s["Pa"], vocab=s["V"], seed=50), dev)
    args3 = (batch["input_ids"], batch["token_type_ids"], batch["attention_mask"])

    def forward(scores):
        def f():
            model.return_scores = scores
            with torch.no_grad():
                return model(**batch)[1]
        return f
    legs = [("a_forward", forward(True)), ("b_forward_no_scores", forward(False)), ("c_predict", lambda: model.predict(*args3)),
            ("d_predict_attn_top", lambda: model.predict(*args3, return_attention="top")),
            ("e_predict_attn_all", lambda: model.predict(*args3, return_attention="all"))]
    for _, fn in legs:                                        # warm-up of every leg at this shape
        for _ in range(3):
            fn()
    times = {n: [] for n, _ in legs}
    for r in range(rounds):
        order = legs if r % 2 == 0 else legs[::-1]
        for n, fn in order:
            fn()
            times[n].append(timed(fn, calls))
    res = {}
    for n, fn in legs:
        t = sorted(times[n])
        res[n] = dict(ms=t[len(t) // 2], spread_ms=t[-1] - t[0], peak_bytes=peak_of(fn))
    model.return_scores = True
    base = min(res["a_forward"]["ms"], res["b_forward_no_scores"]["ms"])
    res["predict_over_forward"] = res["c_predict"]["ms"] / base
    for n, _ in legs:
        print(f"{name:10s} {n:22s} {res[n]['ms']:9.3f} ms/call  spread {res[n]['spread_ms']:.3f} ms  peak {res[n]['peak_bytes'] / 2 ** 20:9.1f} MiB")
    print(f"{name:10s} predict / min(a, b) = {res['predict_over_forward']:.4f}")
    for n in ("d_predict_attn_top", "e_predict_attn_all"):
        res[n]["over_predict_ms"] = res[n]["ms"] - res["c_predict"]["ms"]
        print(f"{name:10s} {n} - c_predict = {res[n]['over_predict_ms'] * 1e3:+.1f} us")
    del model
    torch.cuda.empty_cache()
    return res


def bench_kernel(dev):
    from msa_amd import ops
    heads, H = 12, 768
    lens = [50] * 16 + [550] * 32
    M = sum(lens)
    layout = ops.SeqLayout(lens, heads, dev)
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(M, 3 * H, generator=g).to(torch.bfloat16).to(dev)
    kb = ops.pad_key_bias(torch.zeros(M, device=dev), layout)
    q_rows = layout.seq_start.to(torch.int32).contiguous()
    fn = lambda: ops.attn_fwd_first(qkv, kb, layout, H, q_rows)
    for _ in range(10):
        fn()
    ts = sorted(timed(fn, 200) for _ in range(3))
    ms = ts[1]
    nbytes = M * 2 * H * 2 + len(lens) * H * 2 * 2 + M * 4 * heads          # K, V | query rows, output | key bias per head
    res = dict(ms=ms, spread_ms=ts[-1] - ts[0], bytes=nbytes, bytes_per_s=nbytes / (ms * 1e-3), share_of_copy_bandwidth=nbytes / (ms * 1e-3) / COPY_BW)
    print(f"attn_fwd_first headline layout: {ms * 1e3:.1f} us (spread {res['spread_ms'] * 1e3:.1f} us), {nbytes / 1e6:.1f} MB read -> "
          f"{res['bytes_per_s'] / 1e12:.2f} TB/s = {100 * res['share_of_copy_bandwidth']:.1f} % of the 6.3 TB/s of a long copy (bandwidth share)")
    return res


def bench_probs_kernel(dev):
    from msa_amd import ops
    heads, H = 12, 768
    lens = [50] * 16 + [550] * 32
    M = sum(lens)
    layout = ops.SeqLayout(lens, heads, dev)
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(M, 3 * H, generator=g).to(torch.bfloat16).to(dev)
    kb = ops.pad_key_bias(torch.zeros(M, device=dev), layout)
    q_rows = layout.seq_start.to(torch.int32).contiguous()
    out = torch.empty((len(lens), heads, max(lens)), device=dev, dtype=torch.float32)
    fn = lambda: ops.attn_probs_first(qkv, kb, layout, H, q_rows, out=out)
    for _ in range(10):
        fn()
    ts = sorted(timed(fn, 200) for _ in range(3))
    ms = ts[1]
    k_bytes, store = M * H * 2, out.numel() * 4
    nbytes = k_bytes + store + len(lens) * H * 2 + M * 4 * heads              # K | probabilities | query rows | key bias per head
    res = dict(ms=ms, spread_ms=ts[-1] - ts[0], bytes=nbytes, k_bytes=k_bytes, store_bytes=store, bytes_per_s=nbytes / (ms * 1e-3),
               share_of_copy_bandwidth=nbytes / (ms * 1e-3) / COPY_BW)
    print(f"attn_probs_first headline layout: {ms * 1e3:.1f} us (spread {res['spread_ms'] * 1e3:.1f} us), {k_bytes / 1e6:.1f} MB K read + "
          f"{store / 1e6:.1f} MB store, {nbytes / 1e6:.1f} MB in all -> {res['bytes_per_s'] / 1e12:.2f} TB/s = "
          f"{100 * res['share_of_copy_bandwidth']:.1f} % of the 6.3 TB/s of a long copy (bandwidth share)")
    return res


def bench_tokens(name, s, calls, rounds, dev):
    torch.manual_seed(0)
    model = MMBertForPretraining(MMBertConfig(vocab_size=s["V"], hidden_size=s["H"], num_hidden_layers=s["L"], num_attention_heads=s["heads"],
                                              intermediate_size=s["I"]))
    model.bert.set_joint_embeddings("mosei")
    model.set_alpha_beta(1.0, 1.0)
    model.to(dev).eval()
    batch = batch_to(synthetic_batch(s["B"], s["T"], s["Pv"], s["Pa"], vocab=s["V"], seed=50), dev)
    args3 = (batch["input_ids"], batch["token_type_ids"], batch["attention_mask"])
    labels = batch["masked_labels"]
    masks = [(l >= 0) & (l < s["V"]) for l in labels]
    n = int(sum(int(m.sum()) for m in masks))
    tokens = sum(l.numel() for l in labels)

    def today():
        model.return_scores = True
        with torch.no_grad():
            out = model(**batch)[0]
            res = []
            for p, k in enumerate((7, 9, 11)):
                lp = torch.log_softmax(out[k][masks[p]].float(), -1)
                res.append((torch.topk(lp, 5, dim=-1), lp.gather(1, labels[p][masks[p]][:, None])))
        return res
    legs = [("ta_forward_scores_topk", today), ("tb_predict_tokens", lambda: model.predict_tokens(*args3, masked_labels=labels, top_k=5))]
    for _, fn in legs:
        for _ in range(3):
            fn()
    times = {k: [] for k, _ in legs}
    for r in range(rounds):
        for k, fn in (legs if r % 2 == 0 else legs[::-1]):
            fn()
            times[k].append(timed(fn, calls))
    res = dict(labelled_rows=n, tokens=tokens)
    for k, fn in legs:
        t = sorted(times[k])
        res[k] = dict(ms=t[len(t) // 2], spread_ms=t[-1] - t[0], peak_bytes=peak_of(fn))
        print(f"{name:10s} {k:24s} {res[k]['ms']:9.3f} ms/call  spread {res[k]['spread_ms']:.3f} ms  peak {res[k]['peak_bytes'] / 2 ** 20:9.1f} MiB")
    res["tb_over_ta"] = res["tb_predict_tokens"]["ms"] / res["ta_forward_scores_topk"]["ms"]
    print(f"{name:10s} {n} labelled rows of {tokens}: predict_tokens / (forward + topk) = {res['tb_over_ta']:.4f} in time, "
          f"{res['tb_predict_tokens']['peak_bytes'] / max(1, res['ta_forward_scores_topk']['peak_bytes']):.4f} in peak memory")
    del model
    torch.cuda.empty_cache()
    return res


def bench_topk_kernel(dev, rows):
    from msa_amd import ops
    V, Vp = 30522, 30528
    out = {}
    for n in rows:
        g = torch.Generator().manual_seed(n)
        logits = (3.0 * torch.randn(n, Vp, generator=g)).to(torch.bfloat16).to(dev)
        labels = torch.randint(0, V, (n,), generator=g).to(dev)
        bounds = torch.tensor([0, n], dtype=torch.int32, device=dev)
        legs = [("ce_fwd", lambda: ops.ce_fwd(logits, V, labels, bounds, 1))] + \
               [(f"vocab_topk_k{k}", (lambda k=k: ops.vocab_topk(logits, V, k, labels))) for k in (1, 5, 8)]
        r = {}
        for name, fn in legs:
            for _ in range(10):
                fn()
            ts = sorted(timed(fn, 200) for _ in range(3))
            r[name] = dict(us=ts[1] * 1e3, spread_us=(ts[-1] - ts[0]) * 1e3, tb_per_s=n * Vp * 2 / (ts[1] * 1e-3) / 1e12)
        for k in (1, 5, 8):
            r[f"vocab_topk_k{k}"]["over_ce_fwd"] = r[f"vocab_topk_k{k}"]["us"] / r["ce_fwd"]["us"]
        for name, _ in legs:
            print(f"n = {n:5d}  {name:16s} {r[name]['us']:8.1f} us (spread {r[name]['spread_us']:.1f})  {r[name]['tb_per_s']:.2f} TB/s of logits read"
                  + (f"  x{r[name]['over_ce_fwd']:.2f} of ce_fwd" if "over_ce_fwd" in r[name] else ""))
        out[str(n)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="headline,refdef32,refdef256")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--tokens", action="store_true")
    ap.add_argument("--topk-kernel", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_predict.py needs the GPU: there is no CPU path and no number to report without one")
    dev = torch.device("cuda", 0)
    out = dict(calls=a.calls, rounds=a.rounds, shapes={})
    for name in [x for x in a.shapes.split(",") if x]:
        out["shapes"][name] = bench_shape(name, SHAPES[name], a.calls, a.rounds, dev)
    if a.kernel:
        out["attn_fwd_first"] = bench_kernel(dev)
        out["attn_probs_first"] = bench_probs_kernel(dev)
    if a.tokens:
        out["tokens"] = {name: bench_tokens(name, SHAPES[name], a.calls, a.rounds, dev) for name in ("headline", "refdef32")}
    if a.topk_kernel:
        rows = [out["tokens"]["headline"]["labelled_rows"]] if a.tokens else [360]
        out["vocab_topk"] = bench_topk_kernel(dev, rows + [4096])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
