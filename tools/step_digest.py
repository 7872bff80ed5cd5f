#!/usr/bin/env python3
"""SHA-256 digests of two deterministic train steps, for bit identity between two trees: the public model API only, so the same file runs
against either tree by PYTHONPATH (as tools/ab_tree.sh runs two trees), one process per tree on the same GPU; the outputs must be equal
line for line.

    PYTHONPATH=<tree> python tools/step_digest.py > digest.txt

Configuration B of tests/test_step_stages_gpu.py (hidden 256, 3 layers, 4 heads, intermediate 1024, vocab 4096, mosei), batches
``synthetic_batch(4, 24, 200, 130, vocab=4096)``, deterministic mode, train mode (all dropouts on), two steps of the project's AdamW.  Per
case -- each with the defaults and with ``composite_layers = False`` -- one line each for: the loss and every returned output of both steps,
every parameter's ``.grad`` after the first backward, every parameter after the second step.  On one model of the plain, the Q/V-adapter and
the dense-adapter case also ``predict(return_attention="all")`` and ``predict_tokens``.
"""
import hashlib
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (behind PYTHONPATH: another tree named there wins)
import torch  # noqa: E402
from msa_amd import ops  # noqa: E402
from msa_amd.data import batch_to, synthetic_batch  # noqa: E402
from msa_amd.model import MMBertConfig, MMBertForPretraining  # noqa: E402
from msa_amd.optim import AdamW  # noqa: E402

DEV = "cuda"
DENSE = ("attention_output", "intermediate", "ffn_output")
PLAIN = dict(skip_padded_backward=False, sparse_top_layer_backward=False, sparse_mlm_backward=False, defer_wgrads=False)
CASES = [("plain", dict(), None),
         ("shortcuts off", PLAIN, None),
         ("defer_wgrads", dict(defer_wgrads=True), None),
         ("freeze(embeddings, layers=1)", dict(), lambda m: m.freeze(embeddings=True, layers=1)),
         ("freeze(layer_weights): bias-only", dict(), lambda m: m.freeze(layers=0, layer_weights=True)),
         ("lora r=4 q+v", dict(), lambda m: m.add_lora(r=4, targets=("query", "value"), seed=3)),
         ("lora r=4 dense", dict(), lambda m: m.add_lora(r=4, targets=DENSE, seed=3)),
         ("lora r=4 q+k+v+dense", dict(), lambda m: m.add_lora(r=4, targets=("query", "key", "value") + DENSE, seed=3)),
         ("label-only", dict(), None)]
PREDICT = ("plain", "lora r=4 q+v", "lora r=4 dense")


def tensors(v, path=""):
    """(path, tensor) of every tensor in a nest of tuples, lists and dicts, in a fixed order."""
    if torch.is_tensor(v):
        yield path, v
    elif isinstance(v, dict):
        for k in sorted(v, key=str):
            yield from tensors(v[k], f"{path}.{k}")
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            yield from tensors(x, f"{path}[{i}]")


def digest(v):
    h = hashlib.sha256()
    for path, t in tensors(v):
        t = t.detach().contiguous().cpu()
        h.update(f"{path} {t.dtype} {tuple(t.shape)}".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def batch(seed, label_only):
    b = batch_to(synthetic_batch(4, 24, 200, 130, dataset="mosei", vocab=4096, seed=seed), DEV)
    return dict(b, masked_labels=None) if label_only else b


def run(name, flags, prepare, composite):
    tag = f"{name} | {'composite' if composite else 'per-launch'}"
    torch.manual_seed(0)
    m = MMBertForPretraining(MMBertConfig(vocab_size=4096, hidden_size=256, num_hidden_layers=3, num_attention_heads=4, intermediate_size=1024))
    m.bert.set_joint_embeddings("mosei")
    m.to(DEV).train()
    m.manual_seed(29)
    for k, v in flags.items():
        setattr(m, k, v)
    if not composite:
        m.composite_layers = False
    if prepare is not None:
        prepare(m)
    opt = AdamW(list(m.parameters()), lr=1e-3, weight_decay=0.01)
    for step in (1, 2):
        out, logits = m(**batch(60 + step, name == "label-only"))
        out[0].mean().backward()
        print(f"{tag} | step {step} loss {digest(out[0])} outputs {digest((out, logits))}")
        if step == 1:
            print(f"{tag} | step 1 grads {digest({n: p.grad for n, p in m.named_parameters() if p.grad is not None})}")
        opt.step()
        opt.zero_grad()
    print(f"{tag} | step 2 parameters {digest(dict(m.named_parameters()))}")
    if name in PREDICT and composite:
        b = batch(70, False)
        ids = (b["input_ids"], b["token_type_ids"], b["attention_mask"])
        print(f"{tag} | predict(return_attention='all') {digest(m.predict(*ids, return_attention='all'))}")
        print(f"{tag} | predict_tokens {digest(m.predict_tokens(*ids, masked_labels=b['masked_labels']))}", flush=True)


ops.set_deterministic(True)
for name, flags, prepare in CASES:
    for composite in (True, False):
        run(name, flags, prepare, composite)
torch.cuda.synchronize()
