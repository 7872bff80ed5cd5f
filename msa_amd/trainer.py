"""Counterpart of the reference's training loop (REF:trainer.py:13-101) and of the input producers it
calls (REF:model_utils.py:6-143): same packing, same stepping rule, same return value.

Differences, all deliberate and documented in DESIGN.md:
* tensors are built on / moved to the GPU once per step and loss bookkeeping stays on the device
  (the reference calls ``.item()`` >= 3x per step, REF:trainer.py:85-93: a device sync each);
* ``quirk_step=True`` keeps ``(step+1) & gradient_accumulation_step == 0`` (REF:trainer.py:96 -- at
  gas=1 the optimizer steps every SECOND micro-batch); ``False`` gives the intended modulo;
* with a ``parallel.DataParallel`` wrapper the gradient exchange happens only on stepping micro-batches.
"""
from __future__ import annotations

import types
from typing import Optional

import torch
from torch.nn.utils.rnn import pad_sequence

PAD, CLS, SEP, MASK = 0, 101, 102, 103
_mask_calls = 0          # fallback call counter (only when the CUDA generator's offset cannot be read)


def _device_mask_seed(device) -> int:
    """The per-call seed of the device-side masking kernel, taken from torch's default CUDA generator of ``device``: its seed and
    its philox OFFSET, which this call advances by 4 (what one ``torch.bernoulli`` launch would consume).  So ``torch.manual_seed(s)``
    (seed := s, offset := 0) reproduces the masks from that point on, ``get_rng_state`` / ``set_rng_state`` capture them, and other
    CUDA draws in between shift them -- like a torch draw.  The data-parallel rank is folded in: ranks seeded alike still draw
    different selection patterns.  NOT the bits torch.bernoulli would produce (counter RNG of csrc/common.h; selection / replacement
    probabilities are quantised to 1/65536)."""
    global _mask_calls
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    try:
        off = gen.get_offset()
        gen.set_offset(off + 4)
    except (AttributeError, RuntimeError):                    # (older torch: no offset accessors -> process-wide call counter)
        _mask_calls += 1
        off = 4 * _mask_calls
    rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
    return (gen.initial_seed() * 1000003 + (off // 4) * 8191 + rank * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def mask_tokens(inputs: torch.Tensor, args, generator: Optional[torch.Generator] = None, special_ids=(CLS, SEP), mask_id=MASK):
    """REF:model_utils.py:6-39 on the tensor's own device: Bernoulli(mlm_probability) selection with
    special tokens excluded (:17-23), labels -100 elsewhere (:28), 80 % of the selected positions
    -> [MASK] (:30-32, in place like the reference); the 10 % random-token branch is commented out
    in the reference (:34-37) and therefore absent.
    ``special_ids``: [CLS] and [SEP] -- what ``get_special_tokens_mask(already_has_special_tokens=True)`` of the pinned
    transformers 2.8 flags.  [PAD] is NOT excluded: the reference's PAD branch (:24-26) calls the non-in-place
    ``masked_fill`` and drops the result, so padding positions are selected at the same 15 % (label 0, 80 % -> [MASK]);
    pass ``special_ids=(PAD, CLS, SEP)`` for the intended rule (a deviation from the reference).  With ``generator=None``
    on CPU the draws are the reference's own (same two ``torch.bernoulli`` calls in the same order on the global RNG:
    pinned by tests/golden/mask_tokens.npz)."""
    if inputs.is_cuda and generator is None and inputs.dtype == torch.int64 and len(special_ids) <= 3:
        # on the GPU: one launch of the library's counter-RNG masking kernel (mmbert_mlm_mask) instead of ~10 element-wise
        # torch kernels; the per-call seed is drawn from torch's default CUDA generator (seed + offset, see _device_mask_seed), so
        # torch.manual_seed() / the CUDA RNG state govern it; pass a ``generator`` for torch's own bernoulli draws
        from . import ops
        x = inputs if inputs.is_contiguous() else inputs.contiguous()
        labels = ops.mlm_mask(x, float(args.mlm_probability), _device_mask_seed(inputs.device),
                              special_ids=tuple(special_ids), mask_id=mask_id)
        if x is not inputs:
            inputs.copy_(x)
        return inputs, labels
    labels = inputs.clone()
    prob = torch.full(labels.shape, float(args.mlm_probability), device=inputs.device)
    special = torch.zeros_like(inputs, dtype=torch.bool)
    for s in special_ids:
        special |= inputs == s
    prob.masked_fill_(special, 0.0)
    masked = torch.bernoulli(prob, generator=generator).bool()
    labels[~masked] = -100
    replaced = torch.bernoulli(torch.full(labels.shape, 0.8, device=inputs.device), generator=generator).bool() & masked
    inputs[replaced] = mask_id
    return inputs, labels


def collate(examples):
    """REF:model_utils.py:51-143 output contract: (text_batch, visual_batch, speech_batch,
    attention_batch, segments, rawData) with the reference's dtypes and quirks -- text mask 0 at
    PAD (:118-120); pair masks ``feature != 0`` (float64 visual :124-125, int64 speech :132-133);
    text-with-pair masks stay all ones (``==`` instead of ``=``, :128,136)."""
    te, tl, tti, ts, twv, ve, vl, vti, vs, tws, se, sl, sti, ss, seg, raw = zip(*examples)
    for a, b, c, d, e in zip(te, ve, se, twv, tws):
        assert len(a) == len(b) == len(c) == len(d) == len(e)                # :92
    sent_dtype = torch.long if torch.as_tensor(ts[0]).dtype == torch.int64 else torch.float
    mk_sent = lambda x: torch.tensor([float(v) if sent_dtype == torch.float else int(v) for v in x], dtype=sent_dtype)
    if torch.as_tensor(ts[0]).numel() > 1:                                   # a vector label per item (multi-label head): float32 [B, C]
        mk_sent = lambda x: torch.stack([torch.as_tensor(v, dtype=torch.float32).reshape(-1) for v in x])
    text = pad_sequence([torch.as_tensor(t) for t in te], batch_first=True, padding_value=0)
    text_mask = torch.ones(text.shape, dtype=torch.float64)
    text_mask[text == 0] = 0
    vis = torch.as_tensor(_stack(ve))
    vis_mask = torch.ones(vis.shape, dtype=torch.float64)
    vis_mask[vis == 0] = 0
    sp = torch.as_tensor(_stack(se))
    sp_mask = torch.ones(sp.shape, dtype=torch.int64)
    sp_mask[sp == 0] = 0
    twv_t, tws_t = torch.as_tensor(_stack(twv)), torch.as_tensor(_stack(tws))
    twv_mask = torch.ones(twv_t.shape, dtype=torch.float64)                 # quirk: never zeroed
    tws_mask = torch.ones(tws_t.shape, dtype=torch.int64)
    lab = lambda x: torch.tensor([int(v) for v in x], dtype=torch.int64)
    text_batch = (text, lab(tl), pad_sequence(list(tti), batch_first=True, padding_value=0).long(), text_mask, mk_sent(ts))
    visual_batch = (twv_t, vis, lab(vl), pad_sequence(list(vti), batch_first=True, padding_value=0), vis_mask, mk_sent(vs))
    speech_batch = (tws_t, sp, lab(sl), pad_sequence(list(sti), batch_first=True, padding_value=0), sp_mask, mk_sent(ss))
    return text_batch, visual_batch, speech_batch, (twv_mask, tws_mask), list(seg), list(raw)


def _stack(seq):
    import numpy as np
    return np.stack([np.asarray(x) for x in seq])


def pack_step_inputs(batch, args, device, generator=None):
    """REF:trainer.py:42-64: MLM masking (re-drawn independently for text / twv / tws), label
    duplication for the pair positions, tuple packing -- returns the model's keyword arguments.
    ``args.label_only`` (not a reference argument; ``default_args()`` has it False): the label-only step of
    ``MMBertForPretraining.forward`` -- no MLM masking (nothing is drawn from ``generator`` or the device's mask seed), the ids as they
    are, ``masked_labels=None``; train_epoch / eval_epoch / train and dataset.DeviceBatchBuilder.epoch pack through here."""
    text_batch, visual_batch, speech_batch, attention_batch = batch[:4]
    dev = torch.device(device)
    t0, v0, s0 = text_batch[0].to(dev), visual_batch[0].to(dev), speech_batch[0].to(dev)
    if getattr(args, "label_only", False):
        return dict(
            input_ids=(t0, visual_batch[1].to(dev), speech_batch[1].to(dev), v0, s0),
            token_type_ids=(text_batch[2].to(dev), visual_batch[3].to(dev), speech_batch[3].to(dev)),
            attention_mask=(text_batch[3].to(dev), (attention_batch[0].to(dev), visual_batch[4].to(dev)),
                            (attention_batch[1].to(dev), speech_batch[4].to(dev))),
            masked_labels=None,
            ap_label=(visual_batch[2].to(dev), speech_batch[2].to(dev)),
            sentiment=text_batch[-1].to(dev),
        )
    if args.mlm:
        text_inputs, text_labels = mask_tokens(t0.clone(), args, generator)
        twv_ids, v_labels = mask_tokens(v0.clone(), args, generator)
        tws_ids, s_labels = mask_tokens(s0.clone(), args, generator)
    else:
        text_inputs, text_labels, twv_ids, v_labels, tws_ids, s_labels = t0, t0, v0, v0, s0, s0
    v_labels = torch.cat((v_labels, v_labels), dim=-1)                       # REF:trainer.py:50 (needs P == T)
    s_labels = torch.cat((s_labels, s_labels), dim=-1)                       # REF:trainer.py:53
    return dict(
        input_ids=(text_inputs, visual_batch[1].to(dev), speech_batch[1].to(dev), twv_ids, tws_ids),
        token_type_ids=(text_batch[2].to(dev), visual_batch[3].to(dev), speech_batch[3].to(dev)),
        attention_mask=(text_batch[3].to(dev), (attention_batch[0].to(dev), visual_batch[4].to(dev)),
                        (attention_batch[1].to(dev), speech_batch[4].to(dev))),
        masked_labels=(text_labels, v_labels, s_labels),
        ap_label=(visual_batch[2].to(dev), speech_batch[2].to(dev)),
        sentiment=text_batch[-1].to(dev),
    )


def should_step(step: int, gas: int, quirk: bool = True) -> bool:
    return (((step + 1) & gas) == 0) if quirk else (((step + 1) % gas) == 0)


def train_epoch(args, model, traindata, optimizer, scheduler, tokenizer=None, *, device="cuda", dp=None, quirk_step=True,
                generator=None, shuffle=True, batches=None):
    """One epoch.  ``traindata``: a Dataset of the reference's 16-tuples (collated here), or pass
    ``batches`` = an iterable of ready model-kwargs dicts (the synthetic generator).
    Returns the reference's 6-tuple (REF:trainer.py:101): (train_loss, text_loss, visual_loss,
    speech_loss, ap_loss_of_the_LAST_step, label_loss) each divided by the number of steps.
    ``args.max_grad_norm`` (optional; the reference has no such argument and ``default_args()`` leaves it out): clip the accumulated
    gradient to that global L2 norm in every optimizer step, fused into the step (``AdamW.clip_grad_norm_``)."""
    if batches is None:
        from torch.utils.data import DataLoader, RandomSampler, SequentialSampler
        sampler = RandomSampler(traindata) if shuffle else SequentialSampler(traindata)
        loader = DataLoader(traindata, sampler=sampler, batch_size=args.train_batch_size, collate_fn=collate)
        batches = (pack_step_inputs(b, args, device, generator) for b in loader)
    gas = args.gradient_accumulation_step
    max_grad_norm = getattr(args, "max_grad_norm", None)                   # (not a reference argument: None = no clipping)
    model.train()
    train_loss = torch.zeros((), device=device)
    label_loss = torch.zeros((), device=device)
    ap_loss = torch.zeros((), device=device)
    n = 0
    for step, kwargs in enumerate(batches):
        stepping = should_step(step, gas, quirk_step)
        ctx = dp.no_sync() if (dp is not None and not stepping) else _null()
        with ctx:
            outputs, _ = model(**kwargs)
            loss = outputs[0]
            loss.mean().backward()                                           # REF:trainer.py:83
        train_loss += loss.detach().mean()
        label_loss += outputs[5].detach().mean()
        ap_loss = outputs[4].detach()
        n += 1
        if stepping:                                                         # REF:trainer.py:96-99
            if dp is not None:
                dp.finish_backward()
            if max_grad_norm is not None:                                    # the accumulated gradient, once per step
                optimizer.clip_grad_norm_(max_grad_norm)
            optimizer.step()
            scheduler.step()
            optimizer.zero_grad()
    if n == 0:
        return (0.0,) * 6
    return (float(train_loss) / n, 0.0, 0.0, 0.0, float(ap_loss) / n, float(label_loss) / n)


def on_input_stream(model, batches):
    """Wraps an iterable of model-kwargs dicts whose tensors are BUILT ON THE GPU (dataset.DeviceBatchBuilder, the MLM masking
    kernel): every batch is produced on ``model.input_stream`` instead of the compute stream and TAGGED for the model (its first
    tensor is remembered until the next batch is asked for), so that forward() runs the step prologue on the input stream too --
    batch building and the prologue then run ahead of the previous step's backward / optimizer tail, and the host enqueues a step
    ahead of the GPU (a slow host no longer shows up as GPU idle time).  Only the tagged batch takes that path: an eval_epoch or a
    plain train_epoch afterwards, whose batches are built on the compute stream, is synchronised as usual (the model's own
    ``async_prologue`` switch is left alone).  The source tensors the builder reads must be complete (a resident dataset).
    ``train_epoch(..., batches=on_input_stream(model, builder_batches))``."""
    side = model.input_stream

    def mark(x, main):
        if torch.is_tensor(x):
            if x.is_cuda:
                x.record_stream(main)              # allocated on the input stream's pool, read by the compute stream
        elif isinstance(x, (tuple, list)):
            for y in x:
                mark(y, main)
        elif isinstance(x, dict):
            for y in x.values():
                mark(y, main)

    def first_tensor(b):
        ids = b.get("input_ids")
        return ids[0] if isinstance(ids, (tuple, list)) else ids

    it = iter(batches)
    try:
        while True:
            main = torch.cuda.current_stream()
            with torch.cuda.stream(side):
                try:
                    b = next(it)
                except StopIteration:
                    return
            mark(b, main)
            model.__dict__["_input_stream_batch"] = first_tensor(b)
            yield b
            model.__dict__["_input_stream_batch"] = None
    finally:                                       # exhausted, closed or abandoned: nothing stays tagged
        model.__dict__["_input_stream_batch"] = None


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def default_args(**kw):
    """The reference's argparse defaults that the loop reads (REF:train.py:24-42)."""
    d = dict(train_batch_size=32, mlm=True, mlm_probability=0.15, gradient_accumulation_step=1, learning_rate=5e-4,
             warmup_proportion=1.0, n_epochs=200, max_seq_length=40, label_only=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def balanced_class_weights(labels, C):
    """Class weights that undo the imbalance of ``labels`` (integer classes in [0, C)): N / (C * max(count_c, 1)), float32 [C] -- sklearn's
    ``class_weight="balanced"``, with an absent class counted once so that every weight stays finite."""
    y = torch.as_tensor(labels).reshape(-1).long()
    if y.numel() and (int(y.min()) < 0 or int(y.max()) >= int(C)):
        raise ValueError(f"balanced_class_weights: labels outside [0, {C})")
    count = torch.bincount(y, minlength=int(C)).clamp(min=1).to(torch.float64)
    return (float(y.numel()) / (float(C) * count)).to(torch.float32)


def balanced_pos_weight(labels):
    """Positive weights that undo the imbalance of multi-hot ``labels`` [N, C] (< 0: not annotated, left out): per column
    #negatives / max(#positives, 1) over its annotated entries, float32 [C] -- the usual ``pos_weight`` of a binary cross-entropy."""
    y = torch.as_tensor(labels).to(torch.float64)
    if y.dim() != 2:
        raise ValueError(f"balanced_pos_weight: labels [N, C], got {tuple(y.shape)}")
    valid = y >= 0
    pos = ((y > 0.5) & valid).sum(0).to(torch.float64)
    neg = ((y <= 0.5) & valid).sum(0).to(torch.float64)
    return (neg / pos.clamp(min=1.0)).to(torch.float32)


def apply_loss_options(model, args, train_dataset=None):
    """``model.set_loss_options`` from the optional ``args.label_loss`` ("mse" | "l1" | "huber"), ``args.huber_delta``, ``args.class_weights``
    (a sequence of C values, or "balanced": ``balanced_class_weights`` of ``train_dataset``'s labels), ``args.label_smoothing`` and
    ``args.mlm_label_smoothing``; for a multi-label head ``args.pos_weight`` (a sequence of C values, or "balanced":
    ``balanced_pos_weight`` of ``train_dataset``'s label vectors), ``args.thresholds`` and ``args.multilabel_smoothing``.
    ``default_args()`` has none of them: a model is then left exactly as it is (options set by hand stay).
    Returns whether anything was set."""
    names = ("label_loss", "huber_delta", "class_weights", "label_smoothing", "mlm_label_smoothing", "pos_weight", "thresholds", "multilabel_smoothing")
    if not any(hasattr(args, n) for n in names):
        return False
    cw = getattr(args, "class_weights", None)
    if isinstance(cw, str):
        if cw != "balanced":
            raise ValueError(f"args.class_weights = {cw!r}: a sequence of weights or \"balanced\"")
        if train_dataset is None:
            raise ValueError("args.class_weights = \"balanced\" needs the training set's labels (train_dataset)")
        C = int(model.num_labels)
        cw = balanced_class_weights([int(train_dataset[i][3]) for i in range(len(train_dataset))], C)     # (an example's 4th field: its label)
    pw = getattr(args, "pos_weight", None)
    if isinstance(pw, str):
        if pw != "balanced":
            raise ValueError(f"args.pos_weight = {pw!r}: a sequence of weights or \"balanced\"")
        if train_dataset is None:
            raise ValueError("args.pos_weight = \"balanced\" needs the training set's labels (train_dataset)")
        pw = balanced_pos_weight(torch.stack([torch.as_tensor(train_dataset[i][3], dtype=torch.float32).reshape(-1) for i in range(len(train_dataset))]))
        pw = pw.clamp(min=torch.finfo(torch.float32).tiny)      # (a column without negatives: the smallest weight > 0)
    model.set_loss_options(regression=getattr(args, "label_loss", "mse"), huber_delta=getattr(args, "huber_delta", 1.0), class_weights=cw,
                           label_smoothing=getattr(args, "label_smoothing", 0.0), mlm_label_smoothing=getattr(args, "mlm_label_smoothing", 0.0),
                           pos_weight=pw, thresholds=getattr(args, "thresholds", None), multilabel_smoothing=getattr(args, "multilabel_smoothing", 0.0))
    return True


def apply_freeze(model, args):
    """``model.freeze`` from the optional ``args.freeze_embeddings`` (bool), ``args.freeze_layers`` (a count k for layers 0 .. k-1, or an
    iterable of layer indices) and ``args.freeze_layer_weights`` (bool: the dense weight matrices of the layers left trainable).
    ``default_args()`` has none of them: a model is then left exactly as it is (``requires_grad`` flags set by hand stay).  Call it before
    ``build_optimizer``, which leaves frozen parameters out of its groups.  Returns the names it froze."""
    names = ("freeze_embeddings", "freeze_layers", "freeze_layer_weights")
    if not any(hasattr(args, n) for n in names):
        return []
    return model.freeze(embeddings=bool(getattr(args, "freeze_embeddings", False)), layers=getattr(args, "freeze_layers", 0),
                        layer_weights=bool(getattr(args, "freeze_layer_weights", False)))


def apply_lora(model, args):
    """``model.add_lora`` from the optional ``args.lora_rank`` (4, 8 or 16), ``args.lora_alpha`` (default 2 x rank), ``args.lora_targets``
    (default query + value; any of query / key / value / attention_output / intermediate / ffn_output, or "all-linear"),
    ``args.lora_layers`` (default all), ``args.lora_freeze_base`` (default True), ``args.lora_seed`` and ``args.lora_dropout`` (default 0:
    the dropout of the adapters' input in train mode).
    ``default_args()`` has none of them: without ``lora_rank`` (or with None) nothing happens.  Call it before the optimizer is built
    (``build_optimizer`` does, for a model that has no adapters yet).  Returns whether adapters were added."""
    r = getattr(args, "lora_rank", None)
    if r is None:
        return False
    model.add_lora(r=r, alpha=getattr(args, "lora_alpha", None) or 2.0 * r, targets=getattr(args, "lora_targets", None) or ("query", "value"),
                   layers=getattr(args, "lora_layers", None), freeze_base=bool(getattr(args, "lora_freeze_base", True)),
                   seed=getattr(args, "lora_seed", None), dropout=getattr(args, "lora_dropout", None) or 0.0)
    return True


def build_optimizer(model, args, num_train_optimization_steps, mode="hf"):
    """REF:train.py:76-97: two parameter groups by NAME substring, AdamW, linear warm-up with
    warmup = N and total = warmup_proportion * N.
    ``args.layer_lr_decay`` / ``args.head_learning_rate`` (optional; not reference arguments, ``default_args()`` leaves them out): the
    groups of optim.layerwise_param_groups (layer-wise lr decay, a learning rate of its own for the parts a BERT checkpoint lacks).
    ``args.ema_decay`` / ``args.ema_warmup`` (optional, likewise): an exponential moving average of the weights, kept inside the
    optimizer step (``AdamW.ema``); ``train`` then validates, tests and saves under the averaged weights.
    Frozen parameters (``requires_grad == False``: apply_freeze, model.freeze) are in no group.
    ``args.lora_rank`` (optional, likewise): ``apply_lora`` runs first when the model has no adapters yet, so the groups hold them.
    ``args.optimizer = "lamb"`` (optional, likewise) with ``args.lamb_always_adapt`` / ``args.lamb_max_trust``: ``optim.LAMB`` over the
    same groups (``mode`` does not apply: LAMB has one definition)."""
    from .optim import AdamW, get_linear_schedule_with_warmup, layerwise_param_groups
    if not getattr(model, "_lora", None):
        apply_lora(model, args)
    layer_decay, head_lr = getattr(args, "layer_lr_decay", None), getattr(args, "head_learning_rate", None)
    if layer_decay is not None or head_lr is not None:
        groups = layerwise_param_groups(model, args.learning_rate, layer_decay=1.0 if layer_decay is None else layer_decay, head_lr=head_lr)
    else:
        no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        groups = [{"params": [p for n, p in named if not any(nd in n for nd in no_decay)], "weight_decay": 0.01},
                  {"params": [p for n, p in named if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]
    kind = getattr(args, "optimizer", None)                                  # (not a reference argument: absent = AdamW)
    if kind is None or kind == "adamw":
        opt = AdamW(groups, lr=args.learning_rate, mode=mode)
    elif kind == "lamb":
        from .optim import LAMB
        opt = LAMB(groups, lr=args.learning_rate, always_adapt=bool(getattr(args, "lamb_always_adapt", False)),
                   max_trust=getattr(args, "lamb_max_trust", None))
    else:
        raise ValueError(f"build_optimizer: args.optimizer must be 'adamw' or 'lamb', got {kind!r}")
    if getattr(args, "ema_decay", None) is not None:
        opt.ema(args.ema_decay, warmup=bool(getattr(args, "ema_warmup", False)))
    sched = get_linear_schedule_with_warmup(opt, num_warmup_steps=num_train_optimization_steps,
                                            num_training_steps=args.warmup_proportion * num_train_optimization_steps)
    return opt, sched


# ================================================================================================
# evaluation, metrics, epoch loop (REF:trainer.py:103-290)
# ================================================================================================
def eval_epoch(args, model, valdata, tokenizer=None, *, device="cuda", generator=None, batches=None):
    """REF:trainer.py:103-199.  The model in eval mode under ``no_grad``; MLM masking is applied at evaluation too
    when ``args.mlm`` (the reference does); shuffled order (RandomSampler) like the reference.  Returns its 8-tuple
    (dev_loss, text_loss, visual_loss, speech_loss, ap_loss, label_loss, preds, labels), every loss divided by the number
    of steps -- ``text/visual/speech_loss`` are 0 because the model returns ``None`` for them, and ``ap_loss`` is the LAST
    step's value divided by the number of steps (REF:trainer.py:199 divides the loop variable, not a sum)."""
    import numpy as np
    if batches is None:
        from torch.utils.data import DataLoader, RandomSampler
        loader = DataLoader(valdata, sampler=RandomSampler(valdata), batch_size=args.val_batch_size, collate_fn=collate)
        batches = (pack_step_inputs(b, args, device, generator) for b in loader)
    model.eval()
    dev_loss = torch.zeros((), device=device)
    label_loss = torch.zeros((), device=device)
    ap_loss = torch.zeros((), device=device)
    preds, labels = [], []
    n = 0
    with torch.no_grad():
        for kwargs in batches:
            outputs, logits = model(**kwargs)
            dev_loss += outputs[0].mean()
            label_loss += outputs[5].mean()
            ap_loss = outputs[4]
            preds.append(logits.detach().float() if logits.is_floating_point() else logits.detach())     # (a class head: int64 class ids)
            labels.append(kwargs["sentiment"].detach())
            n += 1
    if n == 0:
        return (0.0,) * 6 + (np.zeros((0,)), np.zeros((0,)))
    preds = torch.cat(preds).cpu().numpy()                          # one device->host transfer per epoch, not per step
    labels = torch.cat(labels).cpu().numpy()
    return (float(dev_loss) / n, 0.0, 0.0, 0.0, float(ap_loss) / n, float(label_loss) / n, preds, labels)


def pack_predict_inputs(batch, device):
    """The three arguments of ``model.predict`` from one ``collate`` batch: the utterance as it is (no MLM masking), no labels."""
    text_batch, visual_batch, speech_batch, attention_batch = batch[:4]
    dev = torch.device(device)
    return dict(
        input_ids=(text_batch[0].to(dev), visual_batch[1].to(dev), speech_batch[1].to(dev), visual_batch[0].to(dev), speech_batch[0].to(dev)),
        token_type_ids=(text_batch[2].to(dev), visual_batch[3].to(dev), speech_batch[3].to(dev)),
        attention_mask=(text_batch[3].to(dev), (attention_batch[0].to(dev), visual_batch[4].to(dev)),
                        (attention_batch[1].to(dev), speech_batch[4].to(dev))),
    )


def predict_epoch(args, model, data, *, device="cuda", batches=None, return_attention=None):
    """The label-free counterpart of ``eval_epoch`` (what the reference's ``sampling.py`` is for; that script does not run against its
    own model's signature): ``model.predict`` over ``data`` in SEQUENTIAL order -- row i of the result is item i of the dataset -- on the
    utterances as they are (no MLM masking: ``eval_epoch`` masks because the reference's evaluation does; a prediction does not).
    ``data``: a Dataset of the reference's 16-tuples (collated here, ``args.test_batch_size``, else ``args.val_batch_size``), or pass
    ``batches`` = an iterable of model-kwargs dicts (keys other than ``input_ids`` / ``token_type_ids`` / ``attention_mask``, such as
    labels, are ignored).  Returns the predictions as one float32 array [N, 1] -- from a model with a C-class head (``num_labels=C``
    / ``set_num_labels``) the predicted classes, one int64 array [N], with a multi-label head the decisions, int64 [N, C] --: one
    device->host transfer at the end.  Leaves
    ``model.training`` as it found it.

    ``return_attention`` = ``"top"`` | ``"all"`` (``model.predict``'s argument): returns ``(preds, dict)`` with ``attention`` and
    ``attention_mass`` as numpy arrays per pass, concatenated over the dataset on the sample axis (axis 1) in dataset order, and
    ``attention_layers``.  The maps go to the host batch by batch; every batch must have the same key widths (T, T + V, T + A), else
    ``ValueError``.  Host memory of ``"all"``: L * N * heads * S * 4 bytes per pass (12 layers, 12 heads, S = 550: 317 KB per sample and
    pass); ``"top"`` is 1 / L of it."""
    import numpy as np
    if return_attention is not None and return_attention is not False:
        return _predict_epoch_attention(args, model, data, device, batches, return_attention)
    if batches is None:
        from torch.utils.data import DataLoader, SequentialSampler
        bs = getattr(args, "test_batch_size", None) or args.val_batch_size
        loader = DataLoader(data, sampler=SequentialSampler(data), batch_size=bs, collate_fn=collate)
        batches = (pack_predict_inputs(b, device) for b in loader)
    preds = [model.predict(kw["input_ids"], kw["token_type_ids"], kw["attention_mask"]) for kw in batches]
    if not preds:
        from .model import _class_head, _multi_head
        if _multi_head(model):
            return np.zeros((0, _multi_head(model)), dtype=np.int64)
        return np.zeros((0,), dtype=np.int64) if _class_head(model) else np.zeros((0, 1), dtype=np.float32)
    preds = torch.cat(preds)
    return (preds.float() if preds.is_floating_point() else preds).cpu().numpy()


def _predict_epoch_attention(args, model, data, device, batches, return_attention):
    """``predict_epoch`` with the [CLS] attention maps (see there)."""
    import numpy as np
    if batches is None:
        from torch.utils.data import DataLoader, SequentialSampler
        bs = getattr(args, "test_batch_size", None) or args.val_batch_size
        loader = DataLoader(data, sampler=SequentialSampler(data), batch_size=bs, collate_fn=collate)
        batches = (pack_predict_inputs(b, device) for b in loader)
    preds, att, mass, layers = [], {}, {}, None
    for kw in batches:
        p, ex = model.predict(kw["input_ids"], kw["token_type_ids"], kw["attention_mask"], return_attention=return_attention)
        preds.append(p)
        layers = ex["attention_layers"]
        for store, key in ((att, "attention"), (mass, "attention_mass")):
            for n, v in ex[key].items():
                have = store.setdefault(n, [])
                if have and have[0].shape[-1] != v.shape[-1]:
                    raise ValueError(f"predict_epoch(return_attention=...): the {n} maps of two batches differ in their key width "
                                     f"({have[0].shape[-1]} and {v.shape[-1]}); pad the batches to one length")
                have.append(v.cpu().numpy())
    if not preds:
        from .model import _class_head
        empty = np.zeros((0,), dtype=np.int64) if _class_head(model) else np.zeros((0, 1), dtype=np.float32)
        return empty, dict(attention={}, attention_mass={}, attention_layers=[])
    preds = torch.cat(preds)
    preds = (preds.float() if preds.is_floating_point() else preds).cpu().numpy()
    cat = lambda d: {n: np.concatenate(v, axis=1) for n, v in d.items()}
    return preds, dict(attention=cat(att), attention_mass=cat(mass), attention_layers=list(layers))


def mlm_eval_epoch(args, model, data, tokenizer=None, *, device="cuda", generator=None, batches=None, top_k=5):
    """Masked-token quality per modality pass -- what ``eval_epoch`` cannot report (``forward`` returns ``None`` for the three MLM
    losses): ``model.predict_tokens`` over ``data`` in SEQUENTIAL order, the batches from ``pack_step_inputs`` (masked like
    ``eval_epoch``'s when ``args.mlm``; every position labelled with its own id when not, as the reference packs them), or pass
    ``batches`` = an iterable of model-kwargs dicts (``input_ids`` / ``token_type_ids`` / ``attention_mask`` / ``masked_labels``).
    Returns {"text" | "visual" | "speech": dict(count = labelled positions, loss = token-weighted mean negative log-likelihood over the
    epoch, perplexity = exp(loss), top1 / topk = share of positions whose label is the first / among the first ``top_k`` predictions,
    mrr = mean of 1 / (rank + 1))} -- ``loss`` is the PLAIN negative log-likelihood whatever ``model.mlm_label_smoothing`` is (smoothing shapes
    the training objective, not the reported likelihood); a pass without labelled positions (an empty dataset: every pass) gives zeros and count = 0.  The
    sums stay on the device: one device->host transfer at the end.  Leaves ``model.training`` as it found it."""
    import math
    names = ("text", "visual", "speech")
    if batches is None:
        from torch.utils.data import DataLoader, SequentialSampler
        loader = DataLoader(data, sampler=SequentialSampler(data), batch_size=args.val_batch_size, collate_fn=collate)
        batches = (pack_step_inputs(b, args, device, generator) for b in loader)
    k = int(top_k)
    acc = None                                                     # [3, 5] float64: count, sum of -log p, rank = 0, rank < k, sum of 1 / (rank + 1)
    for kw in batches:
        res = model.predict_tokens(kw["input_ids"], kw["token_type_ids"], kw["attention_mask"], masked_labels=kw["masked_labels"], top_k=k)
        rows = []
        for n in names:
            rank = res[n]["label_rank"].to(torch.float64)
            nll = -res[n]["label_logprob"].to(torch.float64)
            rows.append(torch.stack((rank.new_tensor(float(rank.numel())), nll.sum(), (rank == 0).sum().to(torch.float64),
                                     (rank < k).sum().to(torch.float64), (1.0 / (rank + 1.0)).sum())))
        rows = torch.stack(rows)
        acc = rows if acc is None else acc + rows
    out = {}
    host = None if acc is None else acc.cpu().tolist()
    for p, n in enumerate(names):
        cnt, nll, top1, topk, mrr = host[p] if host is not None else (0.0,) * 5
        if cnt == 0:
            out[n] = dict(count=0, loss=0.0, perplexity=0.0, top1=0.0, topk=0.0, mrr=0.0)
            continue
        loss = nll / cnt
        out[n] = dict(count=int(cnt), loss=loss, perplexity=math.exp(min(loss, 700.0)), top1=top1 / cnt, topk=topk / cnt, mrr=mrr / cnt)
    return out


def _weighted_f1(y_true, y_pred):
    """F1 per class weighted by the class's support in ``y_true`` (sklearn ``f1_score(average="weighted")``)."""
    import numpy as np
    y_true, y_pred = np.asarray(y_true).reshape(-1), np.asarray(y_pred).reshape(-1)
    total, score = y_true.size, 0.0
    for c in np.unique(np.concatenate((y_true, y_pred))):
        tp = float(np.sum((y_pred == c) & (y_true == c)))
        fp = float(np.sum((y_pred == c) & (y_true != c)))
        fn = float(np.sum((y_pred != c) & (y_true == c)))
        f1 = 2 * tp / (2 * tp + fp + fn) if (2 * tp + fp + fn) > 0 else 0.0
        score += f1 * float(np.sum(y_true == c)) / max(total, 1)
    return score


def test_CE_score_model(preds, y_test):
    """REF:trainer.py:201-215 (classification heads): (accuracy, mean absolute error, weighted F1) of class predictions."""
    import numpy as np
    preds, y_test = np.asarray(preds), np.asarray(y_test)
    mae = float(np.mean(np.absolute(preds - y_test)))
    return float(np.mean(preds.reshape(-1) == y_test.reshape(-1))), mae, _weighted_f1(y_test, preds)


def test_MSE_score_model(preds, y_test, use_zero=False):
    """REF:trainer.py:217-228 (regression heads, num_labels 1 / 7): MAE of the raw scores, then accuracy and weighted F1 of
    the sign (>= 0) -- note the broadcasting of the reference: ``preds`` is [N,1], ``y_test`` [N], so its MAE is the mean over
    the [N,N] difference table; kept (callers compare epochs with it), documented here."""
    import numpy as np
    preds, y_test = np.asarray(preds), np.asarray(y_test)
    mae = float(np.mean(np.absolute(preds - y_test)))
    p, y = (preds >= 0), (y_test >= 0)
    if p.ndim == 2 and y.ndim == 1:                                  # sklearn flattens a [N,1] prediction column
        p = p.reshape(-1)
    return float(np.mean(p == y)), mae, _weighted_f1(y, p)

def test_multilabel_score_model(preds, y_test):
    """Multi-label heads (decisions [N, C] against multi-hot targets [N, C]; entries with ``y_test < 0`` are left out, a target counts as
    positive above 0.5): per label and averaged over the labels, ``accuracy``, ``weighted_accuracy`` = (TPR + TNR) / 2 -- a rate over
    no entries counts 0 -- and ``f1`` (2 TP / (2 TP + FP + FN), 0 without positives on either side); ``mae`` = the mean |decision - target|
    over the annotated entries.  Returns dict(accuracy, weighted_accuracy, f1, mae: floats; per_label: dict of three [C] lists).  CMU-MOSEI's
    emotion protocol (weighted accuracy and F1 per emotion)."""
    import numpy as np
    preds, y = np.asarray(preds), np.asarray(y_test, dtype=np.float64)
    if preds.shape != y.shape or y.ndim != 2:
        raise ValueError(f"test_multilabel_score_model: decisions {preds.shape} against targets {y.shape}; both [N, C]")
    acc, wacc, f1 = [], [], []
    for c in range(y.shape[1]):
        v = y[:, c] >= 0
        p, t = preds[v, c] > 0, y[v, c] > 0.5
        tp, tn = float(np.sum(p & t)), float(np.sum(~p & ~t))
        fp, fn = float(np.sum(p & ~t)), float(np.sum(~p & t))
        n = tp + tn + fp + fn
        acc.append((tp + tn) / n if n else 0.0)
        wacc.append(((tp / (tp + fn) if tp + fn else 0.0) + (tn / (tn + fp) if tn + fp else 0.0)) / 2.0)
        f1.append(2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
    valid = y >= 0
    mae = float(np.mean(np.absolute(preds[valid] - y[valid]))) if valid.any() else 0.0
    mean = lambda x: float(np.mean(x)) if len(x) else 0.0
    return dict(accuracy=mean(acc), weighted_accuracy=mean(wacc), f1=mean(f1), mae=mae, per_label=dict(accuracy=acc, weighted_accuracy=wacc, f1=f1))


test_multilabel_score_model.__test__ = False
test_CE_score_model.__test__ = False                                # names start with "test_": not pytest cases
test_MSE_score_model.__test__ = False


def _dated_dir(path):
    """``path/<YYYYMMDD>-NN`` with the first unused NN, created: where train() below saves (the reference's directory naming, REF:utils.py:35-50;
    the reference's logging / path utilities themselves are out of scope)."""
    import datetime
    import os
    os.makedirs(path, exist_ok=True)
    stamp = datetime.datetime.now().strftime("%Y%m%d")
    i = 0
    while os.path.exists(os.path.join(path, f"{stamp}-{i:02d}")):
        i += 1
    out = os.path.join(path, f"{stamp}-{i:02d}")
    os.mkdir(out)
    return out


def train(args, model, train_dataset, val_dataset, test_dataset, optimizer, scheduler, tokenizer=None, logger=None, *, device="cuda",
          dp=None, save_root="./model_save", numpy_root="./numpy_save", patience_limit=25, epoch_batches=None):
    """REF:trainer.py:230-290: per epoch train -> validate -> test; the state dict is saved (``model_<epoch>.pt``, the
    reference's checkpoint format = its state-dict keys) whenever the TEST accuracy improves; after ``patience_limit`` epochs
    without improvement the best predictions / targets go to ``predict.npy`` / ``target.npy`` and the loop stops.
    ``epoch_batches``: optional callable ``(split, epoch) -> iterable of model kwargs`` replacing the datasets (synthetic data).
    ``args.max_grad_norm``, when present, reaches every epoch's train_epoch (global-norm clipping).
    ``args.label_loss`` / ``huber_delta`` / ``class_weights`` / ``label_smoothing`` / ``mlm_label_smoothing``, when present, are set on the
    model first (apply_loss_options); ``args.freeze_embeddings`` / ``freeze_layers`` / ``freeze_layer_weights`` likewise (apply_freeze).  A multi-label model is scored by ``test_multilabel_score_model``: "acc" is then the mean weighted
    accuracy over the labels, "f_score" the mean F1.
    An optimizer with a weight EMA (``AdamW.ema``; ``args.ema_decay`` through build_optimizer): each epoch's validation, test and saved
    state dict use the averaged weights (``optimizer.ema_weights()``); training goes on from the trained ones.
    Returns a dict with the best epoch's numbers and the per-epoch history."""
    import os
    import numpy as np
    log = logger.info if logger is not None else (lambda *a, **k: None)
    apply_loss_options(model, args, train_dataset)
    apply_freeze(model, args)
    save_dir = _dated_dir(save_root)
    log("Model save path: {}".format(save_dir))
    score = test_MSE_score_model if getattr(args, "num_labels", 7) in (1, 7) else test_CE_score_model
    if getattr(model, "multi_label", False):                          # the model-selection number: the mean weighted accuracy
        def score(preds, y):
            r = test_multilabel_score_model(preds, y)
            return r["weighted_accuracy"], r["mae"], r["f1"]
    best = dict(epoch=-1, acc=0.0, loss=float("inf"), mae=None, f_score=None, preds=None, labels=None, path=None)
    history = []
    patience = 0
    rank0 = dp is None or torch.distributed.get_rank() == 0
    for epoch in range(int(args.n_epochs)):
        patience += 1
        tb = epoch_batches("train", epoch) if epoch_batches else None
        tr = train_epoch(args, model, train_dataset, optimizer, scheduler, tokenizer, device=device, dp=dp, batches=tb)
        log("[Train Epoch {}] Joint Loss : {} AP Loss : {} Label Loss : {}".format(epoch + 1, tr[0], tr[4], tr[5]))
        # (an optimizer with a weight EMA: the epoch is judged and saved under the averaged weights, swapped out again before the next epoch)
        averaged = optimizer.ema_weights() if getattr(optimizer, "_ema_decay", None) is not None else _null()
        with averaged:
            va = eval_epoch(args, model, val_dataset, tokenizer, device=device, batches=epoch_batches("val", epoch) if epoch_batches else None)
            log("[Val Epoch {}] Joint Loss : {} AP Loss : {} Label Loss : {}".format(epoch + 1, va[0], va[4], va[5]))
            te = eval_epoch(args, model, test_dataset, tokenizer, device=device, batches=epoch_batches("test", epoch) if epoch_batches else None)
            acc, mae, f_score = score(te[6], te[7])
            if dp is not None and torch.distributed.get_world_size() > 1:
                # ranks evaluate with their own sampler order and MLM draws, so their metrics can differ in the last digits: rank 0's
                # numbers decide the save rule and the patience stop on EVERY rank (a rank that stopped alone would leave the
                # others waiting in the next epoch's gradient all-reduce)
                t = torch.tensor([acc, mae, f_score], dtype=torch.float64, device=device)
                torch.distributed.broadcast(t, src=0)
                acc, mae, f_score = (float(x) for x in t.tolist())
            log("[Epoch {}] Test_ACC : {}, Test_MAE : {}, Test_F_Score: {}".format(epoch + 1, acc, mae, f_score))
            history.append(dict(epoch=epoch + 1, train_loss=tr[0], valid_loss=va[0], test_acc=acc, test_mae=mae, test_f_score=f_score))
            if acc > best["acc"]:
                path = os.path.join(save_dir, "model_" + str(epoch + 1) + ".pt")
                if rank0:
                    torch.save(model.state_dict(), path)
                    if getattr(model, "_lora", None):                # ... and the small per-task adapter file beside it
                        torch.save(model.lora_state_dict(), os.path.join(save_dir, "lora_" + str(epoch + 1) + ".pt"))
                best.update(epoch=epoch, acc=acc, loss=va[0], mae=mae, f_score=f_score, preds=te[6], labels=te[7], path=path if rank0 else None)
                patience = 0
        if patience == patience_limit:
            if rank0 and best["preds"] is not None:
                out = _dated_dir(numpy_root)
                np.save(os.path.join(out, "predict.npy"), best["preds"])
                np.save(os.path.join(out, "target.npy"), best["labels"])
            break
    log("[Best Epoch {}] Best_ACC : {}, Best_MAE : {}, Best_F_Score: {}".format(best["epoch"] + 1, best["acc"], best["mae"], best["f_score"]))
    best["history"] = history
    best["save_dir"] = save_dir
    return best
