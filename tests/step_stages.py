"""Every launch of a real training step, recorded and recomputed in float64 from its own recorded operands.

Not a test module (pytest does not collect it): ``from tests import step_stages as SS``.  Importing it needs no GPU.

``record(model)`` wraps the ``msa_amd.ops`` entry points a training step goes through (``SPIED``, plus ``LnDeferred.flush``: the deferred
LayerNorm reduce) and restores them on exit.  While they are wrapped the model takes its per-launch path (``ops.launches_unwrapped()`` is
false); the composite layer calls are bit-identical to it (tests/test_model_gpu.py::test_composite_layer_calls_are_bit_identical).  For
every call a ``Call`` keeps: the op name, a clone of every tensor operand taken BEFORE the call on the stream the call is issued on
(``a``: the bound arguments by name; layouts, row inverses and the deferred collector as small snapshots), every non-tensor keyword, a
clone AFTER the call of every operand the op writes (``post``: output buffers handed in, accumulated gradients) and clones of what it
returns (``ret``).  The recorder keeps the original tensors alive until it exits, so an address is never handed out twice while it
records: a storage address identifies a buffer.  It changes nothing else -- the step's results are bit-identical with and without it.

``recompute(call)`` maps the recorded operands and keywords of one call onto the float64 reference of that op and judges the recorded
outputs by THAT reference's ``check`` -- no tolerance of its own:

    gemm_nt (bias, gelu + aux, resid, dropout, gelu_bwd_u, fp32 out)   gemm_ref.nt          gemm_nt_splitk          gemm_ref.splitk
    gemm_tn / gemm_tn_grouped (W0, bias sums, per-problem flags)       gemm_ref.tn / tn_grouped
    attn_fwd / attn_bwd (packed layouts, kv_len, q_limit, dropout)     attention_ref.reference
    ln_fwd / ln_bwd (row maps, both dropouts, dx2)                     rowwise_ref.ln_fwd / ln_bwd
    ln_bwd_reduce (LnDeferred.flush)                                   the float64 sum of its calls' rowwise_ref.ln_bwd sums
    ce_fwd / ce_bwd                                                    rowwise_ref.ce_fwd / ce_bwd
    embed_gather / embed_scatter / pair_proj_fwd / pair_proj_bwd       embed_ref.gather / scatter / pair_fwd / pair_bwd
    gather_rows / scatter_rows_zero / attn_q_limit                     exact (layout_ref.scatter_ref for the stamped inverse)
    gelu_bwd                                                           ``gelu_bwd_ref`` below
    lora_qkv_fwd / lora_qkv_bwd (dict operands, h row slices, dres=None) lora_ref.fwd / bwd, judged by lora_ref.check
    lora_dense_fwd / lora_dense_bwd (ADD with the GEMM's triple, GELU + aux,   lora_dense_ref.fwd / bwd, judged by lora_dense_ref.check
        dx in place, gelu_u, h row slices, h=None on gathered rows)
    colsum_grouped (per-problem accumulate flags)                      colsum_ref: M 2^-24 sum|x| + 2^-23 |ref|

Dropout keep masks are rebuilt from the (stream, thr16, scale) triple recorded IN the call, through ``ops.dropout_mask`` /
``ops.attn_dropout_mask`` on a GPU and through their exact CPU references (tests/layout_ref.py) without one.  An adapter that cannot
express a keyword raises: an unrecomputed launch is a failure, never a skip.

``gelu_bwd_ref``: du = bf16(dy * gelu'(u)) on bf16 operands -- gemm_ref's GELU' epilogue with the accumulator replaced by the exact bf16
``dy``: val = dy * gelu'(u), one fp32 product (acc = |gelu'(u)| |dy|, times C_ACC 2^-24), the erf approximation GELUP_ABS |dy| and the
bf16 rounding of the output; judged by ``gemm_ref.check``.  Its emulation (fp32 product, bf16 rounding) reaches 0.5 of the bound
(tests/test_step_stages_reference_cpu.py).

``check_dataflow(calls, model)`` checks the wiring with exact comparisons only:

 1. the trunk's op sequence is the table below for the flags in force (``FWD_LAYER`` per layer and forward pass; per backward pass and
    layer, top down, ``BWD_DENSE`` or one of ``BWD_TOP_SPARSE``);
 2. every operand a call reads is bit-equal to what the last writer of those addresses left there (a shadow copy of every storage the
    recorded calls wrote, replayed in issue order): forward chains, every saved activation backward reads, accumulated gradients --
    in-place reuse, aliasing and a read that overtook its producer on another stream all show here;
 3. each backward stage reads the residual, the GELU' operand, the LayerNorm statistics and the attention operands of the SAME layer's
    forward stage, each forward stage its predecessor's output, each weight-gradient problem its two stages (``_wiring``); the row lists
    of the sparse top layer agree with each other; ``kv_len`` is the count the recorded key bias implies;
 4. every ``W*T`` operand is the transpose of the bf16 working copy the forward read, and that copy is the parameter rounded to bf16;
 5. forward and backward of a dropout site carry the same triple, two different sites different streams;
 6. every gradient buffer a stage wrote is the view named for that stage, at the address of the parameter's ``.grad``;
 7. ``check_dense_adapter_wiring``: every dense-seam adapter launch against its neighbours -- forward, its ``x`` / ``y`` are the ``A`` operand
    and the output of the GEMM directly in front, which carried the residual and the SAME dropout triple (ADD mode) or neither GELU nor
    ``aux`` (GELU mode: the adapter's ``aux`` is what the layer's ``du`` stage reads as ``gelu_bwd_u``); backward, ``dx`` / ``dy`` / ``gelu_u``
    are the output, the ``A`` operand and the ``gelu_bwd_u`` of the GEMM directly in front, ``x`` the layer's forward activation, ``h`` a
    leading-row view of the forward adapter's ``h_out`` (None exactly on gathered rows), ``accumulate is True`` and ``gA`` / ``gB`` the
    ``.grad`` views of the adapter's parameters.  (Check 5 counts an ADD-mode adapter launch to its GEMM's site: ``lora_z1`` -> ``z1``,
    ``lora_z2`` -> ``z2``; recomputing the launch from its own recorded triple would pass with any triple.)

A step under a freeze.TrainablePlan and / or with adapters is judged by ``check_dataflow_frozen``: the frozen form of check 1 (forward all
L layers, backward L-1 .. ``stop``, no ``dx`` stage where backward ends without an embedding stage, ``lora_fwd`` directly behind ``qkv`` and
``lora_bwd`` directly behind ``attn_bwd`` on adapter layers, the dense targets' stages ``lora_z1`` / ``lora_g`` / ``lora_z2`` directly behind
``z1`` / ``g`` / ``z2`` and ``lora_du`` / ``lora_dy1`` / ``lora_dctx`` directly behind ``du`` / ``dy1`` / ``dctx``), checks 2, 4, 5, 7 and ``kv_len``
unchanged, and one more exact check,
``check_frozen_writes``: no recorded call writes into the part of the flat gradient buffer that belongs to a frozen parameter, and the
weight-gradient problems written are exactly the weights whose mode is "full", the MLM transform and -- iff ``word_table`` -- the tied
table.  Checks 3 and 6 (``_wiring``, ``check_grad_views``) assume a full backward and are not extended to it.

The seam between the last encoder LayerNorm of the forward pass and the first launch of the encoder's backward is recorded too.  The
level-launch heads take addresses in a ``_HeadsStepMl`` record: model._HeadsStepFn hangs its operand tuples onto the record as plain
attributes (no launch, no argument changes), ``_HeadsStepFn.tensors(a)`` makes {field: tensor} of them and the recorder clones those -- before the call on the stream it is
issued on (the side stream for the prelaunched and the backward levels), after it what the levels write -- with the record's scalar
fields (``HEAD_SCALARS``, ``lo``, ``hi``).  A frozen head parameter's gradient view (computed and dropped: model._gv) is left out of what
the call wrote.  The prologue's ``ret`` holds its named views and every word of the ``prologue_sizes`` extent of both buffers.

    heads_step_fwd (judged once level 7 has run) / heads_step_dmlm /     heads_ref, heads_cls_ref (``ncls``), heads_multilabel_ref (``multi_label``),
        heads_step_bwd (``heads_case``: first = the recorded rows            loss_options_ref (an option on): that reference's ``expected`` /
        ``first_rows`` of ``y``, the recorded parameters, prior = the        ``check_all``; ``pred`` exactly
        gradient views as the backward call found them)
    prologue (both ``rowset`` settings, every output word)               layout_ref.prologue_ref, exact
    active_rows / compact_rows / pack_i64                                layout_ref.active_rows_ref / compact_ref / pack_ref, exact

The heads' references hold where fp32 and float64 take the same side of every kink (``heads_expected``): the ratios reached are kept in
``call.meta["precondition"]`` and ``preconditions(calls)`` asserts them.

 8. ``check_seam`` (its docstring names every check): the heads' ``y`` / ``first_rows`` against the top layer's ``ln2`` and the layout, what
    levels 1 - 6 wrote against what level 7 found, ``mlm`` against ``ce_fwd``'s losses, ``ce_bwd``'s ``gscale`` against ``heads_step_dmlm``, the
    row list handed to ``compact_rows``, the heads' 22 gradient operands against the parameters' ``.grad``, every attention call's key
    bias / ``kv_len`` and the MLM head's row list against the step's prologue, alternating prologue buffer sets -- and the [CLS] rows of
    the output gradient the top layer's backward reads, written by an unrecorded ATen copy / ``index_add_``: ``check_seam`` states what the
    whole matrix must hold (compact: the last MLM product's rows, then the RNE bf16 of the recorded ``dfirst``; dense: torch's bf16
    ``index_add_`` onto what the MLM head left) and ``check_producers`` compares every row with it.  Part of ``check_dataflow`` and
    ``check_dataflow_frozen`` (where ``check_frozen_writes`` sees the heads' writes like any other).

Still not covered: the 19-launch and the eager heads (``coop_heads = False``: no recorded ``dfirst``, the [CLS] rows of the dense output
gradient may then differ from the shadow, no other row), ``forward_fused``, the optimizer launches, ``predict*``'s heads (``heads_predict``).
"""
from __future__ import annotations

import contextlib
import inspect
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from tests import attention_ref as A
from tests import colsum_ref as CS
from tests import embed_ref as E
from tests import gemm_ref as G
from tests import layout_ref as LR
from tests import lora_dense_ref as DR
from tests import lora_ref as LO
from tests import rowwise_ref as R

SPIED = ("gemm_nt", "gemm_nt_splitk", "gemm_tn", "gemm_tn_grouped", "attn_fwd", "attn_bwd", "attn_q_limit", "ln_fwd", "ln_bwd", "gelu_bwd",
         "embed_gather", "embed_scatter", "pair_proj_fwd", "pair_proj_bwd", "ce_fwd", "ce_bwd", "gather_rows", "scatter_rows_zero",
         "lora_qkv_fwd", "lora_qkv_bwd", "lora_dense_fwd", "lora_dense_bwd", "colsum_grouped",
         "prologue", "active_rows", "compact_rows", "pack_i64")
# the level-launch heads: their operands are addresses in a ``_HeadsStepMl`` record; model._HeadsStepFn.tensors(a) gives the tensors behind
# them (field name -> tensor), which is what ``heads_spy`` clones
HEADS = ("heads_step_fwd", "heads_step_bwd", "heads_step_dmlm")
HEAD_SCALARS = ("B", "H", "tanh_lo", "ncls", "nmlm", "alpha", "beta", "ldy", "loss_kind", "huber_delta", "label_smoothing", "multi_label")
# record field -> parameter name (heads_ref.PARAMS / FWD_ONLY); its gradient view is the field "g" + name
HEAD_PARAM = {"Wp": "bert.pooler.dense.weight", "bp": "bert.pooler.dense.bias", "Wal": "cls.align.weight", "bal": "cls.align.bias",
              "Wsr": "cls.seq_relationship.weight", "bsr": "cls.seq_relationship.bias", "Wat": "attn.weight", "bat": "attn.bias",
              "Wc1": "classifier1_1.weight", "bc1": "classifier1_1.bias", "Wc2": "classifier1_2.weight", "bc2": "classifier1_2.bias"}
for _m, (_g, _q) in enumerate(zip(("vt", "vv", "vs"), ("cpc_zt.net", "cpc_zv.net", "cpc_za.net"))):
    HEAD_PARAM.update({f"vw{_m}": _g + ".weight", f"vb{_m}": _g + ".bias", f"Wq{_m}": _q + ".weight", f"bq{_m}": _q + ".bias"})
HEAD_GRADS = {"g" + k: v for k, v in HEAD_PARAM.items() if k not in ("Wsr", "bsr")}
HEAD_FWD_FINAL = ("logits", "t_rel", "rel")                     # final after levels 1 - 6 (with the workspace's P / T views)
HEAD_FWD_OUT = HEAD_FWD_FINAL + ("ws", "pred", "loss", "aux", "out5")
# operands an op writes (cloned again after the call); ACCUMULATES: of those, the ones whose previous value the op reads
WRITES = {"gemm_nt": ("out", "aux"), "gemm_nt_splitk": ("out",), "gemm_tn": ("W", "bias_out"), "gemm_tn_grouped": ("problems",),
          "attn_fwd": ("ctx", "lse"), "attn_bwd": ("dqkv",), "ln_fwd": ("out", "stats"), "ln_bwd": ("dx", "dx2", "dgamma", "dbeta", "dbias2"),
          "gelu_bwd": ("du",), "embed_gather": ("out",), "embed_scatter": ("gword", "gtype", "gpos"), "pair_proj_fwd": ("out",),
          "pair_proj_bwd": ("dW", "db"), "ce_bwd": ("dlogits",), "lora_qkv_fwd": ("qkv", "h_out"), "lora_qkv_bwd": ("gA", "gB"),
          "lora_dense_fwd": ("y", "aux", "h_out"), "lora_dense_bwd": ("dx", "gA", "gB"), "colsum_grouped": ("problems",),
          "prologue": ("bufs",), "heads_step_fwd": HEAD_FWD_OUT, "heads_step_dmlm": ("dmlm",),
          "heads_step_bwd": ("dfirst", "dmlm", "ws") + tuple(HEAD_GRADS)}
ACCUMULATES = {"gemm_tn": ("bias_out",), "embed_scatter": ("gword", "gtype", "gpos"), "pair_proj_bwd": ("dW", "db"), "pair_proj_fwd": ("out",),
               "ln_fwd": ("out",),          # (the last two write some rows of a larger matrix: the others keep their values)
               "lora_qkv_fwd": ("qkv",), "lora_qkv_bwd": ("gA", "gB"),    # (colsum_grouped: per problem, like gemm_tn_grouped)
               "lora_dense_fwd": ("y",), "lora_dense_bwd": ("dx", "gA", "gB"),    # (gA / gB of both adapter backwards: when ``accumulate``)
               "heads_step_bwd": tuple(HEAD_GRADS) + ("ws",),   # (ws: backward reads what the forward levels left in the workspace)
               "prologue": ("bufs",)}                            # (the persistent sets are larger than one step's extent)

# ---- the op sequence of the trunk (check 1): stage names, see ``_stage``
FWD_LAYER = ("qkv", "attn_fwd", "z1", "ln1", "g", "z2", "ln2")            # model._EncoderFn._layer_forward (z1 .. ln2: _forward_behind_attention)
BWD_DENSE = ("ln2_bwd", "du", "dy1", "ln1_bwd", "dctx", "attn_bwd", "dx")  # ... _layer_backward (ln2_bwd .. dctx: _backward_before_attention)
BWD_TOP_SPARSE = (                                                        # ... _last_layer_sparse (the same body on the gathered rows)
    ("gather_rows8", "ln2_bwd", "du", "dy1", "ln1_bwd", "dctx", "scatter_rows_zero", "attn_q_limit", "attn_bwd", "dx"),    # compact hand-over
    ("gather_rows1", "gather_rows8", "ln2_bwd", "du", "dy1", "ln1_bwd", "dctx", "attn_q_limit", "attn_bwd", "dx"))         # dense dy, gathered
# (gather_rows<n>: n tensors gathered in the launch -- 8 saved activations of the top layer, 1 = the output gradient; the MLM head's own
# gather of 6 is not part of the trunk)
_NT_STAGE = {"Wqkv": "qkv", "Wo": "z1", "W1": "g", "W2": "z2", "W2T": "du", "W1T": "dy1", "WoT": "dctx", "WqkvT": "dx",
             "Wt": "mlm_t0", "word_h": "logits", "wordT": "mlm_dt", "WtT": "mlm_dy"}
# the dense-seam adapter launches: target -> stage (forward: directly behind the GEMM stage z1 / g / z2, backward: behind du / dy1 / dctx)
DENSE_FWD_STAGE = {"attention_output": "lora_z1", "intermediate": "lora_g", "ffn_output": "lora_z2"}
DENSE_BWD_STAGE = {"ffn_output": "lora_du", "intermediate": "lora_dy1", "attention_output": "lora_dctx"}
_QKV_TARGETS = ("query", "key", "value")
_LN_STAGE = {"ln1_g": "ln1", "ln2_g": "ln2", "emb_ln_g": "emb_ln", "joint_ln_g": "joint_ln", "mlm_ln_g": "mlm_ln"}
_TRANSPOSED = {"W2T": "W2", "W1T": "W1", "WoT": "Wo", "WqkvT": "Wqkv", "WtT": "Wt", "wordT": "word_h"}
_PARAM_OF = {"Wqkv": "attention.self.query.weight", "Wo": "attention.output.dense.weight", "W1": "intermediate.dense.weight",
             "W2": "output.dense.weight", "bqkv": "attention.self.query.bias", "bo": "attention.output.dense.bias",
             "b1": "intermediate.dense.bias", "b2": "output.dense.bias", "ln1_g": "attention.output.LayerNorm.weight",
             "ln1_b": "attention.output.LayerNorm.bias", "ln2_g": "output.LayerNorm.weight", "ln2_b": "output.LayerNorm.bias"}
_PARAM_OF_W = {"word_pad": "bert.embeddings.word_embeddings.weight", "word": "bert.embeddings.word_embeddings.weight",
               "type": "bert.embeddings.token_type_embeddings.weight", "pos": "bert.embeddings.position_embeddings.weight",
               "emb_ln_g": "bert.embeddings.LayerNorm.weight", "emb_ln_b": "bert.embeddings.LayerNorm.bias",
               "joint_ln_g": "bert.jointEmbeddings.LayerNorm.weight", "joint_ln_b": "bert.jointEmbeddings.LayerNorm.bias",
               "Wv_w": "bert.jointEmbeddings.Wv.weight", "Wv_b": "bert.jointEmbeddings.Wv.bias", "Ws_w": "bert.jointEmbeddings.Ws.weight",
               "Ws_b": "bert.jointEmbeddings.Ws.bias", "pred_bias": "cls.predictions.bias", "bt": "cls.predictions.transform.dense.bias",
               "mlm_ln_g": "cls.predictions.transform.LayerNorm.weight", "mlm_ln_b": "cls.predictions.transform.LayerNorm.bias",
               "Wt": "cls.predictions.transform.dense.weight"}


# ------------------------------------------------------------------------------------------------ recorded values
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class Rec:
    """A recorded tensor: a clone (``t``, on the tensor's device; ``cpu()`` caches the host copy) and where the original lived --
    storage address and size, offset, shape, strides."""
    __slots__ = ("t", "_cpu", "live", "sptr", "sbytes", "off", "shape", "stride", "dtype", "ptr")

    def __init__(self, t, hold=True):
        self.t = t.detach().clone()
        self._cpu = None
        self.live = t if hold else None
        st = t.untyped_storage()
        self.sptr, self.sbytes, self.off = st.data_ptr(), st.nbytes(), t.storage_offset()
        self.shape, self.stride, self.dtype, self.ptr = tuple(t.shape), tuple(t.stride()), t.dtype, t.data_ptr()

    def cpu(self):
        if self._cpu is None:
            self._cpu = self.t.cpu()
        return self._cpu

    def region(self):
        """What identifies the buffer a row-matrix lives in, whatever number of leading rows a view of it has."""
        return (self.ptr, self.stride, self.shape[1:], self.dtype)


@dataclass
class LayoutSnap:
    lens: list
    heads: int
    split: bool
    dropped: bool
    elem_base: list
    bias_start: object
    seq_start: object
    kv_len: object = None
    inv: object = None


@dataclass
class Call:
    op: str
    a: dict
    post: dict = field(default_factory=dict)
    ret: object = None
    meta: dict = field(default_factory=dict)
    index: int = -1


def _c(x):
    """Host value of a recorded tensor / plain tensor / None."""
    if x is None:
        return None
    return x.cpu() if isinstance(x, Rec) else x.detach().cpu() if torch.is_tensor(x) else x


def _snap(v, hold=True):
    if torch.is_tensor(v):
        return Rec(v, hold)
    if isinstance(v, (list, tuple)):
        return type(v)(_snap(x, hold) for x in v)
    if type(v) is dict:                                          # (the adapters' {target: tensor} operands)
        return {k: _snap(x, hold) for k, x in v.items()}
    if hasattr(v, "lens") and hasattr(v, "heads") and hasattr(v, "seq_start"):
        base = getattr(v, "base", v)
        split = bool(getattr(v, "split", False))
        return LayoutSnap(list(v.lens), int(v.heads), split, bool(getattr(v, "dropped", False)), list(base.elem_base_host),
                          _snap(base.bias_start, False), _snap(v.seq_start, False), _snap(v.kv_len, False) if split else None,
                          _snap(v.inv, False) if split else None)
    if hasattr(v, "table") and hasattr(v, "stamp"):
        return dict(table=_snap(v.table, False), stamp=int(v.stamp), nlist=int(v.nlist))
    if hasattr(v, "flush") and hasattr(v, "items"):
        return "deferred"
    return v


def _snap_prologue(pro, args):
    """What ``ops.prologue`` returned, as Recs: its named views and the WHOLE ``prologue_sizes`` extent of both buffers (``all_f`` /
    ``all_i``: every output word, the sequence counts between ``valid`` and ``idx`` included)."""
    from msa_amd import ops
    lens, B, rowset = list(args["pass_lens"]), int(args["B"]), bool(args["rowset"])
    bias_len, _ni = ops.prologue_sizes(lens, B)
    nf, ni = ops.prologue_sizes(lens, B, rowset)
    kb = pro.key_bias
    all_f = torch.as_strided(kb, (nf,), (1,), kb.storage_offset() - (bias_len if rowset else 0))
    all_i = torch.as_strided(pro.kv_len, (ni,), (1,), pro.kv_len.storage_offset())
    out = {k: _snap(getattr(pro, k)) for k in ("key_bias", "kv_len", "valid", "idx", "words") + (("rank",) if rowset else ())}
    out.update(all_f=_snap(all_f), all_i=_snap(all_i))
    return out


def _recs(v):
    if isinstance(v, Rec):
        yield v
    elif isinstance(v, (list, tuple)):
        for x in v:
            yield from _recs(x)
    elif type(v) is dict:
        for x in v.values():
            yield from _recs(x)


def synth(op, a, ret=None, post=None, meta=None):
    """A Call built from live tensors (the CPU chain of tests/test_step_stages_reference_cpu.py): ``a`` as the op was handed it, ``post``
    / ``ret`` as it left them."""
    return Call(op, {k: _snap(v) for k, v in a.items()}, {k: _snap(v) for k, v in (post or {}).items()}, _snap(ret), dict(meta or {}))


# ------------------------------------------------------------------------------------------------ the recorder
@contextlib.contextmanager
def record(model=None):
    """Wraps the spied ``msa_amd.ops`` entry points; yields the list the calls are appended to (complete when the block exits: it
    synchronises, indexes the calls and lets go of the original tensors)."""
    from msa_amd import ops
    calls, orig, by_ptr, by_ws = [], {}, {}, {}

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def spy(*args, **kw):
            b = sig.bind(*args, **kw)
            b.apply_defaults()
            call = Call(name, {k: _snap(v) for k, v in b.arguments.items()})
            call.meta["stream"] = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0
            call.meta["det"] = bool(ops.deterministic()) if name == "embed_scatter" else None
            out = fn(*args, **kw)
            call.ret = _snap_prologue(out, b.arguments) if name == "prologue" else _snap(out)
            for k in WRITES.get(name, ()):
                if b.arguments.get(k) is not None and not isinstance(b.arguments[k], bool):
                    call.post[k] = _snap(b.arguments[k])
            if name == "ln_bwd":
                for k in ("dgamma", "dbeta"):
                    by_ptr[b.arguments[k].data_ptr()] = b.arguments[k]
                d = b.arguments.get("deferred")
                if d is not None:
                    by_ws[d.items[-1][0]] = call
            calls.append(call)
            return out
        return spy

    flush0 = ops.LnDeferred.flush

    def flush(self):
        items = list(self.items)
        if not items:
            return flush0(self)
        targets = [(by_ptr[it[1]], by_ptr[it[2]]) for it in items]
        call = Call("ln_bwd_reduce", dict(pre=[(_snap(g), _snap(b)) for g, b in targets], H=self.H))
        call.meta["calls"] = [by_ws[it[0]] for it in items]
        call.meta["stream"] = torch.cuda.current_stream().cuda_stream
        out = flush0(self)
        call.post["grads"] = [(_snap(g), _snap(b)) for g, b in targets]
        calls.append(call)
        return out

    def heads_spy(name, fn):
        def spy(a, lo=1, hi=7 if name == "heads_step_fwd" else 6):
            from msa_amd.model import _HeadsStepFn
            tens = _HeadsStepFn.tensors(a)                       # (raises on a record no train step of the model made)
            call = Call(name, {k: _snap(v) for k, v in tens.items()})
            call.a.update({k: getattr(a, k) for k in HEAD_SCALARS}, lo=lo, hi=hi)
            call.meta["stream"] = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0
            call.meta["record"] = id(a)
            # a frozen parameter's gradient is computed into its span of the flat buffer and dropped (model._gv): nothing reads it
            call.meta["dropped"] = sorted(g for g in HEAD_GRADS if g in tens and not tens[g[1:]].requires_grad)
            out = fn(a) if name == "heads_step_dmlm" else fn(a, lo, hi)
            writes = [k for k in WRITES[name] if k in tens and k not in call.meta["dropped"]]
            if name == "heads_step_fwd" and hi < 7:
                writes = [k for k in writes if k not in ("loss", "aux", "out5")]
            for k in writes:
                call.post[k] = _snap(tens[k])
            keep.append(a)
            calls.append(call)
            return out
        return spy

    keep = []
    for n in SPIED:
        orig[n] = getattr(ops, n)
        setattr(ops, n, wrap(n, orig[n]))
    for n in HEADS:
        orig[n] = getattr(ops, n)
        setattr(ops, n, heads_spy(n, orig[n]))
    ops.LnDeferred.flush = flush
    try:
        yield calls
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    finally:
        for n, f in orig.items():
            setattr(ops, n, f)
        ops.LnDeferred.flush = flush0
        for i, c in enumerate(calls):
            c.index = i
            for r in list(_recs(list(c.a.values()))) + list(_recs(list(c.post.values()))) + list(_recs(c.ret)):
                r.live = None


# ------------------------------------------------------------------------------------------------ dropout masks
def _on_gpu():
    return torch.cuda.is_available()


def flat_mask(n, drop):
    """The keep mask of elements 0 .. n-1 of a dropout site, from the triple the call carried."""
    if _on_gpu():
        from msa_amd import ops
        return ops.dropout_mask(int(n), tuple(drop), "cuda").cpu()
    return torch.from_numpy(LR.dropout_mask_ref(int(n), int(drop[0]), int(drop[1])))


def attn_masks(lay: LayoutSnap, drop):
    if not drop or not drop[1]:
        return None
    out = []
    for s, S in enumerate(lay.lens):
        if _on_gpu():
            from msa_amd import ops
            m = torch.stack([ops.attn_dropout_mask(S, lay.elem_base[s], h, tuple(drop), "cuda") for h in range(lay.heads)]).cpu()
        else:
            m = torch.from_numpy(np.stack([LR.attn_dropout_mask_ref(S, lay.elem_base[s], h, int(drop[0]), int(drop[1])) for h in range(lay.heads)]))
        out.append(m)
    return out


def _on(drop):
    return bool(drop) and bool(drop[1])


# ------------------------------------------------------------------------------------------------ adapters
def gelu_bwd_ref(dy, u, emu=False):
    """mmbert_gelu_bwd: du = bf16(dy * gelu'(u)), see the module docstring."""
    d, gp = dy.to(torch.float64).reshape(1, -1), G.gelu_grad64(u.to(torch.float64).reshape(1, -1))
    if emu:
        return G._bf(G._f32(d * G._f32(gp))).reshape(dy.shape)
    return G.Ref(d * gp, gp.abs() * d.abs(), G.GELUP_ABS * d.abs(), G.U_BF16, (1, 4096))


def _nt_tile(M, N, K, epi):
    if _on_gpu():
        from msa_amd import ops
        r, c = ops.gemm_nt_describe(M, N, K, epi, with_queue=ops.dynamic_tile_queue)["tile"].split("x")
        return int(r), int(c)
    return (128, 128)


def _r_gemm_nt(c):
    a = c.a
    A_, B_ = _c(a["A"]), _c(a["B"])
    M, K = A_.shape
    N = B_.shape[0]
    drop, keep = a.get("drop"), None
    if _on(drop):
        if a["resid"] is None:
            raise NotImplementedError("gemm_nt: dropout without a residual")
        keep = flat_mask(M * N, drop).view(M, N)
    if a.get("gelu") and (a.get("resid") is not None or a.get("gelu_bwd_u") is not None):
        raise NotImplementedError("gemm_nt: gelu together with resid / gelu_bwd_u")
    epi = (1 if a["bias"] is not None else 0) | (2 if a["gelu"] else 0) | (4 if a["resid"] is not None else 0) | \
          (8 if a["gelu_bwd_u"] is not None else 0) | (16 if a["out_f32"] else 0)
    ad = a.get("alpha_dev")
    ref = G.nt(A_, B_, bias=_c(a["bias"]), gelu=bool(a["gelu"]), resid=_c(a["resid"]), keep=keep, drop_scale=drop[2] if keep is not None else 1.0,
               gelu_u=_c(a["gelu_bwd_u"]), alpha=a["alpha"], alpha_dev=None if ad is None else float(_c(ad).reshape(-1)[0]),
               out_f32=bool(a["out_f32"]), tile=_nt_tile(M, N, K, epi))
    res = [("out", G.check(_c(c.ret), ref["out"], "gemm_nt out").worst)]
    if a["aux"] is not None:
        if not a["gelu"]:
            raise NotImplementedError("gemm_nt: aux without gelu")
        res.append(("aux", G.check(_c(c.post["aux"]), ref["aux"], "gemm_nt aux").worst))
    return res


def _r_splitk(c):
    ref = G.splitk(_c(c.a["A"]), _c(c.a["B"]), resid=_c(c.a["resid"]))
    return [("out", G.check(_c(c.ret), ref["out"], "gemm_nt_splitk").worst)]


def _tn_splits(M, N, K):
    if _on_gpu():
        import ctypes
        from msa_amd import _lib
        sp = ctypes.c_int(0)
        _lib.load().mmbert_gemm_tn_workspace(M, N, K, ctypes.byref(sp))
        return max(1, sp.value)
    return 1


def _r_gemm_tn(c):
    a = c.a
    A_, B_ = _c(a["A"]), _c(a["B"])
    ad = a.get("alpha_dev")
    ref = G.tn(A_, B_, W0=_c(a["W"]), bias0=_c(a["bias_out"]), with_bias=a["bias_out"] is not None, alpha=a["alpha"],
               alpha_dev=None if ad is None else float(_c(ad).reshape(-1)[0]), accumulate=bool(a["accumulate"]),
               splits=_tn_splits(A_.shape[0], A_.shape[1], B_.shape[1]))
    res = [("W", G.check(_c(c.post["W"]), ref["W"], "gemm_tn W").worst)]
    if a["bias_out"] is not None:
        res.append(("bias", G.check(_c(c.post["bias_out"]), ref["bias"], "gemm_tn bias").worst))
    return res


def tn_flags(c):
    acc, n = c.a["accumulate"], len(c.a["problems"])
    return [bool(x) for x in acc] if isinstance(acc, (list, tuple)) else [bool(acc)] * n


def _r_tn_grouped(c):
    probs = [tuple(_c(x) for x in p) for p in c.a["problems"]]
    refs = G.tn_grouped(probs, tn_flags(c), alpha=c.a["alpha"])
    res = []
    for i, (r, p) in enumerate(zip(refs, c.post["problems"])):
        res.append(("W", G.check(_c(p[2]), r["W"], f"gemm_tn_grouped problem {i} W").worst))
        if p[3] is not None:
            res.append(("bias", G.check(_c(p[3]), r["bias"], f"gemm_tn_grouped problem {i} bias").worst))
    return res


def _token_bias(c, seq, pos):
    """The additive key bias per token of the original order: ops.attn_* take it padded per sequence (ops.pad_key_bias) or per token."""
    kb = _c(c.a["key_bias"]).float()
    if kb.numel() == seq.numel():
        return kb
    return kb[_c(c.a["layout"].bias_start).long()[seq] + pos]


def _attn_inputs(c):
    """The call's operands in the ORIGINAL row order: (layout, qkv, key bias per token with the keys behind kv_len removed, the
    original row of every packed row or None, bool [tokens]: the rows backward covers)."""
    lay = c.a["layout"]
    if lay.dropped:
        raise NotImplementedError("attention: the region-B-dropped packing")
    lens, M = lay.lens, sum(lay.lens)
    seq = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    pos = torch.cat([torch.arange(n) for n in lens])
    bias = _token_bias(c, seq, pos).double()
    kv = _c(lay.kv_len) if lay.split else _c(c.a.get("kv_len"))
    region_a = torch.ones(M, dtype=torch.bool)
    if kv is not None:
        kv = kv.long()
        bias = torch.where(pos >= kv[seq], torch.full_like(bias, -1.0e30), bias)
        if lay.split:
            region_a = pos < kv[seq]
    return lay, bias, (_c(lay.inv).long() if lay.split else None), region_a, seq, pos


def _unpacked(t, inv, M):
    """Packed rows -> original order; rows the packed matrix does not hold (backward's region B) read as zero."""
    if inv is None:
        return t
    t2 = torch.cat((t, t.new_zeros((1,) + tuple(t.shape[1:]))))
    return t2[inv.clamp(max=t.shape[0])]


def _r_attn_fwd(c):
    lay, bias, inv, _ra, _s, _p = _attn_inputs(c)
    M = sum(lay.lens)
    drop = c.a.get("drop")
    ref = A.reference(_unpacked(_c(c.a["qkv"]), inv, M), bias, lay.lens, lay.heads, attn_masks(lay, drop), drop[2] if _on(drop) else 1.0)
    got = {"ctx": _unpacked(_c(c.ret[0]), inv, M).double(), "lse": _unpacked(_c(c.ret[1]), inv, M).double()}
    return sorted(A.check(got, ref, lay.lens, lay.heads, "attn_fwd").items())


def _r_attn_bwd(c):
    lay, bias, inv, region_a, seq, pos = _attn_inputs(c)
    M = sum(lay.lens)
    drop = c.a.get("drop")
    dctx = _unpacked(_c(c.a["dctx"]), inv, M)
    ql = _c(c.a.get("q_limit"))
    if ql is not None:
        beyond = pos >= ql.long()[seq]
        assert float(dctx[beyond].float().abs().max()) == 0.0 if bool(beyond.any()) else True, "attn_bwd: a non-zero dctx row at or past q_limit"
    ref = A.reference(_unpacked(_c(c.a["qkv"]), inv, M), bias, lay.lens, lay.heads, attn_masks(lay, drop), drop[2] if _on(drop) else 1.0, dctx)
    d = _unpacked(_c(c.ret), inv, M).double()
    H = d.shape[1] // 3
    got = {"dq": d[:, :H], "dk": d[:, H:2 * H], "dv": d[:, 2 * H:]}
    return sorted(A.check(got, ref, lay.lens, lay.heads, "attn_bwd", rows=None if bool(region_a.all()) else region_a).items())


def _r_q_limit(c):
    lay = c.a["layout"]
    st = _c(lay.seq_start).long()
    rows = _c(c.a["rows32"]).long()
    s = torch.searchsorted(st, rows, right=True) - 1
    want = torch.zeros(len(lay.lens), dtype=torch.long).scatter_reduce_(0, s, rows - st[s] + 1, "amax")
    assert torch.equal(_c(c.ret).long(), want), "attn_q_limit differs from 1 + the largest listed query index per sequence"
    return [("out", 0.0)]


def _site_keep(drop, rows, H):
    return flat_mask(rows * H, drop).view(rows, H) if _on(drop) else None


def _r_ln_fwd(c):
    a = c.a
    x = _c(a["x"])
    H = x.shape[1]
    M = a["M"] if a["M"] is not None else (_c(a["in_rows"]).numel() if a["in_rows"] is not None else x.shape[0])
    drop = a.get("drop")
    ref = R.ln_fwd(x, _c(a["gamma"]), _c(a["beta"]), a["eps"], M=M, in_rows=_c(a["in_rows"]), out_rows=_c(a["out_rows"]),
                   keep=_site_keep(drop, M + a["drop_row0"], H), dscale=drop[2] if _on(drop) else 1.0, drop_row0=a["drop_row0"])
    y, mean, rstd = c.ret
    res = [("y", R.check(_c(y), ref["y"], "ln_fwd y").worst)]
    if mean is not None:
        res += [("mean", R.check(_c(mean), ref["mean"], "ln_fwd mean").worst), ("rstd", R.check(_c(rstd), ref["rstd"], "ln_fwd rstd").worst)]
    return res


def ln_bwd_refs(c, dgamma0=None, dbeta0=None):
    a = c.a
    if a.get("dbias2") is not None:
        raise NotImplementedError("ln_bwd: dbias2")
    x = _c(a["x"])
    H = x.shape[1]
    M = a["M"] if a["M"] is not None else _c(a["mean"]).numel()
    dr = _c(a["drop_rows"])
    site = int(dr.max()) + 1 if dr is not None and dr.numel() else M
    po, pr = a.get("post_drop"), a.get("pre_drop")
    return R.ln_bwd(_c(a["dy"]), x, _c(a["mean"]), _c(a["rstd"]), _c(a["gamma"]), M=M, dy_rows=_c(a["dy_rows"]), x_rows=_c(a["x_rows"]),
                    dx_rows=_c(a["dx_rows"]), drop_rows=dr, dy_row_limit=a["dy_row_limit"], post_keep=_site_keep(po, site, H),
                    post_scale=po[2] if _on(po) else 1.0, pre_keep=_site_keep(pr, site, H), pre_scale=pr[2] if _on(pr) else 1.0,
                    dx2=a["dx2"] is not None, dgamma0=dgamma0, dbeta0=dbeta0, adds=8)


def _r_ln_bwd(c):
    deferred = c.a.get("deferred") is not None
    ref = ln_bwd_refs(c) if deferred else ln_bwd_refs(c, _c(c.a["dgamma"]), _c(c.a["dbeta"]))
    c.meta["refs"] = ref
    res = [("dx", R.check(_c(c.ret), ref["dx"], "ln_bwd dx").worst)]
    if c.a["dx2"] is not None:
        res.append(("dx2", R.check(_c(c.post["dx2"]), ref["dx2"], "ln_bwd dx2").worst))
    if not deferred:
        res += [(k, R.check(_c(c.post[k]), ref[k], "ln_bwd " + k).worst) for k in ("dgamma", "dbeta")]
    return res


def _r_ln_reduce(c):
    """The gamma / beta gradients after the reduce against value before + the float64 sums of every call folded into them."""
    groups = {}
    for j in range(len(c.meta["calls"])):
        groups.setdefault(c.a["pre"][j][0].ptr, []).append(j)
    res = []
    for js in groups.values():
        refs = [c.meta["calls"][j].meta.get("refs") or ln_bwd_refs(c.meta["calls"][j]) for j in js]
        for q, k in enumerate(("dgamma", "dbeta")):
            pre = _c(c.a["pre"][js[0]][q]).double()
            tot = R.Ref(pre + sum(r[k].val for r in refs), sum(r[k].acc for r in refs) + 8.0 * pre.abs(), 0.0, R.U_F32)
            res.append((k, R.check(_c(c.post["grads"][js[-1]][q]), tot, f"ln_bwd_reduce {k} ({len(js)} calls)").worst))
    return res


def _r_gelu_bwd(c):
    return [("du", G.check(_c(c.ret).reshape(1, -1), gelu_bwd_ref(_c(c.a["dy"]), _c(c.a["u"])), "gelu_bwd").worst)]


def _r_ce_fwd(c):
    a = c.a
    if float(a.get("smoothing") or 0.0) != 0.0:
        raise NotImplementedError("ce_fwd: label smoothing")
    nseg = a["nseg"]
    ref = R.ce_fwd(_c(a["logits"]), _c(a["labels"]), a["V"], _c(a["seg_bounds"]), nseg)
    loss, inv, lse = c.ret
    cnt = ref["count"].clamp(min=1).double()
    assert bool(((_c(inv)[:nseg].double() * cnt - 1.0).abs() <= 2.0 ** -23).all()), "ce_fwd: inv_count"
    return [("loss", R.check(_c(loss), ref["loss"], "ce loss").worst), ("row_lse", R.check(_c(lse), ref["row_lse"], "ce row_lse").worst)]


def _r_ce_bwd(c):
    a = c.a
    if float(a.get("smoothing") or 0.0) != 0.0:
        raise NotImplementedError("ce_bwd: label smoothing")
    lab, rows = _c(a["labels"]), _c(a["rows"])
    dl = _c(c.ret)
    worst = 0.0
    for j, ref in R.ce_bwd(_c(a["logits"]), lab, a["V"], _c(a["seg_bounds"]), a["nseg"], _c(a["gscale"]), _c(a["lse"]), rows=rows):
        worst = max(worst, R.check(dl[j], ref, "ce dlogits", gathered=True).worst)
    src = torch.arange(lab.numel()) if rows is None else rows.long()
    labelled = (lab[src] >= 0) & (lab[src] < a["V"])
    assert int((dl[:src.numel()][~labelled].view(torch.int16) != 0).sum()) == 0, "ce_bwd: unlabelled rows of dlogits not exactly zero"
    return [("dlogits", worst)]


def _r_embed_gather(c):
    a = c.a
    ref = E.gather(_c(a["ids"]).reshape(-1), None if a["tts"] is None else _c(a["tts"]).reshape(-1), _c(a["word"]), _c(a["type_"]), _c(a["pos"]), a["T"])
    return [("out", E.check(_c(c.ret), ref, "embed_gather").worst)]


def _r_embed_scatter(c):
    a = c.a
    ref = E.scatter(_c(a["ids"]).reshape(-1), None if a["tts"] is None else _c(a["tts"]).reshape(-1), _c(a["d"]), a["T"], _c(a["gword"]),
                    _c(a["gtype"]), _c(a["gpos"]), V=a.get("vocab"), det=bool(c.meta.get("det")))
    return [(k, E.check(_c(c.post[k]), ref[k], "embed_scatter " + k).worst) for k in ("gword", "gtype", "gpos") if k in ref]


def _pair(c):
    feat = _c(c.a["feat"])
    B, P, _D = feat.shape
    return feat, E.pair_rows(B, P, c.a["T"], c.a.get("seq_len"), c.a.get("offset"))


def _r_pair_fwd(c):
    feat, rows = _pair(c)
    ref = E.pair_fwd(feat, _c(c.a["W"]), _c(c.a["bias"]), rows=rows)
    out0, out1 = _c(c.a["out"]), _c(c.post["out"])
    other = torch.ones(out0.shape[0], dtype=torch.bool)
    other[rows] = False
    assert torch.equal(out0[other].view(torch.int16), out1[other].view(torch.int16)), "pair_proj_fwd wrote a row outside its pair block"
    return [("out", E.check(out1, ref, "pair_proj_fwd").worst)]


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count) if _on_gpu() else E.CUS


def _r_pair_bwd(c):
    feat, rows = _pair(c)
    ref = E.pair_bwd(feat, _c(c.a["J"])[rows], _c(c.a["dJ"])[rows], _c(c.a["dW"]), _c(c.a["db"]), cus=_cus())
    return [("dW", E.check(_c(c.post["dW"]), ref["dW"], "pair_proj_bwd dW").worst), ("db", E.check(_c(c.post["db"]), ref["db"], "pair_proj_bwd db").worst)]


def _bits(t):
    return t.contiguous().view(_BITS[t.element_size()])


def _r_gather_rows(c):
    idx = _c(c.a["idx32"]).long()
    for j, (s, o) in enumerate(zip(c.a["srcs"], c.ret)):
        assert torch.equal(_bits(_c(s)[idx]), _bits(_c(o))), f"gather_rows: output {j} is not its source's listed rows"
    return [("out", 0.0)]


def _r_scatter_rows(c):
    inv = c.a["inverse"]
    take = torch.from_numpy(LR.scatter_ref(_c(inv["table"]).numpy(), inv["stamp"], inv["nlist"], c.a["nrows"]))
    for j, (s, o) in enumerate(zip(c.a["srcs"], c.ret)):
        s = _c(s)
        want = torch.where((take >= 0)[:, None], s[take.clamp(min=0)], torch.zeros_like(s[:1]))
        assert torch.equal(_bits(want), _bits(_c(o))), f"scatter_rows_zero: output {j}"
    return [("out", 0.0)]


def _cd(d):
    return {t: _c(v) for t, v in (d or {}).items()}


def _r_lora_fwd(c):
    """ops.lora_qkv_fwd against tests/lora_ref.fwd on the qkv the call FOUND: the updated qkv (untargeted thirds bit for bit) and h_out."""
    a = c.a
    ref = LO.fwd(_c(a["x"]), _c(a["qkv"]), _cd(a["A"]), _cd(a["B"]), a["targets"], a["scale"])
    res = [("qkv", LO.check(_c(c.post["qkv"]), ref["qkv"], "lora_qkv_fwd qkv"))]
    if a["h_out"] is not None:
        res.append(("h", LO.check(_c(c.post["h_out"]), ref["h"], "lora_qkv_fwd h")))
    return res


def _r_lora_bwd(c):
    """ops.lora_qkv_bwd against tests/lora_ref.bwd: the gradients of the entries of gA / gB the call was handed, from the values it found
    there, and the new residual gradient it returned."""
    a = c.a
    if a["h"] is None:
        raise NotImplementedError("lora_qkv_bwd: h recomputed from x and A")
    if a.get("workspace") is not None:
        raise NotImplementedError("lora_qkv_bwd: a caller's workspace")
    A_, B_ = _cd(a["A"]), _cd(a["B"])
    gA0, gB0 = _cd(a["gA"]), _cd(a["gB"])
    names = LO._names(a["targets"])
    zero = lambda d, like: {t: d.get(t, torch.zeros(like[t].shape)) for t in names}           # noqa: E731
    ref = LO.bwd(_c(a["dqkv"]), _c(a["x"]), _c(a["h"]), A_, B_, a["targets"], a["scale"], dres=_c(a["dres"]), gA0=zero(gA0, A_), gB0=zero(gB0, B_),
                 accumulate=bool(a["accumulate"]))
    res = []
    for key, k, g0 in (("gA", "dA", gA0), ("gB", "dB", gB0)):
        for t in g0:
            res.append((f"{k}[{t}]", LO.check(_c(c.post[key][t]), ref[k][t], f"lora_qkv_bwd {k}[{t}]")))
    if a["dres"] is not None:
        res.append(("dres", LO.check(_c(c.ret), ref["dres"], "lora_qkv_bwd dres")))
    else:
        assert c.ret is None, "lora_qkv_bwd returned a tensor without dres"
    return res


def _r_lora_dense_fwd(c):
    """ops.lora_dense_fwd against tests/lora_dense_ref.fwd on the y the call FOUND (what the projection's GEMM left): the updated y --
    in ADD mode the elements the recorded triple drops bit for bit (the reference builds its own keep mask from it) --, aux and h_out
    where they were handed in."""
    a = c.a
    drop = a.get("drop")
    ref = DR.fwd(_c(a["x"]), _c(a["y"]), _c(a["A"]), _c(a["B"]), a["scale"], int(a["mode"]), drop=None if drop is None else tuple(drop))
    res = [("y", DR.check(_c(c.post["y"]), ref["y"], "lora_dense_fwd y"))]
    if a["aux"] is not None:
        if int(a["mode"]) != DR.GELU:
            raise NotImplementedError("lora_dense_fwd: aux outside the GELU mode")
        res.append(("aux", DR.check(_c(c.post["aux"]), ref["aux"], "lora_dense_fwd aux")))
    if a["h_out"] is not None:
        res.append(("h", DR.check(_c(c.post["h_out"]), ref["h"], "lora_dense_fwd h")))
    return res


def _r_lora_dense_bwd(c):
    """ops.lora_dense_bwd against tests/lora_dense_ref.bwd: dx on the dx the call found, gA / gB from the values found there (from zeros
    when ``accumulate`` is false); ``h=None`` (the gathered rows of the sparse top layer): the reference recomputes h from x and A."""
    a = c.a
    if a.get("workspace") is not None:
        raise NotImplementedError("lora_dense_bwd: a caller's workspace")
    ref = DR.bwd(_c(a["dy"]), _c(a["x"]), _c(a["h"]), _c(a["A"]), _c(a["B"]), a["scale"], dx=_c(a["dx"]), gelu_u=_c(a["gelu_u"]),
                 gA0=_c(a["gA"]), gB0=_c(a["gB"]), accumulate=bool(a["accumulate"]))
    res = []
    for key, k in (("gA", "dA"), ("gB", "dB")):
        if a[key] is not None:
            res.append((k, DR.check(_c(c.post[key]), ref[k], f"lora_dense_bwd {k}")))
    if a["dx"] is not None:
        res.append(("dx", DR.check(_c(c.post["dx"]), ref["dx"], "lora_dense_bwd dx")))
    else:
        assert c.ret is None, "lora_dense_bwd returned a tensor without dx"
    return res


def colsum_flags(c):
    acc, n = c.a["accumulate"], len(c.a["problems"])
    return [bool(x) for x in acc] if isinstance(acc, (list, tuple)) else [bool(acc)] * n


def _r_colsum(c):
    """ops.colsum_grouped, per problem, against the float64 column sum within tests/colsum_ref.py's bound."""
    ad = c.a.get("alpha_dev")
    scale = float(c.a["alpha"]) * (1.0 if ad is None else float(_c(ad).reshape(-1)[0]))
    res = []
    for j, ((x, out0), (_x, out1), acc) in enumerate(zip(c.a["problems"], c.post["problems"], colsum_flags(c))):
        x, out0, out1 = _c(x), _c(out0), _c(out1)
        if x.shape[0] == 0:
            assert torch.equal(out0, out1), f"colsum_grouped problem {j}: M = 0 and the output changed"
            continue
        q = CS.ratio(out1, x, out0, acc, scale)
        assert q <= 1.0, f"colsum_grouped problem {j} ({x.shape[0]} x {x.shape[1]}): error / bound = {q:.3g}"
        res.append(("out", q))
    return res


# ---- the level-launch heads: a Case of the reference the record's fields select, judged by that reference's expected / check_all
def heads_case(c, d=1.0, prior=None):
    """(reference module, Case, Opts or None) of a recorded heads call: ``first`` = the recorded rows ``first_rows`` of ``y`` as fp32 (or the
    fp32 ``first`` operand), the recorded fp32 parameters, labels, MLM losses, alpha / beta; the reference by the record's fields --
    heads_multilabel_ref (``multi_label``), loss_options_ref (an option of the label loss on), heads_cls_ref (``ncls``), else heads_ref."""
    from tests import heads_cls_ref as HCR, heads_multilabel_ref as HML, heads_ref as HR, loss_options_ref as LOR
    a = c.a
    B, H, ncls = int(a["B"]), int(a["H"]), int(a["ncls"])
    if "y" in a:
        if int(a["ldy"]) != a["y"].stride[0]:
            raise NotImplementedError(f"heads: ldy {a['ldy']} is not the row stride of y {a['y'].stride}")
        first = _c(a["y"])[_c(a["first_rows"]).long()].float()
    else:
        first = _c(a["first"]).float()
    assert tuple(first.shape) == (3 * B, H), f"heads: the [CLS] rows are {tuple(first.shape)}, the record says B = {B}, H = {H}"
    params = {n: _c(a[f]).float() for f, n in HEAD_PARAM.items()}
    if "ap2" in a:
        ap_v, ap_s = _c(a["ap"]).reshape(-1), _c(a["ap2"]).reshape(-1)
    else:
        ap_v, ap_s = _c(a["ap"]).reshape(-1)[:B], _c(a["ap"]).reshape(-1)[B:]
    mlm = _c(a["mlm"]).float() if int(a["nmlm"]) else None
    assert mlm is None or mlm.numel() == int(a["nmlm"]), "heads: nmlm is not the size of the recorded mlm operand"
    kw = dict(B=B, H=H, first=first, params=params, ap_v=ap_v, ap_s=ap_s, alpha=float(a["alpha"]), beta=float(a["beta"]), mlm=mlm, d=float(d),
              prior=dict(prior or {}))
    opt_on = bool(a["loss_kind"]) or float(a["label_smoothing"]) != 0.0 or "cls_weight" in a
    if a["multi_label"]:
        if a["loss_kind"] or "cls_weight" in a or not ncls:
            raise NotImplementedError("heads: a multi-label record with a loss kind / class weights / no classes")
        case = HML.Case(sent=None, num_labels=ncls, C=ncls, y=None, t=_c(a["multi_target"]).float().reshape(B, ncls), **kw)
        return HML, case, HML.Opts(pos_weight=_c(a.get("pos_weight")), eps=float(a["label_smoothing"]), thr=_c(a.get("threshold")))
    if "pos_weight" in a or "threshold" in a:
        raise NotImplementedError("heads: pos_weight / threshold outside the multi-label head")
    if ncls:
        case = HCR.Case(sent=None, num_labels=ncls, C=ncls, y=_c(a["sent_cls"]).reshape(-1), **kw)
    else:
        case = HR.Case(sent=_c(a["sent"]).float().reshape(-1), num_labels=1 if a["tanh_lo"] else 7, **kw)
    if opt_on:
        if ncls and a["loss_kind"]:
            raise NotImplementedError("heads: a loss kind on the class head")
        o = LOR.Opts(kind=LOR.KINDS[int(a["loss_kind"])], delta=float(a["huber_delta"]) if int(a["loss_kind"]) == 2 else 1.0,
                     eps=float(a["label_smoothing"]), weight=_c(a.get("cls_weight")))
        return LOR, case, o
    return (HCR if ncls else HR), case, None


def heads_expected(c, d=1.0, prior=None):
    """(module, expected) of a recorded heads call.  The references' bounds hold only where fp32 and float64 agree on the side of every
    kink (relu: heads_ref.kink_ratio; the argmax: heads_cls_ref.gap_ratio; the thresholds: heads_multilabel_ref.decision_ratio; L1 /
    Huber: loss_options_ref.loss_kink_ratio) -- conditions, not tolerances.  The ratios reached on the recorded operands are left in
    ``call.meta["precondition"]``; every output is judged whatever they are (no element or sample is ever left out), a miss under a
    violated condition says that it is one (``_heads_worst``), and ``preconditions(calls)`` asserts them: tests/test_step_seam_gpu.py
    does, on inputs it chose for that; the suites that record a step at the initialisation scale judge the heads as they find them."""
    from tests import heads_cls_ref as HCR, heads_multilabel_ref as HML, heads_ref as HR, loss_options_ref as LOR
    mod, case, o = heads_case(c, d, prior)
    exp = mod.expected(case) if o is None else mod.expected(case, o)
    pre = {"kink_ratio": HR.kink_ratio(case)}
    if mod is HML:
        pre["decision_ratio"] = HML.decision_ratio(case, o, exp)
    elif int(c.a["ncls"]):
        pre["gap_ratio"] = HCR.gap_ratio(case, exp)
    elif mod is LOR and o.kind != "mse":
        pre["loss_kink_ratio"] = LOR.loss_kink_ratio(case, o, exp)
    c.meta["precondition"] = pre
    return mod, exp


def _violated(pre):
    from tests import heads_ref as HR
    bad = {k: round(v, 3) for k, v in pre.items() if not v >= HR.KINK}
    return (f"PRECONDITION of the heads' reference violated: {bad} < {HR.KINK} on the recorded [CLS] rows (fp32 and float64 may take "
            "different sides of a kink there; the bound does not apply): choose another seed") if bad else ""


def preconditions(calls):
    """{condition: the smallest ratio reached} over the recomputed heads calls; raises where one is below heads_ref.KINK."""
    pre = {}
    for c in calls:
        for k, v in c.meta.get("precondition", {}).items():
            pre[k] = min(pre.get(k, math.inf), v)
    assert not _violated(pre), _violated(pre)
    return pre


_HEADS_EXP = {}                                                 # record id -> (module, expected) of its backward (dmlm and the six levels)


def _heads_worst(mod, got, exp, what, pre=None):
    worst = {}
    try:
        mod.check_all(got, exp, what, worst)
    except AssertionError as e:
        raise AssertionError(f"{e}" + (" -- " + _violated(pre) if pre and _violated(pre) else "")) from None
    return [(k, max(w[0], w[1])) for k, w in sorted(worst.items())] + ([("pred", 0.0)] if "pred" in got else [])


def _r_heads_fwd(c):
    """Forward outputs are judged once level 7 has run (a levels-1-6 call leaves them half made: ``check_seam`` holds what it wrote to the
    level-7 recording bit for bit)."""
    if int(c.a["hi"]) < 7:
        return []
    mod, exp = heads_expected(c)
    got = {k: _c(c.post[k]) for k in ("loss", "aux", "out5") + HEAD_FWD_FINAL}
    if "pred" in c.post:
        got["pred"] = _c(c.post["pred"])
    return _heads_worst(mod, got, exp, "heads_step_fwd", c.meta["precondition"])


def _heads_bwd_exp(c):
    key = c.meta.get("record")
    if key not in _HEADS_EXP:
        prior = {n: _c(c.a[g]).float() for g, n in HEAD_GRADS.items()}
        _HEADS_EXP[key] = heads_expected(c, float(_c(c.a["dloss"]).reshape(-1)[0]), prior) + (c.meta["precondition"],)
    c.meta["precondition"] = _HEADS_EXP[key][2]
    return _HEADS_EXP[key][:2]


def _r_heads_dmlm(c):
    mod, exp = _heads_bwd_exp(c)
    return _heads_worst(mod, {"dmlm": _c(c.post["dmlm"])}, exp, "heads_step_dmlm", c.meta.get("precondition"))


def _r_heads_bwd(c):
    if (int(c.a["lo"]), int(c.a["hi"])) != (1, 6):
        raise NotImplementedError("heads_step_bwd: a partial range of levels")
    mod, exp = _heads_bwd_exp(c)
    _HEADS_EXP.pop(c.meta.get("record"), None)
    got = {"dfirst": _c(c.post["dfirst"])}
    if int(c.a["nmlm"]):
        got["dmlm"] = _c(c.post["dmlm"])
    got.update({n: _c(c.post[g]) for g, n in HEAD_GRADS.items() if g in c.post})
    return _heads_worst(mod, got, exp, "heads_step_bwd", c.meta.get("precondition"))


# ---- the prologue and the row lists: exact
def _mask_f32(r):
    """The fp32 value the prologue reads from a recorded mask: float64 rounds (numpy RNE), every other mask dtype converts exactly."""
    t = _c(r)
    return t.numpy().astype(np.float32) if t.dtype == torch.float64 else t.float().numpy()


def prologue_words(ref, tokens, rowset):
    """(fp32 words, int words, mask of the int words the prologue writes) of ``prologue_sizes``'s extent from layout_ref's dict."""
    f = np.concatenate([ref["key_bias"]] + ([ref["key_bias_perm"]] if rowset else []))
    n = len(ref["idx"])
    idx, wrote = np.zeros(max(tokens, 1), dtype=np.int64), np.zeros(max(tokens, 1), dtype=bool)
    idx[:n], wrote[:n] = ref["idx"], True
    parts = [ref["kv_len"], ref["valid"], ref["seq_cnt"], idx, ref["words"]] + ([ref["rank"]] if rowset else [])
    mask = np.concatenate([np.ones(len(p), dtype=bool) if p is not idx else wrote for p in parts])
    return f, np.concatenate(parts).astype(np.int64), mask


def _r_prologue(c, ref_fn=None):
    a = c.a
    lens, B, rowset = list(a["pass_lens"]), int(a["B"]), bool(a["rowset"])
    segs = [(_mask_f32(m), int(p), int(o)) for m, p, o in a["segs"]]
    labels = None if a["labels"] is None else _c(a["labels"]).numpy()
    ref = (ref_fn or LR.prologue_ref)(segs, lens, B, labels, int(a["vocab"]), rowset)
    want_f, want_i, mask = prologue_words(ref, B * sum(lens), rowset)
    got_f, got_i = _c(c.ret["all_f"]).numpy(), _c(c.ret["all_i"]).numpy().astype(np.int64)
    assert got_f.size == want_f.size and got_i.size == want_i.size, "prologue: the recorded extent is not prologue_sizes'"
    bad = np.nonzero(LR.f32_bits(got_f) != LR.f32_bits(want_f))[0]
    assert bad.size == 0, f"prologue: {bad.size} key-bias words differ from layout_ref.prologue_ref (first at {int(bad[0])})"
    bad = np.nonzero((got_i != want_i) & mask)[0]
    assert bad.size == 0, f"prologue: {bad.size} int words differ from layout_ref.prologue_ref (first at {int(bad[0])})"
    nseq = len(lens) * B
    for k, want in (("kv_len", ref["kv_len"]), ("valid", ref["valid"]), ("words", ref["words"])):
        assert np.array_equal(_c(c.ret[k]).numpy().astype(np.int64), want), f"prologue: the view {k}"
    assert np.array_equal(_c(c.ret["idx"]).numpy()[:len(ref["idx"])].astype(np.int64), ref["idx"]), "prologue: the view idx"
    kb = ref["key_bias_perm"] if rowset else ref["key_bias"]
    assert np.array_equal(LR.f32_bits(_c(c.ret["key_bias"]).numpy()), LR.f32_bits(kb)), "prologue: the view key_bias"
    assert c.ret["kv_len"].shape == (nseq,)
    return [("out", 0.0)]


def _r_active_rows(c):
    want = LR.active_rows_ref(_c(c.a["labels"]).reshape(-1).numpy(), int(c.a["V"]))
    idx, cnt = _c(c.ret[0]).numpy().astype(np.int64), int(_c(c.ret[1]).reshape(-1)[0])
    assert cnt == want.size and np.array_equal(idx[:cnt], want), "active_rows differs from layout_ref.active_rows_ref"
    return [("out", 0.0)]


def _r_compact_rows(c):
    rm = c.a["row_map"]
    want = LR.compact_ref(_c(c.a["rows"]).numpy(), _c(c.a["extra"]).numpy(), None if rm is None else _c(rm).numpy())
    for j, r in enumerate(c.ret):
        assert np.array_equal(_c(r).numpy().astype(np.int64), want), f"compact_rows: output {j} differs from layout_ref.compact_ref"
    return [("out", 0.0)]


def _r_pack_i64(c):
    want = LR.pack_ref([s if isinstance(s, tuple) else _c(s).numpy() for s in c.a["segments"]])
    got = _c(c.ret[0]).numpy()
    assert got.size >= want.size and np.array_equal(got[:want.size], want), "pack_i64 differs from layout_ref.pack_ref"
    offs = np.concatenate(([0], np.cumsum([s[0] if isinstance(s, tuple) else s.t.numel() for s in c.a["segments"]])[:-1]))
    assert list(c.ret[1]) == [int(x) for x in offs], "pack_i64: the start offsets"
    return [("out", 0.0)]


ADAPTERS = {"heads_step_fwd": _r_heads_fwd, "heads_step_dmlm": _r_heads_dmlm, "heads_step_bwd": _r_heads_bwd, "prologue": _r_prologue,
            "active_rows": _r_active_rows, "compact_rows": _r_compact_rows, "pack_i64": _r_pack_i64,
            "gemm_nt": _r_gemm_nt, "gemm_nt_splitk": _r_splitk, "gemm_tn": _r_gemm_tn, "gemm_tn_grouped": _r_tn_grouped, "attn_fwd": _r_attn_fwd,
            "attn_bwd": _r_attn_bwd, "attn_q_limit": _r_q_limit, "ln_fwd": _r_ln_fwd, "ln_bwd": _r_ln_bwd, "ln_bwd_reduce": _r_ln_reduce,
            "gelu_bwd": _r_gelu_bwd, "ce_fwd": _r_ce_fwd, "ce_bwd": _r_ce_bwd, "embed_gather": _r_embed_gather, "embed_scatter": _r_embed_scatter,
            "pair_proj_fwd": _r_pair_fwd, "pair_proj_bwd": _r_pair_bwd, "gather_rows": _r_gather_rows, "scatter_rows_zero": _r_scatter_rows,
            "lora_qkv_fwd": _r_lora_fwd, "lora_qkv_bwd": _r_lora_bwd, "lora_dense_fwd": _r_lora_dense_fwd, "lora_dense_bwd": _r_lora_dense_bwd,
            "colsum_grouped": _r_colsum}


def recompute(call):
    """[(output name, worst ratio to its reference's bound)] of one recorded call; raises where an output misses its bound (the
    reference's own ``check``) or the adapter cannot express the call."""
    if call.op not in ADAPTERS:
        raise NotImplementedError(f"no reference adapter for {call.op}")
    try:
        return ADAPTERS[call.op](call)
    except AssertionError as e:
        raise AssertionError(f"call {call.index} ({call.op}, stage {call.meta.get('stage')} layer {call.meta.get('layer')}): {e}") from None


SEAM_OPS = HEADS + ("prologue", "active_rows", "compact_rows", "pack_i64")


def recompute_all(calls, model=None, only=None):
    """Every call recomputed: {op kind: [number of calls, worst ratio]}.  ``model``: the calls are given their stage names first (a
    failure then says which stage of which layer it was).  ``only``: the op kinds to recompute (tests/test_step_seam_gpu.py: ``SEAM_OPS``
    -- the trunk's launches of the same configurations are recomputed by tests/test_step_stages_gpu.py); the others are counted."""
    if model is not None:
        annotate(calls, model)
    out = {}
    _HEADS_EXP.clear()
    for c in calls:
        worst = max([float(r) for _, r in (recompute(c) if only is None or c.op in only else ())] + [0.0])
        n, w = out.get(c.op, (0, 0.0))
        out[c.op] = (n + 1, max(w, worst))
    return out


# ------------------------------------------------------------------------------------------------ dataflow
def names_of(model):
    """{address: [names]} of the model's weight, working-copy, transposed-copy and gradient views ("l3.W1T", "g_word_pad", ...)."""
    out = {}
    for i, lw in enumerate(model._lw):
        for k, v in lw.items():
            if torch.is_tensor(v):
                out.setdefault(v.data_ptr(), []).append(f"l{i}.{k}")
        dl = lw.get("lora_dense")                                # the dense-seam adapters: "l3.dense:A:ffn_output", ...
        for k in ("A", "B", "gA", "gB") if dl else ():
            for t, v in dl[k].items():
                out.setdefault(v.data_ptr(), []).append(f"l{i}.dense:{k}:{t}")
    for k, v in model._w.items():
        if torch.is_tensor(v):
            out.setdefault(v.data_ptr(), []).append(k)
    return out


def _name(names, rec, among=None):
    for n in names.get(rec.ptr, []) if rec is not None else []:
        base = n.split(".")[-1]
        if among is None or base in among:
            return n
    return None


def _stage(c, names, qkv_layer, dqkv_layer=None):
    """(stage name, layer or None) of a call, from the weight / gamma operand it carries (the adapter launches: from the qkv / dqkv
    matrix they work on)."""
    op = c.op
    if op in ("lora_dense_fwd", "lora_dense_bwd"):               # (layer and target from the A operand's address)
        n = next((n for n in names.get(c.a["A"].ptr, []) if ".dense:A:" in n), None)
        if n is None:
            return op, None
        t = n.rsplit(":", 1)[1]
        c.meta["target"] = t
        return (DENSE_FWD_STAGE if op == "lora_dense_fwd" else DENSE_BWD_STAGE)[t], int(n.split(".", 1)[0][1:])
    if op == "lora_qkv_fwd":
        return "lora_fwd", qkv_layer.get(c.a["qkv"].region())
    if op == "lora_qkv_bwd":
        return "lora_bwd", (dqkv_layer or {}).get(c.a["dqkv"].region())
    if op in ("gemm_nt", "gemm_nt_splitk"):
        n = _name(names, c.a["B"], _NT_STAGE)
        if n is None:
            return op, None
        l, _, k = n.rpartition(".")
        return _NT_STAGE[k], int(l[1:]) if l else None
    if op in ("ln_fwd", "ln_bwd"):
        n = _name(names, c.a["gamma"], _LN_STAGE)
        if n is None:
            return op, None
        l, _, k = n.rpartition(".")
        return _LN_STAGE[k] + ("_bwd" if op == "ln_bwd" else ""), int(l[1:]) if l else None
    if op in ("attn_fwd", "attn_bwd"):
        return op, qkv_layer.get(c.a["qkv"].region())
    if op == "gather_rows":
        return f"gather_rows{len(c.a['srcs'])}", None
    return op, None


def annotate(calls, model):
    names = names_of(model)
    qkv_layer, dqkv_layer = {}, {}
    for c in calls:
        st, layer = _stage(c, names, qkv_layer, dqkv_layer)
        c.meta["stage"], c.meta["layer"] = st, layer
        if st == "qkv":
            qkv_layer[c.ret.region()] = layer
        elif st == "attn_bwd":
            dqkv_layer[c.ret.region()] = layer
    return names


def _with(form, behind, stage, drop=None):
    out = []
    for s in form:
        if s != drop:
            out.append(s)
        if s == behind:
            out.append(stage)
    return tuple(out)


def adapter_stages(lora):
    """{layer: (has Q/K/V adapters, the dense targets it has)} of an adapter record (model._lora: "targets", "layers"); a bare collection of
    layer indices stands for Q/K/V adapters on those layers (the older form of the argument)."""
    if not lora:
        return {}
    if isinstance(lora, dict):
        layers, targets = tuple(lora["layers"]), tuple(lora["targets"])
    else:
        layers, targets = tuple(lora), _QKV_TARGETS[:1]
    qkv = any(t in _QKV_TARGETS for t in targets)
    return {l: (qkv, tuple(t for t in DENSE_FWD_STAGE if t in targets)) for l in layers}


def _fwd_form(ad):
    f = FWD_LAYER
    if ad is not None:
        if ad[0]:
            f = _with(f, "qkv", "lora_fwd")
        for t in ad[1]:
            f = _with(f, DENSE_FWD_STAGE[t][len("lora_"):], DENSE_FWD_STAGE[t])
    return f


def _bwd_form(f, ad):
    if ad is not None:
        if ad[0]:
            f = _with(f, "attn_bwd", "lora_bwd")
        for t in ad[1]:
            f = _with(f, DENSE_BWD_STAGE[t][len("lora_"):], DENSE_BWD_STAGE[t])
    return f


def check_sequence(calls, L, stop=0, no_dx=False, lora=(), backward=True, lora_layers=None):
    """Check 1: the trunk's stages in issue order are, per forward pass, FWD_LAYER for layers 0 .. L-1 and, per backward pass, for
    layers L-1 .. ``stop``, BWD_DENSE or (top layer only) one of BWD_TOP_SPARSE.  The frozen form (freeze.TrainablePlan): forward runs all
    L layers, backward the layers L-1 .. ``stop`` (none when ``stop >= L``), and with ``no_dx`` (the embedding stage does not run) layer
    ``stop`` has no ``dx`` stage.  ``lora``: the adapter record (``adapter_stages``; a bare collection of layers: Q/K/V adapters there).  On
    its layers ``lora_fwd`` sits directly behind ``qkv`` and ``lora_bwd`` directly behind ``attn_bwd`` (Q/K/V targets), and each dense
    target's stage directly behind its GEMM's: ``lora_z1`` / ``lora_g`` / ``lora_z2`` behind ``z1`` / ``g`` / ``z2``, ``lora_du`` / ``lora_dy1``
    / ``lora_dctx`` behind ``du`` / ``dy1`` / ``dctx`` -- in BWD_DENSE and in both BWD_TOP_SPARSE forms.  ``backward`` False (a forward
    under ``no_grad``): no backward stage at all.  ``lora_layers``: the older name of ``lora``."""
    if lora_layers is not None:
        lora = lora_layers
    helpers = ("gather_rows8", "gather_rows1", "scatter_rows_zero", "attn_q_limit")
    if stop or no_dx or lora or not backward:
        return _check_sequence_frozen(calls, L, stop, no_dx, adapter_stages(lora), helpers, backward)
    trunk = [c for c in calls if c.meta["layer"] is not None or c.meta["stage"] in helpers]
    seq = [(c.meta["stage"], c.meta["layer"]) for c in trunk]
    i, passes = 0, {"fwd": 0, "bwd": 0}
    strip = lambda part: [s for s, _ in part]
    while i < len(seq):
        if seq[i] == ("qkv", 0):
            for l in range(L):
                part = seq[i:i + 7]
                assert strip(part) == list(FWD_LAYER) and all(x[1] == l for x in part), f"forward of layer {l}: {part}"
                i += 7
            passes["fwd"] += 1
            continue
        for l in reversed(range(L)):
            forms = [BWD_DENSE] + (list(BWD_TOP_SPARSE) if l == L - 1 else [])
            for f in forms:
                part = seq[i:i + len(f)]
                if strip(part) == list(f) and all(x[1] in (l, None) for x in part):
                    i += len(f)
                    break
            else:
                raise AssertionError(f"backward of layer {l}: {seq[i:i + 10]} is none of {forms}")
        passes["bwd"] += 1
    assert passes["fwd"] >= 1 and passes["fwd"] == passes["bwd"], passes
    return passes


def _check_sequence_frozen(calls, L, stop, no_dx, adapters, helpers, backward=True):
    trunk = [c for c in calls if c.meta["layer"] is not None or c.meta["stage"] in helpers]
    assert not any(c.meta["stage"] in ("lora_fwd", "lora_bwd") and c.meta["layer"] is None for c in calls), "an adapter launch on no layer's qkv / dqkv"
    assert not any(c.op in ("lora_dense_fwd", "lora_dense_bwd") and c.meta["layer"] is None for c in calls), "a dense adapter launch on no layer's adapter"
    seq = [(c.meta["stage"], c.meta["layer"]) for c in trunk]
    i, passes = 0, {"fwd": 0, "bwd": 0}
    strip = lambda part: [s for s, _ in part]                    # noqa: E731
    while i < len(seq):
        if seq[i] == ("qkv", 0):
            for l in range(L):
                f = _fwd_form(adapters.get(l))
                part = seq[i:i + len(f)]
                assert strip(part) == list(f) and all(x[1] == l for x in part), f"forward of layer {l}: {part} is not {f}"
                i += len(f)
            passes["fwd"] += 1
            continue
        assert backward, f"a forward pass without backward, yet the trunk ran {seq[i:i + 5]} behind it"
        assert stop < L, f"no encoder layer is trainable, yet the trunk ran {seq[i:i + 5]} behind its forward pass"
        for l in reversed(range(stop, L)):
            forms = [BWD_DENSE] + (list(BWD_TOP_SPARSE) if l == L - 1 else [])
            forms = [_bwd_form(f, adapters.get(l)) for f in forms]
            if no_dx and l == stop:
                forms = [_with(f, None, None, drop="dx") for f in forms]
            for f in forms:
                part = seq[i:i + len(f)]
                if strip(part) == list(f) and all(x[1] in (l, None) for x in part):
                    i += len(f)
                    break
            else:
                raise AssertionError(f"backward of layer {l}: {seq[i:i + 14]} is none of {forms}")
        passes["bwd"] += 1
    assert passes["fwd"] >= 1 and passes["bwd"] == (passes["fwd"] if stop < L and backward else 0), passes
    return passes


class Shadow:
    """What the recorded calls left in every storage they wrote, element by element (check 2)."""

    def __init__(self):
        self.mem = {}

    def _views(self, r: Rec):
        key = (r.sptr, r.dtype)
        if key not in self.mem:
            n = r.sbytes // torch.empty(0, dtype=r.dtype).element_size()
            self.mem[key] = (torch.zeros(n, dtype=_BITS[torch.empty(0, dtype=r.dtype).element_size()]), torch.zeros(n, dtype=torch.bool))
        v, k = self.mem[key]
        return torch.as_strided(v, r.shape, r.stride, r.off), torch.as_strided(k, r.shape, r.stride, r.off)

    def read(self, r: Rec, what, allow_rows=None):
        if (r.sptr, r.dtype) not in self.mem or 0 in r.stride and r.t.numel() > 1:
            return
        v, k = self._views(r)
        got = r.cpu().view(_BITS[r.cpu().element_size()])
        bad = k & (v != got)
        if allow_rows is not None:
            bad[allow_rows] = False
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from what their last writer left (first at {tuple(bad.nonzero()[0].tolist())})"

    def write(self, r: Rec):
        v, k = self._views(r)
        v.copy_(r.cpu().view(_BITS[r.cpu().element_size()]))
        k.fill_(True)


def check_producers(calls, expect=None):
    """Check 2, see the module docstring.  One writer is no recorded launch: the ATen copy / ``index_add_`` that puts the heads' [CLS]-row
    gradients into the output gradient the trunk's backward reads (model._MLMHeadFn.backward, _ClsRowsFn.backward).  ``expect`` (from
    ``check_seam``): {call index: [(the recorded operand, its expected contents or None, rows, name)]} -- before that call's operands are
    read, the expected contents are written into the shadow, so the operand must equal them bit for bit in every row; with None for the
    contents (a step whose heads are not the level-launch form: no recorded ``dfirst`` to expect anything from) the listed rows may
    differ, no other."""
    sh = Shadow()
    for c in calls:
        allow, named = {}, {}
        for r, want, rows, name in (expect or {}).get(c.index, ()):
            named[id(r)] = name + ": "
            if want is None:
                allow[id(r)] = rows
            else:
                v, k = sh._views(r)
                v.copy_(_bits(want).view(v.shape))
                k.fill_(True)
        pure = set(WRITES.get(c.op, ())) - set(ACCUMULATES.get(c.op, ()))
        for k, v in c.a.items():
            if c.op == "gemm_tn_grouped" and k == "problems":
                for j, (p, acc) in enumerate(zip(v, tn_flags(c))):
                    for q, r in enumerate(p):
                        if r is not None and (q != 2 or acc):
                            sh.read(r, f"call {c.index} ({c.op}) problem {j} operand {q}")
                continue
            if c.op == "colsum_grouped" and k == "problems":
                for j, (p, acc) in enumerate(zip(v, colsum_flags(c))):
                    sh.read(p[0], f"call {c.index} ({c.op}) problem {j} operand X")
                    if acc:
                        sh.read(p[1], f"call {c.index} ({c.op}) problem {j} output (accumulated onto)")
                continue
            if c.op in ("lora_qkv_bwd", "lora_dense_bwd") and k in ("gA", "gB") and not c.a["accumulate"]:
                continue
            if c.op == "gemm_tn" and k == "W" and not c.a["accumulate"]:
                continue
            if k in pure:
                continue
            for r in _recs(v):
                sh.read(r, f"{named.get(id(r), '')}call {c.index} ({c.op}, {c.meta.get('stage')}) operand {k}", allow.get(id(r)))
        for r in list(_recs(list(c.post.values()))) + list(_recs(c.ret)):
            if r.sbytes:
                sh.write(r)


def bf16_rne(t):
    """fp32 -> bf16, round to nearest even, by integer arithmetic on the bit patterns (layout_ref.bf16_rne)."""
    b = LR.bf16_rne(LR.f32_bits(t.detach().cpu().float().contiguous().numpy()))
    return torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16).reshape(t.shape)


def _eq(x, y):
    x, y = _c(x), _c(y)
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))


def _view_of(r: Rec, whole: Rec):
    """The recorded contents of ``whole`` at the elements the contiguous 1-D view ``r`` covers, or None where ``r`` is no such view."""
    lo = r.off - whole.off
    if r.sptr != whole.sptr or r.dtype != whole.dtype or lo < 0 or lo + r.t.numel() > whole.t.numel() or r.stride not in ((1,), ()):
        return None
    return whole.cpu().reshape(-1)[lo:lo + r.t.numel()]


def _ws_views(ws, B, H):
    """(P, T) of a recorded heads workspace (ops.heads_step_outputs: the library's own offsets), or None where the library is not there."""
    try:
        from msa_amd import ops
        return ops.heads_step_outputs(_c(ws), B, H)
    except Exception:
        return None


def check_seam(calls, model=None):
    """The hand-overs between the last encoder LayerNorm of the forward pass and the first launch of the encoder's backward, exact, on
    annotated calls.  Every check carries its name in its failure message:

      prologue consumers   every attn_fwd / attn_bwd key bias is a view of the step's prologue output and bit-equal to it, ``kv_len`` (an
                           unsplit layout's) likewise; the MLM head's gather index is a view of the prologue's ``idx``, of its host count
      alternating buffers  two consecutive prologue calls handed persistent buffers use different sets (a step's backward is held to the
                           set its own forward wrote by "prologue consumers": the next prologue comes after it)
      heads y              the heads' ``y`` is the region the top layer's ``ln2`` wrote, bit-equal to what it left
      heads first_rows     ``first_rows`` is the first row of every sequence of the recorded layout, pass by pass
      heads forward finals what levels 1 - 6 wrote (logits, t_rel, rel, the workspace's P / T) is what level 7 found and left
      mlm losses           level 7's ``mlm`` is bit-equal to the per-pass losses ``ce_fwd`` returned, in pass order
      dmlm twice           ``heads_step_dmlm``'s words and the scratch copy level 6 writes are bit-equal
      gscale               ``ce_bwd``'s ``gscale`` is bit-equal to what ``heads_step_dmlm`` wrote (without it: to level 6's ``dmlm``)
      compact row list     ``compact_rows`` is handed the prologue's labelled rows (its host count of them) and ``first_rows``
      label-only step      a step whose heads carry no MLM loss records no MLM-head op, and its row list is empty plus ``first_rows``
      heads gradient views each of the 22 gradient operands of ``heads_step_bwd`` is the ``.grad`` of the parameter named for it
      compact hand-over    (through ``check_producers``) the matrix the top layer's backward reads: rows [:n] the last MLM ``gemm_nt``
                           output, rows [n:] the round-to-nearest-even bf16 of the recorded ``dfirst`` in ``first_rows`` order
      dense hand-over      (likewise) the rows ``first_rows`` equal torch's own bf16 ``index_add_`` of bf16(dfirst) onto the matrix the MLM
                           head left (its dense product, or zeros with the labelled rows copied in), every other row is untouched

    Returns (``expect`` for ``check_producers``, {check name: times it ran})."""
    top = max([c.meta["layer"] for c in calls if c.meta.get("layer") is not None] + [0])
    params = dict(model.named_parameters()) if hasattr(model, "named_parameters") else None
    views = getattr(model, "head_grad_views", None)
    expect, ran = {}, {}
    st = {}

    def tick(k):
        ran[k] = ran.get(k, 0) + 1

    def fresh(pro):
        return dict(pro=pro, lens=None, lay=None, ln2=None, ce_f=None, heads={}, h7=None, dm=None, hb=None, mlm_dy=None, cr=None, mlm_ops=[], gathered={})
    st = fresh(None)
    prev_pro = None
    for c in calls:
        stage, l = c.meta.get("stage"), c.meta.get("layer")
        w = f"call {c.index} ({c.op}, {stage})"
        if c.op == "prologue":
            if prev_pro is not None and prev_pro.a["bufs"] is not None and c.a["bufs"] is not None:
                same = [x.sptr == y.sptr for x, y in zip(prev_pro.a["bufs"], c.a["bufs"])]
                assert not any(same), f"alternating buffers: {w} writes the buffer set of the previous step's prologue (call {prev_pro.index})"
                tick("alternating buffers")
            st, prev_pro = fresh(c), c
            continue
        if c.op in ("attn_fwd", "attn_bwd"):
            st["lens"], st["lay"] = list(c.a["layout"].lens), c.a["layout"]
            pro = st["pro"]
            if pro is not None:
                got = _view_of(c.a["key_bias"], pro.ret["all_f"])
                assert got is not None, f"prologue consumers: {w}: key_bias is no view of the output of this step's prologue (call {pro.index})"
                assert _eq(got, _c(c.a["key_bias"]).reshape(-1)), f"prologue consumers: {w}: key_bias differs from what the prologue wrote"
                kv = None if c.a["layout"].split else c.a.get("kv_len")
                if kv is not None:
                    got = _view_of(kv, pro.ret["all_i"])
                    assert got is not None and kv.off == pro.ret["kv_len"].off, f"prologue consumers: {w}: kv_len is not the prologue's kv_len view"
                    assert _eq(got, _c(kv).reshape(-1)) and _eq(_c(kv), _c(pro.ret["kv_len"])), f"prologue consumers: {w}: kv_len differs from what the prologue wrote"
                tick("prologue consumers")
        if stage == "ln2" and l == top:
            st["ln2"] = c
        if stage in ("mlm_t0", "logits", "mlm_dt", "mlm_dy", "mlm_ln", "mlm_ln_bwd") or c.op in ("ce_fwd", "ce_bwd", "gelu_bwd"):
            st["mlm_ops"].append(c)
        if c.op == "ce_fwd":
            st["ce_f"] = c
        if c.op == "active_rows":
            st["ar"] = c
        if stage == "mlm_dy":
            st["mlm_dy"] = c
        if c.op == "gather_rows":
            for s, o in zip(c.a["srcs"], c.ret):
                st["gathered"][o.region()] = (c, s)
            if len(c.a["srcs"]) == 6 and st["pro"] is not None:       # the MLM head's gather of its labelled rows
                pro, ar = st["pro"], st.get("ar")                    # (a caller without the prologue's list: ops.active_rows made one)
                n = int(_c(pro.ret["words"])[len(_c(pro.ret["kv_len"]))])
                whole = pro.ret["idx"] if ar is None else ar.ret[0]
                got = _view_of(c.a["idx32"], whole)
                assert got is not None and c.a["idx32"].off == whole.off, f"prologue consumers: {w}: the gather index is no prefix view of the prologue's idx"
                assert c.a["idx32"].t.numel() == n, f"prologue consumers: {w}: {c.a['idx32'].t.numel()} gathered rows, the prologue's host word says {n}"
                assert _eq(got, _c(c.a["idx32"])), f"prologue consumers: {w}: the gather index differs from the prologue's idx"
                tick("prologue consumers")
        if c.op == "heads_step_fwd":
            a, rec = c.a, c.meta.get("record")
            if "y" in a:
                ln2 = st["ln2"]
                assert ln2 is not None, f"heads y: {w}: no ln2 of the top layer was recorded in front of the heads"
                out = ln2.ret[0]
                lay = st.get("lay")
                if a["y"].sptr != out.sptr and lay is not None and lay.split and lay.inv is not None:
                    # (the inference packing: the encoder's output is gathered back into the caller's row order by torch, no recorded launch)
                    want = _unpacked(_c(out), _c(lay.inv).long(), sum(lay.lens))
                    assert _eq(a["y"], want), f"heads y: {w}: y is not the top layer's ln2 output in the caller's row order"
                else:
                    assert a["y"].region() == out.region() and a["y"].shape == out.shape, f"heads y: {w}: y is not the region the top layer's ln2 wrote"
                    assert _eq(a["y"], out), f"heads y: {w}: y differs from what the top layer's ln2 left"
                tick("heads y")
                assert st["lens"] is not None, f"heads first_rows: {w}: no attention layout recorded"
                want = torch.tensor([0] + st["lens"][:-1]).cumsum(0)
                fr = _c(a["first_rows"]).reshape(-1).long()
                assert fr.numel() == want.numel() == 3 * int(a["B"]) and torch.equal(fr, want), \
                    f"heads first_rows: {w}: {fr.tolist()} is not the first row of every sequence {want.tolist()}"
                tick("heads first_rows")
            if int(a["lo"]) > 1:
                prev = st["heads"].get(rec)
                assert prev is not None and int(prev.a["hi"]) == int(a["lo"]) - 1, f"heads forward finals: {w}: levels from {a['lo']} without the levels below"
                for k in HEAD_FWD_FINAL:
                    assert _eq(prev.post[k], a[k]) and _eq(a[k], c.post[k]), f"heads forward finals: {w}: {k} changed behind levels 1 - {prev.a['hi']}"
                have_ws = "ws" in prev.post and "ws" in a and "ws" in c.post
                v0, v1, v2 = (_ws_views(x, int(a["B"]), int(a["H"])) for x in (prev.post["ws"], a["ws"], c.post["ws"])) if have_ws else (None,) * 3
                if v0 is not None:
                    for k, x, y, z in zip("PT", v0, v1, v2):
                        assert _eq(x, y) and _eq(y, z), f"heads forward finals: {w}: the workspace's {k} changed behind levels 1 - {prev.a['hi']}"
                tick("heads forward finals")
            if int(a["hi"]) == 7:
                st["h7"] = c
                if int(a["nmlm"]):
                    ce = st["ce_f"]
                    assert ce is not None, f"mlm losses: {w}: nmlm = {a['nmlm']} and no ce_fwd recorded in this step"
                    assert _eq(_c(a["mlm"]).reshape(-1), _c(ce.ret[0]).float().reshape(-1)[:int(a["nmlm"])]) and int(a["nmlm"]) == int(ce.a["nseg"]), \
                        f"mlm losses: {w}: mlm {_c(a['mlm']).tolist()} is not what ce_fwd returned, in pass order {_c(ce.ret[0]).tolist()}"
                    tick("mlm losses")
            st["heads"][rec] = c
        if c.op == "heads_step_dmlm":
            st["dm"] = c
        if c.op == "heads_step_bwd":
            st["hb"] = c
            if st["dm"] is not None:
                assert st["dm"].meta.get("record") == c.meta.get("record") and _eq(st["dm"].post["dmlm"], c.post["dmlm"]), \
                    f"dmlm twice: {w}: level 6's scratch copy differs from what heads_step_dmlm wrote"
                tick("dmlm twice")
            have = params is not None or views is not None
            for g, n in HEAD_GRADS.items() if have else ():
                if g in c.meta.get("dropped", ()):
                    continue
                v = params[n].grad if params is not None else views[n]
                assert v is not None and g in c.a and c.a[g].ptr == v.data_ptr() and c.a[g].shape == tuple(v.shape), \
                    f"heads gradient views: {w}: {g} is not the .grad view of {n}"
            if have:
                tick("heads gradient views")
        if c.op == "ce_bwd":
            src = st["dm"] if st["dm"] is not None else st["hb"]
            if src is not None:
                assert _eq(_c(c.a["gscale"]).reshape(-1), _c(src.post["dmlm"]).reshape(-1)), \
                    f"gscale: {w}: gscale {_c(c.a['gscale']).tolist()} is not what {src.op} (call {src.index}) wrote {_c(src.post['dmlm']).tolist()}"
                tick("gscale")
        if c.op == "compact_rows":
            st["cr"] = c
            hb, pro = st["hb"], st["pro"]
            if hb is not None and "first_rows" in hb.a:
                assert torch.equal(_c(c.a["extra"]).long(), _c(hb.a["first_rows"]).long()), f"compact row list: {w}: the extra rows are not the heads' first_rows"
                if pro is not None and st.get("ar") is None:
                    n = int(_c(pro.ret["words"])[len(_c(pro.ret["kv_len"]))])
                    assert torch.equal(_c(c.a["rows"]).long(), _c(pro.ret["idx"]).long()[:n]), \
                        f"compact row list: {w}: the labelled rows are not the prologue's idx[:{n}] (its host count)"
                tick("compact row list")
        if stage == "ln2_bwd" and l == top:
            _handover(c, st, expect, tick, w)
        if c.op == "heads_step_bwd" and not int(c.a["nmlm"]):
            assert not st["mlm_ops"], f"label-only step: {w}: no MLM loss, yet the step recorded {[x.op for x in st['mlm_ops']]}"
            tick("label-only step")
    return expect, ran


def _handover(c, st, expect, tick, w):
    """The output gradient the top layer's backward reads (its ``ln2_bwd``'s ``dy``, or the source of the gather in front of it): what
    ``check_seam`` expects of it, left in ``expect`` for ``check_producers``."""
    dy = c.a["dy"]
    user, m = c, dy
    if dy.region() in st["gathered"] and len(st["gathered"][dy.region()][0].a["srcs"]) == 1:
        user, m = st["gathered"][dy.region()]
    hb, cr, last = st["hb"], st["cr"], st["mlm_dy"]
    lens = st["lens"] or []
    cls_rows = torch.tensor([0] + lens[:-1]).cumsum(0) if lens else None
    if hb is None:                                               # the 19-launch / eager heads: no recorded dfirst to expect anything from
        if cr is None and cls_rows is not None and c.a.get("dy_rows") is None:
            expect.setdefault(user.index, []).append((m, None, cls_rows[cls_rows < m.shape[0]], "dense hand-over (heads not recorded)"))
        return
    df = bf16_rne(_c(hb.post["dfirst"]))
    fr = _c(hb.a["first_rows"]).long() if "first_rows" in hb.a else cls_rows
    if cr is not None and cr.index > hb.index:                   # compact: labelled rows ‖ first_rows
        n, nf = cr.a["rows"].t.numel(), cr.a["extra"].t.numel()
        assert m is dy and dy.shape[0] == n + nf, f"compact hand-over: {w}: dy has {dy.shape[0]} rows, the row list {n} + {nf}"
        assert df.shape[0] == nf, f"compact hand-over: {w}: {df.shape[0]} rows of dfirst for {nf} [CLS] rows"
        if n:
            assert last is not None and last.ret.ptr == dy.ptr and last.ret.shape[0] == n, f"compact hand-over: {w}: rows [:{n}] are not the last MLM gemm_nt's output"
            want = torch.cat((_c(last.ret), df))
        else:
            assert not st["mlm_ops"], f"label-only step: {w}: an empty labelled-row list, yet the step recorded {[x.op for x in st['mlm_ops']]}"
            want = df
        expect.setdefault(user.index, []).append((m, want, None, "compact hand-over"))
        tick("compact hand-over")
        return
    rows = sum(lens)
    if last is not None and last.ret.sptr == m.sptr:             # the MLM head's dense product, the [CLS] rows added in place
        base = _c(last.ret).clone()
    else:                                                        # zeros, the labelled rows' gradients copied in (none on a label-only step)
        base = torch.zeros((rows, m.shape[1]), dtype=torch.bfloat16)
        if last is not None:
            pro = st["pro"]
            assert pro is not None, f"dense hand-over: {w}: no prologue recorded to take the labelled rows from"
            n = int(_c(pro.ret["words"])[len(_c(pro.ret["kv_len"]))])
            assert last.ret.shape[0] >= n, f"dense hand-over: {w}: {last.ret.shape[0]} rows from the MLM head for {n} labelled rows"
            base[_c(pro.ret["idx"]).long()[:n]] = _c(last.ret)[:n]
    base.index_add_(0, fr, df)                                   # torch's own bf16 index_add_ (one rounding of the sum per element)
    expect.setdefault(user.index, []).append((m, base[:m.shape[0]], None, "dense hand-over"))
    tick("dense hand-over")


def _same(x: Rec, y: Rec, what):
    assert x is not None and y is not None and x.region() == y.region(), f"{what}: not the expected buffer"


def _wiring(calls, names, L):
    """Check 3 (and 6 for the weight-gradient problems)."""
    fwd, bwd = {}, {}
    gathered, scattered = {}, {}                               # output region -> (source Rec, row list Rec)
    last_gather = None
    for c in calls:
        st, l = c.meta["stage"], c.meta["layer"]
        if c.op == "gather_rows":
            for s, o in zip(c.a["srcs"], c.ret):
                gathered[o.region()] = (s, c.a["idx32"])
            last_gather = c
        if c.op == "scatter_rows_zero":
            for s, o in zip(c.a["srcs"], c.ret):
                scattered[o.region()] = s
        if l is None:
            if c.op == "gemm_tn_grouped":
                _wgrad_wiring(c, names, fwd, bwd, gathered)
            continue
        root = lambda r: gathered[r.region()][0] if r.region() in gathered else r       # noqa: E731
        w = f"layer {l} {st}"
        if st in FWD_LAYER:
            if st == "qkv":
                fwd[l] = {}
                bwd.pop(l, None)
                if l > 0:
                    _same(c.a["A"], fwd[l - 1]["ln2"].ret[0], w + " input = the layer below's output")
            f = fwd[l]
            if st == "attn_fwd":
                _same(c.a["qkv"], f["qkv"].ret, w + " qkv")
            elif st == "z1":
                _same(c.a["A"], f["attn_fwd"].ret[0], w + " A = ctx")
                _same(c.a["resid"], f["qkv"].a["A"], w + " residual = the layer's input")
            elif st == "ln1":
                _same(c.a["x"], f["z1"].ret, w + " x = z1")
            elif st == "g":
                _same(c.a["A"], f["ln1"].ret[0], w + " A = y1")
            elif st == "z2":
                _same(c.a["A"], f["g"].ret, w + " A = g")
                _same(c.a["resid"], f["ln1"].ret[0], w + " residual = y1")
            elif st == "ln2":
                _same(c.a["x"], f["z2"].ret, w + " x = z2")
            f[st] = c
            continue
        f, b = fwd[l], bwd.setdefault(l, {})
        dxo = lambda lb: lb.post["dx2"] if "dx2" in lb.post else lb.ret                 # noqa: E731  (the dropped gradient, where there is a dropout)
        if st in ("ln2_bwd", "ln1_bwd"):
            ln, z = ("ln2", "z2") if st == "ln2_bwd" else ("ln1", "z1")
            _same(c.a["x"], f[z].ret, w + f" x = {z}")
            _same(root(c.a["mean"]), f[ln].ret[1], w + " mean")
            _same(root(c.a["rstd"]), f[ln].ret[2], w + " rstd")
            for k in ("mean", "rstd"):
                if c.a[k].region() in gathered:
                    idx = gathered[c.a[k].region()][1]
                    for rk in ("x_rows", "drop_rows"):
                        assert c.a[rk] is not None and torch.equal(_c(c.a[rk]), _c(idx)), w + f": {rk} is not the row list its statistics were gathered with"
            want = f["z2" if st == "ln2_bwd" else "z1"].a["drop"]
            assert tuple(c.a["pre_drop"] or (0, 0, 1.0)) == tuple(want or (0, 0, 1.0)), w + ": pre_drop is not the forward's triple"
            if st == "ln1_bwd":
                _same(c.a["dy"], b["dy1"].ret, w + " dy = dy1")
        elif st == "du":
            _same(c.a["A"], dxo(b["ln2_bwd"]), w + " A = dz2 (dropped)")
            _same(root(c.a["gelu_bwd_u"]), f["g"].post["aux"], w + " gelu_bwd_u = the forward's aux u")
        elif st == "dy1":
            _same(c.a["A"], b["du"].ret, w + " A = du")
            _same(c.a["resid"], b["ln2_bwd"].ret, w + " residual = dz2")
        elif st == "dctx":
            _same(c.a["A"], dxo(b["ln1_bwd"]), w + " A = dz1 (dropped)")
        elif st == "attn_bwd":
            _same(c.a["qkv"], f["qkv"].ret, w + " qkv")
            _same(c.a["ctx"], f["attn_fwd"].ret[0], w + " ctx")
            _same(c.a["lse"], f["attn_fwd"].ret[1], w + " lse")
            d = c.a["dctx"]
            if d.region() in scattered:
                _same(scattered[d.region()], b["dctx"].ret, w + " dctx = the scattered rows of dctx")
            elif d.shape[0] == b["dctx"].ret.shape[0]:           # (few rows put back by torch's index_copy_ are no recorded launch)
                _same(d, b["dctx"].ret, w + " dctx")
            assert tuple(c.a["drop"] or (0, 0, 1.0)) == tuple(f["attn_fwd"].a["drop"] or (0, 0, 1.0)), w + ": dropout triple differs from the forward's"
            assert c.a["layout"].lens == f["attn_fwd"].a["layout"].lens
        elif st == "dx":
            _same(c.a["A"], b["attn_bwd"].ret, w + " A = dqkv")
            r = c.a["resid"]
            if r.region() in scattered:
                _same(scattered[r.region()], b["ln1_bwd"].ret, w + " residual = the scattered rows of dz1")
            elif r.shape[0] == b["ln1_bwd"].ret.shape[0]:
                _same(r, b["ln1_bwd"].ret, w + " residual = dz1")
        b[st] = c
        b["_gather"] = last_gather
    return fwd, bwd


_WG = {"g_W1": ("du", "ret", "ln1", 0, "g_b1"), "g_W2": ("ln2_bwd", "dxo", "g", "ret", "g_b2"), "g_Wqkv": ("attn_bwd", "ret", "qkv", "A", "g_bqkv"),
       "g_Wo": ("ln1_bwd", "dxo", "attn_fwd", 0, "g_bo")}


def _wgrad_wiring(c, names, fwd, bwd, gathered):
    root = lambda r: gathered[r.region()][0] if r.region() in gathered else r           # noqa: E731
    for j, (A_, B_, W, bias) in enumerate(c.a["problems"]):
        n = _name(names, W, set(_WG) | {"g_word_pad", "g_Wt"})
        assert n is not None, f"weight-gradient problem {j}: W is no gradient view of the model"
        l, _, k = n.rpartition(".")
        if k not in _WG:
            want_b = {"g_word_pad": "g_pred_bias", "g_Wt": "g_bt"}[k]
            assert bias is not None and want_b in names.get(bias.ptr, []), f"problem {j} ({n}): bias buffer is not {want_b}"
            continue
        l = int(l[1:])
        sa, ka, sb, kb, bn = _WG[k]
        ca, cb = bwd[l][sa], fwd[l][sb]
        wantA = (ca.post["dx2"] if "dx2" in ca.post else ca.ret) if ka == "dxo" else ca.ret
        wantB = cb.a["A"] if kb == "A" else cb.ret if kb == "ret" else cb.ret[kb]
        _same(A_, wantA, f"problem {j} ({n}) A = layer {l} {sa}")
        _same(root(B_), wantB, f"problem {j} ({n}) B = layer {l} {sb}")
        assert bias is not None and f"l{l}.{bn}" in names.get(bias.ptr, []), f"problem {j} ({n}): bias buffer is not l{l}.{bn}"


def check_transposes(calls, names, model=None):
    """Check 4."""
    seen = {}
    params = dict(model.named_parameters()) if hasattr(model, "named_parameters") else {}
    for c in calls:
        if c.op not in ("gemm_nt", "gemm_nt_splitk"):
            continue
        n = _name(names, c.a["B"], set(_TRANSPOSED) | set(_TRANSPOSED.values()))
        if n is None:
            continue
        l, _, k = n.rpartition(".")
        if k in _TRANSPOSED:
            src = seen.get((l, _TRANSPOSED[k]))
            assert src is not None, f"{n}: its forward weight was never read in the recording"
            Wf, WT = _c(src), _c(c.a["B"])
            assert torch.equal(_bits(WT[:, :Wf.shape[0]]), _bits(Wf.t()[:WT.shape[0]])), f"call {c.index}: {n} is not the transpose of the bf16 working copy"
        else:
            seen[(l, k)] = c.a["B"]
            pn = (f"bert.encoder.layer.{l[1:]}." + _PARAM_OF[k]) if l else _PARAM_OF_W.get("word" if k == "word_h" else k)
            if pn in params:
                p = params[pn].detach()
                if k == "Wqkv":
                    pre = pn[:-len("query.weight")]
                    p = torch.cat([params[pre + x + ".weight"].detach() for x in ("query", "key", "value")])
                Wc = _c(c.a["B"])
                assert torch.equal(_bits(Wc[:p.shape[0]]), _bits(p.to(torch.bfloat16).cpu())), f"call {c.index}: {n} is not the parameter {pn} rounded to bf16"


def check_dropout_sites(calls):
    """Check 5: one triple per site (a site = a stage of a layer / an embedding launch group), different streams between sites."""
    site = {}
    for c in calls:
        st, l = c.meta["stage"], c.meta["layer"]
        for k, key in (("drop", {"lora_z1": "z1", "lora_z2": "z2"}.get(st, st)), ("pre_drop", {"ln2_bwd": "z2", "ln1_bwd": "z1"}.get(st)), ("post_drop", {"emb_ln_bwd": "emb_ln", "joint_ln_bwd": "joint_ln"}.get(st))):
            d = c.a.get(k)
            if not _on(d) or key is None:
                continue
            if key == "attn_bwd":
                key = "attn_fwd"
            ident = (c.meta.get("pass"), l, key) if key != "joint_ln" else (c.meta.get("pass"), l, key, tuple(d))
            site.setdefault(ident, set()).add(tuple(d))
    for ident, triples in site.items():
        assert len(triples) == 1, f"dropout site {ident}: forward and backward carry different triples {triples}"
    streams = [next(iter(t))[0] for t in site.values()]
    assert len(set(streams)) == len(streams), "two dropout sites share a stream"
    return len(site)


def check_kv_len(calls):
    """kv_len of every attention call against the number of leading keys behind which the recorded key bias masks every key."""
    for c in calls:
        if c.op not in ("attn_fwd", "attn_bwd"):
            continue
        lay = c.a["layout"]
        kv = _c(lay.kv_len) if lay.split else _c(c.a.get("kv_len"))
        if kv is None:
            continue
        seq = torch.repeat_interleave(torch.arange(len(lay.lens)), torch.tensor(lay.lens))
        kb = _token_bias(c, seq, torch.cat([torch.arange(n) for n in lay.lens]))
        for s, S in enumerate(lay.lens):
            live = (kb[seq == s] > A.MASKED).nonzero()
            want = int(live.max()) + 1 if live.numel() else 0
            # (a split layout's region A also holds the masked-out rows that carry a label: its key count may exceed the live keys -- the
            # bias still masks those --, it must never fall short of them)
            ok = int(kv[s]) >= want if lay.split else (int(kv[s]) == want or (want == 0 and int(kv[s]) <= 1))
            assert ok, f"call {c.index} ({c.op}): kv_len[{s}] = {int(kv[s])}, the key bias says {want}"


def check_grad_views(calls, names, model):
    """Check 6 for the gradient buffers the other stages write: the LayerNorm gradients of a stage, the embedding tables, the pair
    projections -- and every gradient view sits at its parameter's ``.grad``."""
    for c in calls:
        st, l = c.meta["stage"], c.meta["layer"]
        if c.op == "ln_bwd":
            base = st[:-len("_bwd")] + "_"
            pre = f"l{l}." if l is not None else ""
            for k, suffix in (("dgamma", "g"), ("dbeta", "b")):
                assert pre + "g_" + base + suffix in names.get(c.a[k].ptr, []), f"call {c.index} ({st}): {k} is not {pre}g_{base}{suffix}"
        elif c.op == "embed_scatter":
            for k, n in (("gword", "g_word"), ("gtype", "g_type"), ("gpos", "g_pos")):
                assert c.a[k] is None or n in names.get(c.a[k].ptr, []), f"embed_scatter {k} is not {n}"
        elif c.op == "pair_proj_bwd":
            nw = _name(names, c.a["dW"], {"g_Wv_w", "g_Ws_w"})
            assert nw is not None and nw[:-1] + "b" in names.get(c.a["db"].ptr, []), "pair_proj_bwd: dW / db are not one projection's gradients"
    if not hasattr(model, "named_parameters"):
        return
    params = dict(model.named_parameters())
    for i, lw in enumerate(model._lw):
        for k, pn in _PARAM_OF.items():
            g = params[f"bert.encoder.layer.{i}.{pn}"].grad
            assert g is not None and g.data_ptr() == lw["g_" + k].data_ptr(), f"l{i}.g_{k} is not the .grad of {pn}"
    label_only = not any(c.op == "ce_fwd" for c in calls)         # (a label-only step: its backward does not reach the MLM-only parameters)
    for k, pn in _PARAM_OF_W.items():
        if "g_" + k in model._w:
            g = params[pn].grad
            if label_only and k in ("pred_bias", "bt", "mlm_ln_g", "mlm_ln_b", "Wt"):
                assert g is None, f"a label-only step left a gradient on the MLM-only parameter {pn}"
                continue
            assert g is not None and g.data_ptr() == model._w["g_" + k].data_ptr(), f"g_{k} is not the .grad of {pn}"


def _drop_of(d):
    return None if d is None else tuple(d)


def check_dense_adapter_wiring(calls, model):
    """Exact: every dense-seam adapter launch (``lora_dense_fwd`` / ``lora_dense_bwd``) against its neighbours -- the GEMM directly in
    front, the same layer's forward stages, the layer's adapter views -- and nothing else, so it holds for the full and the frozen form
    of a step (the calls are annotated).  Forward: ``x`` is the region of that GEMM's ``A`` operand, ``y`` the region it returned; ADD
    mode: the GEMM carried ``resid`` and the same ``drop``, ``aux is None``; GELU mode: the GEMM carried no ``gelu``, ``aux``, ``resid`` or
    ``drop``, and where the same layer's ``du`` stage runs later, the adapter was handed an ``aux`` and it is the region that stage reads as
    ``gelu_bwd_u`` (through the gather on the sparse top layer).  Backward: ``dx`` is what the GEMM in front returned, ``dy`` its ``A`` operand, ``gelu_u`` its ``gelu_bwd_u`` for
    ``lora_du`` and None for the other two; ``x`` is the layer's forward ``g`` output / ``ln1`` output / attention context (or a gather of
    it); ``h`` a leading-row view of what the layer's forward adapter wrote to ``h_out`` -- None exactly on the gathered path;
    ``accumulate is True``; ``gA`` / ``gB`` sit at ``model._lw[l]["lora_dense"]["gA" / "gB"][t]``, the ``.grad`` of the adapter's parameters
    (check 6 for the adapters), and are left out exactly for a parameter that takes no gradient.  Returns the number of launches checked."""
    fwd, fad, aux_of, gathered, n = {}, {}, {}, {}, 0
    root = lambda r: gathered[r.region()] if r is not None and r.region() in gathered else r      # noqa: E731
    for i, c in enumerate(calls):
        st, l = c.meta.get("stage"), c.meta.get("layer")
        if c.op == "gather_rows":
            for s, o in zip(c.a["srcs"], c.ret):
                gathered[o.region()] = s
        if l is not None and st in FWD_LAYER:
            if st == "qkv":
                fwd[l], fad[l] = {}, {}
                aux_of.pop(l, None)
            fwd.setdefault(l, {})[st] = c
        if st == "du" and "intermediate" in fad.get(l, {}):      # (the GEMM in front of that adapter wrote no aux: the adapter must have)
            assert l in aux_of, f"layer {l} du: backward reads a pre-activation, yet the layer's intermediate adapter was handed no aux to write"
            _same(root(c.a["gelu_bwd_u"]), aux_of[l], f"layer {l} du: gelu_bwd_u = the aux the layer's intermediate adapter wrote")
        if c.op not in ("lora_dense_fwd", "lora_dense_bwd"):
            continue
        assert l is not None, f"call {c.index} ({c.op}): A is no dense adapter of the model"
        t, w = c.meta["target"], f"call {c.index} (layer {l} {st})"
        g = calls[i - 1] if i else None
        n += 1
        if c.op == "lora_dense_fwd":
            assert g is not None and g.op == "gemm_nt" and (g.meta["stage"], g.meta["layer"]) == (st[len("lora_"):], l), w + ": not directly behind its projection's GEMM"
            _same(c.a["x"], g.a["A"], w + " x = the GEMM's A operand")
            _same(c.a["y"], g.ret, w + " y = what the GEMM returned")
            if int(c.a["mode"]) == DR.ADD:
                assert st in ("lora_z1", "lora_z2"), w + ": ADD mode on the FFN-up seam"
                assert g.a["resid"] is not None, w + ": the GEMM in front carried no residual"
                assert _drop_of(g.a["drop"]) == _drop_of(c.a["drop"]), w + f": drop {_drop_of(c.a['drop'])} is not the GEMM's {_drop_of(g.a['drop'])}"
                assert c.a["aux"] is None, w + ": aux in ADD mode"
            else:
                assert st == "lora_g", w + ": GELU mode outside the FFN-up seam"
                assert not g.a["gelu"] and g.a["aux"] is None and g.a["resid"] is None and not _on(g.a["drop"]) and not _on(c.a["drop"]), \
                    w + ": the GEMM in front of a GELU-mode adapter carried gelu / aux / resid / drop"
                if c.a["aux"] is not None:
                    aux_of[l] = c.a["aux"]
            fad.setdefault(l, {})[t] = c
            continue
        assert g is not None and g.op in ("gemm_nt", "gemm_nt_splitk") and (g.meta["stage"], g.meta["layer"]) == (st[len("lora_"):], l), \
            w + ": not directly behind its input-gradient GEMM"
        _same(c.a["dx"], g.ret, w + " dx = what the GEMM returned")
        _same(c.a["dy"], g.a["A"], w + " dy = the GEMM's A operand")
        if st == "lora_du":
            _same(c.a["gelu_u"], g.a["gelu_bwd_u"], w + " gelu_u = the GEMM's gelu_bwd_u")
        else:
            assert c.a["gelu_u"] is None, w + ": gelu_u outside the FFN-down seam"
        f = fwd.get(l, {})
        want = {"lora_du": lambda: f["g"].ret, "lora_dy1": lambda: f["ln1"].ret[0], "lora_dctx": lambda: f["attn_fwd"].ret[0]}[st]()
        _same(root(c.a["x"]), want, w + " x = the layer's forward " + {"lora_du": "g", "lora_dy1": "ln1 output", "lora_dctx": "attention context"}[st])
        on_gather = c.a["x"].region() in gathered
        assert (c.a["h"] is None) == on_gather, w + (": h handed in with gathered operands" if on_gather else ": h = None on full rows")
        if not on_gather:
            ho = fad.get(l, {}).get(t)
            assert ho is not None and ho.a["h_out"] is not None, w + ": the layer's forward adapter kept no h"
            _same(c.a["h"], ho.a["h_out"], w + " h = what the layer's forward adapter wrote")
            assert c.a["h"].shape[0] <= ho.a["h_out"].shape[0] and c.a["h"].shape[0] == c.a["dy"].shape[0], w + ": h is no leading-row view of h_out"
        assert c.a["accumulate"] is True, w + ": accumulate is not True"
        dl = model._lw[l].get("lora_dense")
        assert dl is not None and t in dl["targets"], w + ": the layer has no such adapter"
        for k, pk in (("gA", "pA"), ("gB", "pB")):
            p = dl.get(pk, {}).get(t)
            if p is not None:
                assert (c.a[k] is not None) == bool(p.requires_grad), w + f": {k} handed in = {c.a[k] is not None}, requires_grad = {bool(p.requires_grad)}"
            if c.a[k] is None:
                continue
            v = dl[k][t]
            assert c.a[k].ptr == v.data_ptr() and c.a[k].shape == tuple(v.shape), w + f": {k} is not the layer's gradient view of the adapter"
            if p is not None:
                assert p.grad is not None and p.grad.data_ptr() == v.data_ptr(), w + f": {k} is not the .grad of its parameter"
    return n


def check_dataflow(calls, model):
    """All six checks of the module docstring; returns (forward / backward passes seen, dropout sites seen)."""
    names = annotate(calls, model)
    L = len(model._lw)
    n = 0
    for c in calls:                                              # the forward pass a call belongs to (dropout sites are per pass)
        if c.op == "embed_gather":
            n += 1
        c.meta["pass"] = n
    passes = check_sequence(calls, L)
    expect, _ran = check_seam(calls, model)
    check_producers(calls, expect)
    _wiring(calls, names, L)
    check_kv_len(calls)
    check_transposes(calls, names, model)
    sites = check_dropout_sites(calls)
    check_grad_views(calls, names, model)
    check_dense_adapter_wiring(calls, model)
    return passes, sites


_MODE_KEY = {"w1": "W1", "w2": "W2", "qkv": "Wqkv", "o": "Wo"}


def expected_wgrad_problems(plan, L):
    """The gradient views the step's weight-gradient problems write, from the plan alone (None: nothing frozen): the weights whose mode
    is "full", the MLM transform, and the tied table iff ``word_table``."""
    from msa_amd import freeze as FZ
    if plan is None:
        return {f"l{i}.g_{k}" for i in range(L) for k in _MODE_KEY.values()} | {"g_Wt", "g_word_pad"}
    out = {f"l{i}.g_{_MODE_KEY[key]}" for i, modes in plan.layers.items() for key, m in modes.items() if m == FZ.FULL} | {"g_Wt"}
    return out | ({"g_word_pad"} if plan.word_table else set())


def _extent(r: Rec):
    """[first, last + 1) of the storage elements a recorded view covers."""
    if not all(r.shape):
        return r.off, r.off
    return r.off, r.off + sum((n - 1) * st for n, st in zip(r.shape, r.stride)) + 1


def check_frozen_writes(calls, names, plan, L, grads, offset, numel, backward=True):
    """Exact: no recorded call writes into the part of the flat gradient buffer ``grads`` that belongs to a parameter the plan has
    frozen -- every region a call wrote (``post``, ``ret``) inside that buffer lies in trainable spans or in the padding between
    parameters -- and the weight-gradient problems written are exactly ``expected_wgrad_problems``.  ``grads``: the buffer (its storage
    address and size are all that is used; a ``Rec`` will do), ``offset`` / ``numel``: the storage's maps.  The adapters' gradients count like
    any other write: ``gA`` / ``gB`` of ``lora_qkv_bwd`` and of ``lora_dense_bwd``.  ``backward`` False (a forward under ``no_grad``): no
    weight-gradient problem at all.  Returns the number of write regions inside the buffer."""
    g = grads if isinstance(grads, Rec) else Rec(grads, False)
    frozen = sorted((offset[n], offset[n] + numel[n], n) for n in (plan.frozen if plan is not None else ()) if numel[n] > 0)
    inside = 0
    for c in calls:
        for r in list(_recs(list(c.post.values()))) + list(_recs(c.ret)):
            if r.sptr != g.sptr or r.dtype != g.dtype or not r.sbytes:
                continue
            lo, hi = _extent(r)
            inside += 1
            for a, b, n in frozen:
                assert hi <= a or lo >= b, (f"call {c.index} ({c.op}, stage {c.meta.get('stage')} layer {c.meta.get('layer')}) writes elements "
                                            f"[{max(lo, a)}, {min(hi, b)}) of the gradient buffer: the span of the frozen {n}")
    wrote = set()
    for c in calls:
        if c.op in ("gemm_tn_grouped", "gemm_tn"):
            for W in ([p[2] for p in c.a["problems"]] if c.op == "gemm_tn_grouped" else [c.a["W"]]):
                n = _name(names, W, {"g_" + k for k in _MODE_KEY.values()} | {"g_Wt", "g_word_pad"})
                assert n is not None, f"call {c.index} ({c.op}): a weight-gradient problem writes no gradient view of the model"
                wrote.add(n)
    want = expected_wgrad_problems(plan, L) if backward else set()
    assert wrote == want, f"weight-gradient problems written: unexpected {sorted(wrote - want)}, missing {sorted(want - wrote)}"
    return inside


def check_dataflow_frozen(calls, model, plan, lora=None, backward=True):
    """The dataflow checks for a step under a freeze.TrainablePlan and / or adapters (``lora`` = model._lora): the frozen form of check 1,
    checks 2 (``check_producers``), ``check_kv_len``, 4 (``check_transposes``) and 5 (``check_dropout_sites``) unchanged,
    ``check_dense_adapter_wiring`` and ``check_frozen_writes``.  ``backward`` False: a forward under ``no_grad``, no backward stage may run.  ``_wiring`` and ``check_grad_views`` (checks 3 and 6) assume a full backward and are NOT part of it.
    Returns (passes, dropout sites, write regions inside the gradient buffer)."""
    names = annotate(calls, model)
    L = len(model._lw)
    n = 0
    for c in calls:
        if c.op == "embed_gather":
            n += 1
        c.meta["pass"] = n
    stop = 0 if plan is None else plan.stop
    passes = check_sequence(calls, L, stop, plan is not None and not plan.embedding_stage, lora or (), backward)
    expect, _ran = check_seam(calls, model)
    check_producers(calls, expect)
    check_kv_len(calls)
    check_transposes(calls, names, model)
    sites = check_dropout_sites(calls)
    check_dense_adapter_wiring(calls, model)
    f = model._flat
    return passes, sites, check_frozen_writes(calls, names, plan, L, f.grads, f.offset, f.numel, backward)


def check_accumulation(calls, names):
    """The weight-gradient launches of the recording: {gradient name: [accumulate flag per write, in issue order]} -- and every write
    that accumulates starts from what the previous writer left (part of check 2), every write that does not starts a new sum."""
    out = {}
    for c in calls:
        if c.op == "gemm_tn_grouped":
            for p, acc in zip(c.a["problems"], tn_flags(c)):
                for n in names.get(p[2].ptr, [None]):
                    out.setdefault(n, []).append(acc)
        elif c.op == "gemm_tn":
            for n in names.get(c.a["W"].ptr, [None]):
                out.setdefault(n, []).append(bool(c.a["accumulate"]))
    return out


def check_tied_word_gradient(calls):
    """The gradient with two producers per backward pass -- the tied decoder's weight gradient (a weight-gradient problem of the MLM head)
    and the embedding lookup's rows added onto it (embed_scatter) -- against the float64 sum over BOTH stages' recorded operands: the
    scatter's reference started from the EXACT value of the decoder product instead of the fp32 buffer it found, its bound widened by
    that product's own bound (gemm_ref.tn: accumulation term + the fp32 rounding of its output).  Returns the worst ratio per pass."""
    out = []
    for c in calls:
        if c.op in ("gemm_tn_grouped", "gemm_tn"):
            probs = c.a["problems"] if c.op == "gemm_tn_grouped" else [(c.a["A"], c.a["B"], c.a["W"], c.a["bias_out"])]
            flags = tn_flags(c) if c.op == "gemm_tn_grouped" else [bool(c.a["accumulate"])]
            c.meta["_probs"] = list(zip(probs, flags))
        elif c.op == "embed_scatter" and c.a["gword"] is not None:
            gw = c.a["gword"]
            src = None
            for q in calls[:c.index][::-1]:
                for p, acc in q.meta.get("_probs", []):
                    if p[2].ptr == gw.ptr:
                        src = (p, acc)
                        break
                if src is not None:
                    break
            assert src is not None, "embed_scatter: no decoder weight-gradient problem wrote the tied table's gradient before it"
            (A_, B_, W0, _b), acc = src
            tn = G.tn(_c(A_), _c(B_), W0=_c(W0), accumulate=acc)["W"]
            Vr = gw.shape[0]
            ref = E.scatter(_c(c.a["ids"]).reshape(-1), None if c.a["tts"] is None else _c(c.a["tts"]).reshape(-1), _c(c.a["d"]), c.a["T"],
                            tn.val[:Vr], _c(c.a["gtype"]), _c(c.a["gpos"]), det=bool(c.meta.get("det")))["gword"]
            rows = ref.rows
            more = tn.acc[rows] + G.C_OUT * G.U_F32 * tn.val[rows].abs() / (G.C_ACC * G.EPS24)
            out.append(E.check(_c(c.post["gword"]), R.Ref(ref.val, ref.acc + more, 0.0, R.U_F32, rows, None), "tied word gradient, both producers").worst)
    return out
