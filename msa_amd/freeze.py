"""Which work of a train step runs when some parameters have ``requires_grad == False``.

``trainable_plan`` is a pure function of ``{name: trainable}``, the layer count and the flat storage's offset / numel maps: it needs no
GPU and no model.  The model reads the flags at every forward (``_GpuModelBase._read_trainable``), keeps the record of the last distinct
set and hands it to the trunk and the MLM head of that forward; their backward uses the record its forward saw.
"""
from __future__ import annotations

import re
from types import MappingProxyType
from typing import Dict, Mapping, NamedTuple, Optional

from .flat import ALIGN, FROZEN as NEVER       # (the block size of the flat buffer; the parameters the reference never differentiates)

WORD = "bert.embeddings.word_embeddings.weight"
_LAYER = re.compile(r"bert\.encoder\.layer\.(\d+)\.")

# the four weight-gradient problems of an encoder layer: key -> (weight names, bias names) below "bert.encoder.layer.<i>."
PROBLEMS = {
    "w1": (("intermediate.dense.weight",), ("intermediate.dense.bias",)),
    "w2": (("output.dense.weight",), ("output.dense.bias",)),
    "qkv": (tuple(f"attention.self.{x}.weight" for x in ("query", "key", "value")), tuple(f"attention.self.{x}.bias" for x in ("query", "key", "value"))),
    "o": (("attention.output.dense.weight",), ("attention.output.dense.bias",)),
}
FULL, BIAS, NONE = "full", "bias", "none"


class TrainablePlan(NamedTuple):
    """``first_layer`` = b, the lowest encoder layer with a trainable parameter (L: none).  ``embedding_stage``: whether the embedding
    stage's backward runs (a ``bert.embeddings.*`` or differentiated ``bert.jointEmbeddings.*`` parameter is trainable).  ``stop``: the
    lowest layer whose backward runs -- b when the embedding stage does not run, else 0; layer ``stop`` computes no input gradient when
    the embedding stage does not run.  ``layers[i]`` for every running layer: {"qkv" | "o" | "w1" | "w2": "full" (the weight-gradient
    problem runs, bias riding on it) | "bias" (no weight-gradient tile; the bias gradient comes from the grouped column sum) | "none"}.
    ``word_table``: whether the tied word-embedding table's gradient runs (the MLM decoder's weight gradient, the word rows of the
    embedding scatter).  ``frozen``: the names whose ``.grad`` is None."""
    first_layer: int
    embedding_stage: bool
    stop: int
    layers: Mapping[int, Mapping[str, str]]
    word_table: bool
    frozen: frozenset


def never_trainable(name: str) -> bool:
    return any(name.startswith(f) for f in NEVER)


def check_packed_neighbours(trainable: Mapping[str, bool], offset: Mapping[str, int], numel: Mapping[str, int]) -> None:
    """A 256-element block of the flat buffer holds ONE decision (the optimizer's per-block flags): packed neighbours that share a block
    (the q / k / v biases and a LayerNorm's weight and bias below H = 256; the q / k / v weights when H * H % 256 != 0) and differ in
    ``requires_grad`` raise NotImplementedError naming both."""
    names = sorted((n for n in offset if numel[n] > 0 and not never_trainable(n)), key=lambda n: offset[n])
    for a, b in zip(names, names[1:]):
        if (offset[a] + numel[a] - 1) // ALIGN >= offset[b] // ALIGN and bool(trainable[a]) != bool(trainable[b]):
            fa, fb = (("trainable", "frozen") if trainable[a] else ("frozen", "trainable"))
            raise NotImplementedError(f"requires_grad: {a} ({fa}) and {b} ({fb}) share a 256-element block of the flat buffer (packed "
                                      "neighbours): freeze or unfreeze them together")


def trainable_plan(trainable: Mapping[str, bool], L: int, offset: Mapping[str, int], numel: Mapping[str, int]) -> Optional[TrainablePlan]:
    """The record for the set ``trainable`` ({parameter name: requires_grad}), or None when every parameter is trainable (the step then
    makes the launches it always made).  The flat.FROZEN parameters are never trainable whatever their flag says: they decide no work, and
    are in ``frozen`` (their ``.grad`` reads None) when their flag is False."""
    frozen = frozenset(n for n, t in trainable.items() if not t)
    if not frozen:
        return None
    tr: Dict[str, bool] = {n: bool(t) for n, t in trainable.items() if not never_trainable(n)}
    check_packed_neighbours(tr, offset, numel)
    b = L
    for n, t in tr.items():
        m = _LAYER.match(n)
        if t and m:
            b = min(b, int(m.group(1)))
    embedding_stage = any(t for n, t in tr.items() if n.startswith("bert.embeddings.") or n.startswith("bert.jointEmbeddings."))
    stop = 0 if embedding_stage else b
    layers = {}
    for i in range(stop, L):
        p = f"bert.encoder.layer.{i}."
        modes = {}
        for key, (ws, bs) in PROBLEMS.items():
            if any(tr.get(p + w, False) for w in ws):
                modes[key] = FULL
            elif any(tr.get(p + x, False) for x in bs):
                modes[key] = BIAS
            else:
                modes[key] = NONE
        layers[i] = MappingProxyType(modes)
    return TrainablePlan(b, embedding_stage, stop, MappingProxyType(layers), bool(tr.get(WORD, False)), frozen)


def resolve_freeze(names, L: int, *, embeddings=False, layers=0, layer_weights=False):
    """The parameter names ``model.freeze(...)`` affects, among ``names`` (in their order)."""
    if isinstance(layers, bool):
        raise ValueError("freeze: layers is a count k (layers 0 .. k-1) or an iterable of layer indices")
    if isinstance(layers, int):
        if not 0 <= layers <= L:
            raise ValueError(f"freeze: layers={layers} out of range for a model of {L} encoder layers")
        idx = set(range(layers))
    else:
        idx = set()
        for i in layers:
            if not (isinstance(i, int) and 0 <= i < L):
                raise ValueError(f"freeze: layer {i!r} out of range for a model of {L} encoder layers")
            idx.add(i)
    weights = {w for ws, _ in PROBLEMS.values() for w in ws}
    out = []
    for n in names:
        m = _LAYER.match(n)
        if m:
            i = int(m.group(1))
            if i in idx or (layer_weights and n[m.end():] in weights):
                out.append(n)
        elif embeddings and (n.startswith("bert.embeddings.") or n.startswith("bert.jointEmbeddings.")):
            out.append(n)
    return out
