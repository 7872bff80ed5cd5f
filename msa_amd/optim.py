"""AdamW + linear warm-up schedule with the reference's construction API (REF:train.py:76-97),
executed as ONE HIP kernel over the model's flat fp32 buffers (mmbert_adamw): update, weight decay,
bf16 working-copy refresh and zero_grad in a single pass over 28 B/parameter.

``mode="hf"`` (default) is transformers-2.8 ``optimization.AdamW`` -- the class the reference
imports (eps 1e-6, bias correction, decay applied after the update); ``mode="torch"`` is
``torch.optim.AdamW``, the optimizer the golden fixture G8 was generated with.

``LAMB`` is the layer-wise adaptive alternative for large global batches on the same binding (mmbert_lamb: three launches, a trust ratio
per parameter tensor).
"""
from __future__ import annotations

import contextlib
import math
from typing import Iterable, List, Union

import torch

from . import ops
from .flat import FROZEN


def _clip_args(max_norm, norm_type):
    """(max_norm, norm_type) as floats for the native clip; norm_type other than 2 and inf: NotImplementedError."""
    max_norm, norm_type = float(max_norm), float(norm_type)
    if not max_norm >= 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm must be >= 0, got {max_norm}")
    if norm_type != 2.0 and norm_type != math.inf:
        raise NotImplementedError(f"clip_grad_norm_: the native clip takes norm_type 2 or inf, got {norm_type}")
    return max_norm, norm_type


def adamw_slots(hyper):
    """What mmbert_adamw_grouped does with the groups' (lr, beta1, beta2, eps, weight_decay) tuples: groups with equal tuples share a
    slot.  Returns (slot of each group, the distinct tuples in first-seen order); more than ops.ADAMW_MAX_GROUPS groups or
    ops.ADAMW_MAX_SLOTS distinct tuples raise NotImplementedError."""
    hyper = [tuple(float(x) for x in h) for h in hyper]
    if len(hyper) > ops.ADAMW_MAX_GROUPS:
        raise NotImplementedError(f"AdamW: {len(hyper)} param groups, the fused step takes at most {ops.ADAMW_MAX_GROUPS}: "
                                  "merge the groups that share lr, betas, eps and weight_decay")
    index = {}
    slots = [index.setdefault(h, len(index)) for h in hyper]
    if len(index) > ops.ADAMW_MAX_SLOTS:
        raise NotImplementedError(f"AdamW: {len(index)} distinct (lr, betas, eps, weight_decay) combinations in one step, the fused step "
                                  f"takes at most {ops.ADAMW_MAX_SLOTS}: merge groups (e.g. coarser layer-wise lr decay)")
    return slots, list(index)


def ema_decay_at(decay, updates, warmup=False):
    """The decay of EMA update number ``updates`` (0 for the first ``step()`` after the copy that enabling makes): ``decay``, or with
    ``warmup`` ``min(decay, (1 + updates) / (10 + updates))`` -- early averages follow the weights, late ones use ``decay``.  A pure
    host function in double: the kernel only ever sees its value."""
    decay = float(decay)
    return min(decay, (1.0 + updates) / (10.0 + updates)) if warmup else decay


class AdamW:
    kind = "adamw"                          # state_dict()["optimizer"]: load_state_dict refuses another kind's state

    def __init__(self, params: Union[Iterable[torch.nn.Parameter], List[dict]], lr=1e-3, betas=(0.9, 0.999), eps=1e-6,
                 weight_decay=0.0, correct_bias=True, mode="hf"):
        params = list(params)
        if params and isinstance(params[0], dict):
            self.param_groups = [dict(g, params=list(g["params"])) for g in params]
        else:
            self.param_groups = [dict(params=params, weight_decay=weight_decay)]
        for g in self.param_groups:
            g.setdefault("weight_decay", weight_decay)
            g.setdefault("lr", lr)
            g.setdefault("betas", tuple(betas))
            g.setdefault("eps", eps)
            g["initial_lr"] = g["lr"]
        if not correct_bias:
            raise NotImplementedError("correct_bias=False is not used by the reference")
        self.betas, self.eps, self.mode = betas, eps, {"hf": 0, "torch": 1}[mode]
        self.grad_scale = 1.0               # set to 1/world_size by parallel.DataParallel
        self._lazy_zero = True
        self._flat = None
        self._steps = 0
        self._clip = None                   # clip_grad_norm_'s device scalars until the next step() applies them (or zero_grad() drops them)
        self._ema = None                    # fp32 average of flat.params (ema(): +4 B/parameter), updated inside the step's kernel
        self._ema_decay, self._ema_warmup, self.ema_updates = None, False, 0
        self._swapped = False               # swap_ema(): flat.params holds the averages, _ema the trained weights

    # The dense weights' gradients (3/4 of the parameters) are not zero-filled between steps: the next backward's weight-gradient
    # launches overwrite them (flat.FlatParams lazy zero; torch's zero_grad(set_to_none=True) semantics).  False: fill with zeros.
    # A plain switch at ANY time (as an attribute it was baked into the kernel's flag array at the first step, and turning it
    # off later left the fused zero_grad skipping blocks whose gradients were then accumulated into for ever): the setter rebuilds the
    # flag array, and only blocks this optimizer owns ever carry the "leave it to the next backward" bit.
    @property
    def lazy_zero(self) -> bool:
        return self._lazy_zero

    @lazy_zero.setter
    def lazy_zero(self, on: bool):
        on = bool(on)
        if on != self._lazy_zero:
            self._lazy_zero = on
            if self._flat is not None:
                self._build_flags()

    def _build_flags(self):
        flags = self._base_flags.clone()
        if self._lazy_zero:
            lazy = self._flat.lazy_block_mask().to(flags.dtype)
            lazy[flags == 2] = 0                 # frozen / not owned by this optimizer: never stepped, so never dropped either
            flags |= lazy                        # + 4: the fused zero_grad leaves these blocks to the next backward's overwriting launches
        self._flags = flags.to(self._flat.device)

    @property
    def lr(self) -> float:
        return self.param_groups[0]["lr"]

    def _hyper(self):
        """(lr, beta1, beta2, eps, weight_decay) of every group, read afresh (schedulers and users change them between steps); keys that
        would change the update but are not implemented raise."""
        out = []
        for i, g in enumerate(self.param_groups):
            for key, bad in (("amsgrad", True), ("maximize", True), ("correct_bias", False)):
                if key in g and bool(g[key]) == bad:
                    raise NotImplementedError(f"AdamW: param group {i} sets {key}={bad}, which the fused AdamW does not implement")
            b1, b2 = g["betas"]
            out.append((float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"])))
        return out

    def _bind(self):
        flat = None
        for g in self.param_groups:
            for p in g["params"]:
                ref = getattr(p, "_mmb_flat", None)
                if ref is None or ref[0] is None:
                    raise RuntimeError("AdamW: parameter is not backed by msa_amd flat storage -- run one forward "
                                       "pass (or model._ensure_ready) on the GPU before the first optimizer step")
                if flat is None:
                    flat = ref[0]
                elif ref[0] is not flat:
                    raise RuntimeError("AdamW: parameters belong to different flat storages")
        self._check_current(flat)
        if len(self.param_groups) > ops.ADAMW_MAX_GROUPS:
            raise NotImplementedError(f"AdamW: {len(self.param_groups)} param groups, the fused step takes at most {ops.ADAMW_MAX_GROUPS}: "
                                      "merge the groups that share lr, betas, eps and weight_decay")
        self._build_maps(flat)               # (first: a refused grouping leaves the optimizer unbound)
        self._m = torch.zeros_like(flat.params)
        self._v = torch.zeros_like(flat.params)
        self._flat = flat
        self._build_flags()
        if self._ema_decay is not None:
            self._ema = flat.params.clone()

    @staticmethod
    def _check_current(flat):
        """Raises when the model's parameters no longer view ``flat`` -- the model built a new storage since (``.to()`` / ``.cuda()`` /
        ``.float()``, ``set_num_labels``, ``parameters_changed()`` after a re-pointed parameter): a step would update buffers that nothing
        reads any more.  One pointer comparison, at every optimizer call, before anything is launched: build a new optimizer then."""
        if not flat.owns_any():
            raise RuntimeError("AdamW: the model was re-materialised (e.g. moved) after this storage was created: its parameters "
                               "live in a new flat storage -- build the optimizer again")

    def _build_maps(self, flat):
        """The kernel's per-block maps: flags (decay bit from each group's weight_decay > 0; blocks this optimizer does not step are
        frozen) and group_of_block.  A 256-element block holds one group: packed neighbours that share a block (the q/k/v biases, a
        LayerNorm's weight and bias; the q/k/v weights when H * H % 256 != 0) in different groups raise.  Listed parameters that the
        model's last forward saw frozen (flat.frozen) are skipped as torch skips ``grad is None``: their blocks stay "not owned"."""
        frozen = self._frozen = flat.frozen
        self._unreached = flat.unreached     # (in ``frozen`` for the steps that do not reach them only: _follow_frozen lets them back)
        self._listed = frozenset(flat.name_at(p._mmb_flat[1]) for g in self.param_groups for p in g["params"])
        flags = flat.flags.clone().cpu()
        flags[flags != 2] = 3                # 3 = not owned by this optimizer -> treated as frozen below
        group = torch.zeros_like(flags)
        owner = torch.full(flags.shape, -1, dtype=torch.int64)      # index into ``names`` of a parameter in the block
        names, gidx, active, decay = [], [], set(), []
        for gi, g in enumerate(self.param_groups):
            decay.append(g["weight_decay"] > 0)
            f = 1 if decay[-1] else 0
            for p in g["params"]:
                _, off = p._mmb_flat
                name = flat.name_at(off)
                if any(name.startswith(fr) for fr in FROZEN) or name in frozen:
                    continue                 # grad is always None in the reference / the parameter is frozen -> optimizer skips it
                b0, b1 = off // 256, (off + p.numel() + 255) // 256
                prev = owner[b0:b1]
                for j in sorted(set(prev[prev >= 0].tolist())):
                    if names[j] == name:
                        raise ValueError(f"AdamW: {name} appears in more than one parameter group")
                    if gidx[j] != gi:
                        raise NotImplementedError(f"AdamW: {names[j]} (param group {gidx[j]}) and {name} (param group {gi}) share a 256-element "
                                                  "block of the flat buffer (packed neighbours): put them in the same param group")
                names.append(name)
                gidx.append(gi)
                owner[b0:b1] = len(names) - 1
                flags[b0:b1] = f
                group[b0:b1] = gi
                active.add(gi)
        flags[flags == 3] = 2
        self._base_flags = flags
        self._group_of_block = group.to(flat.device)
        self._active = sorted(active)
        self._decay = tuple(decay)
        self._names = names                  # the parameters this optimizer steps (clip_grad_norm_ measures these)

    def _follow_frozen(self):
        """The model's frozen set changed since the maps were built: rebuilt.  Freezing more parameters keeps their m and v; a parameter
        of this optimizer that became trainable after the first step() raises.  Parameters a label-only step does not reach
        (flat.unreached: gradient None for that step) are skipped the same way -- p, m, v, the bf16 copies and the EMA keep their bits, no
        weight decay, no moment decay -- and come back without raising: their m and v are the ones they had, under the shared step count."""
        flat = self._flat
        if flat.frozen == self._frozen:
            return
        back = sorted(n for n in ((self._frozen - self._unreached) - flat.frozen) & self._listed if not any(n.startswith(fr) for fr in FROZEN))
        if back and self._steps > 0:
            raise NotImplementedError(f"AdamW: {back[0]}" + (f" (and {len(back) - 1} more)" if len(back) > 1 else "") + " became trainable after this "
                                      "optimizer's first step(): the fused step keeps ONE step count for all parameters, so the parameter's "
                                      "bias correction would be wrong -- build a new optimizer")
        self._build_maps(flat)
        self._build_flags()

    def clip_grad_norm_(self, max_norm, norm_type=2.0) -> torch.Tensor:
        """Global gradient-norm clipping fused into the next ``step()``: returns the total norm (0-d fp32 device tensor) of the gradient
        that step will apply -- this optimizer's parameters except flat.FROZEN, times ``grad_scale`` (under DataParallel the mean over
        ranks) -- and has the step multiply every gradient by ``min(1, max_norm / (norm + 1e-6))`` as the AdamW kernel reads it.
        Unlike ``torch.nn.utils.clip_grad_norm_``, ``.grad`` is NOT modified: the coefficient stays on the device until ``step()``
        applies it (one reduction pass, no host sync, no write pass).  A second call before ``step()`` replaces the coefficient;
        ``zero_grad()`` without a step drops it.  norm_type: 2 or inf."""
        max_norm, norm_type = _clip_args(max_norm, norm_type)
        self._refuse_swapped("clip_grad_norm_()")
        if self._flat is None:
            self._bind()
        flat = self._flat
        self._check_current(flat)
        flat.join_side_writers()             # (see step(): nothing may still add into the gradients read here)
        flat.reconcile_grads()               # a .grad the caller set to None counts as zero
        flat.settle()                        # a dropped lazy gradient counts as zero
        self._follow_frozen()                # (frozen parameters are left out of the norm)
        segs, nseg = flat.segments(self._names, FROZEN)
        out = ops.grad_norm(flat.grads, segs, nseg, max_norm=max_norm, norm_type=norm_type, gscale=self.grad_scale,
                            workspace=flat.norm_workspace())
        self._clip = out
        return out[0]

    # ---- exponential moving average of the weights ----
    def ema(self, decay=0.999, warmup=False):
        """Keeps an fp32 exponential moving average of the flat parameters, updated inside every ``step()``'s kernel (mmbert_adamw_ema:
        +8 B/parameter of traffic, no launch, no sync; p, m, v and the bf16 copy keep the bits they have without it).  The average starts
        as a copy of the parameters -- at once when the optimizer is bound, else at its first use -- which is
        ``torch.optim.swa_utils.AveragedModel``'s first ``update_parameters``; every step then does ``ema += (1 - d) (p - ema)`` with
        ``d = ema_decay_at(decay, ema_updates, warmup)``.  Called again it changes ``decay`` / ``warmup`` and keeps the average.
        Frozen parameters and those this optimizer does not own keep their copy.  Under parallel.DataParallel nothing is exchanged: equal
        parameters on every rank give equal averages.  Returns self."""
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"AdamW.ema: decay must be in [0, 1), got {decay}")
        self._ema_decay, self._ema_warmup = decay, bool(warmup)
        if self._flat is not None and self._ema is None:
            self._ema = self._flat.params.clone()
        return self

    def ema_reset(self):
        """Starts the average again from the current parameters (after a ``load_state_dict`` into the model)."""
        self._refuse_swapped("ema_reset()")
        self.ema_updates = 0
        if self._ema is not None:
            self._ema.copy_(self._flat.params)

    def _refuse_swapped(self, what):
        if self._swapped:
            raise RuntimeError(f"AdamW.{what} while the EMA weights are swapped in (swap_ema() / ema_weights()): the averages are not "
                               "trained -- swap back first")

    def _need_ema(self, what):
        if self._ema_decay is None:
            raise RuntimeError(f"AdamW.{what}: no EMA -- call ema(decay) first")
        if self._flat is None:
            self._bind()
        self._check_current(self._flat)

    def swap_ema(self):
        """Exchanges the parameters with their averages in place (one launch that also rewrites the bf16 working copy; the transposed
        copies follow): every path of the model -- forward, predict, predict_tokens, state_dict() -- then sees the averaged weights,
        until the next call swaps back, bit for bit.  Version counters, m / v, the gradients and the lazy-zero state are untouched.
        While swapped, step(), clip_grad_norm_() and state_dict() raise."""
        self._need_ema("swap_ema()")
        flat = self._flat
        flat.join_side_writers()
        flat.wait_transposes()               # (a side-stream transposed-copy launch may still read the bf16 copy rewritten here)
        ops.ema_swap(flat.params, self._ema, flat.half)
        flat.refresh_transposes()
        flat.mark_synced()
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """``with opt.ema_weights():`` -- the model runs on the averaged weights inside, on the trained ones again after (swap_ema twice)."""
        self._refuse_swapped("ema_weights()")
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def ema_state_dict(self):
        """The averaged weights under the model's ``state_dict()`` keys, as clones (buffers and anything outside the flat storage as the
        model holds them); nothing is swapped."""
        self._need_ema("ema_state_dict()")
        flat = self._flat
        model = flat._owner()
        if model is None:
            raise RuntimeError("AdamW.ema_state_dict(): the model of this storage is gone")
        src = flat.params if self._swapped else self._ema
        base, out = flat.params.data_ptr(), {}
        for k, t in model.state_dict().items():
            o = t.data_ptr() - base
            if t.dtype == torch.float32 and t.is_contiguous() and t.numel() > 0 and 0 <= o and o + 4 * t.numel() <= 4 * flat.total:
                out[k] = src[o // 4:o // 4 + t.numel()].view(t.shape).clone()
            else:
                out[k] = t.clone()
        return out

    def step(self):
        self._refuse_swapped("step()")
        hyper = self._hyper()
        if self._flat is None:
            self._bind()
        self._check_current(self._flat)
        self._follow_frozen()
        if tuple(h[4] > 0 for h in hyper) != self._decay:
            self._build_maps(self._flat)     # a group's weight_decay turned on or off since the flags were built
            self._build_flags()
        launch = self._plan(hyper)           # (the limits: raise before anything is launched)
        flat = self._flat
        self._steps += 1
        flat.join_side_writers()             # (left by a backward that raised: nothing may still add into the gradients the kernel reads and zeroes)
        flat.wait_transposes()               # (a step without a backward in between: the last step's transposed copies still read the bf16 copy)
        flat.reconcile_grads()               # a .grad the caller set to None counts as zero
        flat.settle()                        # a lazy gradient no backward has written since the last step counts as zero
        flat.attach_lazy()
        clip, self._clip = self._clip, None
        launch(clip)
        flat.refresh_transposes(side=True)
        flat.mark_synced()
        flat.grads_dirty = False
        if self.lazy_zero:
            flat.drop_lazy()

    def _plan(self, hyper):
        """Which kernel this step's update is, from the groups' hyper-parameters: checks the limits and returns the function of the clip
        scalars (or None) that launches it, once step() has settled the gradients.  The part of step() a subclass replaces (LAMB)."""
        act = [hyper[i] for i in self._active] or hyper[:1]
        wds = {h[4] for h in act if h[4] > 0}
        grouped = any(h[:4] != act[0][:4] for h in act) or len(wds) > 1
        if grouped:
            adamw_slots(hyper)
        lr, beta1, beta2, eps, _ = act[0]
        wd = wds.pop() if wds else 0.0
        return lambda clip: self._launch(hyper, grouped, lr, beta1, beta2, eps, wd, clip)

    def _launch(self, hyper, grouped, lr, beta1, beta2, eps, wd, clip):
        flat = self._flat
        if self._ema is not None:            # the same update with the weight average folded in: one kernel for the three routes below
            ops.adamw_ema(flat.params, flat.grads, self._m, self._v, flat.half, self._flags, self._group_of_block if grouped else None,
                          hyper if grouped else [(lr, beta1, beta2, eps, wd)], self._ema,
                          ema_decay=ema_decay_at(self._ema_decay, self.ema_updates, self._ema_warmup), step=self._steps,
                          gscale=self.grad_scale, coef=None if clip is None else clip[2:3], mode=self.mode, zero_grad=True)
            self.ema_updates += 1
        elif grouped:                        # per-group hyper-parameters: each block reads its own group's coefficients
            ops.adamw_grouped(flat.params, flat.grads, self._m, self._v, flat.half, self._flags, self._group_of_block, hyper,
                              step=self._steps, gscale=self.grad_scale, coef=None if clip is None else clip[2:3], mode=self.mode,
                              zero_grad=True)
        elif clip is None:                   # one set for every group (the reference's two groups): the single-set kernel
            ops.adamw(flat.params, flat.grads, self._m, self._v, flat.half, self._flags, lr=lr, beta1=beta1, beta2=beta2, eps=eps, wd=wd,
                      step=self._steps, gscale=self.grad_scale, mode=self.mode, zero_grad=True)
        else:                                # clip_grad_norm_ ran: its coefficient (x grad_scale) from the device
            ops.adamw_devscale(flat.params, flat.grads, self._m, self._v, flat.half, self._flags, clip[2:3], lr=lr, beta1=beta1,
                               beta2=beta2, eps=eps, wd=wd, step=self._steps, mode=self.mode, zero_grad=True)

    def zero_grad(self, set_to_none: bool = False):
        self._clip = None                    # a clip coefficient no step() applied belongs to the gradients dropped here
        flat = self._flat
        if flat is None:
            # (not bound before the first step(); the parameters may already live in a model's flat storage: join its side streams first)
            refs = (getattr(p, "_mmb_flat", None) for g in self.param_groups for p in g["params"])
            storage = next((r[0] for r in refs if r is not None), None)
            if storage is not None:
                storage.join_side_writers()
            for g in self.param_groups:
                for p in g["params"]:
                    if p.grad is not None:
                        p.grad.zero_()
            return
        self._check_current(flat)
        flat.join_side_writers()             # (left by a backward that raised: see step())
        if flat.grads_dirty:                 # step() already zeroed the buffer in the same kernel
            flat.grads.zero_()
            flat.grads_dirty = False
            flat.stale.clear()
            flat.attach_lazy()
        else:
            flat.detach_lazy()               # the dropped gradients read None (torch: set_to_none) until the next backward writes them

    def state_dict(self):
        self._refuse_swapped("state_dict()")
        return dict(optimizer=self.kind, steps=self._steps, m=None if self._flat is None else self._m, v=None if self._flat is None else self._v,
                    lrs=[g["lr"] for g in self.param_groups], ema=self._ema, ema_decay=self._ema_decay, ema_warmup=self._ema_warmup,
                    ema_updates=self.ema_updates)

    def load_state_dict(self, sd):
        self._refuse_swapped("load_state_dict()")
        if sd.get("optimizer", self.kind) != self.kind:      # (a dict from before the key existed is an AdamW's or the caller's business)
            raise ValueError(f"{type(self).__name__}.load_state_dict: the state is a {sd['optimizer']!r} optimizer's, this one is {self.kind!r}: "
                             "m and v mean the same, the step they were taken with does not")
        if self._flat is None:
            self._bind()
        if sd.get("ema_decay") is not None:  # (a dict without the ema keys, or saved with the EMA off, leaves the EMA as it is)
            self.ema(sd["ema_decay"], sd.get("ema_warmup", False))
            self.ema_updates = int(sd.get("ema_updates", 0))
            if sd.get("ema") is not None:
                self._ema.copy_(sd["ema"])
        self._steps = sd["steps"]
        if sd["m"] is not None:
            self._m.copy_(sd["m"])
            self._v.copy_(sd["v"])
        for g, lr in zip(self.param_groups, sd["lrs"]):
            g["lr"] = lr


LAMB_MIXED_ENTRIES = 4                     # (first quad, unit) pairs of one mixed-block record (include/mmbert_hip.h, mmbert_lamb)


def lamb_unit_maps(spans, nblk, others=()):
    """mmbert_lamb's maps of trust units onto 256-element blocks, on the host (numpy int32): ``spans[T]`` = (offset, length) in elements
    of unit T, disjoint; ``others``: spans of tensors that are in no unit (not stepped) but may share a block with one.  Returns
    (unit_of_block [nblk], mixed [nmixed, 8], ranges [nunits, 2]).  A block that one unit has to itself from its first element (whatever
    follows the unit's end is padding) is pure: its entry is the unit.  Any other block that holds a unit gets -(k + 1) and record k:
    (first quad, unit) pairs in ascending order, -1 for a stretch of ``others``, padding joined to the stretch before it, unused pairs
    (64, -1).  Record 0 is "no unit" alone: every block without a unit names it (frozen blocks are not looked up at all).  A unit that starts
    inside a block off a multiple of 4 elements raises ValueError, more than LAMB_MIXED_ENTRIES stretches in one block NotImplementedError."""
    import numpy as np
    pieces, whole = {}, []
    for unit, (off, length) in [(t, s) for t, s in enumerate(spans)] + [(-1, s) for s in others]:
        off, length = int(off), int(length)
        if length <= 0:
            continue
        if off < 0 or off + length > nblk * 256:
            raise ValueError(f"lamb_unit_maps: span ({off}, {length}) outside the {nblk} blocks")
        first, start, end = off // 256, off % 256, off + length
        if start % 4:
            raise ValueError(f"lamb_unit_maps: span ({off}, {length}) starts inside block {first} at element {start}, not a multiple of 4")
        lo, hi = first + (1 if start else 0), end // 256       # the blocks [lo, hi) are the span's from their first to their last element
        if hi > lo:
            whole.append((lo, hi, unit))
        if start:
            pieces.setdefault(first, []).append((start // 4, unit))
        if end % 256 and (hi > first or not start):
            pieces.setdefault(hi, []).append((0, unit))
    records = [[0, -1] + [64, -1] * (LAMB_MIXED_ENTRIES - 1)]                     # record 0: "no unit", shared
    unit_of_block = np.full(nblk, -1, dtype=np.int32)
    taken = np.zeros(nblk, dtype=bool)
    for lo, hi, unit in whole:
        if taken[lo:hi].any():
            raise ValueError(f"lamb_unit_maps: overlapping spans in blocks {lo} .. {hi - 1}")
        taken[lo:hi] = True
        unit_of_block[lo:hi] = unit                                                # (-1 for ``others``: record 0)
    for b in sorted(pieces):
        ps = sorted(pieces[b])
        if taken[b] or any(a[0] == c[0] for a, c in zip(ps, ps[1:])):
            raise ValueError(f"lamb_unit_maps: overlapping spans in block {b}")
        if ps[0][0] > 0:
            ps.insert(0, (0, -1))
        ps = [x for j, x in enumerate(ps) if j == 0 or x[1] >= 0 or ps[j - 1][1] >= 0]         # neighbouring "no unit" stretches are one
        if len(ps) == 1 and ps[0][1] >= 0:
            unit_of_block[b] = ps[0][1]
        elif any(u >= 0 for _, u in ps):
            if len(ps) > LAMB_MIXED_ENTRIES:
                raise NotImplementedError(f"LAMB: block {b} of the flat buffer holds {len(ps)} stretches of different tensors, the fused step "
                                          f"takes {LAMB_MIXED_ENTRIES}")
            unit_of_block[b] = -(len(records) + 1)
            records.append([x for q in ps for x in q] + [64, -1] * (LAMB_MIXED_ENTRIES - len(ps)))
    mixed = np.asarray(records, dtype=np.int32).reshape(-1, 2 * LAMB_MIXED_ENTRIES)
    ranges = np.asarray([(o // 256, (o + k + 255) // 256) if k > 0 else (0, 0) for o, k in spans], dtype=np.int32).reshape(-1, 2)
    return unit_of_block, mixed, ranges


class LAMB(AdamW):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning", Algorithm 2 with bias correction; apex ``FusedLAMB``'s defaults) on
    AdamW's binding to the flat storage: the same flags, lazy zero, frozen and unreached parameters, per-group hyper-parameters,
    ``clip_grad_norm_`` / ``grad_scale``, EMA, ``zero_grad`` and schedulers.  Per element ``u = mhat / (sqrt(vhat) + eps) + wd p``; per
    parameter tensor ``r = ||p|| / ||u||`` (1 when either norm is 0, and for tensors of a group with weight_decay 0 unless
    ``always_adapt``), capped at ``max_trust`` when given; ``p -= lr r u``.  One step is mmbert_lamb's three launches, no host sync."""
    kind = "lamb"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, always_adapt=False, max_trust=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        if max_trust is not None and not float(max_trust) > 0.0:
            raise ValueError(f"LAMB: max_trust must be > 0 or None, got {max_trust}")
        self.always_adapt, self.max_trust = bool(always_adapt), None if max_trust is None else float(max_trust)
        self._ratios_valid = False

    def _build_maps(self, flat):
        """AdamW's per-block maps, then the trust units: one per stepped parameter, in the order of ``self._names``."""
        super()._build_maps(flat)
        names = self._names
        group_of = {flat.name_at(p._mmb_flat[1]): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
        live = (self._base_flags != 2).tolist()
        stepped = set(names)
        others = [(flat.offset[n], flat.numel[n]) for n in flat.order if n not in stepped and flat.numel[n] > 0
                  and any(live[flat.offset[n] // 256:(flat.offset[n] + flat.numel[n] - 1) // 256 + 1])]
        unit_of_block, mixed, ranges = lamb_unit_maps([(flat.offset[n], flat.numel[n]) for n in names], flat.total // 256, others)
        units = torch.zeros(max(len(names), 1), 4, dtype=torch.int32)
        for t, n in enumerate(names):
            units[t, 0], units[t, 1] = int(ranges[t][0]), int(ranges[t][1])
            units[t, 2] = 1 if (self.always_adapt or self.param_groups[group_of[n]]["weight_decay"] > 0) else 0
        dev = flat.device
        self._unit_of_block = torch.from_numpy(unit_of_block).to(dev)
        self._mixed = torch.from_numpy(mixed).to(dev)
        self._units = units.to(dev)
        self._ratios = torch.zeros(units.shape[0], 3, dtype=torch.float32, device=dev)
        self._lamb_ws = torch.empty(max(ops.lamb_workspace_bytes(flat.total // 256, len(mixed)) // 4, 2), dtype=torch.float32, device=dev)
        self._ratios_valid = False

    def _plan(self, hyper):
        adamw_slots(hyper)                   # (mmbert_lamb's limits are the grouped AdamW's)
        return lambda clip: self._launch_lamb(hyper, clip)

    def _launch_lamb(self, hyper, clip):
        flat, ema = self._flat, self._ema
        ops.lamb(flat.params, flat.grads, self._m, self._v, flat.half, self._flags, self._group_of_block, hyper, self._unit_of_block,
                 self._mixed, self._units, step=self._steps, gscale=self.grad_scale, coef=None if clip is None else clip[2:3],
                 zero_grad=True, max_trust=self.max_trust, ratios=self._ratios, workspace=self._lamb_ws, ema=ema,
                 ema_decay=0.0 if ema is None else ema_decay_at(self._ema_decay, self.ema_updates, self._ema_warmup))
        if ema is not None:
            self.ema_updates += 1
        self._ratios_valid = True

    def trust_ratios(self):
        """{parameter name: (trust ratio, ||p||, ||u||)} of the last ``step()`` as Python floats, for the parameters that step updated
        (frozen and unreached ones are absent); {} before the first step.  Reads the device: the one call here that syncs."""
        if self._flat is None or not self._ratios_valid:
            return {}
        rows = self._ratios.cpu().tolist()
        return {n: tuple(rows[t]) for t, n in enumerate(self._names)}


_NO_DECAY = ("bias", "LayerNorm.bias", "LayerNorm.weight")               # REF:train.py:78 (trainer.build_optimizer)


def layerwise_param_groups(model, lr, *, weight_decay=0.01, layer_decay=1.0, head_lr=None):
    """AdamW param groups for fine-tuning from a BERT checkpoint with layer-wise learning-rate decay.  Encoder layer i of L gets
    ``lr * layer_decay ** (L - i)``, ``bert.embeddings.*`` ``lr * layer_decay ** (L + 1)``, ``bert.pooler.*`` ``lr``; everything a BERT
    checkpoint does not carry (``bert.jointEmbeddings.*``, ``cls.*``, the fusion head ``classifier1_*`` / ``attn`` / ``vt`` / ``vv`` /
    ``vs``, the ``cpc_*`` nets) gets ``head_lr`` (default ``lr``).  Weight decay follows the reference's rule by name (none for biases
    and LayerNorm parameters).  Parameters with the same (lr, weight_decay) share one group, in the order of ``named_parameters()``:
    with the defaults that is exactly trainer.build_optimizer's two groups."""
    import re
    named = list(model.named_parameters())
    layer = re.compile(r"bert\.encoder\.layer\.(\d+)\.")
    L = 1 + max((int(m.group(1)) for m in (layer.match(n) for n, _ in named) if m), default=-1)
    head_lr = lr if head_lr is None else head_lr
    groups = {}
    for n, p in named:
        if not p.requires_grad:
            continue                         # frozen (model.freeze / requires_grad_(False)): in no group
        m = layer.match(n)
        if m:
            glr = lr * layer_decay ** (L - int(m.group(1)))
        elif n.startswith("bert.embeddings."):
            glr = lr * layer_decay ** (L + 1)
        elif n.startswith("bert.pooler."):
            glr = lr
        else:
            glr = head_lr
        wd = 0.0 if any(nd in n for nd in _NO_DECAY) else weight_decay
        groups.setdefault((glr, wd), []).append(p)
    return [{"params": ps, "lr": glr, "weight_decay": wd} for (glr, wd), ps in groups.items()]


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` with torch's signature and semantics -- ``.grad`` is scaled in place, the total norm (0-d fp32
    device tensor) returned, parameters whose ``.grad`` is None skipped -- on the HIP global-norm kernel when every parameter is backed
    by ONE msa_amd flat storage (two launches for the norm, one for the scaling, no host sync).
    When a parallel.DataParallel drives that storage, ``.grad`` holds the SUM over ranks (the 1/world average is applied inside the
    AdamW kernel): the norm here is the norm of the averaged gradient, the one the step applies -- which torch's own clip, measuring the
    sum, gets ``world`` times too large.  ``error_if_nonfinite=True`` reads the norm back to the host (one sync).  ``foreach`` is
    accepted for compatibility and ignored.  Anything else (parameters outside a flat storage, or spread over several) goes to torch's
    clip unchanged; on the native path norm_type is 2 or inf.  ``AdamW.clip_grad_norm_`` is the fused form that leaves ``.grad`` alone."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    flat, names = None, []
    for p in params:
        ref = getattr(p, "_mmb_flat", None)
        if ref is None or ref[0] is None or (flat is not None and ref[0] is not flat):
            flat = None
            break
        flat = ref[0]
        o = ref[1]
        if p.grad.data_ptr() != flat.grads.data_ptr() + 4 * o or not p.grad.is_contiguous() or p.data_ptr() != flat.params.data_ptr() + 4 * o:
            flat = None                      # (a .grad the caller replaced, or a re-materialised parameter: not the flat buffer's view)
            break
        names.append(flat.name_at(o))
    if flat is None:
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    max_norm, norm_type = _clip_args(max_norm, norm_type)
    flat.join_side_writers()
    flat.settle()                            # (a dropped lazy gradient counts as zero, as its .grad view would read it)
    segs, nseg = flat.segments(names)
    out = ops.grad_norm(flat.grads, segs, nseg, max_norm=max_norm, norm_type=norm_type, gscale=flat.grad_scale,
                        workspace=flat.norm_workspace())
    norm = out[0]
    if error_if_nonfinite and not bool(torch.isfinite(norm)):
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be clipped. "
                           "To disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
    ops.grad_scale_(flat.grads, segs, nseg, out[1:2])
    return norm


class LinearWarmupSchedule:
    """``transformers.get_linear_schedule_with_warmup`` (LambdaLR semantics: lr = initial_lr * lambda(step),
    lambda(0) applied at construction).  The reference calls it with warmup == total (REF:train.py:93-97)."""

    def __init__(self, optimizer: AdamW, num_warmup_steps, num_training_steps):
        self.opt, self.warmup, self.total = optimizer, num_warmup_steps, num_training_steps
        self.last_step = 0
        self._apply()

    def _lambda(self, step):
        if step < self.warmup:
            return float(step) / float(max(1, self.warmup))
        return max(0.0, float(self.total - step) / float(max(1, self.total - self.warmup)))

    def _apply(self):
        lam = self._lambda(self.last_step)
        for g in self.opt.param_groups:
            g["lr"] = g["initial_lr"] * lam

    def step(self):
        self.last_step += 1
        self._apply()

    def get_last_lr(self):
        return [g["lr"] for g in self.opt.param_groups]


def get_linear_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps):
    return LinearWarmupSchedule(optimizer, num_warmup_steps, num_training_steps)
