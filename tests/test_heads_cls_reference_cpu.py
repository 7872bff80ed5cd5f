"""tests/heads_cls_ref.py on the CPU, and the host side of the C-class label head.

The restatement of the heads with a C-wide ``classifier1_2`` equals float64 autograd through the oracle's pieces to 1e-12, the
emulation of the kernels' fp32 roundings stays inside the derived bounds on every case, every value-only mutation is rejected on at
least one case, and every case the GPU test uses satisfies the gap condition (each sample's two largest float64 logits at least
KINK = 64 bounds apart), so ``pred`` is compared on every sample.

Largest emulation ratio over every case here: 0.34 (normwise, the joint loss at B = 17, H = 80, C = 6, d = 2^10); the class head's own outputs:
logits 0.21, classifier1_2 weight 0.17, bias 0.06, label loss 0.10.  Smallest margin of a mutation (error / bound; > 1 is rejected):
1.7e5, the last class lost from gbc2; then softmax over the batch axis 2.5e5, dT through row 0 of Wc2 4.8e5, the one-hot term dropped
6.7e5, gWc2 rows permuted 7.5e5, the label read as 0 1.1e6, 1/B dropped 7.1e6; ``pred`` = the second largest is rejected by the exact
comparison.

Host side: the constructor's / ``from_pretrained``'s ``num_labels``, ``set_num_labels``, a bare ``model.num_labels = 3`` still
refused by ``predict()``, ``synthetic_batch`` unchanged without its new keyword, ``predict_epoch`` on no batches, the ctypes mirror of
``mmbert_heads_step`` against the library and the header, and the serialized-load scan of the class-head level kernels."""
import ctypes
import hashlib
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import heads_cls_ref as HCR
from tests import heads_ref as HR

torch.set_num_threads(min(16, torch.get_num_threads()))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [dict(B=1, H=16, C=2, nmlm=0, d=1.0), dict(B=3, H=80, C=3, nmlm=3, d=-0.37), dict(B=17, H=80, C=6, nmlm=256, d=2.0 ** 10, ap="zeros"),
         dict(B=16, H=64, C=16, nmlm=3, d=-0.37, ap="ones"), dict(B=33, H=256, C=6, nmlm=3, d=-0.37), dict(B=65, H=64, C=2, nmlm=0, d=1.0, beta=0.0)]

GPU_STEP, GPU_MODEL_FORM, gpu_step_case, gpu_model_form_case = HCR.GPU_STEP, HCR.GPU_MODEL_FORM, HCR.gpu_step_case, HCR.gpu_model_form_case


def _case(i, kw):
    kw = dict(kw)
    B, H, C = kw.pop("B"), kw.pop("H"), kw.pop("C")
    return HCR.make_case(B, H, 40 + i, C, **kw)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_restatement_equals_float64_autograd_and_emulation_passes(i):
    c = _case(i, CASES[i])
    ref = HCR.reference(c)
    rs = HCR.restate(c)
    for k in HCR.OUTPUTS:
        if ref.get(k) is None:
            assert rs[k] is None, k
            continue
        a, b = ref[k].reshape(-1), rs[k].v.reshape(-1)
        assert float((a - b).abs().max()) <= 1e-12 * max(float(a.abs().max()), 1e-300), k
    assert torch.equal(ref["pred"], rs["pred"])
    assert ref["logits"].shape == (c.B, c.C) and ref["classifier1_2.weight"].shape == (c.C, c.H)
    exp = HCR.expected(c, ref, rs)
    em = HCR.restate(c, emu=True)
    HCR.check_all({k: (v if k == "pred" else v.v) for k, v in em.items() if v is not None}, exp, f"emulation {CASES[i]}")
    worst = {k: HR.ratios(em[k].v.reshape(r.val.shape), r).worst for k, r in exp.items() if k != "pred"}
    assert HCR.gap_ratio(c, exp) >= HCR.KINK
    print(f"\n{CASES[i]}: emulation ratio {max(worst.values()):.3f} ({max(worst, key=worst.get)}); logits {worst['logits']:.3f}, "
          f"classifier1_2 W {worst['classifier1_2.weight']:.3f} b {worst['classifier1_2.bias']:.3f}, label loss {worst['aux']:.3f}")


MUTATIONS = [HCR.softmax_over_batch(), HCR.onehot_dropped(), HCR.inv_b_dropped(), HCR.dT_row0_only(), HCR.gWc2_rows_permuted(),
             HCR.gbc2_last_class_lost(), HCR.label_cast_to_zero(), HCR.pred_second_largest()]


@pytest.mark.parametrize("j", range(len(MUTATIONS)), ids=[m.name for m in MUTATIONS])
def test_mutation_is_rejected(j):
    mut = MUTATIONS[j]
    c = HCR.make_case(16, 64, 7, 6, d=-0.37)
    exp = HCR.expected(c)
    em = HCR.restate(c, emu=True, mutation=mut)
    if mut.name.startswith("pred"):
        assert not torch.equal(em["pred"], exp["pred"])
        with pytest.raises(AssertionError, match="pred"):
            HCR.check_all({"pred": em["pred"]}, exp, mut.name)
        return
    margin = max(HR.ratios(em[k].v.reshape(r.val.shape), r).worst for k, r in exp.items() if k != "pred")
    print(f"\n{mut.name}: margin {margin:.3g}")
    assert margin > 1.0, (mut.name, margin)
    with pytest.raises(AssertionError):
        HCR.check_all({k: v.v for k, v in em.items() if v is not None and k != "pred"}, exp, mut.name)


@pytest.mark.parametrize("i", range(len(GPU_STEP) + len(GPU_MODEL_FORM)))
def test_gpu_cases_keep_every_sample_in_the_pred_comparison(i):
    c = gpu_step_case(i) if i < len(GPU_STEP) else gpu_model_form_case(i - len(GPU_STEP))
    assert HCR.gap_ratio(c) >= HCR.KINK
    assert c.y.dtype == torch.int64 and int(c.y.min()) >= 0 and int(c.y.max()) < c.C
    if c.B >= c.C:
        assert len(set(c.y.tolist())) == c.C


# ------------------------------------------------------------------------------------------------ the host side
def _cfg():
    from msa_amd.model import MMBertConfig
    return MMBertConfig(vocab_size=512, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128)


def test_constructor_and_set_num_labels():
    from msa_amd.model import MMBertForPretraining
    m = MMBertForPretraining(_cfg())
    assert m.num_labels == 7 and m.classifier1_2.weight.shape == (1, 64)
    keys = list(m.state_dict())
    for n, width in ((1, 1), (7, 1), (2, 2), (6, 6), (16, 16)):
        q = MMBertForPretraining(_cfg(), num_labels=n)
        assert q.num_labels == n and q.classifier1_2.weight.shape == (width, 64) and list(q.state_dict()) == keys
    for bad in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="num_labels"):
            MMBertForPretraining(_cfg(), num_labels=bad)
        with pytest.raises(ValueError, match="num_labels"):
            m.set_num_labels(bad)
    assert m.num_labels == 7 and m.classifier1_2.weight.shape == (1, 64)
    m._flat = "stale"
    old = m.classifier1_2
    m.set_num_labels(1)                                         # same width: the layer stays
    assert m.classifier1_2 is old and m.num_labels == 1 and m._flat == "stale"
    m.set_num_labels(6)
    assert m.num_labels == 6 and m.classifier1_2.weight.shape == (6, 64) and m._flat is None
    assert float(m.classifier1_2.bias.detach().abs().max()) == 0.0 and 0.0 < float(m.classifier1_2.weight.detach().std()) < 3 * m.config.initializer_range
    assert list(m.state_dict()) == keys
    m.set_num_labels(7)
    assert m.num_labels == 7 and m.classifier1_2.weight.shape == (1, 64)
    # a checkpoint of another width: torch's size-mismatch error
    with pytest.raises(RuntimeError, match="size mismatch"):
        MMBertForPretraining(_cfg(), num_labels=3).load_state_dict(m.state_dict())


def test_from_pretrained_takes_num_labels(tmp_path):
    import json
    import warnings
    from msa_amd.model import MMBertForPretraining
    src = MMBertForPretraining(_cfg(), num_labels=6)
    conf = dict(vocab_size=512, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128)
    (tmp_path / "config.json").write_text(json.dumps(conf))
    torch.save(src.state_dict(), tmp_path / "pytorch_model.bin")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = MMBertForPretraining.from_pretrained(str(tmp_path), num_labels=6)
        assert m.num_labels == 6 and torch.equal(m.classifier1_2.weight, src.classifier1_2.weight)
        with pytest.raises(RuntimeError, match="size mismatch"):
            MMBertForPretraining.from_pretrained(str(tmp_path))
        with pytest.raises(ValueError, match="num_labels"):
            MMBertForPretraining.from_pretrained(str(tmp_path), num_labels=17)


def test_a_bare_num_labels_attribute_is_still_refused_by_predict():
    from msa_amd.data import synthetic_batch
    from msa_amd.model import MMBertForPretraining
    m = MMBertForPretraining(_cfg())
    m.bert.set_joint_embeddings("mosei")
    m.num_labels = 3
    b = synthetic_batch(2, 16, 30, 20, dataset="mosei", vocab=512, seed=8)
    with pytest.raises(NotImplementedError, match="num_labels.*set_num_labels"):
        m.predict(b["input_ids"], b["token_type_ids"], b["attention_mask"])


def test_a_class_head_refuses_floating_point_labels_before_anything_runs():
    from msa_amd.data import synthetic_batch
    from msa_amd.model import MMBertForPretraining
    m = MMBertForPretraining(_cfg(), num_labels=3)
    m.bert.set_joint_embeddings("mosei")
    b = synthetic_batch(2, 16, 30, 20, dataset="mosei", vocab=512, seed=8)      # fp32 regression targets
    with pytest.raises(TypeError, match="integer class labels"):
        m(**b)


def _digest(x, h):
    if torch.is_tensor(x):
        h.update(str((x.dtype, tuple(x.shape))).encode())
        h.update(x.contiguous().numpy().tobytes())
    elif isinstance(x, (tuple, list)):
        for y in x:
            _digest(y, h)
    elif isinstance(x, dict):
        for k in sorted(x):
            h.update(k.encode())
            _digest(x[k], h)
    return h


def test_synthetic_batch_default_is_unchanged_and_class_labels_are_int64():
    from msa_amd.data import synthetic_batch
    args = (3, 20, 24, 28)
    a = synthetic_batch(*args, vocab=4096, seed=5)
    b = synthetic_batch(*args, vocab=4096, seed=5, num_labels=None)
    assert _digest(a, hashlib.sha256()).hexdigest() == _digest(b, hashlib.sha256()).hexdigest()
    assert a["sentiment"].dtype == torch.float32 and a["sentiment"].shape == (3,)
    for C in (2, 6):
        c = synthetic_batch(64, 20, 24, 28, vocab=4096, seed=5, num_labels=C)
        y = c["sentiment"]
        assert y.dtype == torch.int64 and y.shape == (64,) and int(y.min()) == 0 and int(y.max()) == C - 1
        c2 = synthetic_batch(64, 20, 24, 28, vocab=4096, seed=5)
        for k in a:
            if k != "sentiment":                                # everything drawn before the labels is the same batch
                assert _digest(c[k], hashlib.sha256()).hexdigest() == _digest(c2[k], hashlib.sha256()).hexdigest(), k
        assert torch.equal(y, synthetic_batch(64, 20, 24, 28, vocab=4096, seed=5, num_labels=C)["sentiment"])


def test_predict_epoch_on_no_batches():
    from msa_amd import trainer
    from msa_amd.model import MMBertForPretraining
    r = trainer.predict_epoch(None, MMBertForPretraining(_cfg()), None, batches=[])
    assert r.shape == (0, 1) and r.dtype == np.float32
    r = trainer.predict_epoch(None, MMBertForPretraining(_cfg(), num_labels=2), None, batches=[])
    assert r.shape == (0,) and r.dtype == np.int64
    m = MMBertForPretraining(_cfg())
    m.num_labels = 3                                            # a bare attribute: still the one-output model
    assert trainer.predict_epoch(None, m, None, batches=[]).shape == (0, 1)


def test_struct_mirror_matches_the_library_and_the_header():
    from msa_amd import _lib, ops
    assert _lib.load().mmbert_heads_step_struct_size() == ctypes.sizeof(ops._HeadsStep)
    names = [f[0] for f in ops._HeadsStep._fields_]
    assert "pad0_" not in names and names[names.index("ldy") + 1] == "ncls" and names[-3:] == ["sync", "sent_cls", "pred"]
    assert ops._HeadsStep.ncls.offset == ops._HeadsStep.ldy.offset + 4
    assert ops.heads_step_struct().ncls == 0                    # zero-initialised: every existing caller asks for regression
    hdr = open(os.path.join(ROOT, "include", "mmbert_hip.h")).read()
    body = hdr[hdr.index("typedef struct {\n    int B, H, tanh_lo, nmlm;"):hdr.index("} mmbert_heads_step;")]
    assert "int ldy, ncls;" in body and "pad0_" not in hdr
    assert body.index("unsigned* sync;") < body.index("const int64_t* sent_cls;") < body.index("int64_t* pred;")
    # the workspace's size and the offsets of P and T depend on (B, H) alone
    lib = _lib.load()
    po, fo = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.mmbert_heads_step_outputs(5, 64, ctypes.byref(po), ctypes.byref(fo)) == 0
    assert (po.value, fo.value) == (3 * 5 * 64, 4 * 3 * 5 * 64)


def test_class_head_level_kernels_keep_their_loads_in_flight():
    """tools/scan_serialized_loads.py on csrc/heads_coop.hip: the class-head instantiations of forward level 5 and backward levels 2 and 3
    -- the levels that run on many workgroups -- have no more "one load, then a full drain" sites than the regression instantiations
    of the same levels (the loss level's workgroup 3, one thread per sample over <= 16 classes, is not pinned)."""
    spec = importlib.util.spec_from_file_location("scan_serialized_loads", os.path.join(ROOT, "tools", "scan_serialized_loads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    t = mod.scan_source("heads_coop.hip")

    def one(prefix):
        hits = [v for k, v in t.items() if k.startswith("void " + prefix)]
        assert len(hits) == 1, (prefix, list(t))
        return hits[0]
    for kern, level in (("heads_fwd_level_kernel", 5), ("heads_bwd_level_kernel", 2), ("heads_bwd_level_kernel", 3)):
        reg, cls = one(f"{kern}<{level}, false>"), one(f"{kern}<{level}, true>")
        assert cls[0] > 0 and cls[2] <= reg[2], (kern, level, reg, cls)
    assert one("heads_fwd_level_kernel<7, true>")[0] > 0
