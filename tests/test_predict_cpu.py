"""The label-free prediction path, as far as it can be checked without a GPU: the public calls exist with their signatures, refuse
what they do not implement, and the new C entry points are declared, exported and typed (tests/test_abi_cpu.py holds header, exports
and signatures to each other; the names are asserted here)."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(num_labels=7):
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    m = MMBertForPretraining(MMBertConfig(vocab_size=512, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128))
    m.bert.set_joint_embeddings("mosei")
    m.num_labels = num_labels
    return m


def _cpu_inputs(B=2, T=8, P=6):
    from msa_amd.data import synthetic_batch
    b = synthetic_batch(B, T, P, P, vocab=512, seed=3)
    return b["input_ids"], b["token_type_ids"], b["attention_mask"]


def test_predict_and_predict_epoch_signatures():
    from msa_amd import trainer
    from msa_amd.model import MMBertForPretraining
    sig = inspect.signature(MMBertForPretraining.predict)
    assert list(sig.parameters)[:4] == ["self", "input_ids", "token_type_ids", "attention_mask"]
    assert sig.parameters["return_pooled"].default is False
    fwd = list(inspect.signature(MMBertForPretraining.forward).parameters)
    assert fwd[1:4] == list(sig.parameters)[1:4]                         # forward's first three arguments, unchanged
    sig = inspect.signature(trainer.predict_epoch)
    assert list(sig.parameters)[:3] == ["args", "model", "data"]
    for name, default in (("device", "cuda"), ("batches", None)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default


def test_predict_on_cpu_tensors_raises_the_no_cpu_path_error():
    m = _tiny()
    was = m.training
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.predict(*_cpu_inputs())
    assert m.training is was


def test_predict_refuses_the_classification_head():
    m = _tiny(num_labels=3)
    with pytest.raises(NotImplementedError, match="num_labels"):
        m.predict(*_cpu_inputs())


def test_predict_epoch_leaves_the_model_mode_alone_and_handles_no_batches():
    from msa_amd import trainer
    m = _tiny()
    m.train()
    out = trainer.predict_epoch(trainer.default_args(val_batch_size=4), m, None, batches=[])
    assert out.shape == (0, 1) and m.training


def test_new_entry_points_are_declared_exported_and_typed():
    from msa_amd import _lib, build, ops
    text = open(os.path.join(ROOT, "include", "mmbert_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("mmbert_attn_fwd_first", "mmbert_heads_predict", "mmbert_heads_step_outputs"):
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in mmbert_hip.h"
        assert name in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        if not os.path.exists(build.HIPCC):
            return                                                        # (no library and no compiler here: the declarations were checked)
        build.build(verbose=False)
    lib = _lib.load()
    for name in ("mmbert_attn_fwd_first", "mmbert_heads_predict", "mmbert_heads_step_outputs"):
        assert hasattr(lib, name)
    # the documented way to the pooler / classifier1_1 outputs in the heads' workspace: host-only, inside the workspace, aligned
    import ctypes
    po, fo = ctypes.c_size_t(0), ctypes.c_size_t(0)
    B, H = 5, 192
    assert lib.mmbert_heads_step_outputs(B, H, ctypes.byref(po), ctypes.byref(fo)) == 0
    total = lib.mmbert_heads_step_workspace(B, H) // 4
    assert po.value % 4 == 0 and fo.value % 4 == 0 and po.value + 3 * B * H <= fo.value and fo.value + B * H <= total
    assert lib.mmbert_heads_step_outputs(0, H, ctypes.byref(po), ctypes.byref(fo)) == -1
    assert callable(ops.heads_predict) and callable(ops.heads_step_outputs) and "attn_fwd_first" in ops._UNWRAPPED
