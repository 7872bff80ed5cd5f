"""CPU tests of the adapter dropout's host side: model.add_lora(dropout=...) / set_lora_dropout and where the value lives,
its reset, the adapter file, trainer.apply_lora, the sites of ops.lora_in_drops, the C header."""
import os
import re
import types

import pytest
import torch

from tests import rng_ref as R
from tests.test_lora_cpu import _model, L
from tests.test_rng_reference_cpu import _host_lib, model_sites

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("query", "key", "value", "attention_output", "intermediate", "ffn_output")


def test_the_value_is_validated_and_lives_beside_the_adapter_record():
    m = _model()
    assert m.lora_dropout == 0.0
    with pytest.raises(ValueError, match="no adapters"):
        m.set_lora_dropout(0.1)
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.1", None, True):
        with pytest.raises(ValueError, match="dropout"):
            _model().add_lora(r=8, dropout=bad)
    assert not [n for n, _ in m.named_parameters() if ".lora_" in n]          # a refused call registers nothing
    assert m.add_lora(r=8, alpha=12.0, targets=("query", "value"), layers=[1, 3], dropout=0.05) is m
    assert m.lora_dropout == 0.05
    assert m._lora == dict(r=8, alpha=12.0, targets=("query", "value"), layers=(1, 3))      # its four keys: add_lora(**m._lora) still works
    rec = dict(m._lora)
    m.remove_lora()
    assert m.lora_dropout == 0.0
    m.add_lora(**rec)
    assert m.lora_dropout == 0.0 and m._lora == rec
    m._flat = marker = object()
    assert m.set_lora_dropout(0.25) is m and m.lora_dropout == 0.25 and m._flat is marker    # no rebuild of the flat storage
    assert m.set_lora_dropout(0) is m and m.lora_dropout == 0.0 and isinstance(m.lora_dropout, float)
    for bad in (-1e-9, 1.0, float("nan"), "x", False):
        with pytest.raises(ValueError, match="dropout"):
            m.set_lora_dropout(bad)
    assert m.lora_dropout == 0.0
    m._flat = None


def test_remove_and_merge_reset_it():
    m = _model().add_lora(r=4, targets="all-linear", dropout=0.3)
    assert m.lora_dropout == 0.3 and m._lora["targets"] == ALL
    m.merge_lora()
    assert m.lora_dropout == 0.0 and m._lora is None
    m.add_lora(r=4, dropout=0.2)
    m.remove_lora()
    assert m.lora_dropout == 0.0


def test_adapter_file_round_trip_with_and_without_the_key():
    """The file keeps its four non-tensor keys (existing tests pin them): the dropout is not written.  A file that carries a plain float
    ``dropout`` sets it where the adapters are created; it never enters the comparison of existing adapters."""
    m = _model().add_lora(r=8, alpha=12.0, targets=("query", "ffn_output"), layers=[0, 2], seed=1, dropout=0.1)
    sd = m.lora_state_dict()
    assert sorted(k for k, v in sd.items() if not torch.is_tensor(v)) == ["alpha", "layers", "r", "targets"]
    fresh = _model()
    fresh.load_lora_state_dict(sd)
    assert fresh._lora == m._lora and fresh.lora_dropout == 0.0                 # an absent key means 0
    with_key = dict(sd, dropout=0.2)
    fresh = _model()
    fresh.load_lora_state_dict(with_key)
    assert fresh._lora == m._lora and fresh.lora_dropout == 0.2 and set(fresh._lora) == {"r", "alpha", "targets", "layers"}
    m.load_lora_state_dict(with_key)                                            # existing adapters with another dropout: no "differ", theirs stays
    assert m.lora_dropout == 0.1
    with pytest.raises(ValueError, match="dropout"):
        _model().load_lora_state_dict(dict(sd, dropout=1.0))


def test_apply_lora_reads_the_argument():
    from msa_amd import trainer
    m = _model()
    args = types.SimpleNamespace(lora_rank=4, lora_targets=("value",), lora_dropout=0.1)
    assert trainer.apply_lora(m, args) is True and m.lora_dropout == 0.1 and m._lora["targets"] == ("value",)
    m = _model()
    assert trainer.apply_lora(m, types.SimpleNamespace(lora_rank=4)) is True and m.lora_dropout == 0.0
    m = _model()
    assert trainer.apply_lora(m, types.SimpleNamespace(lora_rank=4, lora_dropout=None)) is True and m.lora_dropout == 0.0
    with pytest.raises(ValueError, match="dropout"):
        trainer.apply_lora(_model(), types.SimpleNamespace(lora_rank=4, lora_dropout=1.0))


def test_sites_of_the_adapter_dropout():
    from msa_amd import ops
    _host_lib()
    assert ops.LORA_DROP_SITES == {"qkv": 3, "attention_output": 4, "intermediate": 5, "ffn_output": 6}
    seed = 17 * 1000003 + 2
    for layer in (0, 3, 11):
        d = ops.lora_in_drops(0.1, seed, layer)
        assert set(d) == set(ops.LORA_DROP_SITES)
        for k, off in ops.LORA_DROP_SITES.items():
            stream, thr, scale = d[k]
            assert stream == R.rng_stream(seed, 8 * layer + off) and thr == R.thr16(0.1) == 6554 and scale == R.drop_scale(thr)
    assert all(v == ops.NO_DROP for v in ops.lora_in_drops(0.0, seed, 5).values())
    new = {8 * i + off for i in range(12) for off in ops.LORA_DROP_SITES.values()}
    assert len(new) == 48 and not new & set(model_sites()) and 4242 not in new
    assert not any(s % 8 == 7 for s in new)                                     # 8 i + 7 stays free
    # the model forms them in ops.py: model.py has no make_drop call for them (tests/test_rng_reference_cpu.py pins that set)
    src = open(os.path.join(ROOT, "msa_amd", "model.py")).read()
    assert "ops.lora_in_drops(pl, seed, i" in src
    assert set(ops.lora_in_drops(0.1, seed, 2, ("qkv", "ffn_output"))) == {"qkv", "ffn_output"}
    assert ops.lora_in_drops(0.1, seed, 2, ("qkv",))["qkv"] == ops.lora_in_drops(0.1, seed, 2)["qkv"]


def test_the_header_declares_the_four_entry_points():
    lib = _host_lib()
    hdr = open(os.path.join(ROOT, "include", "mmbert_hip.h")).read()
    for name in ("mmbert_lora_qkv_fwd_drop", "mmbert_lora_qkv_bwd_drop", "mmbert_lora_dense_fwd_drop", "mmbert_lora_dense_bwd_drop"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert decl, name
        assert re.search(r"unsigned in_stream, unsigned in_thr16, float in_scale", decl.group(1)), name
        assert hasattr(lib, name)
    assert "const int* rows" in re.search(r"\bint mmbert_lora_dense_bwd_drop\(([^;]*)\);", hdr).group(1)
    # the old signatures stand as they were
    assert re.search(r"int mmbert_lora_qkv_fwd\(mmbert_stream_t stream, const void\* x, int ldx, void\* qkv, int ldq, int M, int H, int r, int targets,\s*"
                     r"const void\* const\* A, const void\* const\* B, float scale, void\* h_out, int ldh\);", hdr)
