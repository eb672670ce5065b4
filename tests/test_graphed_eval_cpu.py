"""-m "not gpu": the batched eval-mode BatchNorm statistics entry point (csrc/bn.hip) is declared, exported and sized like
the descriptors ops.eval_bn_table packs; GraphedEval's public surface checks its arguments before touching a device."""
import ctypes
import struct

import pytest
import torch


def test_batched_eval_stats_declared_and_exported():
    from vision_mtl_amd._lib import HEADER, LIB_PATH, lib, parse_header

    protos = parse_header(HEADER)
    assert "vmtl_bn_eval_desc_bytes" in protos and "vmtl_bn_eval_stats_batch" in protos
    assert protos["vmtl_bn_eval_desc_bytes"][1] == []
    assert protos["vmtl_bn_eval_stats_batch"][2] == ["descs", "n", "max_cs", "stream"]
    lib()  # builds the library when missing
    dll = ctypes.CDLL(str(LIB_PATH))
    assert hasattr(dll, "vmtl_bn_eval_desc_bytes") and hasattr(dll, "vmtl_bn_eval_stats_batch")


def test_desc_size_matches_python_packing():
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import lib

    size = lib().raw("vmtl_bn_eval_desc_bytes")()
    # running_mean, running_var, gamma, beta, save_mean, save_invstd, coef_a, coef_c, C, Cs, eps (+ pad)
    assert size == struct.calcsize(ops._EvalBNTable.DESC) == 8 * 8 + 4 * 4


def test_batched_eval_stats_rejects_bad_arguments_on_the_host():
    """Argument validation happens before any launch (no device is touched: a null stream, no table read)."""
    from vision_mtl_amd._lib import lib

    f = lib().raw("vmtl_bn_eval_stats_batch")
    assert f(None, 4, 64, None) == -1
    assert f(ctypes.c_void_p(16), 0, 64, None) == -1
    assert f(ctypes.c_void_p(16), -3, 64, None) == -1
    assert f(ctypes.c_void_p(16), 4, 66, None) == -1
    assert f(ctypes.c_void_p(16), 4, 0, None) == -1


def test_eval_bn_table_is_inert_without_eval_batchnorms():
    """No BatchNorm in eval mode: the context issues nothing, yields None and leaves no lookup in force."""
    from vision_mtl_amd import ops

    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1), torch.nn.BatchNorm2d(4)).train()
    calls = []
    orig, ops._k = ops._k, lambda name, *a, **kw: calls.append(name)
    try:
        with ops.eval_bn_table(m) as t:
            assert t is None and ops.eval_bn.active is None
    finally:
        ops._k = orig
    assert calls == [] and ops.eval_bn.active is None


def test_graphed_eval_rejects_unknown_stage():
    from vision_mtl_amd.graphed import GraphedEval

    with pytest.raises(ValueError, match="stage"):
        GraphedEval(object(), {}, stage="train")
