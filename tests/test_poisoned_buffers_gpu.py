"""The kernel-level tests once more, on poisoned and guard-banded ops._empty buffers (tests/poison.py, "guard" mode).

The swept test functions are imported and called, not copied: their torch / fp64 references, shapes and tolerances are
the assertions.  The harness adds two things: every buffer a node allocates starts as NaN (so a result that depends on
memory no kernel wrote fails the function's own comparison), and every buffer sits between two guard bands that must
still hold the sentinel when the function returns (so a store outside a buffer fails the case).

What a failure means: a NaN in a compared result = some kernel consumed memory no kernel wrote - find the producer and
write what is read, or stop the read; a guard violation = an out-of-bounds store - read the kernel's tail handling.
Neither is ever a reason to exclude the case."""
import importlib
import itertools

import pytest

from tests import poison

pytestmark = pytest.mark.gpu

# every test of these modules is swept
SWEPT_MODULES = ("test_kernels_gpu", "test_conv_small_gpu", "test_resnet_kernels_gpu", "test_se_gate_gpu",
                 "test_stitch_mix_gpu")

# of these modules, the functions that call ops nodes directly and build no model (the bf16 instantiations are
# different kernels from the fp32 ones the modules above reach)
SWEPT_FUNCTIONS = {
    "test_conv_bf16_gpu": ("test_bf16_conv_fwd_dgrad_wgrad", "test_bf16_conv_natural_tail_tile", "test_bf16_conv_split_k",
                           "test_bf16_up2_conv", "test_bf16_conv1x1_cat_wgrad", "test_bf16_matches_emulated_contract"),
    "test_pw_bf16_gpu": ("test_bf16_pw_conv1x1_gemm_kernel", "test_bf16_pw_conv1x1_big_kernel",
                         "test_bf16_pw_conv1x1_big_kernel_four_waves", "test_bf16_pw_conv1x1_cat",
                         "test_bf16_pw_bn_act_conv1x1"),
}

# (full id of the original case, one-line reason).  A reason is valid only if the TEST ITSELF depends on the allocator
# (it patches ops._empty, or asserts something about storage); "reads NaN" or "guard violated" never is.  At most 5 % of
# the cases (tests/test_poisoned_buffers_cpu.py checks the bound and that every id exists).
EXCLUDED = [
    (f"tests/test_conv_small_gpu.py::test_cross_entropy_gradient_consumed_in_place_by_the_decoder_tail[{Ca}-{tr}-plain]",
     "asserts that the decoder tail took the gradient's storage in place, which holds only at storage offset 0 "
     "(its -poison twin, which patches ops._empty itself, stays in the sweep)")
    for Ca in (14, 16, 19, 32) for tr in (True, False)
]


def _id_of(val, argname, idx, ids):
    """pytest's id of one parametrize value (tests/test_poisoned_buffers_cpu.py compares the result with what pytest
    itself collects, so a rule this restatement misses fails there and not silently)."""
    if ids is not None:
        given = ids(val) if callable(ids) else ids[idx]
        if given is not None:
            return str(given)
    if isinstance(val, (str, bool, int, float, complex)) or val is None:
        return str(val)
    return f"{argname}{idx}"


def _cases_of(fn):
    """[(id suffix, {argname: value})] from the function's own parametrize marks; stacked marks give the product."""
    axes = []
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names, values = mark.args[0], mark.args[1]
        names = [n.strip() for n in names.split(",")] if isinstance(names, str) else list(names)
        ids = mark.kwargs.get("ids")
        axis = []
        for idx, val in enumerate(values):
            vals = (val,) if len(names) == 1 else tuple(val)
            assert len(vals) == len(names), (fn.__name__, names, val)
            axis.append(("-".join(_id_of(v, n, idx, ids) for n, v in zip(names, vals)), dict(zip(names, vals))))
        axes.append(axis)
    cases = []
    for combo in itertools.product(*axes):
        kw = {}
        for _, part in combo:
            kw.update(part)
        cases.append(("-".join(i for i, _ in combo), kw))
    return cases


def _sweep():
    out = []
    for modname in SWEPT_MODULES + tuple(SWEPT_FUNCTIONS):
        mod = importlib.import_module(f"tests.{modname}")
        names = SWEPT_FUNCTIONS.get(modname) or [n for n, f in vars(mod).items() if n.startswith("test") and callable(f)
                                                 and getattr(f, "__module__", None) == mod.__name__]
        for name in names:
            fn = getattr(mod, name)
            for suffix, kw in _cases_of(fn):
                out.append((f"tests/{modname}.py::{name}" + (f"[{suffix}]" if suffix else ""), fn, kw))
    excluded = {e for e, _ in EXCLUDED}
    return [c for c in out if c[0] not in excluded]


SWEEP = _sweep()


def original_id(own_id):
    """'test_guarded[test_x_gpu.py::test_y[case0]]' -> 'tests/test_x_gpu.py::test_y[case0]'"""
    assert own_id.startswith("test_guarded[") and own_id.endswith("]"), own_id
    return "tests/" + own_id[len("test_guarded["):-1]


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=full[len("tests/"):]) for full, fn, kw in SWEEP])
def test_guarded(request, fn, kw):
    code = fn.__code__
    fixtures = [a for a in code.co_varnames[:code.co_argcount] if a not in kw]  # dev, vmtl_env, monkeypatch: by name
    args = dict(kw, **{a: request.getfixturevalue(a) for a in fixtures})
    with poison.patched("guard") as p:
        fn(**args)
    print(f"{p.count} buffers from ops._empty, all guards intact")
