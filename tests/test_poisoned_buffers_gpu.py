"""The kernel-level tests once more, on poisoned and guard-banded ops._empty buffers (tests/poison.py, "guard" mode).

The swept test functions are imported and called, not copied: their torch / fp64 references, shapes and tolerances are
the assertions.  The harness adds two things: every buffer a node allocates starts as NaN (so a result that depends on
memory no kernel wrote fails the function's own comparison), and every buffer sits between two guard bands that must
still hold the sentinel when the function returns (so a store outside a buffer fails the case).

What a failure means: a NaN in a compared result = some kernel consumed memory no kernel wrote - find the producer and
write what is read, or stop the read; a guard violation = an out-of-bounds store - read the kernel's tail handling.
Neither is ever a reason to exclude the case.

test_launch_guarded runs the same functions under tests/launch_guard.py alone: there every POINTER ARGUMENT of every
launch - operands the test built, outputs of the tests that call the C ABI directly - sits between two NaN bands, a
store through a pointer include/vmtl.h declares const is reported, and so is a store outside any argument.  A NaN in a
compared result there that test_guarded does not show = a kernel consumed memory outside an operand."""
import importlib
import itertools

import pytest

from tests import launch_guard, poison
from tests.test_conv3x3_halo_gpu import forced_route  # noqa: F401  (a fixture of a swept function, requested by name)

pytestmark = pytest.mark.gpu

# every test of these modules is swept
SWEPT_MODULES = ("test_kernels_gpu", "test_conv_small_gpu", "test_resnet_kernels_gpu", "test_se_gate_gpu",
                 "test_stitch_mix_gpu", "test_dwconv_kernels_gpu", "test_bn_kernels_gpu")

# of these modules, the functions that call ops nodes directly and build no model (the bf16 instantiations are
# different kernels from the fp32 ones the modules above reach)
SWEPT_FUNCTIONS = {
    "test_conv_bf16_gpu": ("test_bf16_conv_fwd_dgrad_wgrad", "test_bf16_conv_natural_tail_tile", "test_bf16_conv_split_k",
                           "test_bf16_up2_conv", "test_bf16_conv1x1_cat_wgrad", "test_bf16_matches_emulated_contract"),
    "test_pw_bf16_gpu": ("test_bf16_pw_conv1x1_gemm_kernel", "test_bf16_pw_conv1x1_big_kernel",
                         "test_bf16_pw_conv1x1_big_kernel_four_waves", "test_bf16_pw_conv1x1_cat",
                         "test_bf16_pw_bn_act_conv1x1"),
    # the halo-tile kernels, called on the tests' own buffers (ops._mid_halo, L.callk into torch.empty)
    "test_conv3x3_halo_gpu": ("test_conv3x3_halo_plain_and_prologue", "test_conv3x3_halo_epilogues",
                              "test_bn_act_conv_on_the_halo_route_matches_torch"),
    "test_conv_up2_halo_gpu": ("test_up2_halo_matches_torch", "test_up2_halo_statistics_rows"),
    # the loss, optimizer, metric, augmentation, balancing and resize kernels: nodes and direct C-ABI calls, no model
    "test_loss_ignore_gpu": ("test_forward_argmax_and_backward_match_torch",
                             "test_c_abi_layouts_write_the_lanes_the_unweighted_kernels_write", "test_silog_with_mask"),
    "test_optim_kernels_gpu": ("test_norm_matches_fp64_and_is_deterministic", "test_clipped_update_matches_fp64",
                               "test_l2_and_decoupled_decay", "test_skip_nonfinite", "test_inplace_clip"),
    "test_eval_accum_gpu": ("test_one_update_matches_the_oracle", "test_unaligned_depth_pair_and_valid_mask"),
    "test_augment_gpu": ("test_apply_matches_oracle", "test_reads_stay_inside_the_crop", "test_identity", "test_gain"),
    "test_task_balance_kernels_gpu": ("test_forward_and_backward_match_the_closed_forms",
                                      "test_parameter_gradient_goes_into_the_arena_slot",
                                      "test_dwa_accumulation_skips_non_finite_steps_and_accumulate_off",
                                      "test_dwa_epoch_updates", "test_geometric_with_a_non_positive_loss_is_nan"),
    "test_device_resize_gpu": ("test_device_transform_matches_host_chain",),
}

# (full id of the original case, one-line reason).  A reason is valid only if the TEST ITSELF depends on the allocator
# (it patches ops._empty, or asserts something about storage); "reads NaN" or "guard violated" never is.  Per sweep at
# most 5 % of the cases (tests/test_poisoned_buffers_cpu.py checks the bound and that every id exists).
EXCLUDED = [
    (f"tests/test_conv_small_gpu.py::test_cross_entropy_gradient_consumed_in_place_by_the_decoder_tail[{Ca}-{tr}-plain]",
     "asserts that the decoder tail took the gradient's storage in place, which holds only at storage offset 0 "
     "(its -poison twin, which patches ops._empty itself, stays in the sweep)")
    for Ca in (14, 16, 19, 32) for tr in (True, False)
]


# test_launch_guarded only: the cases that exist to cross a grid cap.  Every launch copies its operands once more, and
# the tail and alignment paths of these kernels are reached by the small siblings of the same parametrisation.
EXCLUDED_LAUNCH = [
    ("tests/test_eval_accum_gpu.py::test_one_update_matches_the_oracle[2097155-0-19-None-0.001-plain]",
     "2 Mi pixels, there for the stride loop past the grid cap: allocation-heavy under a copy per launch"),
    ("tests/test_eval_accum_gpu.py::test_one_update_matches_the_oracle[2097155-1-14-255-0.1-ignore255]",
     "2 Mi pixels, there for the stride loop past the grid cap: allocation-heavy under a copy per launch"),
    ("tests/test_loss_ignore_gpu.py::test_silog_with_mask[4194307]",
     "4 Mi pixels, there for the block cap of sl_blocks: allocation-heavy under a copy per launch"),
    ("tests/test_dwconv_kernels_gpu.py::test_past_the_grid_cap[past-the-grid-cap-fwd-and-generic-dgrad]",
     "2 Mi work items, there for the stride loop past the grid cap: allocation-heavy under a copy per launch"),
    ("tests/test_dwconv_kernels_gpu.py::test_past_the_grid_cap[past-the-grid-cap-tpl-k3s1-dgrad]",
     "2 Mi work items, there for the stride loop past the grid cap: allocation-heavy under a copy per launch"),
]

LEFT_IN_PLACE_CAP = 0.05  # of the tensor arguments of test_launch_guarded (see the tally test): a condition, not a measurement


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
            if ids is not None and not callable(ids) and ids[idx] is not None:  # a list of ids names whole value sets
                axis.append((str(ids[idx]), dict(zip(names, vals))))
                continue
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
    return out


ALL_CASES = _sweep()
SWEEP = [c for c in ALL_CASES if c[0] not in {e for e, _ in EXCLUDED}]
SWEEP_LAUNCH = [c for c in ALL_CASES if c[0] not in {e for e, _ in EXCLUDED_LAUNCH}]


def original_id(own_id, sweep="test_guarded"):
    """'test_guarded[test_x_gpu.py::test_y[case0]]' -> 'tests/test_x_gpu.py::test_y[case0]'"""
    assert own_id.startswith(sweep + "[") and own_id.endswith("]"), own_id
    return "tests/" + own_id[len(sweep) + 1:-1]


def _call(request, fn, kw):
    code = fn.__code__
    fixtures = [a for a in code.co_varnames[:code.co_argcount] if a not in kw]  # dev, vmtl_env, monkeypatch: by name
    fn(**dict(kw, **{a: request.getfixturevalue(a) for a in fixtures}))


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=full[len("tests/"):]) for full, fn, kw in SWEEP])
def test_guarded(request, fn, kw):
    with poison.patched("guard") as p:
        _call(request, fn, kw)
    print(f"{p.count} buffers from ops._empty, all guards intact")


TALLY = {"cases": 0, "pointers": 0, "relocated": 0, **dict.fromkeys(launch_guard.REASONS, 0)}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=full[len("tests/"):]) for full, fn, kw in SWEEP_LAUNCH])
def test_launch_guarded(request, fn, kw):
    TALLY["cases"] += 1
    g = None
    try:
        with launch_guard.patched() as g:
            _call(request, fn, kw)
    finally:
        assert g is not None, "the harness could not be installed"
        TALLY["pointers"] += g.pointers
        TALLY["relocated"] += g.relocated
        for r in launch_guard.REASONS:
            TALLY[r] += g.left[r]
        print(g.counts())
    print("all guards intact, no const operand written")


def test_launch_guarded_leaves_few_pointers_in_place():
    """Over the whole of test_launch_guarded, at most LEFT_IN_PLACE_CAP of the pointer arguments that point at memory
    were left where they were ("partial", "stream", "capturing").  A None argument is counted and printed under "null",
    but is on neither side of the bound: it has to stay NULL, points at nothing that could be guarded, and no harness
    could change the count - with it the bound would only measure how many optional parameters the entry points have
    (16 % of all pointer arguments when this test was written: 3543 of 21787).  Leaving the None arguments out of the
    denominator as well makes the bound stricter than one over all pointer arguments.
    Asserted after a run of the whole sweep (this test is collected last); a partial selection only prints."""
    left = sum(TALLY[r] for r in launch_guard.REASONS if r != "null")
    print(f"{TALLY['cases']} of {len(SWEEP_LAUNCH)} cases, {TALLY['pointers']} pointer arguments: {TALLY['relocated']} "
          f"relocated, {TALLY['null']} null, {left} left in place: "
          + ", ".join(f"{r} {TALLY[r]}" for r in launch_guard.REASONS if r != "null"))
    assert TALLY["relocated"] + left + TALLY["null"] == TALLY["pointers"]
    if TALLY["cases"] == len(SWEEP_LAUNCH):
        tensors = TALLY["pointers"] - TALLY["null"]
        assert left <= LEFT_IN_PLACE_CAP * tensors, f"{left} of {tensors} tensor arguments left in place"
