"""Operand precision of the implicit-GEMM convolutions and the pointwise GEMMs, chosen by the user.

"fp32" (the default) multiplies exact fp32 operands (v_mfma_f32_16x16x4_f32).  "bf16" rounds every operand of the covered
kernels to bf16 (round-to-nearest-even) and accumulates in fp32 on the bf16 matrix cores: activations, weights,
statistics and gradients stay fp32 in memory, only the product terms change.  Covered: the implicit-GEMM convolution
(forward, split-K, data gradient, its BatchNorm-backward epilogue, the upsample + concat + 3x3 phase convolutions, the
phase-decomposed stride-2 data gradient vmtl_conv2d_dgrad_s2) and the
dense weight gradient (vmtl_conv2d_wgrad, vmtl_conv1x1_cat_wgrad).  "bf16_pw" is "bf16" PLUS the forward and
data-gradient GEMMs of the pointwise (1x1) family under the same contract (vmtl_conv1x1_fwd, _cat_fwd, _cat_dgrad,
_bn_fwd, _bn_res_fwd, _bnbwd, _bnbwd_add: the MobileNetV3 encoder's expand / project convs and MTAN's attention
modules); with a fused BatchNorm + activation prologue the rounded operand is the fp32 activation the node stores.
Everything else stays fp32 in every mode.

    vision_mtl_amd.set_conv_precision("bf16")        # process-wide
    with vision_mtl_amd.conv_precision("bf16_pw"):   # scoped
        loss = module.training_step(batch, 0)
    loss.backward()                                  # uses the precision its forward ran under

torch.get_float32_matmul_precision() is deliberately NOT consulted: scripts set it to "high" for TF32 elsewhere, and
that must not change this library's numerics.
"""
from __future__ import annotations

import contextlib

# mode -> (VMTL_PREC_* of the implicit-GEMM convolutions and weight gradients, VMTL_PREC_* of the pointwise GEMMs).
# The C ABI has two precision values; the modes are routing: which launches get which.
MODES = {"fp32": (0, 0), "bf16": (1, 0), "bf16_pw": (1, 1)}

_mode = "fp32"


def _check(mode) -> str:
    if mode not in MODES:
        raise ValueError(f"conv precision must be one of {sorted(MODES)}, got {mode!r}")
    return mode


def set_conv_precision(mode: str) -> None:
    """Set the process-wide convolution precision: "fp32" (default), "bf16" or "bf16_pw"."""
    global _mode
    _mode = _check(mode)


def get_conv_precision() -> str:
    return _mode


@contextlib.contextmanager
def conv_precision(mode: str):
    """Run the block under `mode`; the previous setting is restored on exit."""
    global _mode
    prev, _mode = _mode, _check(mode)
    try:
        yield
    finally:
        _mode = prev


def conv_prec_code() -> int:
    """VMTL_PREC_* value of the current setting for the implicit-GEMM convolutions and the weight gradients (what an
    autograd node records in forward)."""
    return MODES[_mode][0]


def pw_prec_code() -> int:
    """VMTL_PREC_* value of the current setting for the pointwise GEMMs (forward and data gradient): 1 only under
    "bf16_pw".  Recorded by the autograd nodes next to conv_prec_code()."""
    return MODES[_mode][1]
