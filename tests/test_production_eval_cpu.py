"""No GPU: what tests/test_production_eval_step_gpu.py relies on, checked on the oracles alone.

1. The exempt-share condition.  compare_step exempts a pixel from the arg-max comparison only where the fp64 top-2 logit
   margin is below 2 x bar x max|z|, and caps the exempt share at 1 %.  For every model kind and both stages the fp64 and
   fp32 oracles run at batch 2 of the production spatial size; the fp32 oracle stands in for "an implementation within the
   bar".  The share must stay under the cap and fp32 and fp64 arg-max must agree outside it: the reference alone meets the
   condition, with the inputs, BatchNorm affine parameters and running statistics the GPU test uses.
2. The comparator is not blind: the fp64 output against copies corrupted the way kernels go wrong must fail, the
   uncorrupted fp32 oracle must pass.
3. tests/production.py::census validates its stage argument; "train" stays the default.
"""
import functools
import inspect

import pytest
import torch

from tests.production import STAGES, census, production_census
from tests.test_production_eval_step_gpu import (EXEMPT_CAP, compare_step, exempt_pixels, is_buffer, oracle_runs,
                                                 prepare_model)

# model kind -> (build kind, classes, channel-wise stitching, production spatial size)
KINDS = {"basic": ("basic", 19, None, 128, 256), "resnet34": ("basic_resnet34", 19, None, 128, 256),
         "csnet_layer": ("csnet", 19, False, 128, 256), "csnet_channel": ("csnet", 19, True, 128, 256),
         "mtan": ("mtan", 14, None, 256, 256)}


@functools.lru_cache(maxsize=None)
def _runs(name, stage):
    from oracle.losses import synthetic_batch

    kind, C, cw, H, W = KINDS[name]
    model = prepare_model(kind, C, cw)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    batch = synthetic_batch(2, H, W, C, seed=11, masked=0.1)
    ref, (r32,) = oracle_runs(kind, sd0, batch, stage, threads=(torch.get_num_threads(),))
    return ref, r32, {k: v.clone() for k, v in sd0.items() if is_buffer(k)}


@pytest.mark.parametrize("stage", ["val", "predict"])
@pytest.mark.parametrize("name", list(KINDS))
def test_the_oracle_alone_meets_the_exempt_share_condition(name, stage):
    ref, r32, buffers0 = _runs(name, stage)
    rep = compare_step(stage, r32, ref, [r32], buffers0, f"{name} [{stage}] fp32 oracle")
    exempt = exempt_pixels(ref["segm"], rep["bar_used"])
    disagree = r32["pred"] != ref["pred"]
    print(f"{name} [{stage}]: exempt pixels {rep['exempt']:.4%} at bar {rep['bar_used']:.1e} ({float(exempt_pixels(ref['segm'], 1e-3).double().mean()):.3%} "
          f"at 1e-3); fp32 vs fp64 arg-max disagreements: {int(disagree.sum())} of {disagree.numel()}, "
          f"{int((disagree & ~exempt).sum())} outside the exempt pixels; fp32 oracle error: "
          + ", ".join(f"{k} {v:.1e}" for k, v in sorted(rep["worst"].items())))
    assert rep["exempt"] <= EXEMPT_CAP
    assert not bool((disagree & ~exempt).any())


def _copy(r):
    return {k: ({n: t.clone() for n, t in v.items()} if isinstance(v, dict) else v.clone() if isinstance(v, torch.Tensor) else v)
            for k, v in r.items()}


def _last_image_shifted(r):
    for t, dim in (("segm", 3), ("depth", 2)):
        r[t][-1] = torch.roll(r[t][-1], 1, dims=dim - 1)
    r["pred"] = r["segm"].argmax(1)


def _channel_scaled(r):
    c = int(r["segm"].abs().amax((0, 2, 3)).argmax())
    r["segm"][:, c] *= 1.0 + 1e-3


def _tail_columns_zeroed(r):
    r["segm"][1, :, 4:8, -32:] = 0.0
    r["depth"][1, 4:8, -32:] = 0.0


def _variance_off(r):
    k = sorted(k for k in r["buffers"] if "running_var" in k)[len(r["buffers"]) // 6]
    r["buffers"][k][0] *= 1.01


def _buffer_moved(r):
    k = sorted(k for k in r["buffers"] if "running_mean" in k)[-1]
    r["buffers"][k][-1] += 1e-6


def _counter_stuck(r):
    k = sorted(k for k in r["buffers"] if "num_batches_tracked" in k)[0]
    r["buffers"][k] -= 1


def _counter_moved(r):
    k = sorted(k for k in r["buffers"] if "num_batches_tracked" in k)[0]
    r["buffers"][k] += 1


CORRUPTIONS = [("val", _last_image_shifted), ("predict", _last_image_shifted), ("val", _channel_scaled),
               ("predict", _channel_scaled), ("val", _tail_columns_zeroed), ("predict", _tail_columns_zeroed),
               ("val", _variance_off), ("predict", _buffer_moved), ("val", _counter_stuck), ("predict", _counter_moved)]


@pytest.mark.parametrize("stage,corrupt", CORRUPTIONS, ids=[f"{s}-{f.__name__.strip('_')}" for s, f in CORRUPTIONS])
def test_the_comparator_is_not_blind(stage, corrupt):
    ref, r32, buffers0 = _runs("basic", stage)
    compare_step(stage, _copy(ref), ref, [r32], buffers0, "fp64 against itself")
    compare_step(stage, r32, ref, [r32], buffers0, "the uncorrupted fp32 oracle")
    bad = _copy(ref)
    corrupt(bad)
    with pytest.raises(AssertionError) as e:
        compare_step(stage, bad, ref, [r32], buffers0, corrupt.__name__.strip("_"))
    print(str(e.value).splitlines()[0])


def test_census_validates_its_stage():
    assert STAGES == ("train", "val", "predict")
    for f in (census, production_census):
        assert inspect.signature(f).parameters["stage"].default == "train"
    with pytest.raises(ValueError, match="stage"):
        census("basic", 2, 64, 64, stage="test_time")
    with pytest.raises(ValueError, match="stage"):
        production_census("basic_128x256_bs8", stage="eval")
