"""-m "not gpu": the host side of the dataset-level evaluation metrics (vision_mtl_amd.metrics.EvalAccumulator) and the
fp64 oracle the GPU tests compare the kernels with."""
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import eval_metrics_oracle as O


def test_oracle_on_a_case_worked_out_by_hand():
    """A 2x3 image, 3 classes; class 2 never occurs and is never predicted, pixel (1, 1) is ignored (255) and its depth
    is invalid (0).
      valid pixels (target, prediction): (0,0) (0,1) (1,1) | (1,1) - (0,1)   -> cm = [[1,2,0],[0,2,0],[0,0,0]]
      class 0: tp 1, support 3, predicted 1 -> IoU 1/3, accuracy 1/3, F1 = 2/(2+2+0) = 1/2
      class 1: tp 2, support 2, predicted 4 -> IoU 2/4, accuracy 1,   F1 = 4/(4+0+2) = 2/3
      depth (p, t): (1,2) (2,2) (4,2) | (.5,1) - (3,4): |d| = 1 0 2 .5 1; ratios 2 1 2 2 4/3"""
    mask = torch.tensor([[0, 0, 1], [1, 255, 0]])
    pred = torch.tensor([[0, 1, 1], [1, 0, 1]])
    p = torch.tensor([[1.0, 2.0, 4.0], [0.5, 1.0, 3.0]])
    t = torch.tensor([[2.0, 2.0, 2.0], [1.0, 0.0, 4.0]])
    cm = O.confusion(pred, mask, 3, ignore_index=255)
    assert cm.tolist() == [[1, 2, 0], [0, 2, 0], [0, 0, 0]]
    acc, mag, margin = O.depth_terms(p, t, min_depth=1e-3)
    ln2, ln34 = math.log(2.0), math.log(0.75)
    want = [5, 4.5, 2.25, 3.0, 6.25, 3 * ln2 ** 2 + ln34 ** 2, -ln2 + ln34, 3 * math.log10(2.0) - math.log10(0.75), 1, 2, 2]
    assert acc[:11].tolist() == pytest.approx(want, rel=1e-14, abs=1e-15) and acc[11:].tolist() == [0.0] * 5
    assert acc[[0, 8, 9, 10]].tolist() == [5, 1, 2, 2]
    assert mag[6] == pytest.approx(3 * ln2 - ln34, rel=1e-14) and mag[1] == acc[1]
    assert margin == pytest.approx((2 - 1.953125) / 1.953125, rel=1e-12)  # the ratio 2 is the closest to a threshold
    m = O.finalize(cm, acc, beta=1.0, ignore_index=255)
    assert m["pixel_acc"] == pytest.approx(3 / 5, rel=1e-14)
    assert m["mean_acc"] == pytest.approx((1 / 3 + 1) / 2, rel=1e-14)
    assert m["miou"] == pytest.approx((1 / 3 + 1 / 2) / 2, rel=1e-14)
    assert m["fbeta"] == pytest.approx((3 * 0.5 + 2 * 2 / 3) / 5, rel=1e-14)
    assert m["iou"][:2].tolist() == pytest.approx([1 / 3, 0.5], rel=1e-14) and math.isnan(m["iou"][2])
    assert m["abs_err"] == pytest.approx(0.9) and m["rel_err"] == pytest.approx(0.45) and m["sq_rel"] == pytest.approx(0.6)
    assert m["rmse"] == pytest.approx(math.sqrt(1.25)) and m["log10"] == pytest.approx(want[7] / 5)
    assert m["rmse_log"] == pytest.approx(math.sqrt(want[5] / 5))
    assert m["silog"] == pytest.approx(math.sqrt(want[5] / 5 - (want[6] / 5) ** 2))
    assert (m["delta1"], m["delta2"], m["delta3"]) == (0.2, 0.4, 0.4) and m["n_valid"] == 5 and m["n_pixels"] == 5
    # the per-step convention scores the absent class 0 instead: (1/3 + 1/2 + 0) / 3
    # an in-range ignore index leaves that class out of both means; a prediction clamped at min_depth
    m1 = O.finalize(cm, acc, ignore_index=1)
    assert m1["miou"] == pytest.approx(1 / 3) and m1["mean_acc"] == pytest.approx(1 / 3) and math.isnan(m1["iou"][1])
    acc0 = O.depth_terms(torch.tensor([0.0]), torch.tensor([1.0]), min_depth=0.5)[0]
    assert acc0[0] == 1 and acc0[1] == 0.5 and acc0[6] == pytest.approx(math.log(0.5))
    # nothing valid: NaN, no exception
    empty = O.finalize(torch.zeros(3, 3, dtype=torch.int64), torch.zeros(16, dtype=torch.float64))
    assert all(math.isnan(empty[k]) for k in O.SCALARS[:14]) and empty["n_valid"] == 0 and empty["iou"].isnan().all()


def test_scalar_names_agree_with_the_product():
    from vision_mtl_amd import metrics as M

    assert M.EVAL_SCALARS == O.SCALARS and M.EVAL_ACC_SIZE == 16


def _module(**kw):
    from vision_mtl_amd.lit_module import MTLModule

    return MTLModule(torch.nn.Conv2d(3, 4, 1), num_classes=4, device="cpu", **kw)


def test_default_module_is_unchanged():
    """The accumulator is a class of its own: MTLModule, its hparams and its checkpoint keys are what they were."""
    plain = _module()
    assert not hasattr(plain, "epoch_accumulators")
    assert set(plain.hparams) == {"num_classes", "optim_dict", "lr", "device", "loss_segm_weight", "loss_depth_weight",
                                  "segm_ignore_index", "segm_class_weights"}
    assert set(plain.state_dict()) == {"model.weight", "model.bias"}


@pytest.mark.parametrize("kw", [dict(num_classes=0), dict(num_classes=65), dict(num_classes=2.0), dict(num_classes=True),
                                dict(num_classes=3, ignore_index=-1), dict(num_classes=3, ignore_index=1.0),
                                dict(num_classes=3, min_depth=-1.0), dict(num_classes=3, min_depth=float("nan")),
                                dict(num_classes=3, beta=0.0), dict(num_classes=3, beta=float("inf"))])
def test_constructor_arguments_are_validated(kw):
    from vision_mtl_amd.metrics import EvalAccumulator

    with pytest.raises(ValueError):
        EvalAccumulator(device="cpu", **kw)


def test_no_cpu_fallback_and_argument_pairs():
    from vision_mtl_amd.metrics import EvalAccumulator

    ea = EvalAccumulator(3, device="cpu")
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.update(segm_pred=z, mask=z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.update(depth_pred=torch.ones(4), depth=torch.ones(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.compute()
    assert ea.cm.sum() == 0 and ea.acc.sum() == 0


def test_state_dict_and_merge_on_the_host():
    from vision_mtl_amd.metrics import EvalAccumulator

    a, b = EvalAccumulator(3, ignore_index=255, device="cpu"), EvalAccumulator(3, ignore_index=255, device="cpu")
    a.cm.fill_(2 ** 40)
    a.acc.copy_(torch.arange(16, dtype=torch.float64) / 7)
    cm_ptr, acc_ptr = b.cm.data_ptr(), b.acc.data_ptr()
    sd = a.state_dict()
    assert set(sd) == {"cm", "acc", "num_classes", "ignore_index", "min_depth", "beta"}
    b.load_state_dict(sd)
    assert torch.equal(b.cm, a.cm) and torch.equal(b.acc, a.acc) and (b.cm.data_ptr(), b.acc.data_ptr()) == (cm_ptr, acc_ptr)
    b.merge(a)
    assert torch.equal(b.cm, 2 * a.cm) and torch.equal(b.acc, 2 * a.acc)
    b.reset()
    assert b.cm.sum() == 0 and b.acc.sum() == 0
    with pytest.raises(ValueError, match="ignore_index"):
        EvalAccumulator(3, device="cpu").load_state_dict(sd)
    with pytest.raises(ValueError, match="num_classes"):
        EvalAccumulator(4, ignore_index=255, device="cpu").load_state_dict(sd)
    with pytest.raises(ValueError, match="cm must be int64"):
        b.load_state_dict(dict(sd, cm=sd["cm"].int()))
    with pytest.raises(ValueError):
        EvalAccumulator(3, beta=2.0, ignore_index=255, device="cpu").merge(a)


def _rank_state(rank):
    g = torch.Generator().manual_seed(40 + rank)
    cm = torch.randint(0, 2 ** 40, (5, 5), generator=g)  # far past int32
    acc = torch.rand(16, generator=g, dtype=torch.float64) * 1e6
    acc[[0, 8, 9, 10]] = torch.randint(0, 2 ** 40, (4,), generator=g).double()
    acc[11:] = 0
    return cm, acc


def _worker(rank, world, port, tmp):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from vision_mtl_amd import metrics as M

    dist.init_process_group("gloo", rank=rank, world_size=world)
    cm, acc = _rank_state(rank)
    M.all_reduce_state(cm, acc)  # the function EvalAccumulator.all_reduce uses
    ea = M.EvalAccumulator(5, device="cpu")
    ea.load_state_dict(dict(ea.state_dict(), cm=_rank_state(rank)[0], acc=_rank_state(rank)[1]))
    ea.all_reduce()
    assert torch.equal(ea.cm, cm) and torch.equal(ea.acc, acc)
    torch.save((cm, acc), f"{tmp}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_state_reduction_over_two_gloo_ranks(tmp_path):
    tmp = str(tmp_path / "state.pt")
    port = 29500 + (os.getpid() % 2000)
    mp.start_processes(_worker, args=(2, port, tmp), nprocs=2, join=True, start_method="spawn")
    (cm0, acc0), (cm1, acc1) = _rank_state(0), _rank_state(1)
    for rank in range(2):  # every rank holds the sum
        cm, acc = torch.load(f"{tmp}.{rank}")
        assert torch.equal(cm, cm0 + cm1)  # exact
        assert torch.equal(acc, acc0 + acc1)  # the fp64 sum; the integer counts in it are exact too
        assert acc[[0, 8, 9, 10]].tolist() == (acc0 + acc1)[[0, 8, 9, 10]].tolist()


def test_all_reduce_without_a_process_group_is_a_no_op():
    from vision_mtl_amd import metrics as M

    cm, acc = _rank_state(0)
    M.all_reduce_state(cm, acc)
    assert torch.equal(cm, _rank_state(0)[0]) and torch.equal(acc, _rank_state(0)[1])
