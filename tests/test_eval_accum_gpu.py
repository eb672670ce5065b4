"""-m gpu: the dataset-level metric kernels (csrc/eval_accum.hip) through metrics.EvalAccumulator against their fp64
definition on the CPU (tests/eval_metrics_oracle.py).

What is held: the confusion matrix and the four counts EXACTLY; every floating sum within 1e-9 * sum|term| of the oracle's
(each fp64 term is good to about an ulp, and N <= 2^22 additions give at worst N * 2^-53 = 4.7e-10); finalized values
within 1e-9 relative; NaNs in the same places.  The delta counts can only be exact when no ratio sits on a threshold:
that is a condition on the inputs, asserted on the oracle's side (`margin`).

Pixel counts: 91 (scalar tail, less than one workgroup), 5 883 (odd, several workgroups), 2 * 1024 * 1024 + 3 (past
the grid cap of 1024 workgroups x 1024 pixels: the stride loop runs), and a depth pair offset by one float (unaligned
base: the scalar path)."""
import functools
import math

import pytest
import torch

from tests import eval_metrics_oracle as O

pytestmark = pytest.mark.gpu

SMALL, ODD, BIG = 1 * 7 * 13, 3 * 37 * 53, 2 * 1024 * 1024 + 3
MARGIN = 1e-10


@functools.lru_cache(maxsize=None)
def _inputs(P, seed, C):
    """(segm_pred, mask, depth_pred, depth) on the CPU; read-only, shared between the tests."""
    g = torch.Generator().manual_seed(seed)
    depth_pred = torch.sigmoid(1.5 * torch.randn(P, generator=g))  # a few below min_depth = 1e-3 at the large size
    depth = 0.05 + 0.95 * torch.rand(P, generator=g)
    depth[torch.rand(P, generator=g) < 0.2] = 0.0
    mask = torch.randint(0, C, (P,), generator=g)
    segm_pred = torch.where(torch.rand(P, generator=g) < 0.6, mask, torch.randint(0, C, (P,), generator=g))
    return segm_pred, mask, depth_pred, depth


def _acc(dev, C, **kw):
    from vision_mtl_amd.metrics import EvalAccumulator

    return EvalAccumulator(C, device=dev, **kw)


def _check_state(ea, cm_ref, acc_ref, mag, margin):
    assert margin >= MARGIN, f"a ratio sits on a delta threshold (relative distance {margin:.1e}): choose another seed"
    assert torch.equal(ea.cm.cpu(), cm_ref)
    acc = ea.acc.cpu()
    print("acc", acc.tolist(), "ref", acc_ref.tolist())
    for slot in O.COUNT_SLOTS:
        assert acc[slot] == acc_ref[slot], (slot, acc[slot], acc_ref[slot])
    for slot in O.SUM_SLOTS:
        assert abs(float(acc[slot] - acc_ref[slot])) <= 1e-9 * float(mag[slot]), (slot, acc[slot], acc_ref[slot])
    assert acc[11:].tolist() == [0.0] * 5


def _check_final(got, ref):
    for k in O.SCALARS:
        print(k, got[k], ref[k])
        if math.isnan(ref[k]):
            assert math.isnan(got[k]), (k, got[k])
        else:
            assert abs(got[k] - ref[k]) <= 1e-9 * abs(ref[k]), (k, got[k], ref[k])
    assert torch.equal(got["iou"].isnan(), ref["iou"].isnan())
    keep = ~ref["iou"].isnan()
    assert got["iou"].dtype == torch.float64 and not got["iou"].is_cuda
    assert ((got["iou"][keep] - ref["iou"][keep]).abs() <= 1e-9 * ref["iou"][keep].abs()).all()


CASES = [  # P, seed, C, ignore_index, min_depth, what is done to the labels
    (SMALL, 0, 19, None, 1e-3, "plain"),
    (SMALL, 1, 14, 255, 1e-3, "ignore255"),
    (ODD, 0, 19, None, 1e-3, "absent"),
    (ODD, 1, 14, 255, 1e-3, "ignore255"),
    (ODD, 2, 19, 3, 0.1, "out_of_range"),
    (ODD, 3, 14, 5, 1e-3, "absent"),
    (BIG, 0, 19, None, 1e-3, "plain"),
    (BIG, 1, 14, 255, 0.1, "ignore255"),
]


def _labels(segm_pred, mask, C, what):
    segm_pred, mask = segm_pred.clone(), mask.clone()
    if what == "ignore255":
        mask[::7] = 255
    elif what == "absent":  # class 2 is neither a target nor a prediction: its IoU is NaN and the means leave it out
        mask[mask == 2] = 1
        segm_pred[segm_pred == 2] = 0
    elif what == "out_of_range":
        mask[::11], mask[1::13], segm_pred[2::17], segm_pred[3::19] = -1, C, 300, -5
    return segm_pred, mask


@pytest.mark.parametrize("P,seed,C,ign,min_depth,what", CASES)
def test_one_update_matches_the_oracle(dev, P, seed, C, ign, min_depth, what):
    segm_pred, mask, depth_pred, depth = _inputs(P, seed, C)
    segm_pred, mask = _labels(segm_pred, mask, C, what)
    cm_ref = O.confusion(segm_pred, mask, C, ign)
    acc_ref, mag, margin = O.depth_terms(depth_pred, depth, min_depth)
    if min_depth == 0.1:
        assert int((depth_pred < min_depth).sum()) > 0  # the clamp is exercised
    ea = _acc(dev, C, ignore_index=ign, min_depth=min_depth)
    ea.update(segm_pred=segm_pred.to(dev), mask=mask.to(dev), depth_pred=depth_pred.to(dev), depth=depth.to(dev))
    _check_state(ea, cm_ref, acc_ref, mag, margin)
    _check_final(ea.compute(), O.finalize(cm_ref, acc_ref, 1.0, ign))
    if what == "absent":
        assert math.isnan(float(ea.compute()["iou"][2]))


@pytest.mark.parametrize("P", [SMALL, ODD])
@pytest.mark.parametrize("use_valid", [False, True])
def test_unaligned_depth_pair_and_valid_mask(dev, P, use_valid):
    """The depth pair starts one float past a 16-byte boundary (scalar path); with `valid`, an explicit uint8 / bool mask
    (a subset of the positive targets) takes the place of the min_depth rule - aligned, the mask is read four at a time."""
    _, _, depth_pred, depth = _inputs(P, 2, 19)
    g = torch.Generator().manual_seed(9)
    valid = (depth > 0) & (torch.rand(P, generator=g) < 0.7) if use_valid else None
    acc_ref, mag, margin = O.depth_terms(depth_pred, depth, 1e-3, valid)
    for offset in (1, 0):
        dp, dt = torch.zeros(P + 4, device=dev), torch.zeros(P + 4, device=dev)
        dp[offset:offset + P], dt[offset:offset + P] = depth_pred.to(dev), depth.to(dev)
        assert dp[offset:].data_ptr() % 16 == 4 * offset
        for v in ([None] if valid is None else [valid.to(dev), valid.to(torch.uint8).to(dev)]):
            ea = _acc(dev, 19)
            ea.update(depth_pred=dp[offset:offset + P], depth=dt[offset:offset + P], valid=v)
            _check_state(ea, torch.zeros(19, 19, dtype=torch.int64), acc_ref, mag, margin)
            got = ea.compute()
            _check_final(got, O.finalize(torch.zeros(19, 19, dtype=torch.int64), acc_ref))
            assert math.isnan(got["miou"]) and got["iou"].isnan().all()  # no segmentation part: NaN, no fault


def test_batch_without_valid_depth_then_a_valid_one(dev):
    segm_pred, mask, depth_pred, depth = _inputs(ODD, 0, 19)
    ea = _acc(dev, 19)
    ea.update(depth_pred=depth_pred.to(dev), depth=torch.zeros(ODD, device=dev))
    assert ea.acc.cpu().tolist() == [0.0] * 16
    got = ea.compute()
    assert all(math.isnan(got[k]) for k in O.SCALARS[:14]) and got["n_valid"] == 0 and got["n_pixels"] == 0
    ea.update(segm_pred=segm_pred.to(dev), mask=mask.to(dev), depth_pred=depth_pred.to(dev), depth=depth.to(dev))
    cm_ref = O.confusion(segm_pred, mask, 19)
    acc_ref, mag, margin = O.depth_terms(depth_pred, depth)
    _check_state(ea, cm_ref, acc_ref, mag, margin)
    _check_final(ea.compute(), O.finalize(cm_ref, acc_ref))


@pytest.mark.parametrize("ign", [None, 255, 3])
def test_step_matrix_form_equals_pixel_form(dev, ign):
    from vision_mtl_amd import metrics as M

    segm_pred, mask, depth_pred, depth = _inputs(ODD, 1, 19)
    segm_pred, mask = _labels(segm_pred, mask, 19, "ignore255")
    a, b = _acc(dev, 19, ignore_index=ign), _acc(dev, 19, ignore_index=ign)
    sp, m, dp, dt = segm_pred.to(dev), mask.to(dev), depth_pred.to(dev), depth.to(dev)
    for _ in range(2):
        a.update(segm_pred=sp, mask=m, depth_pred=dp, depth=dt)
        b.update(step_cm=M.confusion_matrix(sp, m, 19, ignore_index=ign), depth_pred=dp, depth=dt)
    assert torch.equal(a.cm, b.cm) and torch.equal(a.acc, b.acc) and int(a.cm.sum()) > 0
    assert torch.equal(a.cm.cpu(), 2 * O.confusion(segm_pred, mask, 19, ign))
    c = _acc(dev, 19, ignore_index=ign)
    c.update(step_cm=M.confusion_matrix(sp, m, 19, ignore_index=ign))  # the segmentation part alone
    assert torch.equal(2 * c.cm, a.cm) and c.acc.cpu().tolist() == [0.0] * 16


def _three(dev, C=19):
    parts = [_inputs(ODD, 0, C), _inputs(SMALL, 1, C), _inputs(ODD, 2, C)]
    return parts, [tuple(x.to(dev) for x in p) for p in parts]


def _run(ea, batches):
    for sp, m, dp, dt in batches:
        ea.update(segm_pred=sp, mask=m, depth_pred=dp, depth=dt)
    return ea


def test_three_updates_equal_the_oracle_on_the_concatenation(dev):
    parts, batches = _three(dev)
    sp, m, dp, dt = (torch.cat([p[i] for p in parts]) for i in range(4))
    cm_ref = O.confusion(sp, m, 19)
    acc_ref, mag, margin = O.depth_terms(dp, dt)
    ea = _run(_acc(dev, 19), batches)
    _check_state(ea, cm_ref, acc_ref, mag, margin)
    _check_final(ea.compute(), O.dataset_metrics(sp, m, dp, dt, 19))
    # two identical runs: bit-identical state (no floating-point atomics); also at the size where the stride loop runs
    again = _run(_acc(dev, 19), batches)
    assert torch.equal(again.cm, ea.cm) and torch.equal(again.acc.view(torch.int64), ea.acc.view(torch.int64))
    big = tuple(x.to(dev) for x in _inputs(BIG, 0, 19))
    one, two = _run(_acc(dev, 19), [big]), _run(_acc(dev, 19), [big])
    assert torch.equal(one.acc.view(torch.int64), two.acc.view(torch.int64)) and torch.equal(one.cm, two.cm)


def test_merge_reset_and_state_dict(dev):
    _, batches = _three(dev)
    whole = _run(_acc(dev, 19), batches)
    first, second = _run(_acc(dev, 19), batches[:2]), _run(_acc(dev, 19), batches[2:])
    first.merge(second)
    assert torch.equal(first.cm, whole.cm)
    a, b = first.acc.cpu(), whole.acc.cpu()
    assert ((a - b).abs() <= 1e-12 * b.abs()).all() and a[[0, 8, 9, 10]].tolist() == b[[0, 8, 9, 10]].tolist()
    # state_dict round trip: exact, into the same storage
    other = _acc(dev, 19)
    ptrs = (other.cm.data_ptr(), other.acc.data_ptr())
    other.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in whole.state_dict().items()})
    assert torch.equal(other.cm, whole.cm) and torch.equal(other.acc.view(torch.int64), whole.acc.view(torch.int64))
    assert (other.cm.data_ptr(), other.acc.data_ptr()) == ptrs
    assert other.compute()["miou"] == whole.compute()["miou"]
    with pytest.raises(ValueError):
        _acc(dev, 14).load_state_dict(whole.state_dict())
    with pytest.raises(ValueError):
        _acc(dev, 19, ignore_index=255).merge(whole)
    whole.reset()
    assert int(whole.cm.abs().sum()) == 0 and whole.acc.cpu().tolist() == [0.0] * 16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        whole.update(segm_pred=torch.zeros(4, dtype=torch.int64), mask=torch.zeros(4, dtype=torch.int64))


def test_a_cell_counts_past_int32(dev):
    """2^31 pixels is 65 536 images at 128x256: an int32 matrix cannot hold an evaluation set."""
    ea = _acc(dev, 19)
    sd = ea.state_dict()
    sd["cm"][4, 7] = 2 ** 31 - 10
    ea.load_state_dict(sd)
    mask = torch.full((100,), 4, dtype=torch.int64, device=dev)
    ea.update(segm_pred=torch.full_like(mask, 7), mask=mask)
    assert int(ea.cm[4, 7]) == 2 ** 31 + 90 and int(ea.cm.sum()) == 2 ** 31 + 90
    from vision_mtl_amd import metrics as M

    ea.update(step_cm=M.confusion_matrix(torch.full_like(mask, 7), mask, 19))
    assert int(ea.cm[4, 7]) == 2 ** 31 + 190
    assert ea.compute()["n_pixels"] == 2 ** 31 + 190


def test_update_makes_no_copy_of_the_step_tensors(dev):
    """The (B,H,W,1) view postprocess_raw_out makes of a (B,1,H,W) map is dense in pixel order: it goes to the kernel as
    it is, as does a (B,H,W,1) target."""
    from vision_mtl_amd.metrics import EvalAccumulator

    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 1, 5, 7, generator=g).to(dev)
    view = x.permute(0, 2, 3, 1)
    assert EvalAccumulator._dense(view, torch.float32, "x").data_ptr() == x.data_ptr()
    ea = _acc(dev, 3)
    t = (0.1 + torch.rand(2, 5, 7, 1, generator=g)).to(dev)
    ea.update(depth_pred=view, depth=t)
    acc_ref, mag, margin = O.depth_terms(x.cpu(), t.cpu())
    _check_state(ea, torch.zeros(3, 3, dtype=torch.int64), acc_ref, mag, margin)
    with pytest.raises(ValueError):
        ea.update(depth_pred=view, depth=t[:1])
    with pytest.raises(TypeError):
        ea.update(segm_pred=torch.zeros(4, device=dev), mask=torch.zeros(4, dtype=torch.int64, device=dev))
