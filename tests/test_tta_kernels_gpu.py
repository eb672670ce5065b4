"""-m gpu: the three test-time-augmentation kernels (csrc/tta.hip) through the C ABI (vmtl_tta_view, vmtl_tta_accumulate,
vmtl_tta_finish), every launch under poison.patched("guard") and launch_guard.patched().

No tolerance is fixed here.  Per quantity the device is allowed 4 x max(the error of the fp32 CPU restatement against the
fp64 one on the same case, 2^-22 of the reference's maximum) (tests/tta_oracle.py: bar); every test prints the device's
share of its bar.  An arg-max must equal the fp64 one wherever the fp64 top-2 margin is at least 2 x the bar of the map
it is taken on; tests/test_tta_cpu.py checks on the CPU that this exempts at most 1 % of the shared cases' pixels and that
the comparator (tta_oracle.compare) fails on planted defects.  What is specified exactly is compared bit for bit: equal
sizes copy, a flip mirrors, the pad lane is +0.0f, the identity view reproduces the logits and ops.sigmoid, the first
maximum wins, two runs agree.

Not run: pixel counts past 2^31 (the 64-bit index decode), which need buffers of tens of GiB."""
import contextlib

import pytest
import torch

from tests import launch_guard, poison, tta_oracle as O

pytestmark = pytest.mark.gpu

MODE = {"prob": 0, "logit": 1}


def _ops():
    from vision_mtl_amd import ops

    return ops


def _bits(x):
    return x.contiguous().view(torch.int32)


@contextlib.contextmanager
def _guarded():
    with poison.patched("guard") as p, launch_guard.patched():
        yield p


def _rand(*shape, seed, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


# ---- the C ABI on device tensors; outputs start out as the poison sentinel (ops._empty under the guard)
def _view(img, ld, size, flip):
    ops = _ops()
    B, H, W, _ = img.shape
    out = ops._empty((B, size[0], size[1], 4), img)
    ops._k("vmtl_tta_view", img=img, ld=ld, out=out, B=B, H=H, W=W, Ho=size[0], Wo=size[1], flip=int(flip))
    return out


def _accumulate(logits, depth_logits, acc, acc_depth, flip, mode, first, weight=1.0, depth_gain=1.0):
    B, C, h, w = logits.shape
    H, W = acc.shape[2:]
    _ops()._k("vmtl_tta_accumulate", logits=logits, depth_logits=depth_logits, acc=acc, acc_depth=acc_depth, B=B, C=C, h=h,
              w=w, H=H, W=W, flip=int(flip), weight=weight, depth_gain=depth_gain, mode=MODE[mode], first=int(first))


def _finish(acc, acc_depth, inv_weight, size, mode, confidence=True):
    ops = _ops()
    B, C, H, W = acc.shape
    segm = torch.full((B, *size), -7, dtype=torch.int64, device=acc.device)
    depth = None if acc_depth is None else ops._empty((B, *size), acc)
    conf = ops._empty((B, *size), acc) if confidence else None
    ops._k("vmtl_tta_finish", acc=acc, acc_depth=acc_depth, inv_weight=inv_weight, segm=segm, depth=depth, confidence=conf,
           B=B, C=C, H=H, W=W, Ho=size[0], Wo=size[1], mode=MODE[mode])
    return {"segm": segm, "depth": depth, "confidence": conf}


def _merge_on_device(dev, views, base, mode, with_depth=True):
    ops = _ops()
    B, C = views[0][0].shape[:2]
    like = views[0][0].to(dev)
    acc = ops._empty((B, C, *base), like)  # poisoned: first=1 must leave no sentinel
    acc_d = ops._empty((B, *base), like) if with_depth else None
    for k, (z, d, flip, s) in enumerate(views):
        _accumulate(z.to(dev), d.to(dev) if with_depth else None, acc, acc_d, flip, mode, first=k == 0)
    return acc, acc_d


def _cpu(out):
    return {k: None if v is None else v.cpu() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------ view
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("ld", [3, 4])
@pytest.mark.parametrize("src, dst", [((7, 13), (5, 9)), ((16, 32), (32, 64)), ((33, 17), (32, 32))])
def test_view_against_fp64(dev, src, dst, ld, B):
    img = torch.rand(B, *src, 3, generator=torch.Generator().manual_seed(B * 100 + src[0]))
    nchw = img.permute(0, 3, 1, 2)
    x = img if ld == 3 else torch.cat([img, torch.full((B, *src, 1), 7.0)], 3)  # a pad lane that must not travel
    with _guarded():
        for flip in (False, True):
            out = _view(x.to(dev), ld, dst, flip).cpu()
            assert not poison.is_sentinel(out).any()
            assert bool((_bits(out[..., 3]) == 0).all())  # +0.0f bit for bit
            r64, r32 = O.view_image(nchw, dst, flip), O.view_image(nchw, dst, flip, torch.float32)
            err, sh = O.share(out[..., :3].permute(0, 3, 1, 2), r32, r64)
            print(f"view {src}->{dst} ld {ld} B {B} flip {flip}: error {err:.3e}, {sh:.3f} of its bar")
            assert sh <= 1.0


@pytest.mark.parametrize("ld", [3, 4])
def test_view_at_equal_size_is_the_input_and_a_flip_its_exact_mirror(dev, ld):
    B, H, W = 3, 9, 21
    img = _rand(B, H, W, 3, seed=5)
    img[0, 0, 0, 0], img[1, 2, 3, 1], img[2, 8, 20, 2] = float("inf"), -0.0, float("-inf")  # l0 * v + 0 * inf would be NaN
    x = img if ld == 3 else torch.cat([img, torch.full((B, H, W, 1), 7.0)], 3)
    with _guarded():
        same = _view(x.to(dev), ld, (H, W), False).cpu()
        mirror = _view(x.to(dev), ld, (H, W), True).cpu()
    assert torch.equal(_bits(same[..., :3]), _bits(img))
    assert torch.equal(_bits(mirror[..., :3]), _bits(torch.flip(img, [2])))
    assert bool((_bits(same[..., 3]) == 0).all()) and bool((_bits(mirror[..., 3]) == 0).all())


def test_view_through_the_op_feeds_the_model_input_contract(dev):
    ops = _ops()
    img = torch.rand(2, 12, 20, 3, generator=torch.Generator().manual_seed(9))
    with _guarded():
        first = ops.hwc_to_model_input(img.to(dev))            # a (B,3,H,W) view over NHWC storage: ld 4
        v4 = ops.tta_view(first, (8, 16), flip=True)
        v3 = ops.tta_view(img.to(dev), (8, 16), flip=True)     # dataset sample layout: ld 3
        vp = ops.tta_view(img.permute(0, 3, 1, 2).contiguous().to(dev), (8, 16), flip=True)  # plain NCHW: re-laid first
        st = v4._vmtl_nhwc
        assert tuple(v4.shape) == (2, 3, 8, 16) and tuple(st.shape) == (2, 8, 16, 4) and ops.to_nhwc(v4) is st
        assert torch.equal(_bits(v4), _bits(v3)) and torch.equal(_bits(v4), _bits(vp))
    r64 = O.view_image(img.permute(0, 3, 1, 2), (8, 16), True)
    assert O.share(v4.cpu(), O.view_image(img.permute(0, 3, 1, 2), (8, 16), True, torch.float32), r64)[1] <= 1.0


# ------------------------------------------------------------------------------------------------------ accumulate
ACC_VIEWS = ((9, 13, False), (7, 11, True), (12, 20, False), (9, 13, True), (8, 16, True))


def _acc_views(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, C, h, w, generator=g) * 3.0, torch.randn(B, 1, h, w, generator=g) * 1.5, flip, 1.0 + 0.25 * k)
            for k, (h, w, flip) in enumerate(ACC_VIEWS)]


@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("base", [(9, 13), (8, 16)])
@pytest.mark.parametrize("C", [1, 5, 19, 32])
def test_accumulate_against_fp64(dev, C, base, mode):
    views = _acc_views(2, C, seed=C)
    with _guarded():
        # after the first view alone (assigned over a poisoned accumulator), then with every view added
        one, one_d = _merge_on_device(dev, views[:1], base, mode)
        acc, acc_d = _merge_on_device(dev, views, base, mode)
        nod, none = _merge_on_device(dev, views, base, mode, with_depth=False)  # the null depth pair
    assert none is None and torch.equal(_bits(nod), _bits(acc))
    for got, got_d, vs in ((one, one_d, views[:1]), (acc, acc_d, views)):
        assert not poison.is_sentinel(got.cpu()).any() and not poison.is_sentinel(got_d.cpu()).any()
        (a64, d64), (a32, d32) = O.merge(vs, base, mode), O.merge(vs, base, mode, torch.float32)
        (ea, sa), (ed, sd) = O.share(got.cpu(), a32, a64), O.share(got_d.cpu(), d32, d64)
        print(f"accumulate C {C} base {base} {mode}, {len(vs)} view(s): acc error {ea:.3e}, {sa:.3f} of its bar; "
              f"depth error {ed:.3e}, {sd:.3f} of its bar")
        assert sa <= 1.0 and sd <= 1.0


def test_accumulate_weight_and_depth_gain(dev):
    views = _acc_views(1, 5, seed=77)[:3]
    base = (9, 13)
    ops = _ops()
    for mode in O.MODES:
        with _guarded():
            acc, acc_d = ops._empty((1, 5, *base), views[0][0].to(dev)), ops._empty((1, *base), views[0][0].to(dev))
            for k, (z, d, flip, s) in enumerate(views):
                _accumulate(z.to(dev), d.to(dev), acc, acc_d, flip, mode, first=k == 0, weight=0.5 + k, depth_gain=s)
        ref = {}
        for dt in (torch.float64, torch.float32):
            parts = [O.merge_view(z, d, base, flip, mode, 0.5 + k, s, dt) for k, (z, d, flip, s) in enumerate(views)]
            ref[dt] = (parts[0][0] + parts[1][0] + parts[2][0], parts[0][1] + parts[1][1] + parts[2][1])
        sa = O.share(acc.cpu(), ref[torch.float32][0], ref[torch.float64][0])[1]
        sd = O.share(acc_d.cpu(), ref[torch.float32][1], ref[torch.float64][1])[1]
        print(f"weights 0.5, 1.5, 2.5 and depth gains {mode}: {sa:.3f} and {sd:.3f} of their bars")
        assert sa <= 1.0 and sd <= 1.0


def test_identity_view_in_logit_mode_is_the_logits_and_the_sigmoid_node_bit_for_bit(dev):
    ops = _ops()
    z, d = _rand(2, 19, 9, 13, seed=1, std=3.0).to(dev), _rand(2, 1, 9, 13, seed=2, std=4.0).to(dev)
    with _guarded():
        acc, acc_d = ops._empty((2, 19, 9, 13), z), ops._empty((2, 9, 13), z)
        _accumulate(z, d, acc, acc_d, False, "logit", first=True)
        sig = ops.sigmoid(d)
        mirrored, mirrored_d = ops._empty((2, 19, 9, 13), z), ops._empty((2, 9, 13), z)
        _accumulate(torch.flip(z, [3]).contiguous(), torch.flip(d, [3]).contiguous(), mirrored, mirrored_d, True, "logit", first=True)
    assert torch.equal(_bits(acc), _bits(z)) and torch.equal(_bits(acc_d), _bits(sig.view(2, 9, 13)))
    assert torch.equal(_bits(mirrored), _bits(z)) and torch.equal(_bits(mirrored_d), _bits(acc_d))


def test_more_than_32_classes_returns_minus_3(dev):
    ops = _ops()
    z = torch.zeros(1, 33, 4, 4, device=dev)
    acc = torch.zeros(1, 33, 4, 4, device=dev)
    for mode in O.MODES:
        with pytest.raises(RuntimeError, match=r"unsupported configuration \(status -3\)"):
            _accumulate(z, None, acc, None, False, mode, first=True)
        with pytest.raises(RuntimeError, match=r"unsupported configuration \(status -3\)"):
            _finish(acc, None, 1.0, (4, 4), mode)
    with pytest.raises(ValueError, match="classes"):
        ops.tta_accumulate(z, None, acc, None)


# ---------------------------------------------------------------------------------------------------------- finish
@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("size", [(9, 13), (27, 39), (20, 17), (5, 7)])  # equal, 3x, a non-integer ratio, down
@pytest.mark.parametrize("C", [1, 5, 19, 32])
def test_finish_against_fp64(dev, C, size, mode):
    views = _acc_views(2, C, seed=40 + C)[:4]
    acc, acc_d = O.merge(views, (9, 13), mode, torch.float32)  # the device is handed this accumulator
    inv = 1.0 / len(views)
    r64, r32 = O.finish(acc, acc_d, inv, size, mode), O.finish(acc, acc_d, inv, size, mode, torch.float32)
    with _guarded():
        got = _cpu(_finish(acc.to(dev), acc_d.to(dev), inv, size, mode))
        bare = _cpu(_finish(acc.to(dev), None, inv, size, mode, confidence=False))
    assert not poison.is_sentinel(got["depth"]).any() and not poison.is_sentinel(got["confidence"]).any()
    assert bare["depth"] is None and bare["confidence"] is None and torch.equal(bare["segm"], got["segm"])
    assert int(got["segm"].min()) >= 0 and int(got["segm"].max()) < C
    sh = O.compare(got, r32, r64, what=f"finish C {C} -> {size} {mode}")
    print(f"finish C {C} 9x13 -> {size} {mode}: depth {sh['depth']:.3f}, confidence {sh['confidence']:.3f} of their bars; "
          f"tie band {100 * sh['band']:.3f} %")
    if size == (9, 13):  # an exact copy: the depth is inv_weight * acc_depth, rounded once
        assert torch.equal(_bits(got["depth"]), _bits(acc_d * torch.tensor(inv, dtype=torch.float32)))


def test_first_maximum_wins_exactly(dev):
    C = 6
    acc = _rand(2, C, 7, 9, seed=3)
    acc[:, 4] = acc[:, 1]                       # a duplicated channel: wherever it is the maximum, 1 must win over 4
    acc[:, 5] = acc[:, :5].max(1).values        # and a copy of the maximum itself in the last channel
    acc[0, :, 0, 0] = 0.25                      # all equal
    top = acc.max(1, keepdim=True).values
    idx = torch.arange(C).view(1, C, 1, 1).expand_as(acc)
    want = torch.where(acc == top, idx, torch.full_like(idx, C)).min(1).values
    assert int((want == 5).sum()) == 0 and int((want == 4).sum()) == 0 and int((want == 1).sum()) > 0
    with _guarded():
        for mode in O.MODES:
            for conf in (False, True):
                got = _finish(acc.to(dev), None, 0.5, (7, 9), mode, confidence=conf)
                assert torch.equal(got["segm"].cpu(), want), (mode, conf)


def test_finish_beyond_the_grid_cap_strides(dev):
    """2 x 2200 x 2000 output pixels, a thread per column and group of 4 rows, on the 8192 blocks of 256 threads the grid
    is capped at"""
    acc, acc_d = _rand(2, 2, 8, 8, seed=8, std=3.0), torch.rand(2, 8, 8, generator=torch.Generator().manual_seed(9))
    size = (2200, 2000)
    assert 2 * (size[0] // 4) * size[1] > 8192 * 256
    r64, r32 = O.finish(acc, acc_d, 0.5, size, "logit"), O.finish(acc, acc_d, 0.5, size, "logit", torch.float32)
    with _guarded():
        got = _cpu(_finish(acc.to(dev), acc_d.to(dev), 0.5, size, "logit"))
    assert not poison.is_sentinel(got["depth"]).any() and int(got["segm"].min()) >= 0
    print("finish 8x8 -> 2200x2000:", O.compare(got, r32, r64, what="finish beyond the grid cap"))


# ------------------------------------------------------------------------------------------- composed, determinism
@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("name", sorted(O.CASES))
def test_merge_and_finish_of_the_shared_cases(dev, name, mode):
    c = O.case(name)
    r64, r32 = O.reference(name, mode), O.reference(name, mode, torch.float32)
    with _guarded():
        acc, acc_d = _merge_on_device(dev, c["views"], c["base"], mode)
        got = _cpu(_finish(acc, acc_d, 1.0 / len(c["views"]), c["out"], mode))
        again_acc, again_d = _merge_on_device(dev, c["views"], c["base"], mode)
        again = _cpu(_finish(again_acc, again_d, 1.0 / len(c["views"]), c["out"], mode))
    sa, sd = O.share(acc.cpu(), r32["acc"], r64["acc"])[1], O.share(acc_d.cpu(), r32["acc_depth"], r64["acc_depth"])[1]
    sh = O.compare(got, r32, r64, what=f"{name} {mode}")
    print(f"{name} {mode}: acc {sa:.3f}, acc_depth {sd:.3f}, depth {sh['depth']:.3f}, confidence {sh['confidence']:.3f} of "
          f"their bars; tie band {100 * sh['band']:.3f} %")
    assert sa <= 1.0 and sd <= 1.0
    # two runs are bit-identical
    assert torch.equal(_bits(acc), _bits(again_acc)) and torch.equal(_bits(acc_d), _bits(again_d))
    assert torch.equal(got["segm"], again["segm"])
    assert torch.equal(_bits(got["depth"]), _bits(again["depth"]))
    assert torch.equal(_bits(got["confidence"]), _bits(again["confidence"]))
