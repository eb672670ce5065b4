"""The device-side training augmentation without a GPU: the C ABI of vmtl_augment_draw / vmtl_augment_apply (bad
arguments are refused before anything reaches the GPU), the host restatement of the draw, DeviceAugment's argument
checks and state, and the defaults that keep today's step."""
import ctypes
import inspect

import pytest
import torch

SCALES = (1.0, 1.2, 1.5)
# every (H, W) of tests/test_augment_gpu.py
GEOMETRIES = [(13, 18), (37, 70), (32, 48)]


def test_abi_declared_exported_and_refuses_bad_arguments():
    from vision_mtl_amd._lib import lib, parse_header

    protos = parse_header()
    L = lib()
    for name in ("vmtl_augment_draw", "vmtl_augment_apply"):
        assert name in protos and hasattr(L._dll, name)
    _, argtypes, names = protos["vmtl_augment_draw"]
    assert names == ["state", "params", "crop_hw", "B", "H", "W", "S", "flip_threshold", "brightness", "stream"]
    assert argtypes[names.index("brightness")] is ctypes.c_float
    P = 4096  # a fake, aligned address: never dereferenced, every call below is refused first
    ok = dict(state=P, params=P, crop_hw=P, B=2, H=8, W=8, S=3, flip_threshold=1 << 23, brightness=0.0, stream=None)
    f = L.raw("vmtl_augment_draw")
    for change in [dict(state=None), dict(params=None), dict(crop_hw=None), dict(B=0), dict(H=0), dict(W=-1), dict(S=0),
                   dict(S=9), dict(flip_threshold=-1), dict(flip_threshold=(1 << 24) + 1), dict(brightness=-0.1),
                   dict(brightness=1.0), dict(brightness=float("nan")), dict(params=P + 4)]:
        kw = dict(ok, **change)
        assert f(*[kw[n] for n in names]) == -1, change

    _, _, names = protos["vmtl_augment_apply"]
    assert names == ["img", "ld", "mask", "depth", "params", "scales", "crop_hw", "img_out", "mask_out", "depth_out", "B",
                     "H", "W", "S", "stream"]
    n = 2 * 8 * 8
    img, mask, depth, out, mout, dout = (P + k * (1 << 20) for k in range(6))
    ok = dict(img=img, ld=4, mask=mask, depth=depth, params=P, scales=P, crop_hw=P, img_out=out, mask_out=mout,
              depth_out=dout, B=2, H=8, W=8, S=3, stream=None)
    f = L.raw("vmtl_augment_apply")
    bad = [dict(img=None), dict(mask=None), dict(depth=None), dict(params=None), dict(scales=None), dict(crop_hw=None),
           dict(img_out=None), dict(mask_out=None), dict(depth_out=None), dict(ld=2), dict(ld=5), dict(B=0), dict(H=0),
           dict(W=0), dict(S=0), dict(S=9), dict(B=65536), dict(img_out=out + 4), dict(img=img + 4),
           # an output that aliases its input: the same buffer, and ranges that merely overlap
           dict(img_out=img), dict(mask_out=mask), dict(depth_out=depth), dict(img_out=img + 16 * n - 16),
           dict(mask_out=mask + 8 * n - 8), dict(depth=dout + 4 * n - 4), dict(ld=3, img_out=img + 12 * n - 16)]
    for change in bad:
        kw = dict(ok, **change)
        assert f(*[kw[k] for k in names]) == -1, change


def test_host_draw_is_deterministic_and_in_range():
    from vision_mtl_amd.data import augment_crop_table, augment_params_host

    for H, W in GEOMETRIES:
        crops = augment_crop_table(H, W, SCALES)
        assert crops[0] == (H, W) and all(1 <= h <= H and 1 <= w <= W for h, w in crops)
        a = augment_params_host(11, 7, 64, H, W, SCALES, 0.5, 0.2)
        assert a.dtype == torch.int32 and tuple(a.shape) == (64, 8)
        assert torch.equal(a, augment_params_host(11, 7, 64, H, W, SCALES, 0.5, 0.2))
        assert not torch.equal(a, augment_params_host(11, 8, 64, H, W, SCALES, 0.5, 0.2))
        assert not torch.equal(a, augment_params_host(12, 7, 64, H, W, SCALES, 0.5, 0.2))
        assert torch.equal(a[:16], augment_params_host(11, 7, 16, H, W, SCALES, 0.5, 0.2))  # a row depends on b alone
        assert a[:, 5:].eq(0).all()
        seen = set()
        for si, top, left, flip, gbits in a[:, :5].tolist():
            h, w = crops[si]
            assert 0 <= si < 3 and 0 <= top <= H - h and 0 <= left <= W - w and flip in (0, 1)
            seen.add(si)
        assert seen == {0, 1, 2}
        gain = a[:, 4].contiguous().view(torch.float32)
        assert ((gain >= 0.8) & (gain < 1.2)).all() and gain.unique().numel() > 32
    assert augment_crop_table(13, 18, SCALES) == [(13, 18), (10, 15), (8, 12)]
    # p_flip at its ends, brightness 0: no flip / every flip, gain exactly 1
    for p, want in ((0.0, 0), (1.0, 1)):
        a = augment_params_host(3, 0, 256, 13, 18, SCALES, p, 0.0)
        assert a[:, 3].eq(want).all() and a[:, 4].contiguous().view(torch.float32).eq(1.0).all()
    # 64-bit wrap-around of seed and counter
    big = augment_params_host((1 << 63) - 1, (1 << 63) - 1, 8, 13, 18)
    assert big[:, 0].max() <= 2 and big[:, 0].min() >= 0


def test_host_draw_statistics():
    """The bounds the GPU test holds the device draw to (B = 4096, seed 11): each is more than 6 sigma wide."""
    from vision_mtl_amd.data import augment_params_host

    a = augment_params_host(11, 0, 4096, 37, 70, SCALES, 0.5, 0.0)
    assert 0.45 <= a[:, 3].float().mean().item() <= 0.55
    for si in range(3):
        assert 0.28 <= a[:, 0].eq(si).float().mean().item() <= 0.39
    rows = a[a[:, 0] == 2]  # 37x70 at scale 1.5: a 24x46 window, offsets in [0, 13] x [0, 24]
    assert set(rows[:, 1].tolist()) == set(range(14)) and set(rows[:, 2].tolist()) == set(range(25))


def test_constructor_checks():
    from vision_mtl_amd.data import DeviceAugment

    a = DeviceAugment()
    assert a.scales == (1.0, 1.2, 1.5) and a.p_flip == 0.5 and a.brightness == 0.0 and a.seed == 0 and a.counter == 0
    assert a.last_params is None
    DeviceAugment(scales=[1.0] * 8, p_flip=0.0, brightness=0.99, seed=5)
    DeviceAugment(scales=(1.0,), p_flip=1.0)
    for kw in [dict(scales=()), dict(scales=[1.0] * 9), dict(scales=(0.9, 1.0)), dict(scales=(1.0, float("nan"))),
               dict(scales=(1.0, float("inf"))), dict(scales=1.5), dict(p_flip=-0.1), dict(p_flip=1.5),
               dict(brightness=-0.1), dict(brightness=1.0), dict(seed=-1), dict(seed=1.5), dict(seed=1 << 63)]:
        with pytest.raises(ValueError):
            DeviceAugment(**kw)


def test_cpu_tensors_are_refused():
    from tests.augment_oracle import make_params, sample_batch
    from vision_mtl_amd import ops
    from vision_mtl_amd.data import DeviceAugment

    b = sample_batch(2, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceAugment()(b)
    params = make_params([(0, 0, 0, 0, 1.0)] * 2)
    scales, crop = torch.tensor([1.0]), torch.tensor([[8, 8]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.augment_apply(b["img"], b["mask"], b["depth"], params, scales, crop)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.augment_apply(b["img"].permute(0, 2, 3, 1).contiguous(), b["mask"], b["depth"], params, scales, crop)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.augment_draw(torch.zeros(2, dtype=torch.int64), params, crop, 8, 8)


def test_state_dict_round_trip():
    from vision_mtl_amd.data import DeviceAugment

    a = DeviceAugment(seed=11)
    a.set_counter(123)
    assert a.counter == 123 and a.state_dict() == {"seed": 11, "counter": 123}
    b = DeviceAugment(seed=0)
    b.load_state_dict(a.state_dict())
    assert b.seed == 11 and b.counter == 123 and b.state_dict() == a.state_dict()
    for bad in (-1, 1.0, 1 << 63, True):
        with pytest.raises(ValueError):
            a.set_counter(bad)
    with pytest.raises(ValueError):
        b.load_state_dict({"seed": -3, "counter": 0})
    assert b.state_dict() == {"seed": 11, "counter": 123}  # a refused state leaves the object as it was


def test_defaults_keep_todays_step():
    from vision_mtl_amd.graphed import GraphedEval, GraphedStep
    from vision_mtl_amd.lit_module import MTLModule

    module = MTLModule(torch.nn.Linear(2, 2), num_classes=3, device="cpu")
    assert module.train_augment is None
    assert "train_augment" in inspect.getsource(GraphedStep) and "train_augment" not in inspect.getsource(GraphedEval)
    for step in (MTLModule.validation_step, MTLModule.test_step, MTLModule.predict_step, MTLModule.shared_step):
        assert "train_augment" not in inspect.getsource(step)
