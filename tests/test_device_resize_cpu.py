"""The NYUv2 device transform without a GPU: data.collate_raw, data.DeviceTransform's argument checks, the C ABI of
vmtl_nyuv2_resize (bad arguments are refused before anything reaches the GPU) and the new hooks of upload_batch and
MTLModule, whose defaults keep today's behaviour."""
import ctypes
import inspect

import numpy as np
import pytest
import torch


def _raw(H=6, W=8, depth_dtype=np.uint16, seed=0):
    g = np.random.default_rng(seed)
    return {"img": g.integers(0, 256, (H, W, 3), dtype=np.uint8), "mask": g.integers(0, 14, (H, W), dtype=np.uint8),
            "depth": g.integers(0, 60000, (H, W)).astype(depth_dtype)}


@pytest.mark.parametrize("depth_dtype", [np.uint16, np.int32])
def test_collate_raw_keeps_dtypes_and_shapes(depth_dtype):
    from vision_mtl_amd.data import collate_raw

    samples = [_raw(depth_dtype=depth_dtype, seed=i) for i in range(3)]
    samples[1] = {k: torch.from_numpy(v) for k, v in samples[1].items()}  # numpy and torch samples mix
    out = collate_raw(samples, pin=False)
    assert out["img"].dtype == torch.uint8 and tuple(out["img"].shape) == (3, 6, 8, 3)
    assert out["mask"].dtype == torch.uint8 and tuple(out["mask"].shape) == (3, 6, 8)
    want = torch.uint16 if depth_dtype is np.uint16 else torch.int32
    assert out["depth"].dtype == want and tuple(out["depth"].shape) == (3, 6, 8)
    for i, s in enumerate(samples):
        for k in ("img", "mask", "depth"):
            assert torch.equal(out[k][i].to(torch.int64), torch.as_tensor(np.asarray(s[k])).to(torch.int64))


def test_collate_raw_rejects_bad_input():
    from vision_mtl_amd.data import collate_raw

    good = _raw()
    bad = [
        dict(good, img=good["img"].astype(np.float32)),        # already converted
        dict(good, mask=good["mask"].astype(np.int64)),
        dict(good, depth=good["depth"].astype(np.float32)),
        dict(good, img=good["img"][..., :2]),                  # not 3 channels
        dict(good, mask=good["mask"][..., None]),              # wrong rank
        dict(good, depth=good["depth"][:5]),                   # size differs inside the sample
        {k: v for k, v in good.items() if k != "depth"},
    ]
    for b in bad:
        with pytest.raises(ValueError):
            collate_raw([good, b], pin=False)
    with pytest.raises(ValueError):
        collate_raw([good, _raw(H=7)], pin=False)              # samples of different sizes
    with pytest.raises(ValueError):
        collate_raw([good, _raw(depth_dtype=np.int32)], pin=False)  # mixed depth dtypes
    with pytest.raises(ValueError):
        collate_raw([], pin=False)


def test_device_transform_arguments():
    from vision_mtl_amd.data import DeviceTransform

    t = DeviceTransform()
    assert t.size == (256, 256) and t.max_depth == 10.0 and t.dataset == "nyuv2"
    assert DeviceTransform(size=[120, 160]).size == (120, 160)
    for ds in ("cityscapes", "NYUv2", None):
        with pytest.raises(ValueError):
            DeviceTransform(dataset=ds)
    for size in (256, (256,), (0, 256), (256, -1), (2.5, 4), (256, 256, 3), "256x256", (True, 4)):
        with pytest.raises(ValueError):
            DeviceTransform(size=size)
    for md in (0.0, -1.0):
        with pytest.raises(ValueError):
            DeviceTransform(max_depth=md)


def test_abi_declared_and_refuses_bad_arguments():
    """Every refusal below happens before a HIP call: this runs on a machine without a GPU."""
    from vision_mtl_amd._lib import HEADER, lib, parse_header

    protos = parse_header()
    assert "vmtl_nyuv2_resize" in protos and "vmtl_nyuv2_resize_parts" in protos
    _, argtypes, argnames = protos["vmtl_nyuv2_resize"]
    assert argnames == ["img", "mask", "depth", "depth_dtype", "img_out", "mask_out", "depth_out", "part", "B", "Hi",
                        "Wi", "Ho", "Wo", "max_depth", "stream"]
    assert argtypes[argnames.index("max_depth")] is ctypes.c_float
    text = HEADER.read_text()
    assert "#define VMTL_DEPTH_U16 0" in text and "#define VMTL_DEPTH_I32 1" in text

    L = lib()
    parts = L.raw("vmtl_nyuv2_resize_parts")
    assert parts(32, 480, 640, 256, 256, 0) == 32 * 32 * 4  # 8 x 64 output tiles
    assert parts(2, 37, 53, 16, 24, 1) > 0
    for args in [(0, 480, 640, 256, 256, 0), (1, 0, 640, 256, 256, 0), (1, 480, -1, 256, 256, 0),
                 (1, 480, 640, 0, 256, 0), (1, 480, 640, 256, 0, 0), (1, 480, 640, 256, 256, 2),
                 (1, 480, 640, 256, 256, -1)]:
        assert parts(*args) == -1, args

    f = L.raw("vmtl_nyuv2_resize")
    P = 4096  # a fake, 16-byte aligned address: never dereferenced, every call below is refused first
    ok = dict(img=P, mask=P, depth=P, depth_dtype=0, img_out=P, mask_out=P, depth_out=P, part=P, B=2, Hi=48, Wi=64,
              Ho=16, Wo=16, max_depth=10.0, stream=None)
    bad = [dict(img=None), dict(mask=None), dict(depth=None), dict(img_out=None), dict(mask_out=None),
           dict(depth_out=None), dict(part=None), dict(depth_dtype=7), dict(depth_dtype=-1), dict(B=0), dict(Hi=0),
           dict(Wi=-3), dict(Ho=0), dict(Wo=-1), dict(max_depth=0.0), dict(max_depth=-1.0), dict(img=P + 1),
           dict(img_out=P + 4)]
    for change in bad:
        kw = dict(ok, **change)
        assert f(*[kw[n] for n in argnames]) == -1, change


def test_new_hooks_default_to_none():
    from vision_mtl_amd.data import upload_batch
    from vision_mtl_amd.graphed import GraphedStep
    from vision_mtl_amd.lit_module import MTLModule

    p = inspect.signature(upload_batch).parameters["transform"]
    assert p.default is None and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    module = MTLModule(torch.nn.Linear(2, 2), num_classes=3, device="cpu")
    assert module.device_transform is None
    assert "device_transform" in inspect.getsource(GraphedStep.__init__)


def test_upload_batch_with_transform_hands_the_raw_batch_over():
    """On the CPU the transform receives the raw tensors unchanged (the copy to 'cpu' is a no-op) and its result is
    returned as it is; without a transform nothing changes."""
    from vision_mtl_amd.data import collate_raw, upload_batch

    raw = collate_raw([_raw(seed=i) for i in range(2)], pin=False)
    seen = {}

    def transform(b):
        seen.update(b)
        return {"img": "done"}

    assert upload_batch(raw, "cpu", transform=transform) == {"img": "done"}
    assert set(seen) == {"img", "mask", "depth"}
    assert all(torch.equal(seen[k], raw[k]) and seen[k].dtype == raw[k].dtype for k in raw)
    plain = upload_batch({"mask": raw["mask"], "depth": raw["depth"]}, "cpu")
    assert torch.equal(plain["mask"], raw["mask"]) and torch.equal(plain["depth"], raw["depth"])


def test_device_transform_needs_the_gpu():
    from vision_mtl_amd.data import DeviceTransform, collate_raw

    raw = collate_raw([_raw(seed=i) for i in range(2)], pin=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceTransform(size=(4, 4))(raw)
