"""-m gpu: the NYUv2 device transform (csrc/resize.hip through ops / data / MTLModule / GraphedStep) against the host
chain it replaces.  Host oracle, per sample: ToTensor (u8 / 255, integer depth unscaled) + F.interpolate(bilinear,
antialias=True) - what torchvision's Resize calls - with the integer depth rounded back to its dtype, then
data.prepare_sample(dataset="nyuv2") (reference cfg.py:144-155, data_modules/nyuv2.py:100-141)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
MAX_DEPTH = 10.0


def raw_samples(B, H, W, depth_dtype, seed, classes=14):
    """Decoded NYUv2-like samples: noisy image, blocky class-id mask, depth with ~10 % invalid (0) pixels; sample 1
    stays below 1e4 counts so that its `/ max_depth` is not applied while the others' is."""
    g = np.random.default_rng(seed)
    out = []
    for i in range(B):
        img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        blocks = g.integers(0, classes, (H // 4 + 1, W // 4 + 1), dtype=np.uint8)
        mask = np.ascontiguousarray(np.repeat(np.repeat(blocks, 4, 0), 4, 1)[:H, :W])
        hi = 9000 if i == 1 else 65535
        depth = g.integers(0, hi + 1, (H, W))
        depth[g.random((H, W)) < 0.1] = 0
        out.append({"img": img, "mask": mask, "depth": depth.astype(depth_dtype)})
    return out


def host_oracle(sample, size, num_classes=14):
    """(prepared sample, pre-rounding mask*255, pre-rounding depth counts)"""
    from vision_mtl_amd.data import prepare_sample

    rs = lambda x: F.interpolate(x[None], size=size, mode="bilinear", align_corners=False, antialias=True)[0]
    img = rs(torch.from_numpy(sample["img"]).permute(2, 0, 1).float().div(255)).permute(1, 2, 0)
    mask = rs(torch.from_numpy(sample["mask"])[None].float().div(255))[0]
    d = torch.from_numpy(sample["depth"])
    dres = rs(d[None].float())[0]
    counts = dres.round().to(d.dtype)
    prep = prepare_sample({"img": img, "mask": mask, "depth": counts}, num_classes, max_depth=MAX_DEPTH, dataset="nyuv2")
    return prep, mask * 255, dres


def near_half(v):
    return ((v - v.floor()) - 0.5).abs() <= 1e-3


def check_against_oracle(samples, out, size):
    """img within 2e-6; mask and depth bit-equal except where the host's pre-rounding value lies within 1e-3 of
    k + 0.5.  Uniformly spread fractions put ~0.2 % of all pixels in that window, so the bar is on the pixels the
    window actually excused (they differ AND lie in it): fewer than 0.1 %; both counts are printed."""
    B = len(samples)
    Ho, Wo = size
    st = out["img"]._vmtl_nhwc
    assert tuple(st.shape) == (B, Ho, Wo, 4) and st.dtype == torch.float32
    assert tuple(out["img"].shape) == (B, 3, Ho, Wo) and out["img"].data_ptr() == st.data_ptr()
    assert torch.count_nonzero(st[..., 3]).item() == 0, "pad channel"
    assert out["mask"].dtype == torch.int64 and tuple(out["mask"].shape) == (B, Ho, Wo)
    assert out["depth"].dtype == torch.float32 and tuple(out["depth"].shape) == (B, Ho, Wo, 1)
    st, mask, depth = st.cpu(), out["mask"].cpu(), out["depth"].cpu()
    window_n, excused_n, scaled = 0, 0, []
    for i, s in enumerate(samples):
        ref, m255, dres = host_oracle(s, size)
        err = (st[i, ..., :3] - ref["img"]).abs().max().item()
        assert err <= 2e-6, f"sample {i}: img max abs error {err:.3e}"
        ex_m, ex_d = near_half(m255), near_half(dres)
        diff_m, diff_d = mask[i] != ref["mask"], (depth[i] != ref["depth"])[..., 0]
        window_n += int(ex_m.sum()) + int(ex_d.sum())
        excused_n += int((diff_m & ex_m).sum()) + int((diff_d & ex_d).sum())
        bad = diff_m & ~ex_m
        assert not bad.any(), f"sample {i}: {int(bad.sum())} mask pixels differ, e.g. {mask[i][bad][:5]} vs {ref['mask'][bad][:5]}"
        bad = diff_d & ~ex_d
        assert not bad.any(), f"sample {i}: {int(bad.sum())} depth pixels differ"
        scaled.append(bool(dres.round().max() > 1e4))
    n = 2 * B * Ho * Wo
    print(f"{B}x{samples[0]['img'].shape[:2]} -> {size}: {window_n} mask/depth pixels within 1e-3 of k+0.5 "
          f"({window_n / n:.2e}), {excused_n} of them differ and were exempted ({excused_n / n:.2e})")
    assert excused_n / n < 1e-3
    return scaled


GEOMETRIES = [
    (2, 480, 640, 256, 256),  # the reference's NYUv2 geometry (scales 1.875 x 2.5)
    (3, 37, 53, 16, 24),      # odd downscale
    (3, 20, 30, 32, 48),      # upscale
    (2, 24, 40, 24, 40),      # identity
    (3, 100, 150, 45, 70),    # partial tiles on both axes
    (2, 30, 100, 50, 40),     # upscale rows, downscale columns
]


@pytest.mark.parametrize("depth_dtype", [np.uint16, np.int32], ids=["u16", "i32"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "{}x{}x{}->{}x{}".format(*g))
def test_device_transform_matches_host_chain(dev, geo, depth_dtype):
    from vision_mtl_amd.data import DeviceTransform, collate_raw, upload_batch

    B, Hi, Wi, Ho, Wo = geo
    samples = raw_samples(B, Hi, Wi, depth_dtype, seed=Hi * 7 + Wi)
    raw = collate_raw(samples)
    out = upload_batch(raw, dev, transform=DeviceTransform(size=(Ho, Wo), max_depth=MAX_DEPTH))
    torch.cuda.synchronize()
    scaled = check_against_oracle(samples, out, (Ho, Wo))
    assert scaled[1] is False and (B < 3 or scaled[0]), "the max_depth rule is decided per sample"


def _mtan(dev):
    from vision_mtl_amd.models.mtan_model import MTANMiniUnet

    fx = torch.load(os.path.join(G, "mtan_tiny.pt"), weights_only=False)
    c = fx["cfg"]
    m = MTANMiniUnet(3, dict(fx["tasks"]), c["hidden"], c["first"], c["levels"])
    m.load_state_dict(fx["state_dict"])
    return fx, m.to(dev).train()


def _host_batch(samples, size, C):
    from vision_mtl_amd.data import collate

    return collate([host_oracle(s, size, C)[0] for s in samples])


def test_training_step_on_device_transformed_batch(dev):
    from vision_mtl_amd.data import DeviceTransform, collate_raw, upload_batch
    from vision_mtl_amd.lit_module import MTLModule

    fx, model = _mtan(dev)
    C, (B, _, H, W) = fx["cfg"]["C"], fx["batch"]["img"].shape
    samples = raw_samples(B, 2 * H + 11, 2 * W + 5, np.uint16, seed=5, classes=C)
    module = MTLModule(model, num_classes=C, device=str(dev))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    a = module.training_step(upload_batch(collate_raw(samples), dev, transform=DeviceTransform((H, W))), 0)
    model.load_state_dict(sd)
    b = module.training_step(upload_batch(_host_batch(samples, (H, W), C), dev), 0)
    a, b = float(a.detach()), float(b.detach())
    assert abs(a - b) <= 1e-5 * abs(b), f"device-transformed {a} vs host-resized {b}"


def test_graphed_step_with_device_transform_matches_eager(dev):
    """GraphedStep captures the transform: 3 different raw host batches against the eager loop on host-resized ones
    (tolerances of test_train_loop_gpu.py::test_graphed_step_matches_eager_with_changing_batches)."""
    from vision_mtl_amd import dp
    from vision_mtl_amd.data import DeviceTransform, collate_raw
    from vision_mtl_amd.graphed import GraphedStep
    from vision_mtl_amd.lit_module import MTLModule

    fx0, _ = _mtan(dev)
    C, (B, _, H, W) = fx0["cfg"]["C"], fx0["batch"]["img"].shape
    Hi, Wi = 2 * H + 11, 2 * W + 5
    raws = [raw_samples(B, Hi, Wi, np.uint16, seed=40 + i, classes=C) for i in range(3)]
    example = raw_samples(B, Hi, Wi, np.uint16, seed=39, classes=C)

    def run(graphed):
        fx, model = _mtan(dev)
        module = MTLModule(model, num_classes=C, device=str(dev))
        arena = dp.FlatArena(model)
        opt = torch.optim.Adam(module.parameters(), lr=2e-3)
        if graphed:
            module.device_transform = DeviceTransform((H, W))
            gstep = GraphedStep(module, collate_raw(example), arena=arena)
            assert gstep.device_transform is module.device_transform
            assert gstep.static["img"].dtype == torch.uint8 and gstep.static["depth"].dtype == torch.uint16
        model.load_state_dict(fx["state_dict"])
        losses = []
        for smp in raws:
            opt.zero_grad()
            if graphed:
                loss = gstep(collate_raw(smp))
            else:
                arena.rebind_grads()
                loss = module.training_step(module.transfer_batch_to_device(_host_batch(smp, (H, W), C), dev), 0)
            loss.backward()
            opt.step()
            dp.ops.packs.invalidate()
            losses.append(float(loss.detach()))
        return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

    le, sde = run(False)
    lg, sdg = run(True)
    assert le[-1] != le[0]
    for k, (a, b) in enumerate(zip(lg, le)):
        assert abs(a - b) <= 1e-5 * abs(b), f"step {k}: replayed loss {a} vs eager {b}"
    for k in sde:
        if sde[k].is_floating_point():
            err, ref = float((sdg[k].double() - sde[k].double()).abs().max()), float(sde[k].double().abs().max())
            assert err <= 1e-5 * ref + 1e-8, f"{k}: {err:.3e} vs magnitude {ref:.3e}"


def test_predict_with_device_transform(dev):
    from vision_mtl_amd.data import DeviceTransform, collate_raw
    from vision_mtl_amd.lit_module import MTLModule

    fx, model = _mtan(dev)
    C, (B, _, H, W) = fx["cfg"]["C"], fx["batch"]["img"].shape
    module = MTLModule(model.eval(), num_classes=C, device=str(dev))
    module.device_transform = DeviceTransform((H, W))
    batch = module.transfer_batch_to_device(collate_raw(raw_samples(B, 61, 83, np.int32, seed=3, classes=C)), dev)
    assert batch["img"].shape == (B, 3, H, W) and batch["mask"].dtype == torch.int64
    with torch.no_grad():
        pred = module.predict_step(batch, 0)
    torch.cuda.synchronize()
    assert pred["segm"].shape == (B, H, W) and pred["segm"].dtype == torch.int64
    assert pred["depth"].shape == (B, H, W, 1) and pred["depth"].dtype == torch.float32
    assert torch.isfinite(pred["depth"]).all() and len(module.step_outputs["predict"]["loss"]) == 1
