"""-m gpu: the device-side joint training augmentation (csrc/augment.hip through ops / data.DeviceAugment / MTLModule /
GraphedStep) against its definition, torch's CPU F.interpolate per sample (tests/augment_oracle.py).

Bounds.  Image: the kernel restates the oracle's arithmetic, only the order of the bilinear sum's roundings (and their
contraction into FMAs) may differ: at most 8 roundings of values <= 1, below 5e-7 -> atol 1e-6; with a gain one more
rounding, scaled by 1.3 -> atol 2e-6.  Mask and depth are gathers (depth / s is one IEEE division on both sides): equal.
Sizes are the smallest where truncation, clamping and partial workgroup tiles (4 rows x 64 columns) occur."""
import gc
import os

import pytest
import torch

from tests import poison
from tests.augment_oracle import augment_oracle, corner_rows, crop_table, make_params, sample_batch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
SCALES = (1.0, 1.2, 1.5)
# (B, H, W, scale index per sample): 13x18 has crops 13x18, 10x15, 8x12; 37x70 leaves partial tiles on both axes
GEOS = {"3x13x18": (3, 13, 18, (0, 1, 2)), "2x37x70": (2, 37, 70, (1, 2))}
_CACHE = {}


@pytest.fixture(autouse=True)
def _collect_models():
    """A FlatArena and its parameters reference each other, and ops.packs re-packs every live model's weights each step
    (the large operands on the side stream): collect the models of earlier tests before a step is captured here - a
    forward-only capture of the tiny MTAN model never consumes those operands and would end with the side stream
    unjoined - and this test's own models when it ends."""
    gc.collect()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _case(geo, corner, flip, gain=1.0):
    """(host batch, rows, oracle outputs), computed once per case and shared by the tests that use it"""
    key = (geo, corner, flip, gain)
    if key not in _CACHE:
        B, H, W, sidx = GEOS[geo]
        batch = sample_batch(B, H, W, seed=H * 100 + W)
        rows = corner_rows(H, W, SCALES, sidx, corner, flip, gain)
        _CACHE[key] = (batch, rows, augment_oracle(batch["img"], batch["mask"], batch["depth"], rows, SCALES))
    return _CACHE[key]


def _tables(dev, H, W, scales=SCALES):
    return (torch.tensor(scales, dtype=torch.float32, device=dev),
            torch.tensor(crop_table(H, W, scales), dtype=torch.int32, device=dev))


def _device_img(img, layout, dev):
    from vision_mtl_amd import ops

    if layout == "ld3":  # dataset sample layout (B,H,W,3)
        return img.permute(0, 2, 3, 1).contiguous().to(dev)
    if layout == "ld4":  # the model's NHWC input storage
        return ops.hwc_to_model_input(img.permute(0, 2, 3, 1).contiguous().to(dev))
    return img.to(dev)   # plain NCHW


def _apply(batch, rows, layout, dev, scales=SCALES):
    from vision_mtl_amd import ops

    B, _, H, W = batch["img"].shape
    sc, crop = _tables(dev, H, W, scales)
    out = ops.augment_apply(_device_img(batch["img"], layout, dev), batch["mask"].to(dev), batch["depth"].to(dev),
                            make_params(rows).to(dev), sc, crop)
    torch.cuda.synchronize()
    return out


def _check(out, ref, atol, B, H, W):
    img, mask, depth = out
    st = img._vmtl_nhwc
    assert tuple(st.shape) == (B, H, W, 4) and st.dtype == torch.float32 and st.is_contiguous()
    assert tuple(img.shape) == (B, 3, H, W) and img.data_ptr() == st.data_ptr()
    assert mask.dtype == torch.int64 and tuple(mask.shape) == (B, H, W)
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (B, H, W, 1)
    st = st.cpu()
    assert torch.isfinite(st).all() and torch.isfinite(depth).all()
    assert (st[..., 3] == 0).all(), "pad lane"
    err = (st[..., :3].permute(0, 3, 1, 2) - ref[0]).abs().max().item()
    print(f"{B}x{H}x{W}: image max abs error {err:.3e} (bound {atol:.0e})")
    assert err <= atol
    assert torch.equal(mask.cpu(), ref[1]), "mask"
    assert torch.equal(depth.cpu(), ref[2]), "depth"


CASES = [(g, c, f, l) for g in GEOS for c in ("tl", "br") for f in (0, 1) for l in ("ld3", "ld4")]
IDS = ["-".join(map(str, c)) for c in CASES]


@pytest.mark.parametrize("geo,corner,flip,layout", CASES, ids=IDS)
def test_apply_matches_oracle(dev, geo, corner, flip, layout):
    batch, rows, ref = _case(geo, corner, flip)
    B, H, W, _ = GEOS[geo]
    _check(_apply(batch, rows, layout, dev), ref, 1e-6, B, H, W)


def test_apply_takes_a_plain_nchw_image(dev):
    batch, rows, ref = _case("3x13x18", "br", 1)
    _check(_apply(batch, rows, "nchw", dev), ref, 1e-6, 3, 13, 18)


@pytest.mark.parametrize("geo,corner,flip,layout", CASES, ids=IDS)
def test_reads_stay_inside_the_crop(dev, geo, corner, flip, layout):
    """Everything outside each sample's crop window is NaN (image, depth) or a sentinel (mask): a tap read there, even
    with weight 0, shows in the output."""
    batch, rows, ref = _case(geo, corner, flip)
    B, H, W, _ = GEOS[geo]
    crops = crop_table(H, W, SCALES)
    inside = torch.zeros(B, H, W, dtype=torch.bool)
    for b, (si, top, left, _, _) in enumerate(rows):
        inside[b, top:top + crops[si][0], left:left + crops[si][1]] = True
    bad = {"img": torch.where(inside[:, None], batch["img"], torch.tensor(float("nan"))),
           "mask": torch.where(inside, batch["mask"], torch.tensor(-77)),
           "depth": torch.where(inside[..., None], batch["depth"], torch.tensor(float("nan")))}
    _check(_apply(bad, rows, layout, dev), ref, 1e-6, B, H, W)


@pytest.mark.parametrize("layout", ["ld3", "ld4"])
def test_identity(dev, layout):
    batch = sample_batch(2, 13, 18, seed=3)
    img, mask, depth = _apply(batch, [(0, 0, 0, 0, 1.0)] * 2, layout, dev, scales=(1.0,))
    assert torch.equal(img.cpu(), batch["img"]) and (img._vmtl_nhwc[..., 3] == 0).all()
    assert torch.equal(mask.cpu(), batch["mask"]) and torch.equal(depth.cpu(), batch["depth"])


def test_hand_made_rows_are_clamped(dev):
    """Out-of-range scale index and offsets are clamped into the nearest valid row: the result is that row's."""
    batch, rows, ref = _case("3x13x18", "br", 0)
    wild = [(0, -5, -9, 0, 1.0), (1, 1000, 1000, 0, 1.0), (17, 99, 99, 0, 1.0)]
    out = _apply(batch, wild, "ld4", dev)
    want = augment_oracle(batch["img"], batch["mask"], batch["depth"], [(0, 0, 0, 0, 1.0), rows[1], rows[2]], SCALES)
    _check(out, want, 1e-6, 3, 13, 18)


@pytest.mark.parametrize("flip", [0, 1])
def test_gain(dev, flip):
    B, H, W, sidx = GEOS["3x13x18"]
    batch = _case("3x13x18", "tl", flip)[0]
    plain = corner_rows(H, W, SCALES, sidx, "tl", flip, 1.0)
    rows = [(*r[:4], g) for r, g in zip(plain, (0.7, 1.3, 1.3))]
    ref = augment_oracle(batch["img"], batch["mask"], batch["depth"], rows, SCALES)
    out = _apply(batch, rows, "ld4", dev)
    _check(out, ref, 2e-6, B, H, W)
    got = out[0].cpu()
    assert got.max().item() <= 1.0 and got.min().item() >= 0.0
    # where the unclamped product exceeds 1 by more than the bound, the pixel is exactly 1.0
    pre = augment_oracle(batch["img"], batch["mask"], batch["depth"], plain, SCALES)[0]
    gains = torch.tensor([r[4] for r in rows], dtype=torch.float32).view(B, 1, 1, 1)
    clamped = pre * gains > 1.0 + 2e-6
    assert clamped.sum().item() > 20 and (got[clamped] == 1.0).all()
    assert not clamped[0].any() and (ref[0][0] < 0.7001).all()


def test_draw_matches_host(dev):
    from vision_mtl_amd import ops
    from vision_mtl_amd.data import augment_params_host

    H, W, B, c = 13, 18, 8, 5
    _, crop = _tables(dev, H, W)
    for seed, c in ((11, 5), ((1 << 63) - 1, (1 << 40) + 3)):
        state = torch.tensor([seed, c], dtype=torch.int64, device=dev)
        params = torch.full((B, 8), -1, dtype=torch.int32, device=dev)
        for k in range(3):
            ops.augment_draw(state, params, crop, H, W, p_flip=0.5, brightness=0.2)
            assert state.tolist() == [seed, c + k + 1]
            want = augment_params_host(seed, c + k, B, H, W, SCALES, 0.5, 0.2)
            got = params.cpu()
            assert torch.equal(got[:, :4], want[:, :4]) and got[:, 5:].eq(0).all(), (seed, k, got, want)
            g, w = got[:, 4].contiguous().view(torch.float32), want[:, 4].contiguous().view(torch.float32)
            assert ((g - w).abs() <= 1e-6 * w.abs()).all() and ((g >= 0.8) & (g <= 1.2)).all()


def test_draw_statistics(dev):
    from vision_mtl_amd import ops
    from vision_mtl_amd.data import augment_params_host

    H, W, B = 37, 70, 4096
    _, crop = _tables(dev, H, W)
    state = torch.tensor([11, 0], dtype=torch.int64, device=dev)
    params = torch.empty((B, 8), dtype=torch.int32, device=dev)
    ops.augment_draw(state, params, crop, H, W, p_flip=0.5, brightness=0.0)
    got = params.cpu()
    assert torch.equal(got, augment_params_host(11, 0, B, H, W, SCALES, 0.5, 0.0))  # brightness 0: the gain is exactly 1
    share = got[:, 3].float().mean().item()
    scale_share = [got[:, 0].eq(si).float().mean().item() for si in range(3)]
    print(f"flip share {share:.4f}, scale shares {scale_share}")
    assert 0.45 <= share <= 0.55 and all(0.28 <= s <= 0.39 for s in scale_share)


def test_guard_bands(dev):
    with poison.patched("guard") as p:
        for geo, corner, flip, layout in (("3x13x18", "br", 1, "ld3"), ("2x37x70", "tl", 0, "ld4")):
            batch, rows, ref = _case(geo, corner, flip)
            B, H, W, _ = GEOS[geo]
            _check(_apply(batch, rows, layout, dev), ref, 1e-6, B, H, W)
        assert p.count >= 4


def _mtan(dev):
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.models.mtan_model import MTANMiniUnet

    fx = torch.load(os.path.join(G, "mtan_tiny.pt"), weights_only=False)
    c = fx["cfg"]
    m = MTANMiniUnet(3, dict(fx["tasks"]), c["hidden"], c["first"], c["levels"])
    m.load_state_dict(fx["state_dict"])
    return fx, MTLModule(m.to(dev).train(), num_classes=c["C"], device=str(dev))


def test_eager_module(dev):
    from vision_mtl_amd.data import DeviceAugment, augment_params_host

    fx, module = _mtan(dev)
    sd = {k: v.clone() for k, v in module.model.state_dict().items()}
    batch = {k: v.to(dev) for k, v in fx["batch"].items()}
    B, _, H, W = batch["img"].shape
    aug = DeviceAugment(seed=11, brightness=0.2)
    aug.set_counter(40)
    module.train_augment = aug
    a = module.training_step(dict(batch), 0).detach().clone()
    assert aug.counter == 41
    assert torch.equal(aug.last_params.cpu()[:, :4], augment_params_host(11, 40, B, H, W, SCALES, 0.5, 0.2)[:, :4])
    with torch.no_grad():
        module.validation_step(dict(batch), 0)
        module.test_step(dict(batch), 0)
        module.predict_step(dict(batch), 0)
    assert aug.counter == 41, "validation / test / predict never augment"

    _, plain = _mtan(dev)
    plain.model.load_state_dict(sd)
    aug.set_counter(40)
    augmented = aug(dict(batch))
    assert augmented["img"].data_ptr() != batch["img"].data_ptr() and set(augmented) == set(batch)
    b = plain.training_step(augmented, 0).detach()
    assert torch.equal(a, b), f"{float(a)} vs {float(b)}"
    c = plain.training_step(dict(batch), 0).detach()
    assert not torch.equal(a, c), "the augmentation changed nothing"

    restored = DeviceAugment()
    restored.load_state_dict(aug.state_dict())
    assert restored.state_dict() == {"seed": 11, "counter": 41}


def test_captured_step(dev):
    from vision_mtl_amd.data import DeviceAugment, augment_params_host
    from vision_mtl_amd.graphed import GraphedEval, GraphedStep

    fx, module = _mtan(dev)
    batch = fx["batch"]
    B, _, H, W = batch["img"].shape
    aug = DeviceAugment(seed=11)
    aug.set_counter(7)
    module.train_augment = aug
    gstep = GraphedStep(module, batch)
    assert gstep.train_augment is aug and aug.counter == 7, "construction leaves the counter as it was"
    aug.set_counter(100)
    replayed, rows = [], []
    for k in range(2):
        loss = gstep(batch)
        replayed.append(float(loss.detach()))
        rows.append(aug.last_params.cpu().clone())
        assert torch.equal(rows[k], augment_params_host(11, 100 + k, B, H, W, SCALES, 0.5, 0.0))
        assert aug.counter == 101 + k
    assert not torch.equal(rows[0], rows[1])

    geval = GraphedEval(module, batch, stage="val")
    assert not hasattr(geval, "train_augment")
    with torch.no_grad():
        geval(batch)
        geval(batch)
    assert aug.counter == 102, "a GraphedEval never advances the counter"

    aug.set_counter(100)
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    for k in range(2):
        eager = float(module.training_step(dict(dbatch), 0).detach())
        print(f"counter {100 + k}: replayed {replayed[k]!r} eager {eager!r}")
        assert abs(replayed[k] - eager) <= 1e-5 * abs(eager)
    assert replayed[0] != replayed[1]
