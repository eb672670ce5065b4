"""CPU restatement of test-time augmentation and output-size predictions (vision_mtl_amd/inference.py, csrc/tta.hip) with
torch alone, in fp64 (the reference) or fp32 (whose own error against fp64 sets every tolerance), and the case table the
tta tests share.

  view table     h = max(m, round(s * H / m) * m), likewise w; scales as given, unflipped before flipped, duplicate
                 (h, w, flip) rows dropped
  view image     F.interpolate(img, (h, w), mode="bilinear", align_corners=False, antialias=False), then torch.flip in x
  per-view merge torch.flip of the view's logits in x, F.interpolate to the base size, then weight * softmax ("prob") or
                 weight * logits ("logit"); depth: weight * depth_gain * interpolate(flip(sigmoid(depth logits)))
  finish         F.interpolate of the merged map to the output size, arg-max (first maximum), depth = inv_weight *
                 interpolate(merged depth), confidence = max / sum ("prob") or max softmax(inv_weight * map) ("logit")

The bar ("4 x fp32-CPU", as tests/test_production_eval_layers_gpu.py): per quantity, 4 x max(the fp32 restatement's
max-abs error against the fp64 one, 2^-22 of the fp64 maximum).  The tie band of an arg-max: the pixels whose fp64
top-2 margin is below 2 x the bar of the map the arg-max is taken on; outside it the arg-max must be the fp64 one."""
import functools

import torch
import torch.nn.functional as F

MODES = ("prob", "logit")
FLOOR = 2.0 ** -22
FACTOR = 4.0
BAND_MAX = 0.01  # at most 1 % of the pixels may sit in the tie band

# name: (B, C, base (H, W), output (Ho, Wo))
CASES = {"c5": (2, 5, (32, 64), (64, 128)), "c19": (1, 19, (9, 13), (27, 39)), "c14": (2, 14, (32, 32), (32, 32)),
         "c32": (1, 32, (7, 11), (20, 17))}


def view_table(H, W, scales, flip, multiple):
    table, seen = [], set()
    for s in scales:
        h = max(multiple, round(s * H / multiple) * multiple)
        w = max(multiple, round(s * W / multiple) * multiple)
        for f in ((False, True) if flip else (False,)):
            if (h, w, f) not in seen:
                seen.add((h, w, f))
                table.append((h, w, f, s))
    return table


def case_views(H, W):
    """identity, flip, 0.75x, 1.25x flipped (sizes rounded to whole pixels)"""
    return [(H, W, False, 1.0), (H, W, True, 1.0), (max(1, round(0.75 * H)), max(1, round(0.75 * W)), False, 0.75),
            (round(1.25 * H), round(1.25 * W), True, 1.25)]


def interp(x, size):
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False, antialias=False)


def view_image(img, size, flip, dtype=torch.float64):
    """img (B,3,H,W) -> the view (B,3,h,w)"""
    r = interp(img.to(dtype), size)
    return torch.flip(r, [3]) if flip else r


def merge_view(logits, depth_logits, base, flip, mode, weight=1.0, depth_gain=1.0, dtype=torch.float64, undo_flip=True):
    """one view's contribution (acc (B,C,H,W), acc_depth (B,H,W) or None).  undo_flip=False is a planted defect."""
    z = logits.to(dtype)
    if flip and undo_flip:
        z = torch.flip(z, [3])
    z = interp(z, base)
    a = weight * (torch.softmax(z, 1) if mode == "prob" else z)
    if depth_logits is None:
        return a, None
    d = torch.sigmoid(depth_logits.to(dtype))
    if flip and undo_flip:
        d = torch.flip(d, [3])
    return a, (weight * depth_gain) * interp(d, base)[:, 0]


def merge(views, base, mode, dtype=torch.float64, compensate_depth=False, undo_flip=True):
    """views: [(logits, depth_logits, flip, scale)] -> the accumulators after all of them, every weight 1"""
    acc = acc_d = None
    for logits, depth_logits, flip, s in views:
        a, d = merge_view(logits, depth_logits, base, flip, mode, 1.0, s if compensate_depth else 1.0, dtype, undo_flip)
        acc = a if acc is None else acc + a
        if d is not None:
            acc_d = d if acc_d is None else acc_d + d
    return acc, acc_d


def finish(acc, acc_depth, inv_weight, size, mode, dtype=torch.float64):
    """-> dict(map (B,C,Ho,Wo) the resampled merged map, segm, depth, confidence, margin = top-1 minus top-2 of map)"""
    m = interp(acc.to(dtype), size)
    top = m.topk(min(2, m.shape[1]), dim=1).values
    margin = top[:, 0] - top[:, 1] if m.shape[1] > 1 else torch.full_like(top[:, 0], float("inf"))
    conf = m.max(1).values / m.sum(1) if mode == "prob" else torch.softmax(inv_weight * m, 1).max(1).values
    depth = None if acc_depth is None else inv_weight * interp(acc_depth.to(dtype)[:, None], size)[:, 0]
    return {"map": m, "segm": m.argmax(1), "depth": depth, "confidence": conf, "margin": margin}


def bar(x32, x64):
    """the device's allowance for one quantity: 4 x max(fp32 CPU error, 2^-22 of the reference's maximum)"""
    x64 = x64.double()
    return FACTOR * max(float((x32.double() - x64).abs().max()), FLOOR * float(x64.abs().max()))


def share(got, x32, x64):
    """(the device's max-abs error, its share of the bar)"""
    err = float((got.double() - x64.double()).abs().max())
    return err, err / bar(x32, x64)


def tie_band(r32, r64):
    """pixels whose fp64 top-2 margin is below 2 x the bar of the resampled map"""
    return r64["margin"] < 2.0 * bar(r32["map"], r64["map"])


def compare(got, r32, r64, what=""):
    """THE comparator of the GPU tests: got = {"segm", "depth"[, "confidence"]} (B,Ho,Wo) on the CPU against the fp64
    reference r64 with bars from the fp32 restatement r32 (both dicts of finish()).  Raises AssertionError; returns the
    shares of the bars for printing."""
    band = tie_band(r32, r64)
    frac = float(band.double().mean())
    assert frac <= BAND_MAX, f"{what}: {100 * frac:.3f} % of the pixels are in the tie band (a condition on the inputs)"
    wrong = (got["segm"] != r64["segm"]) & ~band
    assert not bool(wrong.any()), f"{what}: arg-max differs from fp64 at {int(wrong.sum())} pixels outside the tie band"
    out = {"band": frac}
    for k in ("depth", "confidence"):
        if got.get(k) is None:
            continue
        assert tuple(got[k].shape) == tuple(r64[k].shape), (what, k, tuple(got[k].shape))
        assert not bool(torch.isnan(got[k]).any()), f"{what}: NaN in {k}"
        err, sh = share(got[k], r32[k], r64[k])
        assert sh <= 1.0, f"{what}: {k} error {err:.3e} is {sh:.2f} of its bar {bar(r32[k], r64[k]):.3e}"
        out[k] = sh
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs of a case: per view N(0, 3^2) logits and N(0, 1.5^2) depth logits, seeded by the name.  Leave unchanged."""
    B, C, (H, W), out = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    views = []
    for h, w, flip, s in case_views(H, W):
        views.append((torch.randn(B, C, h, w, generator=g) * 3.0, torch.randn(B, 1, h, w, generator=g) * 1.5, flip, s))
    return {"name": name, "B": B, "C": C, "base": (H, W), "out": tuple(out), "views": views}


@functools.lru_cache(maxsize=None)
def reference(name, mode, dtype=torch.float64):
    """accumulators and finish() of a case, every view at weight 1, inv_weight 1 / views.  Leave unchanged."""
    c = case(name)
    acc, acc_d = merge(c["views"], c["base"], mode, dtype)
    r = finish(acc, acc_d, 1.0 / len(c["views"]), c["out"], mode, dtype)
    r.update(acc=acc, acc_depth=acc_d)
    return r
