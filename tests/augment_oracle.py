"""Test helper: the DEFINITION of the joint training augmentation (csrc/augment.hip), built with torch on the CPU.

Per sample, with its scale s, crop (h, w), offsets (top, left), flip and gain:
    image      : F.interpolate(img[:, :, top:top+h, left:left+w], size=(H, W), mode="bilinear", align_corners=True)
    mask, depth: the same window with mode="nearest" (the mask as float), depth / s
    then the gain with a clamp to [0, 1] (only when gain != 1), then flip(-1) of all three.
The kernel restates that arithmetic; only the order of the bilinear sum's roundings may differ."""
import numpy as np
import torch
import torch.nn.functional as F


def crop_table(H, W, scales):
    return [(int(H / s), int(W / s)) for s in scales]


def make_params(rows):
    """rows: (scale_idx, top, left, flip, gain) per sample -> the int32 (B, 8) tensor the kernels exchange."""
    out = np.zeros((len(rows), 8), dtype=np.int32)
    for b, (si, top, left, flip, gain) in enumerate(rows):
        out[b, :4] = (si, top, left, int(flip))
        out[b, 4] = np.array([gain], dtype=np.float32).view(np.int32)[0]
    return torch.from_numpy(out)


def corner_rows(H, W, scales, scale_idx, corner, flip, gain=1.0):
    """One row per entry of scale_idx, the window at the top-left ("tl") or bottom-right ("br") corner."""
    crops = crop_table(H, W, scales)
    rows = []
    for si in scale_idx:
        h, w = crops[si]
        rows.append((si, 0, 0, flip, gain) if corner == "tl" else (si, H - h, W - w, flip, gain))
    return rows


def augment_oracle(img, mask, depth, rows, scales):
    """img (B,3,H,W) float32, mask (B,H,W) int64, depth (B,H,W,1) float32, all on the CPU -> the same three, augmented."""
    B, _, H, W = img.shape
    crops = crop_table(H, W, scales)
    oi, om, od = [], [], []
    for b, (si, top, left, flip, gain) in enumerate(rows):
        s, (h, w) = scales[si], crops[si]
        win = (slice(None), slice(None), slice(top, top + h), slice(left, left + w))
        i = F.interpolate(img[b:b + 1][win], size=(H, W), mode="bilinear", align_corners=True)
        m = F.interpolate(mask[b:b + 1, None].float()[win], size=(H, W), mode="nearest")
        d = F.interpolate(depth[b:b + 1, None, :, :, 0][win], size=(H, W), mode="nearest") / s
        if np.float32(gain) != np.float32(1.0):
            i = (i * float(np.float32(gain))).clamp(0.0, 1.0)
        if flip:
            i, m, d = i.flip(-1), m.flip(-1), d.flip(-1)
        oi.append(i[0])
        om.append(m[0, 0].long())
        od.append(d[0, 0, :, :, None])
    return torch.stack(oi), torch.stack(om), torch.stack(od)


def sample_batch(B, H, W, C=13, seed=0, ignore_index=255):
    """img in [0,1), mask in [0,C) with ~5 % ignore_index pixels, depth in [0.002, 0.5) with ~10 % invalid (0) pixels."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, H, W, generator=g)
    mask = torch.randint(0, C, (B, H, W), generator=g)
    mask[torch.rand(B, H, W, generator=g) < 0.05] = ignore_index
    depth = 0.002 + 0.498 * torch.rand(B, H, W, 1, generator=g)
    depth[torch.rand(B, H, W, 1, generator=g) < 0.1] = 0.0
    return {"img": img, "mask": mask, "depth": depth}
