"""Input side of the hot path: the dataset SAMPLE CONTRACT of the reference and
the host->device hand-over, MI355X-first.

The reference's datasets store an image as HWC float in [0,1] (`.npy`, data_modules/cityscapes.py:69-83) or an
8-bit PNG (nyuv2.py:100-141); a host transform (albumentations ToTensorV2 / torchvision ToTensor, cfg.py:103-114,
144-155) transposes every sample to CHW before batching, and `transfer_batch_to_device` (lit_module.py:211-219)
uploads it.  The HIP path stores activations as NHWC, so the host transpose would only be undone on the device.
Here the sample keeps its storage layout: `prepare_sample` applies the reference's value rules (mask -1 ->
C-1, dtypes, depth normalisation, depth as (H, W, 1)), `collate` stacks into PINNED host tensors, and
`upload_batch` copies asynchronously and re-lays the image with ONE kernel (vmtl_hwc_to_nhwc_pad) straight into
the model's input storage.  What the caller sees stays the reference's contract: batch["img"] is a (B, 3, H, W)
float tensor (a channels-last view over that storage; the models pick the storage up without another copy).
Dataset file I/O and DataLoader workers stay out of scope (host code).

NYUv2's host transform also resizes (cfg.py:144-155: ToTensor + Resize((256, 256), antialias=True)), the expensive part
of its input side.  `collate_raw` stacks the samples as the files decode (uint8 image and mask, uint16 / int32 depth),
and `DeviceTransform`, handed to `upload_batch` (or set as `MTLModule.device_transform`), runs that resize and the
loader's value rules as HIP kernels on the uploaded batch.  PNG decode and file reading stay on the host.

Training augmentation (the reference has none: cfg.py:103-155 sets train_transform == test_transform): `DeviceAugment`,
set as `MTLModule.train_augment`, runs the joint random scale-crop + horizontal flip of the multi-task literature on
the batch that is already on the device, with its random parameters drawn on the device (csrc/augment.hip).
"""
from __future__ import annotations

import typing as t

import numpy as np
import torch


def synthetic_batch(B: int, H: int, W: int, C: int, seed: int = 11, masked: float = 0.0) -> dict:
    """SURVEY.md section 8(d) synthetic inputs in the reference's batch contract (seed 11 = reference cfg.py:194):
    img (B,3,H,W) in [0,1), mask (B,H,W) int64 in [0,C), depth (B,H,W,1) in [0.002, 0.5) (`masked`: that share of
    depth pixels set to 0 = invalid)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, H, W, generator=g)
    mask = torch.randint(0, C, (B, H, W), generator=g)
    depth = 0.002 + 0.498 * torch.rand(B, H, W, 1, generator=g)
    if masked > 0:
        depth[torch.rand(B, H, W, 1, generator=g) < masked] = 0.0
    return {"img": img, "mask": mask, "depth": depth}


def prepare_sample(raw: dict, num_classes: int, max_depth: float = 1.0, dataset: str = "cityscapes",
                   void_label: t.Optional[int] = None) -> dict:
    """Value rules of the reference's two datasets on one raw sample {"img": (H,W,3), "mask": (H,W), "depth": (H,W) or
    (H,W,1)} of numpy arrays / tensors, WITHOUT the CHW transpose.

    dataset="cityscapes" (reference data_modules/cityscapes.py:39-67): mask == -1 -> num_classes-1, img float32, mask
    int64, depth float32 divided by max_depth when its maximum exceeds 1 (common_ds.py:47-50).  void_label: the value -1
    maps to instead (e.g. 255, trained with MTLModule(segm_ignore_index=255)); None keeps the reference's rule.
    dataset="nyuv2" (reference data_modules/nyuv2.py:100-141): img divided by 255 when its maximum exceeds 1 (8-bit
    PNG), a mask that a ToTensor transform scaled into [0,1] is multiplied back by 255 (`mask.max() <= 1.0`), mask
    squeezed to (H,W) int64 with NO -1 remap, depth = uint16 PNG value / 1e4 and THEN the max_depth rule
    (NYUv2Config.max_depth = 10: cfg.py:117-155).  Leaving the /1e4 step out trains SILog on targets in the 1e3-1e4
    range with no error, so the dataset has to be named - there is no way to tell a raw uint16 map from metres.

    Both: depth comes back as (H, W, 1) (SILog needs the trailing 1)."""
    if dataset not in ("cityscapes", "nyuv2"):
        raise ValueError(f"prepare_sample: dataset must be 'cityscapes' or 'nyuv2', got {dataset!r}")
    if void_label is not None and dataset != "cityscapes":
        raise ValueError("prepare_sample: void_label remaps Cityscapes' -1; the nyuv2 loader has no such label")
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    img, mask, depth = as_t(raw["img"]).float(), as_t(raw["mask"]).clone(), as_t(raw["depth"]).float().clone()
    if img.dim() != 3 or img.shape[-1] != 3:
        raise ValueError(f"prepare_sample: img must be (H, W, 3), got {tuple(img.shape)}")
    if dataset == "nyuv2":
        if img.max() > 1.0:  # nyuv2.py:118-119
            img = img / 255
        if mask.is_floating_point() and mask.max() <= 1.0:  # nyuv2.py:121-123: ToTensor scaled the class ids by 1/255
            mask = (mask * 255).round()
        mask = mask.squeeze().long()  # nyuv2.py:124
        depth = depth / 1e4  # nyuv2.py:126-127: the depth PNG is uint16, 1e-4 m per count
    else:
        mask = mask.long()
        mask[mask == -1] = num_classes - 1 if void_label is None else int(void_label)  # cityscapes.py:42
    if depth.max() > 1.0:  # common_ds.py:47-50
        depth /= max_depth
    if depth.dim() == 3 and depth.shape[0] == 1 and depth.shape[-1] != 1:  # nyuv2.py:130-131: (1,H,W) -> (H,W,1)
        depth = depth.permute(1, 2, 0)
    if depth.dim() == 2:
        depth = depth.unsqueeze(-1)
    if tuple(mask.shape) != tuple(img.shape[:2]) or tuple(depth.shape) != (*img.shape[:2], 1):
        raise ValueError("prepare_sample: img / mask / depth sizes differ")
    return {"img": img.contiguous(), "mask": mask, "depth": depth.contiguous()}


def collate(samples: t.Sequence[dict], pin: bool = True) -> dict:
    """Stack prepared samples into {"img": (B,H,W,3), "mask": (B,H,W), "depth": (B,H,W,1)}; pinned host memory
    when a GPU is present, so that upload_batch's copies are asynchronous."""
    out = {k: torch.stack([s[k] for s in samples]) for k in ("img", "mask", "depth")}
    if pin and torch.cuda.is_available():
        out = {k: v.pin_memory() for k, v in out.items()}
    return out


def upload_batch(batch: dict, device, transform=None) -> dict:
    """Host batch -> device batch in the reference's contract.  An image stacked in sample layout (B,H,W,3) is
    re-laid by one HIP kernel into the model's NHWC storage and returned as a (B,3,H,W) view of it; everything
    else (an NCHW image included) is an asynchronous copy when pinned (reference lit_module.py:211-219).

    transform: a device transform (DeviceTransform) for a raw batch from collate_raw: every tensor is copied as it is
    (asynchronously when pinned) and the transform produces the batch on the device."""
    from . import ops

    def up(v):
        return v.to(device, non_blocking=v.device.type == "cpu" and v.is_pinned())

    if transform is not None:
        return transform({k: up(v) for k, v in batch.items()})

    out = {}
    for k, v in batch.items():
        if k == "img" and v.dim() == 4 and v.shape[-1] == 3 and v.shape[1] != 3:
            out[k] = ops.hwc_to_model_input(up(v.float()))
        else:
            out[k] = up(v)
    return out


_RAW_DTYPES = {"img": (torch.uint8,), "mask": (torch.uint8,), "depth": (torch.uint16, torch.int32)}


def collate_raw(samples: t.Sequence[dict], pin: bool = True) -> dict:
    """Stack raw decoded NYUv2 samples {"img": (H,W,3) uint8, "mask": (H,W) uint8, "depth": (H,W) uint16 or int32}
    (numpy arrays or tensors: what Pillow returns for the reference's PNGs, nyuv2.py:100-141) WITHOUT any dtype
    conversion, into {"img": (B,H,W,3), "mask": (B,H,W), "depth": (B,H,W)}; pinned when a GPU is present.  The
    DataLoader's collate_fn when DeviceTransform does the sample transform on the device."""
    if len(samples) == 0:
        raise ValueError("collate_raw: no samples")
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    cols = {k: [] for k in _RAW_DTYPES}
    size = None
    for i, smp in enumerate(samples):
        for k, dtypes in _RAW_DTYPES.items():
            if k not in smp:
                raise ValueError(f"collate_raw: sample {i} has no {k!r}")
            v = as_t(smp[k])
            if v.dtype not in dtypes:
                raise ValueError(f"collate_raw: sample {i} {k!r} must be {' or '.join(str(d) for d in dtypes)}, "
                                 f"got {v.dtype}")
            want = 3 if k == "img" else 2
            if v.dim() != want or (k == "img" and v.shape[-1] != 3):
                raise ValueError(f"collate_raw: sample {i} {k!r} must be {'(H, W, 3)' if k == 'img' else '(H, W)'}, "
                                 f"got {tuple(v.shape)}")
            if size is None:
                size = tuple(v.shape[:2])
            if tuple(v.shape[:2]) != size:
                raise ValueError(f"collate_raw: sample {i} {k!r} is {tuple(v.shape[:2])}, expected {size}")
            cols[k].append(v)
    if len({v.dtype for v in cols["depth"]}) != 1:
        raise ValueError("collate_raw: the depth maps of one batch must share a dtype")
    out = {k: torch.stack(v) for k, v in cols.items()}
    if pin and torch.cuda.is_available():
        out = {k: v.pin_memory() for k, v in out.items()}
    return out


class DeviceTransform:
    """The reference's NYUv2 sample transform as HIP kernels on a raw device batch (data.collate_raw, uploaded).

    Reference NYUv2Config.train_transform / test_transform (cfg.py:144-155) are ToTensor() + Resize(size,
    antialias=True), applied per sample to the image, the class-id mask and the uint16 depth PNG by
    NYUv2Dataset.prepare_sample (nyuv2.py:100-141).  Called on {"img": (B,H,W,3) uint8, "mask": (B,H,W) uint8,
    "depth": (B,H,W) uint16 | int32} it returns what prepare_sample(dataset="nyuv2", max_depth=max_depth) gives for
    each resized sample, batched: img (B,3,Ho,Wo) float32 (the model's input storage), mask (B,Ho,Wo) int64, depth
    (B,Ho,Wo,1) float32.  The filter is PyTorch's antialiased bilinear resample, value for value.

    Mask: ToTensor scales the class ids by 1/255; after the resample they are multiplied back and ROUNDED (half to
    even), as prepare_sample does.  The reference truncates there (`.long()`), which turns an id that came back as
    4.9999995 into 4; this project keeps prepare_sample's rounding.  Depth: resampled as float and rounded back to its
    integer type (what Resize does to integer images), then / 1e4, then / max_depth for a sample whose resized maximum
    exceeds 1.  Other keys of the batch pass through unchanged.

    Only dataset="nyuv2": Cityscapes' stored samples are already at the model's size, so its resize is an identity."""

    def __init__(self, size=(256, 256), max_depth: float = 10.0, dataset: str = "nyuv2"):
        if dataset != "nyuv2":
            raise ValueError(f"DeviceTransform: only dataset='nyuv2' is supported, got {dataset!r}")
        if (not isinstance(size, (tuple, list)) or len(size) != 2
                or not all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in size)):
            raise ValueError(f"DeviceTransform: size must be (height, width) of positive ints, got {size!r}")
        if not max_depth > 0:
            raise ValueError(f"DeviceTransform: max_depth must be > 0, got {max_depth!r}")
        self.size, self.max_depth, self.dataset = (int(size[0]), int(size[1])), float(max_depth), dataset

    def __call__(self, batch: dict) -> dict:
        from . import ops

        img, mask, depth = ops.nyuv2_resize(batch["img"], batch["mask"], batch["depth"], self.size, self.max_depth)
        out = dict(batch)
        out.update(img=img, mask=mask, depth=depth)
        return out

    def __repr__(self) -> str:
        return f"DeviceTransform(size={self.size}, max_depth={self.max_depth}, dataset={self.dataset!r})"


# ---- joint training augmentation on the device (csrc/augment.hip)
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _mix64(z: int) -> int:
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def augment_crop_table(H: int, W: int, scales: t.Sequence[float]) -> t.List[t.Tuple[int, int]]:
    """Crop size (int(H / s), int(W / s)) per scale, in Python's double arithmetic: the device reads this table and
    never recomputes it ((int)(H / 1.2f) can differ from the double result)."""
    return [(int(H / s), int(W / s)) for s in scales]


def augment_params_host(seed: int, counter: int, B: int, H: int, W: int, scales: t.Sequence[float] = (1.0, 1.2, 1.5),
                        p_flip: float = 0.5, brightness: float = 0.0) -> torch.Tensor:
    """What vmtl_augment_draw writes for the state {seed, counter}, restated on the host: int32 (B, 8) rows of
    {scale_idx, top, left, flip, gain (float32 bit pattern), 0, 0, 0}.  Counter-based (all arithmetic mod 2^64):

        r24(b, k) = mix(mix(seed + G * (counter + 1)) + G * (8 * b + k + 1)) >> 40

    with mix the splitmix64 finaliser and G = 0x9E3779B97F4A7C15; every range reduction is (r24 * n) >> 24 in integers.
    Columns 0-3 match the device bit for bit; the gain to a rounding of its float expression.  For tests and for users
    who log their augmentations."""
    crops = augment_crop_table(H, W, scales)
    S = len(crops)
    thr = int(round(float(p_flip) * (1 << 24)))
    base = _mix64((seed + _GOLDEN * (counter + 1)) & _M64)
    f32 = np.float32
    out = np.zeros((B, 8), dtype=np.int32)
    for b in range(B):
        r = [_mix64((base + _GOLDEN * (8 * b + k + 1)) & _M64) >> 40 for k in range(5)]
        si = (r[0] * S) >> 24
        h, w = min(max(crops[si][0], 1), H), min(max(crops[si][1], 1), W)
        gain = f32(1.0) + (f32(2.0) * (f32(r[4]) * f32(2.0 ** -24)) - f32(1.0)) * f32(brightness)
        out[b, :4] = (si, (r[1] * (H - h + 1)) >> 24, (r[2] * (W - w + 1)) >> 24, int(r[3] < thr))
        out[b, 4] = np.array([gain], dtype=np.float32).view(np.int32)[0]
    return torch.from_numpy(out)


class DeviceAugment:
    """Joint training augmentation as two HIP launches on a device batch (csrc/augment.hip): MTAN's recipe of the
    multi-task literature.  Per sample one scale s is drawn from `scales`, a window of int(H / s) x int(W / s) is cropped
    at a random offset and resampled back to H x W, and the sample is flipped horizontally with probability `p_flip`.
    Image, mask and depth move together: the image bilinear (align_corners=True), mask and depth nearest, depth divided
    by s.  Nearest sampling blends no labels, so ignore_index pixels and invalid (zero) depth stay what the loss kernels
    expect.  brightness > 0 also multiplies the image by a gain drawn from [1 - brightness, 1 + brightness), clamped to
    [0, 1].

    Called on a device batch in the model's input contract (img as data.upload_batch / DeviceTransform return it, a
    (B,H,W,3) sample-layout tensor, or plain (B,3,H,W); mask int64 (B,H,W); depth (B,H,W,1)) it returns a new dict with
    img / mask / depth replaced; other keys pass through.  Set it as `MTLModule.train_augment`: training_step applies it,
    validation / test / predict never do, and graphed.GraphedStep captures it.

    The random parameters are drawn ON THE DEVICE from the state {seed, counter}; every call (and every replay of a
    captured step) advances the counter by one, with no host involvement.  The rows used by the latest call stay
    readable as `last_params` (one buffer per batch size, overwritten by the next call - static under capture);
    augment_params_host(seed, counter, ...) restates them.  `counter` reads the device (a synchronisation: for logging
    and checkpoints, not for the step loop); set_counter(n) is a device fill.  state_dict() / load_state_dict() carry
    seed and counter, so a resumed run continues the stream.  Data-parallel runs: pass seed + rank, or every rank draws
    the same augmentations."""

    def __init__(self, scales: t.Sequence[float] = (1.0, 1.2, 1.5), p_flip: float = 0.5, brightness: float = 0.0,
                 seed: int = 0):
        from .ops import AUGMENT_MAX_SCALES

        try:
            scales = tuple(float(s) for s in scales)
        except TypeError:
            raise ValueError(f"DeviceAugment: scales must be a sequence of floats, got {scales!r}") from None
        if not 1 <= len(scales) <= AUGMENT_MAX_SCALES:
            raise ValueError(f"DeviceAugment: between 1 and {AUGMENT_MAX_SCALES} scales, got {len(scales)}")
        if not all(np.isfinite(s) and s >= 1.0 for s in scales):
            raise ValueError(f"DeviceAugment: every scale must be finite and >= 1 (a crop is upsampled), got {scales}")
        if not 0.0 <= p_flip <= 1.0:
            raise ValueError(f"DeviceAugment: p_flip must be in [0, 1], got {p_flip!r}")
        if not 0.0 <= brightness < 1.0:
            raise ValueError(f"DeviceAugment: brightness must be in [0, 1), got {brightness!r}")
        self.scales, self.p_flip, self.brightness = scales, float(p_flip), float(brightness)
        self.seed, self._counter = self._check_word("seed", seed), 0
        self._state = None    # int64 (2,) on the batch's device, created by the first call
        self._tables = {}     # (device, H, W) -> (scales float32 (S,), crop_hw int32 (S, 2))
        self._params = {}     # (device, B) -> int32 (B, 8)
        self.last_params = None

    @staticmethod
    def _check_word(name: str, v) -> int:
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < (1 << 63):
            raise ValueError(f"DeviceAugment: {name} must be an int in [0, 2^63), got {v!r}")
        return v

    # ---- state
    def _device_state(self, device) -> torch.Tensor:
        if self._state is None or self._state.device != device:
            if self._state is not None:
                self._counter = self.counter
            self._state = torch.tensor([self.seed, self._counter], dtype=torch.int64).to(device)
        return self._state

    @property
    def counter(self) -> int:
        """Calls made so far plus the start value (reads the device state: synchronises)."""
        return self._counter if self._state is None else int(self._state[1].item())

    def set_counter(self, n: int) -> None:
        self._counter = self._check_word("counter", n)
        if self._state is not None:
            self._state[1].fill_(n)  # a device fill on the current stream, no synchronisation

    def state_dict(self) -> dict:
        return {"seed": self.seed, "counter": self.counter}

    def load_state_dict(self, sd: dict) -> None:
        seed, counter = self._check_word("seed", sd["seed"]), self._check_word("counter", sd["counter"])
        self.seed = seed
        if self._state is not None:
            self._state[0].fill_(seed)
        self.set_counter(counter)

    # ---- the transform
    def _table(self, device, H: int, W: int):
        key = (device, H, W)
        tab = self._tables.get(key)
        if tab is None:
            crops = augment_crop_table(H, W, self.scales)
            if any(h < 1 or w < 1 for h, w in crops):
                raise ValueError(f"DeviceAugment: a {H}x{W} batch is too small for the scales {self.scales}")
            tab = self._tables[key] = (torch.tensor(self.scales, dtype=torch.float32).to(device),
                                       torch.tensor(crops, dtype=torch.int32).to(device))
        return tab

    def __call__(self, batch: dict) -> dict:
        from . import ops

        img = batch["img"]
        if not img.is_cuda:
            raise RuntimeError(f"DeviceAugment: the batch is on {img.device}: the augmentation only runs as HIP kernels "
                               "on an MI355X (there is deliberately no CPU fallback)")
        if img.dim() != 4:
            raise ValueError(f"DeviceAugment: img must be (B, 3, H, W) or (B, H, W, 3), got {tuple(img.shape)}")
        sample_layout = img.shape[-1] == 3 and img.shape[1] != 3
        B, (H, W) = img.shape[0], (img.shape[1:3] if sample_layout else img.shape[2:])
        scales, crop_hw = self._table(img.device, int(H), int(W))
        params = self._params.get((img.device, B))
        if params is None:
            params = self._params[(img.device, B)] = torch.zeros((B, 8), dtype=torch.int32, device=img.device)
        ops.augment_draw(self._device_state(img.device), params, crop_hw, H, W, self.p_flip, self.brightness)
        aimg, amask, adepth = ops.augment_apply(img, batch["mask"], batch["depth"], params, scales, crop_hw)
        self.last_params = params
        out = dict(batch)
        out.update(img=aimg, mask=amask, depth=adepth)
        return out

    def __repr__(self) -> str:
        return (f"DeviceAugment(scales={self.scales}, p_flip={self.p_flip}, brightness={self.brightness}, "
                f"seed={self.seed})")
