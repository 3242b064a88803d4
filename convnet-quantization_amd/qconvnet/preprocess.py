"""Resize(R) -> CenterCrop(C) of decoded u8 images of mixed sizes on the device
(the first two steps of the reference's ImageNet transform,
utils/dataset_manager.py:24-25), byte for byte what torchvision's transforms
give on PIL images (Pillow's bilinear resize).  The result
is the uint8 [N, C, C, 3] batch that QuantizedResNet, evaluate() and the
calibration take as stored: ToTensor, Normalize and the QuantStub are folded
into the stem.

  plan(sizes)                host only: one descriptor per image
  pack(images)               mixed-size images -> one packed u8 buffer + sizes
  resize_center_crop(images) the device batch
"""
from __future__ import annotations

import math

import numpy as np
import torch

# qcn_resize_img_t (include/qconvnet.h)
DESC = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("oh", "<i4"), ("ow", "<i4"),
                 ("top", "<i4"), ("left", "<i4")], align=True)
assert DESC.itemsize == 32
MAX_SCALE = 32   # ceil(in / out) above this (more than 65 taps) is outside the kernels' envelope


def resized_size(h, w, resize):
    """(oh, ow) of torchvision's Resize(int): the short side becomes ``resize``,
    the long one int(resize * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(resize * long / short)
    return (new_long, resize) if w <= h else (resize, new_long)


def crop_offset(size, crop):
    """CenterCrop's first row / column: Python's round (an exact half goes to even)."""
    return int(round((size - crop) / 2.0))


def plan(sizes, resize=256, crop=224):
    """Descriptors (numpy, dtype DESC) for images of ``sizes`` [(h, w), ...]
    packed back to back: the resampled size, the crop window's corner and the
    byte offset of every image.  Host arithmetic only."""
    resize, crop = int(resize), int(crop)
    if resize < 1 or crop < 1:
        raise ValueError("plan: resize and crop must be positive")
    if crop > resize:
        raise ValueError(f"plan: crop {crop} is larger than resize {resize} (CenterCrop would pad)")
    desc = np.zeros(len(sizes), DESC)
    offset = 0
    for i, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError(f"plan: image {i} has size {(h, w)}")
        oh, ow = resized_size(h, w, resize)
        desc[i] = (offset, h, w, oh, ow, crop_offset(oh, crop), crop_offset(ow, crop))
        offset += h * w * 3
    return desc


def outside_envelope(desc):
    """Indices of the images that need more than 65 taps on an axis."""
    return [i for i, d in enumerate(desc)
            if math.ceil(int(d["h"]) / int(d["oh"])) > MAX_SCALE
            or math.ceil(int(d["w"]) / int(d["ow"])) > MAX_SCALE]


def pack(images):
    """(packed, sizes): the bytes of ``images`` (uint8 [H, W, 3] tensors or
    numpy arrays of any sizes) back to back in one 1-D uint8 tensor on the
    images' device, and their [(h, w), ...]."""
    flat, sizes = [], []
    for i, im in enumerate(images):
        t = im
        if isinstance(im, np.ndarray):   # (torch wants a writable array; the bytes are copied below anyway)
            t = torch.from_numpy(np.ascontiguousarray(im) if im.flags.writeable else im.copy())
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"pack: image {i} is neither a tensor nor a numpy array")
        if t.dtype != torch.uint8:
            raise ValueError(f"pack: image {i} is {t.dtype}, expected uint8")
        if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"pack: image {i} has shape {tuple(t.shape)}, expected [H, W, 3]")
        sizes.append((int(t.shape[0]), int(t.shape[1])))
        flat.append(t.contiguous().reshape(-1))
    packed = torch.cat(flat) if flat else torch.empty(0, dtype=torch.uint8)
    return packed, sizes


def check_envelope(desc):
    bad = outside_envelope(desc)
    if bad:
        i = bad[0]
        d = desc[i]
        raise ValueError(f"resize_center_crop: image {i} ({int(d['h'])} x {int(d['w'])} -> "
                         f"{int(d['oh'])} x {int(d['ow'])}) shrinks by more than {MAX_SCALE}x "
                         "on an axis (more than 65 taps)")


def resize_center_crop_packed(src, desc, crop, out=None, workspace=None, desc_dev=None):
    """The device half: ``src`` a packed u8 device buffer, ``desc`` its plan().
    Launches on the current stream without a sync (``desc_dev``: the
    descriptors already on the device; uploaded here when None).  Returns
    (uint8 [N, crop, crop, 3], workspace)."""
    from . import ops
    check_envelope(desc)
    if desc_dev is None:
        desc_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(src.device)
    return ops.resize_crop(src, desc, desc_dev, crop, crop, out=out, workspace=workspace)


def resize_center_crop(images, resize=256, crop=224, device="cuda"):
    """uint8 [N, crop, crop, 3] on ``device``: Resize(resize) -> CenterCrop(crop)
    of every image of ``images`` (uint8 [H, W, 3], mixed sizes), the bytes
    torchvision gives on PIL images.  ValueError for crop > resize, a wrong
    dtype or shape, or an image outside the tap envelope (named)."""
    plan([], resize, crop)   # crop > resize raises before anything is packed
    packed, sizes = pack(images)
    desc = plan(sizes, resize, crop)
    check_envelope(desc)
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(device):
        out, _ = resize_center_crop_packed(packed.to(device), desc, crop)
    return out
