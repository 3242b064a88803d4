"""Write tests/golden/ops_resize.npz: Pillow's Resize(R) -> CenterCrop(C) bytes
for the matrix of tests/resizeref.py.  Run once on a machine with Pillow (the
version is recorded in the file); no test needs Pillow to read it.

Per case NAME = resizeref.case_name(R, C, h, w):
  NAME.out      Pillow's window, u8 [C, C, 3]
  NAME.src_sha  sha256 of the source bytes (resizeref.source(h, w))
  NAME.src      the source itself where it is at most 64 KiB

The transform is torchvision's on a PIL image, spelled out:
Image.resize((ow, oh), BILINEAR) with resizeref.resized_size, then
Image.crop at resizeref.crop_offset.

  python tools/make_resize_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pillow_resize_center_crop(src, r, c):
    from PIL import Image
    import resizeref as R
    h, w, _ = src.shape
    oh, ow = R.resized_size(h, w, r)
    im = Image.fromarray(src, "RGB").resize((ow, oh), Image.BILINEAR)
    top, left = R.crop_offset(oh, c), R.crop_offset(ow, c)
    return np.asarray(im.crop((left, top, left + c, top + c)))


def main():
    import PIL
    import resizeref as R
    z = {"pillow_version": np.array(PIL.__version__)}
    for (r, c), sources in R.MATRIX:
        for h, w in sources:
            name = R.case_name(r, c, h, w)
            src = R.source(h, w)
            out = pillow_resize_center_crop(src, r, c)
            assert out.shape == (c, c, 3) and out.dtype == np.uint8
            z[name + ".out"] = out
            z[name + ".src_sha"] = np.array(R.sha(src))
            if src.nbytes <= R.STORED_SOURCE_BYTES:
                z[name + ".src"] = src
    np.savez_compressed(R.GOLDEN, **z)
    print(f"{R.GOLDEN}: {len(z)} arrays, {os.path.getsize(R.GOLDEN)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
