"""Numpy restatement of torchvision's Resize(R) -> CenterCrop(C) on a PIL image
(Pillow's bilinear Image.resize, then a crop), the arithmetic of DESIGN
section 20, plus the test matrix and the source-image recipe shared by
tests/test_resize_cpu.py, tests/test_gpu_resize.py and
tools/make_resize_golden.py.

Pillow's resize is integer arithmetic on 22-bit fixed-point coefficients made
in double (src/libImaging/Resample.c: precompute_coeffs, bilinear_filter,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc): the
horizontal pass first, over the source rows the vertical taps reach, rounded
to u8; the vertical pass on that u8 image.  Python floats are IEEE doubles and
int() truncates as C's (int) does, so coeffs() below is the C code line by
line."""
from __future__ import annotations

import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ops_resize.npz")
PRECISION_BITS = 22

# ((R, C), [(h, w), ...]): every source of one (R, C) goes in one mixed batch
MATRIX = [
    ((32, 32), [(24, 31), (31, 24), (32, 32), (32, 57), (7, 5), (1, 1), (1, 9),   # crop touches both borders
                (97, 129),                                                         # 7 taps
                (700, 513), (513, 1100),                                           # 33 taps
                (1024, 1024)]),                                                    # envelope edge, 65 taps
    ((40, 24), [(53, 47), (47, 53)]),
    ((40, 25), [(100, 83), (83, 100)]),                                            # odd window, 5 taps
    ((73, 64), [(75, 100), (100, 75), (40, 30)]),                                  # the fused stem's 64^2
    ((264, 260), [(300, 391)]),                                                    # a window wider than a workgroup
]
STORED_SOURCE_BYTES = 1 << 16   # the fixture keeps sources up to here; larger ones by their sha only


def case_name(r, c, h, w):
    return f"r{r}_c{c}_{h}x{w}"


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def source(h, w):
    """Uniform random bytes with a centred block of 255 next to a block of 0,
    each a quarter of the image on a side (numpy PCG64: stable across versions).
    A byte is drawn per pixel up to a short side of 127 and per k x k cell,
    k = short side // 64, above: a 65-tap average of independent pixels would
    leave the window a few dozen values around 127, too few to show a wrong tap."""
    rng = np.random.Generator(np.random.PCG64(1000 * h + w))
    k = max(1, min(h, w) // 64)
    img = rng.integers(0, 256, (-(-h // k), -(-w // k), 3), dtype=np.uint8)
    img = np.ascontiguousarray(img.repeat(k, 0).repeat(k, 1)[:h, :w])
    bh, bw = h // 4, w // 4
    y0, x0 = (h - bh) // 2, w // 2 - bw
    img[y0:y0 + bh, x0:x0 + bw] = 255
    img[y0:y0 + bh, x0 + bw:x0 + 2 * bw] = 0
    return img


def resized_size(h, w, r):
    """torchvision Resize(r): short side -> r, long side -> int(r * long / short)."""
    if w <= h:
        return int(r * h / w), r
    return r, int(r * w / h)


def crop_offset(size, c):
    """torchvision CenterCrop: int(round((size - c) / 2.0)), halves to even."""
    return int(round((size - c) / 2.0))


def coeffs(n_in, n_out, first, count):
    """[(xmin, [k0, k1, ...]), ...] for output samples first .. first + count - 1."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(first, first + count):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((i + xmin - center + 0.5) * ss)) for i in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        out.append((xmin, [int(0.5 + (v / ww) * 4194304.0) for v in w]))
    return out


def _clip8(acc):
    """acc: int64 holding int32-range sums."""
    assert acc.min() >= -(1 << 31) and acc.max() < (1 << 31)
    return np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample_crop(img, oh, ow, top, left, ch, cw):
    """(window u8 [ch, cw, 3], column table, row table): ``img`` resampled to
    (oh, ow), of which only the window is computed."""
    h, w, _ = img.shape
    htab = coeffs(w, ow, left, cw)
    vtab = coeffs(h, oh, top, ch)
    yfirst = vtab[0][0]
    ylast = vtab[-1][0] + len(vtab[-1][1])
    rows = img[yfirst:ylast].astype(np.int64)
    mid = np.empty((ylast - yfirst, cw, 3), np.uint8)
    for c, (xmin, k) in enumerate(htab):
        kk = np.asarray(k, np.int64)
        mid[:, c] = _clip8((rows[:, xmin:xmin + len(k)] * kk[None, :, None]).sum(1))
    mid = mid.astype(np.int64)
    out = np.empty((ch, cw, 3), np.uint8)
    for r, (ymin, k) in enumerate(vtab):
        kk = np.asarray(k, np.int64)
        out[r] = _clip8((mid[ymin - yfirst:ymin - yfirst + len(k)] * kk[:, None, None]).sum(0))
    return out, htab, vtab


def resize_center_crop(img, r, c):
    """(window, column table, row table) of Resize(r) -> CenterCrop(c)."""
    h, w, _ = img.shape
    oh, ow = resized_size(h, w, r)
    return resample_crop(img, oh, ow, crop_offset(oh, c), crop_offset(ow, c), c, c)


_CACHE = {}


def case(r, c, h, w):
    """{'src', 'out', 'htab', 'vtab'} of one matrix case, computed once and never written to."""
    key = (r, c, h, w)
    if key not in _CACHE:
        src = source(h, w)
        out, htab, vtab = resize_center_crop(src, r, c)
        for a in (src, out):
            a.setflags(write=False)
        _CACHE[key] = {"src": src, "out": out, "htab": htab, "vtab": vtab}
    return _CACHE[key]


def table_records(tab, stride, index):
    """(xmin, [k...]) of record ``index`` of a workspace table (int32 words)."""
    rec = tab[index * stride:(index + 1) * stride]
    n = int(rec[1])
    return int(rec[0]), [int(v) for v in rec[2:2 + n]]
