"""Edge inputs of the dynamic int8 conv tests (test_conv_dyn_edges_cpu.py
proves with oracle.qref that each construction does what it claims;
test_gpu_conv_dyn_edges.py feeds them to conv3x3_dyn, conv3x3_dyn_pair,
conv3x3_dyn_pair32 and image_minmax).  Host only: nothing here touches a
device."""
import functools

import numpy as np

import opedge as E
from oracle import qref

F32 = np.float32

# ------------------------------------------------------------------ input ties
# (nimg, h, w, cin, cout) of conv3x3_dyn: one per wave-block class (w <= 8, w <= 16, wider)
TIE_SHAPES = ((2, 4, 6, 20, 5), (2, 6, 12, 16, 70), (1, 4, 40, 4, 8))
# (shift, the zero point it gives): values in [0, 255] and in [-128, 127], scale 1 both times
TIE_SHIFTS = ((0, 0), (128, 128))


def tie_images(n, h, w, c, shift, seed):
    """Multiples of 0.5 in [0, 255] - shift with both ends present in every
    image: scale 1, zero point shift, and x / s + z = k + 0.5 for about half of
    the elements."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 511, (n, h, w, c)).astype(F32) * F32(0.5)
    x[:, 0, 0, 0], x[:, -1, -1, -1] = 0.0, 255.0
    return x - F32(shift)


def scaled(x, scale, zero_point):
    """fmaf(x, fp32(1 / s), fp32(z)): the value quantize_legacy rounds."""
    x = np.asarray(x, F32)
    return qref.fmaf(x, np.full(x.shape, F32(1.0) / F32(scale), F32), np.full(x.shape, F32(zero_point), F32))


def tie_share(x, scale, zero_point):
    """Share of the elements whose scaled value is an exact k + 0.5 inside (0, 255)."""
    t = scaled(x, scale, zero_point).astype(np.float64)
    return float(np.mean((t - np.floor(t) == 0.5) & (t > 0) & (t < 255)))


def quantize_half_away(x, scale, zero_point):
    """quantize_legacy_fma with the wrong rounding (half away from zero; the
    scaled values are >= 0 after the clamp): what the tie cases must tell from
    the contract."""
    t = np.minimum(scaled(x, scale, zero_point), F32(255)).astype(np.float64)
    return np.clip(np.floor(t + 0.5), 0, 255).astype(np.uint8)


def acc_with(quantize, x, wq, rr=False):
    """Contract steps 1-3 per image with ``quantize(x, s, z)`` as step 2:
    int32 accumulators [n, h, w, cout]."""
    ohwi = np.ascontiguousarray(wq.transpose(0, 2, 3, 1))
    acc = []
    for xi in x:
        s, z = qref.choose_qparams_dynamic(xi.min(), xi.max(), reduce_range=rr)
        acc.append(qref.conv3x3_acc_nhwc(quantize(xi, s, z)[None], z, ohwi)[0])
    return np.stack(acc)


# -------------------------------------------------------------------- mid ties
MID_S_W = np.array([0.125], F32)
# (h, w) of conv3x3_dyn_pair's 4-wave and 8-wave class and of conv3x3_dyn_pair32 (a second pixel
# group down), all with cin = cmid = MID_C
MID_MAPS = {"pair4": (6, 5), "pair8": (10, 12), "pair32": (18, 9)}
MID_C, MID_COUT, MID_N = 16, 20, 3


def mid_tie_case(h, w, seed):
    """(x, wa, wb): integers in [0, 255] with 0 and 255 in channel 0, so s_x = 1
    and z_x = 0; layer A copies every channel through its centre tap, weight 4
    on channel 0 and 1 on the others, with s_w = 0.125, no bias and no affine.
    The mid activation is x / 2 in channel 0 and x / 8 in the others: range
    [0, 127.5], s_mid = 0.5, z_mid = 0, and x / 4 is a tie wherever x % 4 == 2.
    Layer B has random full-range weights."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (MID_N, h, w, MID_C)).astype(F32)
    x[:, 0, 0, 0], x[:, -1, -1, 0] = 255.0, 0.0
    wa = np.zeros((MID_C, MID_C, 3, 3), np.int8)
    wa[np.arange(MID_C), np.arange(MID_C), 1, 1] = 1
    wa[0, 0, 1, 1] = 4
    wb = rng.integers(-128, 128, (MID_COUT, MID_C, 3, 3), dtype=np.int8)
    return x, wa, wb


# --------------------------------------------------------------------- classes
# the classes of opedge.DYN_CLASSES that tests/test_gpu_conv_dyn.py leaves out, and "small"
NEW_CLASSES = ("positive", "negzero", "tiny", "subnormal", "onehot", "small")
ALL_CLASSES = E.DYN_CLASSES + ("small",)
# these quantize to one code, the zero point (every accumulator is 0): kept as edges, the only
# inputs exempt from opedge.distinct_ok
SINGLE_CODE = ("zero", "negzero", "tiny", "subnormal")
# (h, w, cin, cmid, cout) of the class tests: odd sizes inside every kernel's smallest class
CLASS_SHAPE = (5, 7, 20, 24, 9)
SMALL_SCALE = F32(6.1e-5)


def class_image(kind, h, w, c, seed):
    if kind == "small":     # scale below 6.1e-5 with both ends non-zero: the amplified range
        return (np.random.default_rng(seed).standard_normal((h, w, c)) * 1e-3).astype(F32)
    return E.dyn_input(kind, 1, h * w * c, seed).reshape(h, w, c)


def class_batch(kinds, h, w, c, seed):
    """One image per entry of ``kinds``, seeds seed, seed + 1, ..."""
    return np.stack([class_image(k, h, w, c, seed + i) for i, k in enumerate(kinds)])


# BATCHES[name] = kinds of its images: three of each new class, then every class once
BATCHES = {k: (k,) * 3 for k in NEW_CLASSES}
BATCHES["mixed"] = ALL_CLASSES


# --------------------------------------------------------------------- deep K
DEEP_CIN = 7310            # CD_MAX_CIN of csrc/conv_dyn.hpp
DEEP_PEAK = 9 * DEEP_CIN * 255 * 127


@functools.lru_cache(maxsize=None)
def deep_k_case(cout):
    """(x [3, 3, 3, 7310], wq [cout, 7310, 3, 3]) with codes 0 and 255 only
    (zero points 0, 0, 255) and weights +-127, channel 0 all 127 and channel 1
    all -127: the centre pixel's accumulators reach +-9 * 7310 * 255 * 127."""
    rng = np.random.default_rng(7)
    x = np.ones((3, 3, 3, DEEP_CIN), F32)                   # z = 0: every pixel is code 255
    x[1] = rng.integers(0, 2, x[1].shape).astype(F32)       # codes 0 and 255
    x[2] = -1.0                                             # z = 255: q - z is -255
    wq = (rng.integers(0, 2, (cout, DEEP_CIN, 3, 3)) * 254 - 127).astype(np.int8)
    wq[0], wq[1] = 127, -127
    return x, wq


# ---------------------------------------------------------------- image_minmax
MINMAX_COUNTS = (257, 343, 1023, 4097, 1024)   # 1024: the float4 kernel's loop, and the scalar one's at an offset


def minmax_images(count, seed):
    """[4, count]: +-100 planted in the first and the last element (images 0 and
    1, both ways round) and both inside the last count % 4 elements where
    there are two (image 2); the last image is left alone."""
    x = np.random.default_rng(seed).standard_normal((4, count)).astype(F32)
    x[0, 0], x[0, -1] = 100.0, -100.0
    x[1, 0], x[1, -1] = -100.0, 100.0
    x[2, -1] = 100.0
    if count % 4 >= 2:
        x[2, count - count % 4] = -100.0
    return x
