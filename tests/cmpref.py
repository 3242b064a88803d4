"""numpy restatement of the fp32-against-fp32 error statistics
(include/qconvnet.h, qcn_qerror_f32_f32).  float32 where the definition says
fp32, float64 sums by np.sum; no code shared with the product.

Per element:  e = double(x) - double(y)
Per channel:  counts = [elements, #(x != y), bits of max |x - y| (fp32)]
              sums   = [sum double(x)^2, sum e^2, sum |e|, sum e]
"""
import numpy as np

F32 = np.float32


def stats(x, y):
    """x and y fp32, both [n, c, ...] with the channel on axis 1 (an NHWC y is
    transposed by the caller).  Returns counts int64 [c, 3], sums float64
    [c, 4]."""
    x = np.asarray(x, F32)
    y = np.asarray(y, F32)
    assert x.shape == y.shape
    c = x.shape[1]
    xs = np.moveaxis(x, 1, 0).reshape(c, -1)
    ys = np.moveaxis(y, 1, 0).reshape(c, -1)
    counts = np.zeros((c, 3), np.int64)
    counts[:, 0] = xs.shape[1]
    counts[:, 1] = (xs != ys).sum(1)
    if xs.shape[1]:
        counts[:, 2] = np.abs((xs - ys).astype(F32)).max(1).view(np.uint32)
    x64 = xs.astype(np.float64)
    e = x64 - ys.astype(np.float64)
    sums = np.stack([np.sum(x64 * x64, axis=1), np.sum(e * e, axis=1), np.sum(np.abs(e), axis=1),
                     np.sum(e, axis=1)], 1)
    return counts, sums


def sqnr_db(x, y):
    """Whole-tensor 10 log10(sum x^2 / sum e^2) in float64."""
    _, s = stats(np.asarray(x, F32).reshape(1, 1, -1), np.asarray(y, F32).reshape(1, 1, -1))
    return 10.0 * np.log10(s[0, 0] / s[0, 1])


def make_case(rng, shape):
    """The checked recipe: x ~ N(0, 1); y = x + N(0, 0.05) with 10 % of the
    elements set equal to x; where there are at least three channels, the
    last one wholly equal and channel 0 with x = 0 and y != 0 (a single
    channel keeps the ordinary recipe, or nothing else would be scored).
    Returns (x, y) fp32 NCHW, both ``shape``."""
    x = rng.standard_normal(shape).astype(F32)
    y = (x + (0.05 * rng.standard_normal(shape)).astype(F32)).astype(F32)
    same = rng.random(shape) < 0.10
    y[same] = x[same]
    c = shape[1]
    if c >= 3:
        y[:, c - 1] = x[:, c - 1]
        x[:, 0] = 0
        y[:, 0] = (0.05 * (1.0 + rng.random(x[:, 0].shape))).astype(F32)
    return x, y


def close(got, ref, n_c):
    """The derived bounds on sums [c, 4] against the restatement.  Columns 0-2
    (sum x^2, e^2, |e|): identical non-negative terms in another order, within
    relative 4 * N_c * 2^-53, a zero on one side a zero on the other.  Column 3
    (sum e): signed terms, within absolute 4 * N_c * 2^-53 * sum |e|."""
    got = np.asarray(got, np.float64).reshape(-1, 4)
    ref = np.asarray(ref, np.float64).reshape(-1, 4)
    eps = 4.0 * n_c * 2.0 ** -53
    g, r = got[:, :3], ref[:, :3]
    if not np.array_equal(g == 0, r == 0):
        return False
    if not np.all(np.abs(g - r) <= eps * np.abs(r)):
        return False
    return bool(np.all(np.abs(got[:, 3] - ref[:, 3]) <= eps * ref[:, 2]))


def excess(got, ref, n_c):
    """(largest relative error of columns 0-2, largest |sum e error| / sum |e|,
    the bound) for printing."""
    got = np.asarray(got, np.float64).reshape(-1, 4)
    ref = np.asarray(ref, np.float64).reshape(-1, 4)
    rel = np.max(np.abs(got[:, :3] - ref[:, :3]) / np.maximum(np.abs(ref[:, :3]), 1e-300))
    sgn = np.max(np.abs(got[:, 3] - ref[:, 3]) / np.maximum(ref[:, 2], 1e-300))
    return rel, sgn, 4.0 * n_c * 2.0 ** -53
