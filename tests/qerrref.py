"""numpy restatement of the quantization-error statistics (include/qconvnet.h,
qcn_qerror_u8_f32).  float32 for the fp32 steps, float64 sums by np.sum; no
code shared with the product.

Per element:  d = scale * float(int(q) - zp)
              lo = scale * float(0 - zp),  hi = scale * float(255 - zp)
              qref = clamp(zp + rne(x * inv), 0, 255),  inv = fp32(1) / scale
              e = double(x) - double(d)
Per channel:  counts = [elements, #(x < lo), #(x > hi), #(qref != q),
                        bits of max |x - d| (fp32)]
              sums   = [sum double(x)^2, sum e^2, sum |e|]
"""
import numpy as np

F32 = np.float32
QPARAMS = ((0.05, 17), (0.0213, 0), (0.11, 128), (0.02, 255))


def dequant(q, scale, zp):
    return (F32(scale) * (q.astype(np.int32) - int(zp)).astype(F32)).astype(F32)


def qref(x, scale, zp):
    inv = F32(1.0) / F32(scale)
    t = np.rint((np.asarray(x, F32) * inv).astype(F32))
    return np.clip(t.astype(np.int64) + int(zp), 0, 255).astype(np.uint8)


def stats(x, q, scale, zp):
    """x fp32 and q u8, both [n, c, ...] with the channel on axis 1 (an NHWC q
    is transposed by the caller).  Returns counts int64 [c, 5], sums float64
    [c, 3]."""
    x = np.asarray(x, F32)
    c = x.shape[1]
    xs = np.moveaxis(x, 1, 0).reshape(c, -1)
    qs = np.moveaxis(np.asarray(q, np.uint8), 1, 0).reshape(c, -1)
    d = dequant(qs, scale, zp)
    lo = F32(scale) * F32(0 - int(zp))
    hi = F32(scale) * F32(255 - int(zp))
    counts = np.zeros((c, 5), np.int64)
    counts[:, 0] = xs.shape[1]
    counts[:, 1] = (xs < lo).sum(1)
    counts[:, 2] = (xs > hi).sum(1)
    counts[:, 3] = (qref(xs, scale, zp) != qs).sum(1)
    if xs.shape[1]:
        counts[:, 4] = np.abs((xs - d).astype(F32)).max(1).view(np.uint32)
    e = xs.astype(np.float64) - d.astype(np.float64)
    x64 = xs.astype(np.float64)
    sums = np.stack([np.sum(x64 * x64, axis=1), np.sum(e * e, axis=1), np.sum(np.abs(e), axis=1)], 1)
    return counts, sums


def sqnr_db(x, q, scale, zp):
    """Whole-tensor 10 log10(sum x^2 / sum e^2) in float64."""
    _, s = stats(np.asarray(x, F32).reshape(1, 1, -1), np.asarray(q).reshape(1, 1, -1), scale, zp)
    return 10.0 * np.log10(s[0, 0] / s[0, 1])


def make_case(rng, shape, scale, zp):
    """The checked recipe: q uniform in [0, 255] with 5 % forced to 0 and 5 %
    to 255; x = d + scale * noise, noise ~ N(0, 0.35) on interior codes and
    N(0, 3) on the two end codes.  Returns (x fp32, q u8), both ``shape``."""
    q = rng.integers(0, 256, shape).astype(np.uint8)
    u = rng.random(shape)
    q[u < 0.05] = 0
    q[u > 0.95] = 255
    end = (q == 0) | (q == 255)
    noise = rng.standard_normal(shape) * np.where(end, 3.0, 0.35)
    x = (dequant(q, scale, zp) + F32(scale) * noise.astype(F32)).astype(F32)
    return x, q


def close(got, ref, n_c):
    """Every sums entry within relative 4 * N_c * 2^-53 of the restatement; a
    zero on one side is a zero on the other."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    if not np.array_equal(got == 0, ref == 0):
        return False
    return bool(np.all(np.abs(got - ref) <= 4.0 * n_c * 2.0 ** -53 * np.abs(ref)))
