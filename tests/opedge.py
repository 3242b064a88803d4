"""Shared inputs and references of the op-edge tests (test_op_edges_cpu.py
pins these references against torch CPU ops; test_gpu_op_edges.py compares
the HIP kernels with them).  Host only: nothing here touches a device."""
import functools

import numpy as np

from oracle import qref

F32 = np.float32


def bits(a):
    """fp32 array as uint32 bit patterns (so the sign of zero counts)."""
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def distinct_ok(a):
    """An expected output is not degenerate: more than 8 distinct values
    where the shape allows (16 elements or more)."""
    a = np.asarray(a)
    return a.size < 16 or np.unique(a).size > 8


# ------------------------------------------------------------ quantize inputs
Q_SCALE = F32(2.0 ** -7)


def quant_input(count, seed):
    """fp32 data around +-200 quantization steps of Q_SCALE, with exact .5
    ties, +-1e9 and +-0.0 at both ends (the float4 body and the count & 3
    tail both see them)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(count) * 70).astype(F32) * Q_SCALE
    sp = np.array([(j + 0.5) * float(Q_SCALE) for j in (-4, -3, -1, 0, 1, 2, 125, 251)] +
                  [1e9, -1e9, 0.0, -0.0], F32)
    k = min(count, sp.size)
    x[count - k:] = sp[:k]
    if count >= 2 * sp.size:
        x[:sp.size] = sp[::-1]
    return x


# --------------------------------------------------- dynamic-Linear input classes
DYN_CLASSES = ("zero", "negzero", "tiny", "positive", "negative", "constant", "huge", "subnormal",
               "onehot", "normal")


def dyn_input(kind, m, k, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((m, k)).astype(F32)
    if kind == "zero":
        return np.zeros((m, k), F32)
    if kind == "negzero":
        return np.full((m, k), -0.0, F32)
    if kind == "tiny":
        return (g * F32(1e-6)).astype(F32)
    if kind == "positive":
        return (np.abs(g) + F32(0.5)).astype(F32)
    if kind == "negative":
        return (-np.abs(g) - F32(0.5)).astype(F32)
    if kind == "constant":
        return np.full((m, k), 1.75, F32)
    if kind == "huge":
        return (g * F32(1e30)).astype(F32)
    if kind == "subnormal":
        return (np.sign(g) * F32(1e-40) * rng.integers(1, 9, (m, k)).astype(F32)).astype(F32)
    if kind == "onehot":
        x = np.zeros((m, k), F32)
        x[m // 2, k // 2] = 3.0
        return x
    return g


def dyn_weights(k, n, seed):
    """s8 weights with -128 present, per-tensor and per-channel scales, bias."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-128, 128, (n, k), dtype=np.int8)
    w.reshape(-1)[0] = -128
    s_pt = np.array([0.0123], F32)
    s_pc = rng.uniform(0.004, 0.03, n).astype(F32)
    b = rng.standard_normal(n).astype(F32)
    return w, s_pt, s_pc, b


# ----------------------------------------------------------- static Linear data
def linear_case(m, k, n, seed):
    rng = np.random.default_rng(seed)
    qx = rng.integers(0, 256, (m, k), dtype=np.uint8)
    w = rng.integers(-128, 128, (n, k), dtype=np.int8)
    qx.reshape(-1)[:2] = (0, 255)[:qx.size]
    w.reshape(-1)[:2] = (-128, 127)[:w.size]
    # one output step is ~1/40 of the accumulator's spread (|x - zx| up to 255)
    s_x, s_wt = F32(0.02), F32(0.003)
    s_wc = rng.uniform(0.002, 0.004, n).astype(F32)
    s_y = F32(float(s_x) * float(s_wt) * 1.2e4 * np.sqrt(k) / 40)
    b = (rng.standard_normal(n) * 10 * float(s_y)).astype(F32)
    return qx, w, s_x, s_wt, s_wc, s_y, b


@functools.lru_cache(maxsize=None)
def head_case(m, k, n2, seed=5):
    """Classifier-head operands and fc1's exact accumulators per input zero
    point (shared by the static and the QDQ head tests)."""
    rng = np.random.default_rng(seed + m + k + n2)
    qx = rng.integers(0, 256, (m, k), dtype=np.uint8)
    w1 = rng.integers(-128, 128, (512, k), dtype=np.int8)
    w2 = rng.integers(-128, 128, (n2, 512), dtype=np.int8)
    qx.reshape(-1)[:2] = (0, 255)
    w1.reshape(-1)[:2] = (-128, 127)
    w2.reshape(-1)[0] = -128
    zx = 37
    acc1 = qref.linear_acc(qx, zx, w1)
    s_x, s_w1t, s_y1 = F32(0.02), F32(2e-4), F32(float(0.02 * 2e-4 * 1.2e4 * np.sqrt(k) / 40))
    s_w1c = rng.uniform(1e-4, 3e-4, 512).astype(F32)
    b1 = (rng.standard_normal(512) * 10 * float(s_y1)).astype(F32)
    s_w2t, s_w2c = F32(2e-3), rng.uniform(1e-3, 3e-3, n2).astype(F32)
    s_y2 = F32(float(s_y1) * 2e-3 * 74 * 60 * np.sqrt(512) / 40)
    b2 = (rng.standard_normal(n2) * 10 * float(s_y2)).astype(F32)
    return dict(qx=qx, w1=w1, w2=w2, zx=zx, acc1=acc1, s_x=s_x, s_w1t=s_w1t, s_w1c=s_w1c, s_y1=s_y1,
                b1=b1, s_w2t=s_w2t, s_w2c=s_w2c, s_y2=s_y2, b2=b2)


def gamma_bound(k):
    """(k+1) u / (1 - (k+1) u), u = 2^-24: the rounding-error bound of k fused
    multiply-adds and one add in fp32, in any order."""
    u = 2.0 ** -24
    return (k + 1) * u / (1 - (k + 1) * u)


# ------------------------------------------------- fp32 hand-offs (resnet_qdq)
# (z, z_next) pairs of the shared parameter sets; the last set is the tie set
HANDOFF_SETS = ((0, 0), (30, 255), (255, 7), (30, 7))


def handoff_params(c, which, seed=0):
    """(s, z, alpha, beta, s_next, z_next) of parameter set ``which``: alpha
    with positive, negative and zero entries, beta with a -0.0; the last set
    has alpha = 1, beta = 0, s_next = 2 s, so exact .5 ties reach the
    quantize."""
    z, z_next = HANDOFF_SETS[which]
    if which == len(HANDOFF_SETS) - 1:
        return F32(0.25), z, np.ones(c, F32), np.zeros(c, F32), F32(0.5), z_next
    rng = np.random.default_rng(100 * seed + which + c)
    idx = np.arange(c)
    alpha = rng.uniform(0.5, 1.5, c).astype(F32)
    alpha[idx % 3 == 1] *= F32(-1)
    alpha[idx % 4 == 2] = 0
    beta = rng.standard_normal(c).astype(F32)
    beta[1] = -0.0     # alpha < 0: q == z gives fma(+0, alpha, -0.0) = -0.0
    beta[2] = -0.0     # alpha == 0
    return F32(0.05), z, alpha, beta, F32(0.1), z_next


def _bn(x, alpha, beta):
    sh = x.shape
    return qref.bn_eval_nhwc(x.reshape(1, 1, -1, sh[-1]), alpha, beta).reshape(sh)


def ref_dq_bn_q(y, s, z, alpha, beta, relu, s_next, z_next):
    """dequantize -> bn_eval_nhwc -> [relu_f32] -> quantize_per_tensor."""
    f = _bn(qref.dequantize(y, s, z), alpha, beta)
    if relu:
        f = qref.relu_f32(f)
    return qref.quantize_per_tensor(f, s_next, z_next)


def ref_stem(y, s, z, alpha, beta, s_next, z_next):
    """... -> relu_f32 -> maxpool3x3s2_f32_nhwc (+ its quantize)."""
    f = qref.maxpool3x3s2_f32_nhwc(qref.relu_f32(_bn(qref.dequantize(y, s, z), alpha, beta)))
    return f, qref.quantize_per_tensor(f, s_next, z_next)


def ref_join(y3, s3, z3, a3, b3, ident, s_next, z_next):
    """relu_f32(bn3(dq(y3)) + identity) (+ its quantize); ``ident`` is the
    fp32 identity or (yd, sd, zd, ad, bd) of the downsample conv."""
    f = _bn(qref.dequantize(y3, s3, z3), a3, b3)
    if isinstance(ident, tuple):
        yd, sd, zd, ad, bd = ident
        ident = _bn(qref.dequantize(yd, sd, zd), ad, bd)
    out = qref.relu_f32((f + ident).astype(F32))
    return out, qref.quantize_per_tensor(out, s_next, z_next)


def wide_range_map(shape, seed):
    """fp32 values spread over six orders of magnitude, both signs."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(F32)


# ------------------------------------------------------------- BatchNorm data
def bn_stats(c, seed):
    """BN buffers with a negative-gamma channel, a zero gamma and a -0.0 shift."""
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal(c).astype(F32)
    var = rng.uniform(0.3, 2.0, c).astype(F32)
    gamma = rng.uniform(0.5, 1.5, c).astype(F32)
    gamma[1] = -gamma[1]
    gamma[2] = 0
    bias = rng.standard_normal(c).astype(F32)
    mean[3], bias[3] = 0, -0.0
    return mean, var, gamma, bias


def channel_affine_case(rows, cols):
    rng = np.random.default_rng(rows + cols)
    x = rng.standard_normal((rows, cols)).astype(F32)
    stats = bn_stats(cols, 9)
    x[0, :] = 0.0       # fma(+0, alpha < 0, ...) and the -0.0 shift of channel 3
    x[-1, 3] = -0.0
    return x, stats


def channel_affine_torch(x, stats, relu):
    """F.batch_norm(training=False) (+ torch.relu) on [rows, cols], on the CPU."""
    import torch
    import torch.nn.functional as tF
    mean, var, gamma, bias = (torch.from_numpy(a) for a in stats)
    t = tF.batch_norm(torch.from_numpy(x), mean, var, gamma, bias, training=False, eps=1e-5)
    return (torch.relu(t) if relu else t).numpy()
