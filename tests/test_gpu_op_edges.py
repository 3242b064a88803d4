"""GPU: the elementwise, Linear and fp32 hand-off kernels called directly at
their edges (count tails, the second grid-stride pass behind every grid cap,
channel counts that are no power of two, remainder K loops, partial feature
blocks, NULL optional operands, one-pixel and odd maps, signed zeros), each
against the numpy oracle, float64 or torch CPU ops.  The references are pinned
against torch in test_op_edges_cpu.py.  Integer outputs and fp32 outputs with
a fixed op order are compared exactly (fp32 as bit patterns); the fp32 GEMMs
against float64 are held to the rounding-error bound E.gamma_bound, nothing
else has a tolerance.  NaN input is outside every contract and not tested."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import opedge as E
from oracle import qref

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _T(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_bits(got, want):
    return np.array_equal(E.bits(got.cpu().numpy() if torch.is_tensor(got) else got), E.bits(want))


COUNTS = (1, 2, 3, 5, 7, 4099, 2_101_155)    # the last: n4 > 2048 * 256, a second pass


# ------------------------------------------------------------ elementwise.hip
@pytest.mark.parametrize("count", COUNTS)
def test_quantize_flat_tail_and_cap(dev, count):
    from qconvnet import ops
    x = E.quant_input(count, count)
    xt = _T(dev)(x.reshape(1, 1, 1, count))
    for zp in (0, 3, 255):
        want = qref.quantize_per_tensor(x, E.Q_SCALE, zp)
        got = ops.quantize(xt, E.Q_SCALE, zp, nhwc=False).cpu().numpy().reshape(-1)
        assert np.array_equal(got, want), (zp, int((got != want).sum()))
        assert E.distinct_ok(want)


@pytest.mark.parametrize("shape", [(2, c, h, w) for c in (1, 2, 3, 5) for h, w in ((1, 1), (7, 9))] +
                         [(9, 3, 256, 256)])     # 589 824 pixels > 2048 * 256
def test_quantize_nhwc_channels_and_cap(dev, shape):
    from qconvnet import ops
    x = E.quant_input(int(np.prod(shape)), shape[1] + shape[2]).reshape(shape)
    want = qref.quantize_per_tensor(qref.nchw_to_nhwc(x), E.Q_SCALE, 3)
    got = ops.quantize(_T(dev)(x), E.Q_SCALE, 3, nhwc=True).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert E.distinct_ok(want)


@pytest.mark.parametrize("count", COUNTS)
def test_dequantize_tail_and_cap(dev, count):
    from qconvnet import ops
    q = np.random.default_rng(count).integers(0, 256, count, dtype=np.uint8)
    q[-min(count, 3):] = (0, 128, 255)[:min(count, 3)]
    qt = _T(dev)(q)
    for zp in (0, 128, 255):
        want = qref.dequantize(q, F32(0.0371), zp)
        assert _same_bits(ops.dequantize(qt, F32(0.0371), zp), want), zp
        assert E.distinct_ok(want)


@pytest.mark.parametrize("shape", [(2, 7, 5, 16), (1, 2, 2, 48), (3, 3, 9, 5), (3, 512, 512, 3),
                                   (33, 128, 128, 64)])
def test_maxpool2x2_odd_maps_and_caps(dev, shape):
    """Odd sides (floor mode), c % 16 != 0 (the byte kernel) and both kernels'
    grid caps: 589 824 bytes and 540 672 16-byte groups of output."""
    from qconvnet import ops
    q = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    want = qref.maxpool2x2_nhwc(q)
    got = ops.maxpool2x2(_T(dev)(q)).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert E.distinct_ok(want)


def _argmax_rows(cols, rng):
    """Rows whose maximum repeats in one lane's stride (c, c + 64), in
    neighbouring lanes (c, c + 1) and sits in the last column; an all-equal
    row, an all -inf row, rows holding +inf; rows with many ties."""
    rows = []
    base = lambda: rng.standard_normal(cols).astype(F32)   # noqa: E731
    for c in (0, 5, 17, 40, 62, 63, 64, 130, cols - 2):
        for d in (64, 1):
            if 0 <= c and c + d < cols:
                r = base()
                r[[c, c + d]] = 9.0
                rows.append(r)
    r = base(); r[cols - 1] = 9.0; rows.append(r)
    rows.append(np.full(cols, 2.5, F32))
    rows.append(np.full(cols, -np.inf, F32))
    r = base(); r[cols // 2] = np.inf; rows.append(r)
    r = base(); r[[cols // 3, cols - 1]] = np.inf; rows.append(r)
    r = np.full(cols, -np.inf, F32); r[cols - 1] = -1e30; rows.append(r)
    for _ in range(3):
        rows.append(rng.integers(0, 4, cols).astype(F32))
    return np.stack(rows)


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 1000])
def test_argmax_strided_lanes_and_ties(dev, cols):
    from qconvnet import ops
    x = _argmax_rows(cols, np.random.default_rng(cols))
    want = np.argmax(x, axis=1)
    T = _T(dev)
    for i in range(x.shape[0]):                       # rows = 1
        got = ops.argmax(T(x[i:i + 1])).cpu().numpy()
        assert np.array_equal(got, want[i:i + 1]), (i, got, want[i])
    for i in range(0, x.shape[0] - 4, 3):             # rows = 5: a second workgroup
        got = ops.argmax(T(x[i:i + 5])).cpu().numpy()
        assert np.array_equal(got, want[i:i + 5]), (i, got, want[i:i + 5])
    assert cols == 1 or np.unique(want).size > min(8, cols // 2)


def test_minmax_tail_cap_zeros_subnormals(dev):
    from qconvnet import ops
    T = _T(dev)
    big = 8_388_613                                   # count / 4 > 2048 * 1024
    x = np.random.default_rng(1).standard_normal(big).astype(F32)
    for lo_at, hi_at in ((big - 1, big - 4), (0, 0)):  # the tail element / the last float4; index 0
        y = x.copy()
        y[lo_at] = -77.0
        if hi_at != lo_at:
            y[hi_at] = 99.0
        mm = ops.minmax_range(T(y)).cpu().numpy()
        assert _same_bits(mm, np.array([y.min(), y.max()], F32))
    for one in (F32(-3.5), F32(1e-41)):
        mm = ops.minmax_range(T(np.array([one], F32))).cpu().numpy()
        assert _same_bits(mm, np.array([one, one], F32))
    mm = ops.minmax_range(T(np.full(1003, 2.25, F32))).cpu().numpy()
    assert _same_bits(mm, np.array([2.25, 2.25], F32))
    z = np.zeros(1003, F32)
    z[::3] = -0.0
    mm = ops.minmax_range(T(z)).cpu().numpy()
    assert mm[0] == 0 and mm[1] == 0
    sub = (np.arange(1, 1004) % 17 + 1).astype(F32) * F32(1e-41)
    sub[5], sub[1000] = F32(-3e-40), F32(5e-39)
    mm = ops.minmax_range(T(sub)).cpu().numpy()
    assert _same_bits(mm, np.array([-3e-40, 5e-39], F32)) and mm[0] != 0 and mm[1] != 0


@pytest.mark.parametrize("rows,cols", [(1, 4), (3, 12), (5, 512), (1100, 2048)])   # 563 200 float4 > cap
def test_channel_affine_equals_torch_batch_norm(dev, rows, cols):
    """Exact against F.batch_norm(training=False) (+ torch.relu) on the CPU,
    the composition test_op_edges_cpu.py pins quant.bn_eval_affine with."""
    from qconvnet import ops, quant as Q
    x, stats = E.channel_affine_case(rows, cols)
    alpha, beta = Q.bn_eval_affine(*stats)
    assert (alpha < 0).any()
    T = _T(dev)
    for relu in (False, True):
        want = E.channel_affine_torch(x, stats, relu)
        got = ops.channel_affine(T(x), T(alpha), T(beta), relu=relu)
        assert _same_bits(got, want), relu
        assert E.distinct_ok(want)


# ----------------------------------------------------------------- linear.hip
@pytest.mark.parametrize("m,k,n", [(1, 128, 1), (33, 128, 65), (70, 384, 130), (5, 640, 64),
                                   (32, 1024, 68), (3, 1, 1), (7, 96, 33), (40, 200, 10)])
def test_linear_static_edges(dev, m, k, n):
    """k = 384 / 640: a remainder after the 4x-unrolled K loop; n = 65 / 130:
    a partial last feature block on the byte-store path, at blockIdx.y > 0 for
    m = 33 / 70; n = 68: a partial block on the 4-byte stores; k % 128 != 0:
    the generic kernel."""
    from qconvnet import ops, quant as Q
    qx, w, s_x, s_wt, s_wc, s_y, b = E.linear_case(m, k, n, m + k + n)
    wsum = w.astype(np.int64).sum(1)
    T = _T(dev)
    xt, wt = T(qx), T(w)
    for zx in (0, 37, 255):
        acc = qref.linear_acc(qx, zx, w)
        corr = T(((128 - zx) * wsum).astype(np.int32))
        for s_w in (s_wt, s_wc):
            u, v, mult = Q.epilogue_constants(s_x, s_w, s_y, b)
            assert all(np.array_equal(a, r) for a, r in zip((u, v, mult),
                                                            qref.requant_constants(s_x, s_w, s_y, b)))
            ut, vt, mt = T(u), T(v), T(mult)
            for relu, zy in ((True, 0), (True, 12), (False, 140)):
                want = qref.requantize(acc, u, v, mult, zy, relu)       # == qref.linear_q
                y = ops.linear_u8(xt, zx, wt, ut, vt, mt, corr, zy, relu)
                assert np.array_equal(y.cpu().numpy(), want), (zx, s_w.size, relu, zy)
                y, yf = ops.linear_u8(xt, zx, wt, ut, vt, mt, corr, zy, relu, y_scale=s_y,
                                      want_fp32=True)
                assert np.array_equal(y.cpu().numpy(), want), (zx, s_w.size, relu, zy)
                assert _same_bits(yf, qref.dequantize(want, s_y, zy))
                assert E.distinct_ok(want)


@pytest.mark.parametrize("m,k,n", [(5, 128, 33), (33, 384, 65), (7, 96, 33), (3, 40, 7), (1, 1, 1)])
def test_linear_dynamic_edges(dev, m, k, n):
    from qconvnet import ops
    w, s_pt, s_pc, b = E.dyn_weights(k, n, k + n)
    T = _T(dev)
    wt, wsum, bt = T(w), T(w.astype(np.int64).sum(1).astype(np.int32)), T(b)
    for kind in E.DYN_CLASSES:
        x = E.dyn_input(kind, m, k, 11)
        xt = T(x)
        for s_w in (s_pt, s_pc):
            st = T(s_w)
            for bias, bias_t in ((b, bt), (None, None)):
                for rr in (True, False):
                    want = qref.linear_dynamic(x, w, s_w, bias, reduce_range=rr)
                    got = ops.linear_dynamic(xt, wt, st, wsum, bias_t, reduce_range=rr)
                    assert _same_bits(got, want), (kind, s_w.size, bias is None, rr)
    assert E.distinct_ok(want)
    # a supplied range wider than the data, and one narrower: both clamps of
    # the LEGACY quantize act
    x = E.dyn_input("normal", m, k, 12)
    for lo, hi in ((x.min() - 2, x.max() + 3), (F32(-0.4), F32(0.3))):
        want = qref.linear_dynamic(x, w, s_pc, b, reduce_range=True, xrange=(F32(lo), F32(hi)))
        got = ops.linear_dynamic(T(x), wt, T(s_pc), wsum, bt, minmax=T(np.array([lo, hi], F32)))
        assert _same_bits(got, want), (lo, hi)
    if m * k >= 16:
        s_x, z_x = qref.choose_qparams_dynamic(F32(-0.4), F32(0.3))
        qx = qref.quantize_legacy_fma(x, s_x, z_x)
        assert (qx == 0).any() and (qx == 255).any()


@pytest.mark.parametrize("k", [1, 63, 64, 65, 512, 4096])
def test_linear_f32_against_float64(dev, k):
    """n > 16: a second 16-output pass; k % 64 != 0: idle lanes in the last
    stride.  Integer data: every partial sum is an integer below 2^24, so any
    summation order is exact and the result equals float64's.  Gaussian data:
    |y - y64| <= gamma (sum |x w| + |b|), gamma = E.gamma_bound(k), the bound
    of k fused multiply-adds and one add in any order."""
    from qconvnet import ops
    rng = np.random.default_rng(k)
    T = _T(dev)
    for m in (1, 5):
        for n in (1, 16, 17, 40):
            xi = rng.integers(-8, 9, (m, k)).astype(F32)
            wi = rng.integers(-8, 9, (n, k)).astype(F32)
            bi = rng.integers(-50, 51, n).astype(F32)
            xg = rng.standard_normal((m, k)).astype(F32)
            wg = rng.standard_normal((n, k)).astype(F32)
            bg = rng.standard_normal(n).astype(F32)
            for relu_in in (False, True):
                for use_b in (True, False):
                    for x, w, b, exact in ((xi, wi, bi, True), (xg, wg, bg, False)):
                        x64 = np.maximum(x, 0).astype(np.float64) if relu_in else x.astype(np.float64)
                        b64 = b.astype(np.float64) if use_b else np.zeros(n)
                        y64 = x64 @ w.astype(np.float64).T + b64
                        got = ops.linear_f32(T(x), T(w), T(b) if use_b else None,
                                             relu_in=relu_in).cpu().numpy()
                        if exact:
                            assert np.array_equal(got.astype(np.float64), y64), (m, n, relu_in, use_b)
                        else:
                            bound = E.gamma_bound(k) * (np.abs(x64) @ np.abs(w.astype(np.float64)).T
                                                        + np.abs(b64))
                            err = np.abs(got.astype(np.float64) - y64)
                            assert (err <= bound).all(), (m, n, relu_in, use_b, (err / bound).max())
                        assert relu_in or m * k == 1 or E.distinct_ok(y64)


# ------------------------------------------------------------- classifier.hip
HEAD_SHAPES = [(128, 1024, 1), (128, 2048, 16), (256, 1024, 16)]


def _head_layers(dev, c, per_channel):
    from qconvnet import ops, quant as Q
    T = _T(dev)
    u1, v1, m1 = Q.epilogue_constants(c["s_x"], c["s_w1c"] if per_channel else c["s_w1t"], c["s_y1"],
                                      c["b1"])
    corr1 = ((128 - c["zx"]) * c["w1"].astype(np.int64).sum(1)).astype(np.int32)
    l1 = NS(wk=T(ops.pack_fc_kmajor(c["w1"])), u=T(u1), v=T(v1), mult=T(m1), corr=T(corr1))
    return l1, (u1, v1, m1)


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("m,k,n2", HEAD_SHAPES)
def test_classifier_static_envelope(dev, m, k, n2, per_channel):
    """The documented envelope's other corners (k = 1024 / 2048, n2 = 1 / 16):
    all rows of fc1, fc2 and the dequantized logits against the oracle."""
    from qconvnet import ops, quant as Q
    c = E.head_case(m, k, n2)
    T = _T(dev)
    l1, (u1, v1, m1) = _head_layers(dev, c, per_channel)
    z1, z2 = 9, 131
    l1.z_y, l1.relu = z1, True
    u2, v2, m2 = Q.epilogue_constants(c["s_y1"], c["s_w2c"] if per_channel else c["s_w2t"], c["s_y2"],
                                      c["b2"])
    l2 = NS(w=T(c["w2"]), u=T(u2), v=T(v2), mult=T(m2), z_y=z2, relu=False, s_y=c["s_y2"])
    y1 = torch.empty((m, 512), dtype=torch.uint8, device=dev)
    y2 = torch.empty((m, n2), dtype=torch.uint8, device=dev)
    y2f = torch.empty((m, n2), dtype=torch.float32, device=dev)
    assert ops.classifier(ops.to_kmajor(T(c["qx"])), l1, l2, ops.classifier_workspace(m, 512, dev),
                          y1, y2, y2f)
    want1 = qref.requantize(c["acc1"], u1, v1, m1, z1, True)              # == qref.linear_q
    want2 = qref.linear_q(want1, z1, c["w2"], u2, v2, m2, z2, False)
    assert np.array_equal(y1.cpu().numpy(), want1)
    assert np.array_equal(y2.cpu().numpy(), want2)
    assert _same_bits(y2f, qref.dequantize(want2, c["s_y2"], z2))
    assert E.distinct_ok(want1) and E.distinct_ok(want2)


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("m,k,n2", HEAD_SHAPES)
def test_classifier_qdq_envelope(dev, m, k, n2, per_channel):
    """fc1 (no ReLU) against the oracle; the fp32 fc2 against float64 of
    relu(s1 (q1 - z1)) @ w2^T + b2: exactly on data whose sums are exact in
    fp32 (s1 = 1/4, w2 in eighths, b2 in 32nds), within E.gamma_bound(512) of
    it on Gaussian weights; also with b2 = NULL."""
    from qconvnet import ops
    c = E.head_case(m, k, n2)
    T = _T(dev)
    l1, (u1, v1, m1) = _head_layers(dev, c, per_channel)
    z1 = 100
    rng = np.random.default_rng(n2 + k)
    w2e = (rng.integers(-8, 9, (n2, 512)) / 8).astype(F32)
    b2e = (rng.integers(-64, 65, n2) / 32).astype(F32)
    w2g = rng.standard_normal((n2, 512)).astype(F32)
    b2g = rng.standard_normal(n2).astype(F32)
    xk, ws = ops.to_kmajor(T(c["qx"])), ops.classifier_workspace(m, 512, dev)
    want1 = qref.requantize(c["acc1"], u1, v1, m1, z1, False)             # == qref.linear_q
    assert E.distinct_ok(want1) and (want1 < z1).any() and (want1 > z1).any()
    for s1, w2, b2, exact in ((F32(0.25), w2e, b2e, True), (F32(0.25), w2e, None, True),
                              (c["s_y1"], w2g, b2g, False), (c["s_y1"], w2g, None, False)):
        l1.z_y, l1.s_y = z1, s1
        l2 = NS(w=T(w2), b=T(b2) if b2 is not None else None)
        y1 = torch.empty((m, 512), dtype=torch.uint8, device=dev)
        y2f = torch.empty((m, n2), dtype=torch.float32, device=dev)
        assert ops.classifier_qdq(xk, l1, l2, ws, y1, y2f)
        assert np.array_equal(y1.cpu().numpy(), want1)
        x64 = np.maximum(qref.dequantize(want1, s1, z1), 0).astype(np.float64)
        b64 = np.zeros(n2) if b2 is None else b2.astype(np.float64)
        y64 = x64 @ w2.astype(np.float64).T + b64
        got = y2f.cpu().numpy().astype(np.float64)
        if exact:
            assert np.array_equal(got, y64), int((got != y64).sum())
        else:
            bound = E.gamma_bound(512) * (x64 @ np.abs(w2.astype(np.float64)).T + np.abs(b64))
            err = np.abs(got - y64)
            assert (err <= bound).all(), (err / bound).max()
        assert E.distinct_ok(y64)


# ------------------------------------------------------------- resnet_qdq.hip
def _u8(shape, seed, z):
    y = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    y.reshape(-1)[::7] = z                  # q == z: the signed zeros of the BN
    return y


@pytest.mark.parametrize("rows,c", [(1, 4), (3, 12), (5, 64), (7, 2048), (17_500, 256)])   # n4 > 4096 * 256
def test_dq_bn_q_edges(dev, rows, c):
    from qconvnet import ops
    T = _T(dev)
    sets = range(len(E.HANDOFF_SETS)) if rows < 17_500 else (2,)   # one reference pair of the large map
    for which in sets:
        s, z, alpha, beta, s_next, z_next = E.handoff_params(c, which)
        y = _u8((rows, c), rows + which, z)
        yt, at, bt = T(y), T(alpha), T(beta)
        for relu in (False, True):
            want = E.ref_dq_bn_q(y, s, z, alpha, beta, relu, s_next, z_next)
            got = ops.dq_bn_q(yt, s, z, at, bt, relu, s_next, z_next).cpu().numpy()
            assert np.array_equal(got, want), (which, relu, int((got != want).sum()))
            # (a ReLU'd map quantized at zero point 255 is 255 everywhere)
            assert E.distinct_ok(want) or (relu and z_next == 255)


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 1, 7, 8), (2, 7, 1, 8), (3, 5, 6, 12), (2, 8, 8, 64),
                                   (1, 9, 9, 64), (21, 112, 112, 64)])     # 1 053 696 lanes > 4096 * 256
def test_dq_bn_relu_maxpool_edges(dev, shape):
    from qconvnet import ops
    T = _T(dev)
    c = shape[3]
    sets = range(len(E.HANDOFF_SETS)) if shape[0] < 21 else (2,)    # one reference of the large map
    for which in sets:
        s, z, alpha, beta, s_next, z_next = E.handoff_params(c, which)
        y = _u8(shape, sum(shape) + which, z)
        if shape[1] * shape[2] == 1:
            y[...] = z        # the one-pixel window keeps the BN's signed zeros
        want_f, want_q = E.ref_stem(y, s, z, alpha, beta, s_next, z_next)
        yt, at, bt = T(y), T(alpha), T(beta)
        f, q = ops.dq_bn_relu_maxpool(yt, s, z, at, bt, s_next, z_next)
        assert f.shape == want_f.shape and _same_bits(f, want_f), which
        assert np.array_equal(q.cpu().numpy(), want_q), which
        f, q = ops.dq_bn_relu_maxpool(yt, s, z, at, bt)                # out_q == NULL
        assert q is None and _same_bits(f, want_f), which
        assert E.distinct_ok(want_f) and (E.distinct_ok(want_q) or z_next == 255)
        if shape[1] * shape[2] == 1 and which < 3:
            assert (E.bits(want_f) == 0x80000000).any()                 # a -0.0 survives ReLU and the pool


@pytest.mark.parametrize("downsample", [False, True])
@pytest.mark.parametrize("rows,c", [(1, 4), (3, 12), (5, 2048), (2049, 2048)])   # 4 196 352 elements
def test_qdq_join_edges(dev, rows, c, downsample):
    from qconvnet import ops
    T = _T(dev)
    sets = range(len(E.HANDOFF_SETS)) if rows < 2049 else (2,)
    for which in sets:
        s3, z3, a3, b3, s_next, z_next = E.handoff_params(c, which)
        sd, zd, ad, bd, _, _ = E.handoff_params(c, (which + 1) % 3, seed=1)
        y3 = _u8((rows, c), rows + which, z3)
        if downsample:
            yd = _u8((rows, c), rows + which + 50, zd)
            ident, ident_t = (yd, sd, zd, ad, bd), (T(yd), sd, zd, T(ad), T(bd))
        else:
            ident = E.wide_range_map((rows, c), rows + which)
            ident.reshape(-1)[::5] = -0.0
            ident_t = T(ident)
        want_f, want_q = E.ref_join(y3, s3, z3, a3, b3, ident, s_next, z_next)
        args = (T(y3), s3, z3, T(a3), T(b3), ident_t)
        f, q = ops.qdq_join(*args, s_next, z_next)
        assert _same_bits(f, want_f), which
        assert np.array_equal(q.cpu().numpy(), want_q), which
        f, q = ops.qdq_join(*args)                                      # out_q == NULL
        assert q is None and _same_bits(f, want_f), which
        assert E.distinct_ok(want_f) and (E.distinct_ok(want_q) or z_next == 255)


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 2, 3, 12), (3, 7, 7, 2048), (2100, 1, 1, 2048)])
def test_avgpool_f32_edges(dev, shape):
    """7x7: three 16-pixel cascade blocks and a remainder; 2100 images of
    2048 channels: 1 075 200 lanes > 4096 * 256."""
    from qconvnet import ops
    x = E.wide_range_map(shape, sum(shape))
    want = qref.avgpool_f32_nhwc(x)
    assert _same_bits(ops.avgpool_f32(_T(dev)(x)), want)
    assert E.distinct_ok(want)


# ------------------------------------------------------- convgen.hip helpers
def _offset_by_one(dev, a):
    """A device copy of ``a`` that starts one byte past a 16-byte boundary."""
    buf = torch.empty(a.size + 1, dtype=torch.uint8, device=dev)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 1
    return view


@pytest.mark.parametrize("count", [16, 31, 32])
def test_add_relu_counts(dev, count):
    from qconvnet import ops
    rng = np.random.default_rng(count)
    a = rng.integers(0, 256, count, dtype=np.uint8)
    b = rng.integers(0, 256, count, dtype=np.uint8)
    T = _T(dev)
    for relu, z_out, za, zb in ((True, 0, 40, 30), (True, 255, 40, 30), (False, 255, 120, 140),
                                (False, 100, 120, 140)):
        p = (F32(0.05), za, F32(0.03), zb, F32(0.08), z_out)
        want = qref.add_relu_q(a, p[0], za, b, p[2], zb, p[4], z_out, relu)
        got = ops.add_relu(T(a), p[0], za, T(b), p[2], zb, p[4], z_out, relu=relu).cpu().numpy()
        assert np.array_equal(got, want), (relu, z_out)
        if z_out != 255:
            assert E.distinct_ok(want)
        elif not relu:
            assert (want < 255).any()                                   # negative sums kept without ReLU
    assert (want < 100).any()


def test_add_relu_unaligned_pointers(dev):
    """Pointers one byte past a 16-byte boundary take the element-wise path."""
    from qconvnet import ops
    rng = np.random.default_rng(40)
    a = rng.integers(0, 256, 40, dtype=np.uint8)
    b = rng.integers(0, 256, 40, dtype=np.uint8)
    want = qref.add_relu_q(a, F32(0.05), 120, b, F32(0.03), 140, F32(0.04), 3, True)
    out = _offset_by_one(dev, np.zeros(40, np.uint8))
    ops.add_relu(_offset_by_one(dev, a), F32(0.05), 120, _offset_by_one(dev, b), F32(0.03), 140,
                 F32(0.04), 3, out=out)
    assert np.array_equal(out.cpu().numpy(), want) and E.distinct_ok(want)


@pytest.mark.parametrize("shape", [(1, 1, 1, 16), (2, 1, 5, 16), (2, 7, 9, 48)])
def test_maxpool3x3s2_small_and_unaligned(dev, shape):
    from qconvnet import ops
    q = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    want = qref.maxpool3x3s2_nhwc(q)
    got = ops.maxpool3x3s2(_T(dev)(q)).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    out = _offset_by_one(dev, np.zeros(want.shape, np.uint8))
    ops.maxpool3x3s2(_offset_by_one(dev, q), out=out)                   # the byte-wise kernel
    assert np.array_equal(out.cpu().numpy(), want) and E.distinct_ok(want)


def test_avgpool_u8_window_limits(dev):
    from qconvnet import _lib, ops
    T = _T(dev)
    q = np.array([0, 7, 128, 255], np.uint8).reshape(1, 1, 1, 4)
    assert np.array_equal(ops.avgpool(T(q), 9).cpu().numpy(), qref.avgpool_q(q, 9))
    q = np.random.default_rng(2).integers(0, 256, (1, 256, 256, 4), dtype=np.uint8)   # hw = 65536
    q[..., 0], q[..., 1] = 255, q[..., 1] // 64
    for zp in (0, 200):
        want = qref.avgpool_q(q, zp)
        assert np.array_equal(ops.avgpool(T(q), zp).cpu().numpy(), want) and np.unique(want).size >= 3
    with pytest.raises(_lib.QcnError, match=r"\(-2\)"):                  # QCN_ERR_UNSUPPORTED, no launch
        ops.avgpool(torch.zeros((1, 65537, 1, 4), dtype=torch.uint8, device=dev), 0)


@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 3, 1, 8), (1, 3, 5, 2)])
def test_stem_pack_small_maps(dev, shape):
    from qconvnet import ops
    x = E.quant_input(int(np.prod(shape)), sum(shape)).reshape(shape)
    want = qref.stem_pack(x, E.Q_SCALE, 114)
    got = ops.stem_pack(_T(dev)(x), E.Q_SCALE, 114).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)


def test_handoff_argument_errors(dev):
    """Rejected on the host (QCN_ERR_ARG, no launch): c % 4 != 0 for the four
    hand-off kernels; qcn_qdq_join_f32 with both or neither identity."""
    from qconvnet import _lib, ops
    T = _T(dev)
    y = torch.zeros((2, 6), dtype=torch.uint8, device=dev)
    a = torch.ones(8, dtype=torch.float32, device=dev)
    bad = pytest.raises(_lib.QcnError, match=r"\(-1\)")
    with bad:
        ops.dq_bn_q(y, 0.1, 0, a, a, True, 0.1, 0)
    with bad:
        ops.dq_bn_relu_maxpool(y.view(1, 1, 2, 6), 0.1, 0, a, a)
    with bad:
        ops.qdq_join(y, 0.1, 0, a, a, torch.zeros((2, 6), dtype=torch.float32, device=dev))
    with bad:
        ops.avgpool_f32(torch.zeros((1, 1, 2, 6), dtype=torch.float32, device=dev))
    y = torch.zeros((2, 8), dtype=torch.uint8, device=dev)
    idf = torch.zeros((2, 8), dtype=torch.float32, device=dev)
    out = torch.empty((2, 8), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    for yd, f in ((p(y), p(idf)), (None, None)):
        rc = ops.lib().qcn_qdq_join_f32(p(y), 0.1, 0, p(a), p(a), yd, 0.1, 0, p(a), p(a), f, 16, 8,
                                        p(out), 0.1, 0, None, None)
        assert rc == _lib.QCN_ERR_ARG
