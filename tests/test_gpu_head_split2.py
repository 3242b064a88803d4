"""GPU: the classifier head from 1024 rows up, where fc1's split-K kernel
splits K over a workgroup's waves and writes two partial planes
(fc_splitk_kernel_wavek + fc_finish*_kernel<2>).  Static head: every row of u8
fc1, u8 fc2 and the fp32 logit bits against the numpy oracle.  QDQ head: fc1
against the oracle, the fp32 fc2 against float64 (exactly on data whose sums are
exact in fp32, within E.gamma_bound(512) on Gaussian weights).  One workspace
across the 1024-row switch: bit-equal to the two static linear kernels.

Shapes: 1024 rows is the smallest batch on this path; k = 1024 gives a wave
one load batch, 2048 two, 3072 three (an odd count behind the loop), 4096 the
unrolled form; 1152 rows give 18 row tiles (no power of two)."""
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


def _fc1_layer(dev, c, per_channel):
    from qconvnet import ops, quant as Q
    T = _T(dev)
    u1, v1, m1 = Q.epilogue_constants(c["s_x"], c["s_w1c"] if per_channel else c["s_w1t"], c["s_y1"],
                                      c["b1"])
    corr1 = ((128 - c["zx"]) * c["w1"].astype(np.int64).sum(1)).astype(np.int32)
    l1 = NS(wk=T(ops.pack_fc_kmajor(c["w1"])), u=T(u1), v=T(v1), mult=T(m1), corr=T(corr1))
    return l1, (u1, v1, m1)


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("m,k,n2", [(1024, 1024, 1), (1024, 2048, 16), (1152, 1024, 10), (1024, 3072, 10)])
def test_static_head_two_planes(dev, m, k, n2, per_channel):
    from qconvnet import ops, quant as Q
    c = E.head_case(m, k, n2)
    T = _T(dev)
    l1, (u1, v1, m1) = _fc1_layer(dev, c, per_channel)
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
    assert np.array_equal(E.bits(y2f.cpu().numpy()), E.bits(qref.dequantize(want2, c["s_y2"], z2)))
    assert E.distinct_ok(want1) and E.distinct_ok(want2)


@pytest.mark.parametrize("per_channel", [False, True])
def test_qdq_head_two_planes(dev, per_channel):
    from qconvnet import ops
    m, k, n2 = 1024, 1024, 10
    c = E.head_case(m, k, n2)
    T = _T(dev)
    l1, (u1, v1, m1) = _fc1_layer(dev, c, per_channel)
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


def test_workspace_reused_across_the_1024_row_switch(dev):
    """m = 1024 (two partial planes), 896 (four), 1024 again on one workspace,
    k = 4096: each run bit-equal to fc1 -> fc2 by the two static linear kernels."""
    from qconvnet import ops, quant as Q
    rng = np.random.default_rng(31)
    m, k, n1, n2 = 1024, 4096, 512, 10
    T = _T(dev)
    qx = rng.integers(0, 256, (m, k), dtype=np.uint8)
    w1 = rng.integers(-128, 128, (n1, k), dtype=np.int8)
    w2 = rng.integers(-128, 128, (n2, n1), dtype=np.int8)
    s_x, s_y1, s_y2, s_w1, s_w2 = F32(0.02), F32(0.05), F32(0.11), F32(2e-4), F32(2e-3)
    b1 = rng.normal(0, 0.5, n1).astype(F32)
    b2 = rng.normal(0, 0.5, n2).astype(F32)
    zx, z1, z2 = 11, 30, 120
    u1, v1, m1 = Q.epilogue_constants(s_x, s_w1, s_y1, b1)
    u2, v2, m2 = Q.epilogue_constants(s_y1, s_w2, s_y2, b2)
    corr1 = ((128 - zx) * w1.astype(np.int64).sum(1)).astype(np.int32)
    corr2 = ((128 - z1) * w2.astype(np.int64).sum(1)).astype(np.int32)
    y1_ref = ops.linear_u8(T(qx), zx, T(w1), T(u1), T(v1), T(m1), T(corr1), z1, True)
    y2_ref, y2f_ref = ops.linear_u8(y1_ref, z1, T(w2), T(u2), T(v2), T(m2), T(corr2), z2, False,
                                    y_scale=s_y2, want_fp32=True)
    assert E.distinct_ok(y1_ref.cpu().numpy()) and E.distinct_ok(y2_ref.cpu().numpy())
    l1 = NS(wk=T(ops.pack_fc_kmajor(w1)), u=T(u1), v=T(v1), mult=T(m1), corr=T(corr1), z_y=z1, relu=True)
    l2 = NS(w=T(w2), u=T(u2), v=T(v2), mult=T(m2), z_y=z2, relu=False, s_y=s_y2)
    ws = ops.classifier_workspace(m, n1, dev)
    for mm in (1024, 896, 1024):
        y1 = torch.zeros((mm, n1), dtype=torch.uint8, device=dev)
        y2 = torch.zeros((mm, n2), dtype=torch.uint8, device=dev)
        y2f = torch.zeros((mm, n2), dtype=torch.float32, device=dev)
        assert ops.classifier(ops.to_kmajor(T(qx[:mm])), l1, l2, ws, y1, y2, y2f)
        torch.cuda.synchronize()
        assert torch.equal(y1, y1_ref[:mm])
        assert torch.equal(y2, y2_ref[:mm])
        assert torch.equal(y2f, y2f_ref[:mm])
