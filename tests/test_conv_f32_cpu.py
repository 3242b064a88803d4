"""CPU: host side of the deterministic fp32 3x3 conv (csrc/conv_f32.hip): the
weight packing against a numpy restatement of the layout documented in
include/qconvnet.h, and the statuses of calls the entry must refuse before any
launch (so they hold without a GPU)."""
import numpy as np
import pytest

from qconvnet import _lib, ops


def packed_ref(w):
    """out[ct][step][lane][s] = w[32 ct + lane % 32][8 G + 2 s + lane // 32][tap],
    step = 72 (G // 8) + tap gc + G % 8; +0 past cin and cout."""
    cout, cin = w.shape[:2]
    ng, nct = -(-cin // 8), 2 * (-(-cout // 64))
    wz = np.zeros((nct * 32, ng * 8, 9), np.float32)
    wz[:cout, :cin] = w.reshape(cout, cin, 9)
    out = np.zeros((nct, 9 * ng, 64, 4), np.float32)
    lane, s = np.meshgrid(np.arange(64), np.arange(4), indexing="ij")
    for ct in range(nct):
        for G in range(ng):
            gc = min(8, ng - 8 * (G // 8))
            for tap in range(9):
                out[ct, 72 * (G // 8) + tap * gc + G % 8] = wz[32 * ct + lane % 32, 8 * G + 2 * s + lane // 32, tap]
    return out.reshape(-1)


@pytest.mark.parametrize("cin,cout", [(3, 64), (5, 7), (64, 128), (68, 33)])
def test_pack_layout(cin, cout):
    w = np.random.default_rng(cin).standard_normal((cout, cin, 3, 3)).astype(np.float32)
    w[w == 0] = 1.0
    got = ops.pack_conv3x3_f32(w)
    ref = packed_ref(w)
    assert got.size == _lib.load().qcn_conv3x3_f32_packed_size(cin, cout) == ref.size
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))   # padded slots are +0
    assert np.count_nonzero(got) == w.size


def status_cases():
    """(label, expected status, status) of qcn_conv3x3_f32; pointers are never read."""
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    P = buf.ctypes.data + (-buf.ctypes.data % 16)

    def call(x=P, nimg=2, h=8, w=8, cin=8, wp=P, cout=8, alpha=None, beta=None, pool=0, y=P):
        return lib.qcn_conv3x3_f32(x, nimg, h, w, cin, 0, wp, cout, None, alpha, beta, 1, pool, 0, y, None)
    A, U = _lib.QCN_ERR_ARG, _lib.QCN_ERR_UNSUPPORTED
    return [("x=null", A, call(x=None)), ("w=null", A, call(wp=None)), ("y=null", A, call(y=None)),
            ("nimg=0", A, call(nimg=0)), ("h=0", A, call(h=0)), ("cout=0", A, call(cout=0)),
            ("alpha without beta", A, call(alpha=P)), ("beta without alpha", A, call(beta=P)),
            ("pool odd h", A, call(h=7, pool=1)), ("pool odd w", A, call(w=7, pool=1)),
            ("w misaligned", A, call(wp=P + 4)),
            ("batch past 2^31 elements", U, call(nimg=(1 << 22) + 1)),
            ("nimg=0 and past 2^31", A, call(nimg=0, h=1 << 16, w=1 << 16))]


def test_status_codes():
    assert [(lbl, got) for lbl, want, got in status_cases() if got != want] == []
    lib = _lib.load()
    assert lib.qcn_conv3x3_f32_packed_size(0, 8) == _lib.QCN_ERR_ARG
    assert lib.qcn_pack_conv3x3_weight_f32(None, 8, 8, None) == _lib.QCN_ERR_ARG
