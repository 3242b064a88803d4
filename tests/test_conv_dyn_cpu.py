"""CPU: host side of the dynamic int8 3x3 conv (csrc/conv_dyn.hip): the weight
packing against a numpy restatement of the layout in include/qconvnet.h, and
the statuses of calls the entries must refuse before any HIP call."""
import numpy as np
import pytest

from qconvnet import _lib, ops


def packed_ref(w):
    cout, cin = w.shape[:2]
    ncg, nct = -(-cin // 16), 4 * (-(-cout // 64))
    steps = (ncg // 16) * 36 + (9 * (ncg % 16) + 3) // 4
    wz = np.zeros((nct * 16, -(-cin // 256) * 256, 9 + 4), np.int8)   # taps 9.. stay 0
    wz[:cout, :cin, :9] = w.reshape(cout, cin, 9)
    out = np.zeros((nct, steps, 64, 16), np.int8)
    lane, b = np.meshgrid(np.arange(64), np.arange(16), indexing="ij")
    for step in range(steps):
        chunk = step // 36
        ncgc = min(16, ncg - 16 * chunk)
        u = 4 * (step - 36 * chunk) + lane // 16
        for ct in range(nct):
            out[ct, step] = wz[16 * ct + lane % 16, 256 * chunk + 16 * (u % ncgc) + b, u // ncgc]
    return out.reshape(-1)


@pytest.mark.parametrize("cin,cout", [(3, 64), (20, 65), (64, 128), (272, 4)])
def test_pack_layout(cin, cout):
    w = np.random.default_rng(cin).integers(-128, 128, (cout, cin, 3, 3), dtype=np.int8)
    w[w == 0] = 1
    got, wsum = ops.pack_conv3x3_dyn(w)
    ref = packed_ref(w)
    assert got.size == _lib.load().qcn_conv3x3_dyn_packed_size(cin, cout) == ref.size
    assert np.array_equal(got, ref) and np.count_nonzero(got) == w.size
    assert np.array_equal(wsum, w.reshape(cout, -1).astype(np.int64).sum(1))


def status_cases():
    """(label, expected status, status) of the conv_dyn entries; pointers are never read."""
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    P = buf.ctypes.data + (-buf.ctypes.data % 16)

    def call(x=P, nimg=2, h=8, w=8, cin=8, st=P, slots=1, wp=P, cout=8, alpha=None, beta=None, pool=0, y=P):
        return lib.qcn_conv3x3_dyn(x, nimg, h, w, cin, 0, st, slots, 0, wp, P, P, 1, cout, None, alpha, beta,
                                   1, pool, 0, y, None, None, None)
    A, U = _lib.QCN_ERR_ARG, _lib.QCN_ERR_UNSUPPORTED
    return [("x=null", A, call(x=None)), ("x_stats=null", A, call(st=None)), ("w=null", A, call(wp=None)),
            ("y=null", A, call(y=None)), ("nimg=0", A, call(nimg=0)), ("h=0", A, call(h=0)),
            ("cout=0", A, call(cout=0)), ("x_slots=0", A, call(slots=0)),
            ("alpha without beta", A, call(alpha=P)), ("beta without alpha", A, call(beta=P)),
            ("pool odd h", A, call(h=7, pool=1)), ("pool odd w", A, call(w=7, pool=1)),
            ("w misaligned", A, call(wp=P + 4)), ("cin past the int32 bound", U, call(cin=7311)),
            ("batch past 2^31 elements", U, call(nimg=(1 << 22) + 1)),
            ("nimg=0 and past 2^31", A, call(nimg=0, h=1 << 16, w=1 << 16)),
            ("minmax x=null", A, lib.qcn_image_minmax_f32(None, 1, 4, P, None)),
            ("minmax count=0", A, lib.qcn_image_minmax_f32(P, 1, 0, P, None))]


def test_status_codes():
    assert [(lbl, got) for lbl, want, got in status_cases() if got != want] == []
    lib = _lib.load()
    assert lib.qcn_conv3x3_dyn_packed_size(0, 8) == _lib.QCN_ERR_ARG
    assert lib.qcn_conv3x3_dyn_packed_size(7310, 8) > 0
    assert lib.qcn_conv3x3_dyn_packed_size(7311, 8) == _lib.QCN_ERR_UNSUPPORTED
    assert lib.qcn_pack_conv3x3_weight_dyn(None, 8, 8, None, None) == _lib.QCN_ERR_ARG
    # slots of the six layers: blocks per image of their grids
    assert [lib.qcn_conv3x3_dyn_stats_slots(*s) for s in
            ((32, 32, 64), (16, 16, 128), (8, 8, 256), (9, 19, 130), (0, 8, 8))] == [4, 2, 1, 6, _lib.QCN_ERR_ARG]
