"""CPU: what the 32 x 32 dynamic int8 conv pair (csrc/conv_dyn_pair32.hip)
decides on the host: the shapes it serves, the statuses of calls it must refuse
before any HIP call, and the values of pairs= that the models accept."""
import ctypes as C

import numpy as np
import pytest

from qconvnet import _lib


@pytest.mark.parametrize("shape,want", [
    ((32, 32, 3, 64, 64), 1), ((17, 8, 16, 8, 8), 1), ((1, 1, 1, 1, 1), 1), ((32, 32, 64, 64, 64), 1),
    ((33, 8, 3, 8, 8), 0), ((8, 33, 3, 8, 8), 0), ((8, 8, 65, 8, 8), 0), ((8, 8, 3, 65, 8), 0),
    ((8, 8, 3, 8, 65), 0), ((0, 8, 3, 8, 8), 0), ((8, 8, 0, 8, 8), 0), ((8, -1, 3, 8, 8), 0),
    ((8, 8, 3, 8, -4), 0)], ids=str)
def test_supported(shape, want):
    assert _lib.load().qcn_conv3x3_dyn_pair32_supported(*shape) == want


def test_status_codes():
    """Pointers are never read: every refusal comes before any HIP call."""
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    P = buf.ctypes.data + (-buf.ctypes.data % 16)

    def layer(w=P, ch=8, alpha=None, beta=None, scale=P):
        return _lib.DynLayer(w, P, scale, 1, ch, None, alpha, beta, 1)

    def call(x=P, nimg=2, h=32, w=32, cin=3, st=P, slots=1, la=None, lb=None, pool=0, y=P, mid=None):
        return lib.qcn_conv3x3_dyn_pair32(x, nimg, h, w, cin, 0, st, slots, 0, C.byref(la or layer()),
                                          C.byref(lb or layer()), pool, 0, y, None, None, mid, None)
    A, U = _lib.QCN_ERR_ARG, _lib.QCN_ERR_UNSUPPORTED
    cases = [("x=null", A, call(x=None)), ("x_stats=null", A, call(st=None)), ("y=null", A, call(y=None)),
             ("A.w=null", A, call(la=layer(w=None))), ("B.w misaligned", A, call(lb=layer(w=P + 4))),
             ("B.w_scale misaligned", A, call(lb=layer(scale=P + 2))), ("mid_qparams misaligned", A, call(mid=P + 1)),
             ("A alpha without beta", A, call(la=layer(alpha=P))), ("cmid=0", A, call(la=layer(ch=0))),
             ("nimg=0", A, call(nimg=0)), ("x_slots=0", A, call(slots=0)),
             ("pool odd h", A, call(h=31, pool=1)), ("pool odd w", A, call(w=7, pool=1)),
             ("33 x 8", U, call(h=33, w=8)), ("8 x 33", U, call(h=8, w=33)), ("cin 65", U, call(cin=65)),
             ("cmid 65", U, call(la=layer(ch=65))), ("cout 65", U, call(lb=layer(ch=65))),
             ("batch past 2^31 elements", U, call(nimg=(1 << 15) + 1, cin=64))]
    assert [(lbl, got) for lbl, want, got in cases if got != want] == []


def test_pairs_argument():
    from models.dynamic_ptq_model import DynamicPTQModel, DynamicQuantConvNet
    from models.static_ptq_model import StaticPTQModel
    for make in (lambda: DynamicQuantConvNet({}, body="hip", pairs="all"),
                 lambda: DynamicQuantConvNet({}, body="torch", pairs="all"),
                 lambda: DynamicPTQModel().quantize(body="hip", pairs="all"),
                 lambda: StaticPTQModel(mode="reference").quantize(body="torch", pairs="all"),
                 lambda: DynamicQuantConvNet({}, body="int8", pairs="some"),
                 lambda: DynamicPTQModel().quantize(body="int8", pairs="some"),
                 lambda: StaticPTQModel(mode="reference").quantize(body="int8", pairs="some")):
        with pytest.raises(ValueError, match="pairs"):
            make()
