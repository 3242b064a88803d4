"""CPU: what the dynamic int8 conv pair (csrc/conv_dyn_pair.hip) decides on the
host: the shapes it serves, the statuses of calls it must refuse before any
HIP call, and where the models accept pairs=True."""
import ctypes as C

import numpy as np
import pytest

from qconvnet import _lib


@pytest.mark.parametrize("shape,want", [
    ((8, 8, 128, 256, 256), 1), ((16, 16, 64, 128, 128), 1), ((1, 1, 3, 1, 1), 1), ((8, 8, 7310, 8, 8), 1),
    ((9, 8, 16, 128, 128), 1), ((17, 8, 16, 8, 8), 0), ((8, 17, 16, 8, 8), 0), ((8, 8, 16, 257, 8), 0),
    ((8, 8, 16, 8, 257), 0), ((16, 16, 16, 129, 8), 0), ((9, 9, 16, 8, 129), 0), ((32, 32, 3, 64, 64), 0),
    ((8, 8, 7311, 8, 8), 0), ((0, 8, 16, 8, 8), 0)], ids=str)
def test_supported(shape, want):
    assert _lib.load().qcn_conv3x3_dyn_pair_supported(*shape) == want


def test_status_codes():
    """Pointers are never read: every refusal comes before any HIP call."""
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    P = buf.ctypes.data + (-buf.ctypes.data % 16)

    def layer(w=P, ch=8, alpha=None, beta=None, scale=P):
        return _lib.DynLayer(w, P, scale, 1, ch, None, alpha, beta, 1)

    def call(x=P, nimg=2, h=8, w=8, cin=8, st=P, slots=1, la=None, lb=None, pool=0, y=P, mid=None):
        return lib.qcn_conv3x3_dyn_pair(x, nimg, h, w, cin, 0, st, slots, 0, C.byref(la or layer()),
                                        C.byref(lb or layer()), pool, 0, y, None, None, mid, None)
    A, U = _lib.QCN_ERR_ARG, _lib.QCN_ERR_UNSUPPORTED
    cases = [("x=null", A, call(x=None)), ("x_stats=null", A, call(st=None)), ("y=null", A, call(y=None)),
             ("A.w=null", A, call(la=layer(w=None))), ("B.w misaligned", A, call(lb=layer(w=P + 4))),
             ("B.w_scale misaligned", A, call(lb=layer(scale=P + 2))), ("mid_qparams misaligned", A, call(mid=P + 1)),
             ("A alpha without beta", A, call(la=layer(alpha=P))), ("B beta without alpha", A, call(lb=layer(beta=P))),
             ("cmid=0", A, call(la=layer(ch=0))), ("nimg=0", A, call(nimg=0)), ("x_slots=0", A, call(slots=0)),
             ("pool odd h", A, call(h=7, pool=1)), ("pool odd w", A, call(w=7, pool=1)),
             ("17 x 8", U, call(h=17)), ("cmid 257 at 8 x 8", U, call(la=layer(ch=257))),
             ("cmid 129 at 16 x 16", U, call(h=16, w=16, la=layer(ch=129))),
             ("cin past the int32 bound", U, call(cin=7311)),
             ("batch past 2^31 elements", U, call(nimg=(1 << 22) + 1))]
    assert [(lbl, got) for lbl, want, got in cases if got != want] == []


def test_pairs_needs_int8_body():
    from models.dynamic_ptq_model import DynamicPTQModel, DynamicQuantConvNet
    from models.static_ptq_model import StaticPTQModel
    for make in (lambda: DynamicQuantConvNet({}, body="hip", pairs=True),
                 lambda: DynamicPTQModel().quantize(body="hip", pairs=True),
                 lambda: StaticPTQModel(mode="reference").quantize(body="torch", pairs=True)):
        with pytest.raises(ValueError, match="pairs"):
            make()
