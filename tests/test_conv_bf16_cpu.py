"""CPU: what the bf16 3x3 conv (csrc/conv_bf16.hip) decides on the host: the
packed size, the pack layout and its rounding against the formula of
include/qconvnet.h, the statuses of calls it must refuse before any HIP call,
and body="bf16" at the models' entry points."""
import numpy as np
import pytest
import torch

from qconvnet import _lib, ops


def geometry(cin, cout):
    """(channel groups, groups per chunk, steps of a full chunk, steps, column tiles)"""
    ng, G = -(-cin // 8), 8 if cout <= 64 else 16 if cout <= 128 else 32
    F = 9 * G // 4
    return ng, G, F, (ng // G) * F + (9 * (ng % G) + 3) // 4, 4 * -(-cout // 64)


@pytest.mark.parametrize("cin,cout,want", [
    (3, 5, 4 * 3 * 1024), (64, 64, 4 * 18 * 1024), (264, 65, 8 * 75 * 1024), (256, 256, 16 * 72 * 1024),
    (0, 8, _lib.QCN_ERR_ARG), (8, -1, _lib.QCN_ERR_ARG), (1 << 24, 1 << 12, _lib.QCN_ERR_UNSUPPORTED)], ids=str)
def test_packed_size(cin, cout, want):
    assert _lib.load().qcn_conv3x3_bf16_packed_size(cin, cout) == want


@pytest.mark.parametrize("cin,cout", [(3, 5), (64, 64), (264, 65)], ids=str)
def test_pack_layout_and_rounding(cin, cout):
    rng = np.random.default_rng(cin)
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    # every third weight on a tie between two bf16 values (low half 0x8000)
    wb = w.view(np.uint32).reshape(-1)
    wb[::3] = (wb[::3] & 0xffff0000) | 0x8000
    ng, G, F, steps, nct = geometry(cin, cout)
    ct, step, lane, b = np.indices((nct, steps, 64, 8))
    chunk = step // F
    ngc = np.minimum(G, ng - G * chunk)
    u = 4 * (step - F * chunk) + lane // 16
    tap, ci = u // ngc, 8 * G * chunk + 8 * (u % ngc) + b
    co = 32 * (ct // 2) + 2 * (lane % 16) + ct % 2
    ok = (tap < 9) & (ci < cin) & (co < cout)
    bits = torch.from_numpy(w).bfloat16().view(torch.int16).numpy().reshape(cout, cin, 9)
    want = np.where(ok, bits[np.where(ok, co, 0), np.where(ok, ci, 0), np.where(ok, tap, 0)], 0)
    got = ops.pack_conv3x3_bf16(w)
    assert got.dtype == np.int16 and np.array_equal(got, want.ravel())


def test_status_codes():
    """Pointers are never read: every refusal comes before any HIP call."""
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    P = buf.ctypes.data + (-buf.ctypes.data % 16)

    def call(x=P, nimg=2, h=8, w=8, cin=8, xf=0, wp=P, cout=8, alpha=None, beta=None, pool=0, yf=0, y=P):
        return lib.qcn_conv3x3_bf16(x, nimg, h, w, cin, xf, wp, cout, None, alpha, beta, 1, pool, yf, y, None)
    A, U = _lib.QCN_ERR_ARG, _lib.QCN_ERR_UNSUPPORTED
    cases = [("x=null", A, call(x=None)), ("w_packed=null", A, call(wp=None)), ("y=null", A, call(y=None)),
             ("nimg=0", A, call(nimg=0)), ("h=0", A, call(h=0)), ("cin=0", A, call(cin=0)),
             ("cout=-1", A, call(cout=-1)), ("pool odd h", A, call(h=7, pool=1)), ("pool odd w", A, call(w=7, pool=1)),
             ("alpha without beta", A, call(alpha=P)), ("beta without alpha", A, call(beta=P)),
             ("w_packed misaligned", A, call(wp=P + 8)), ("x_fmt=3", A, call(xf=3)), ("x_fmt=-1", A, call(xf=-1)),
             ("y_fmt=3", A, call(yf=3)), ("fp32 x misaligned", A, call(x=P + 2)),
             ("fp32 y misaligned", A, call(y=P + 2, yf=1)), ("bf16 x, cin 8, at 8 bytes", A, call(x=P + 8, xf=2)),
             ("bf16 x, cin 3, at 1 byte", A, call(x=P + 1, xf=2, cin=3)),
             ("bf16 y, cout 8, at 2 bytes", A, call(y=P + 2, yf=2)),
             ("bf16 y, cout 5, at 1 byte", A, call(y=P + 1, yf=2, cout=5)),
             ("packed size past 2^31", U, call(cin=1 << 24, cout=1 << 12)),
             ("x past 2^31 elements", U, call(nimg=(1 << 15) + 1, h=32, w=32, cin=64)),
             ("y past 2^31 elements", U, call(nimg=(1 << 15) + 1, h=32, w=32, cout=64, yf=2))]
    assert [(lbl, got) for lbl, want, got in cases if got != want] == []


def test_body_bf16_at_the_entry_points():
    from models.dynamic_ptq_model import BODIES, DynamicPTQModel, DynamicQuantConvNet
    from models.static_ptq_model import StaticPTQModel
    assert "bf16" in BODIES
    for make in (lambda: DynamicQuantConvNet({}, body="bf16", pairs=True),
                 lambda: DynamicPTQModel().quantize(body="bf16", pairs=True),
                 lambda: StaticPTQModel(mode="reference").quantize(body="bf16", pairs=True)):
        with pytest.raises(ValueError, match="pairs"):
            make()
    with pytest.raises(ValueError, match="reference"):
        StaticPTQModel(mode="static").quantize(None, body="bf16")
