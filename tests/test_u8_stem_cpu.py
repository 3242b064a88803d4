"""CPU: raw uint8 NHWC images into the ResNet stem kernels.

The stem kernels quantize fp32 input as q = clamp(zp + rint(x * fp32(1 / s)),
0, 255) (resnet_stem.hip phase A, stem_pack_kernel).  On raw images they look
each byte up in quant.quantize_table(normalize_table(mean, std), s, zp)
instead; the first test restates the kernels' fp32 formula in numpy and checks
that the table is that formula applied to the normalised value of every
(channel, byte) — the exact-by-construction argument for the stem tables.  The
rest are the new C entries' argument checks (no device needed) and the surface
of the binding."""
import ctypes as C

import numpy as np
import pytest
import torch

from qconvnet import data
from qconvnet import quant as Q

F32 = np.float32


def _fixture_qparams():
    import resnetfix
    z = resnetfix.load()
    return F32(z["in_scale"]), int(z["in_zp"])


def kernel_quantize(x, scale, zp):
    """The stem kernels' QuantStub, fp32 step by step."""
    inv = F32(F32(1.0) / F32(scale))
    t = (np.asarray(x, F32) * inv).astype(F32)
    t = np.minimum(np.maximum(t, F32(-1.0e9)), F32(1.0e9))
    q = np.rint(t).astype(np.int64) + int(zp)
    return np.clip(q, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("qp", ["fixture", (0.005, 77)])
def test_stem_table_is_the_kernel_formula(qp):
    s, zp = _fixture_qparams() if qp == "fixture" else (F32(qp[0]), qp[1])
    tab = Q.normalize_table(data.IMAGENET_MEAN, data.IMAGENET_STD)
    qlut = Q.quantize_table(tab, s, zp)
    assert qlut.dtype == torch.uint8 and tuple(qlut.shape) == (3, 256)
    want = kernel_quantize(tab.numpy(), s, zp)
    assert np.array_equal(qlut.numpy(), want)
    # and aten's quantize_per_tensor of the same values
    ref = torch.quantize_per_tensor(tab, float(s), zp, torch.quint8).int_repr()
    assert torch.equal(qlut, ref)
    # monotone in the byte, per channel (mean / std only shift and scale)
    assert (np.diff(qlut.numpy().astype(np.int32), axis=1) >= 0).all()
    if qp != "fixture":   # the synthetic pair saturates at both ends
        assert (qlut == 0).any() and (qlut == 255).any()


def test_fused_sizes_keep_stream_slices_aligned():
    """H * W * 3 bytes per image is a multiple of 4 at both fused sizes, so any
    slice of an aligned batch along N stays on a 4-byte boundary."""
    for s in (224, 64):
        assert (s * s * 3) % 4 == 0 and (s * 3) % 4 == 0


# ------------------------------------------------------------------ C entries
@pytest.fixture(scope="module")
def lib():
    from qconvnet import _lib
    return _lib.load()


def _buf(nbytes, offset=0):
    """A host buffer and the address `offset` bytes past a 16-byte boundary
    (the entries must reject the call before touching any pointer)."""
    raw = np.zeros(nbytes + 32, np.uint8)
    base = raw.ctypes.data
    return raw, C.c_void_p((base + 15) // 16 * 16 + offset)


def _stem_args(img, nimg, h, w, qlut, in_zp, p, cout=64, y_zp=0):
    return [img, nimg, h, w, qlut, in_zp, p, cout, p, p, p, p, y_zp, 1, p, None]


def test_stem_fused_u8_argument_checks(lib):
    from qconvnet._lib import QCN_ERR_ARG, QCN_ERR_UNSUPPORTED
    keep, p = _buf(64)
    f = lib.qcn_resnet_stem_fused_u8_nhwc
    assert f(*_stem_args(None, 1, 64, 64, p, 0, p)) == QCN_ERR_ARG
    assert f(*_stem_args(p, 1, 64, 64, None, 0, p)) == QCN_ERR_ARG
    assert f(*_stem_args(p, 1, 64, 64, p, 0, None)) == QCN_ERR_ARG
    for nimg in (0, -3):
        assert f(*_stem_args(p, nimg, 64, 64, p, 0, p)) == QCN_ERR_ARG
    for zp in (-1, 256):
        assert f(*_stem_args(p, 1, 64, 64, p, zp, p)) == QCN_ERR_ARG
        assert f(*_stem_args(p, 1, 64, 64, p, 0, p, y_zp=zp)) == QCN_ERR_ARG
    for h, w in ((64, 32), (224, 64), (32, 32), (96, 96)):
        assert f(*_stem_args(p, 1, h, w, p, 0, p)) == QCN_ERR_UNSUPPORTED
    assert f(*_stem_args(p, 1, 64, 64, p, 0, p, cout=128)) == QCN_ERR_UNSUPPORTED
    # the fp32 entry's 2^31 element guard
    assert f(*_stem_args(p, 14267, 224, 224, p, 0, p)) == QCN_ERR_UNSUPPORTED
    for off in (1, 2, 3):   # the image rows are dword loads
        keep2, q = _buf(64, off)
        assert f(*_stem_args(q, 1, 64, 64, p, 0, p)) == QCN_ERR_ARG
        assert f(*_stem_args(q, 1, 224, 224, p, 0, p)) == QCN_ERR_ARG
    del keep


def test_stem_pack_u8_argument_checks(lib):
    from qconvnet._lib import QCN_ERR_ARG
    keep, p = _buf(64)
    f = lib.qcn_stem_pack_u8_nhwc
    assert f(None, 1, 8, 8, p, 0, p, None) == QCN_ERR_ARG
    assert f(p, 1, 8, 8, None, 0, p, None) == QCN_ERR_ARG
    assert f(p, 1, 8, 8, p, 0, None, None) == QCN_ERR_ARG
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, -2)):
        assert f(p, n, h, w, p, 0, p, None) == QCN_ERR_ARG
    for zp in (-1, 256):
        assert f(p, 1, 8, 8, p, zp, p, None) == QCN_ERR_ARG
    del keep


def test_python_surface():
    from qconvnet import ops
    assert callable(ops.stem_fused_u8) and callable(ops.stem_pack_u8)
    x = torch.zeros((2, 64, 64, 3), dtype=torch.uint8)   # a host tensor is refused, not copied
    with pytest.raises(ValueError, match="device"):
        ops.stem_pack_u8(x, torch.zeros((3, 256), dtype=torch.uint8), 0)
    with pytest.raises(ValueError, match="device"):
        ops.stem_fused_u8(x, torch.zeros((3, 256), dtype=torch.uint8), 0, None)
