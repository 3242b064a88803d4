"""CPU: raw uint8 NHWC image input.

ToTensor -> Normalize -> QuantStub of a u8 image is a function of (channel,
byte).  The product replaces the per-pixel arithmetic by two 3 x 256 tables
(qconvnet.quant.normalize_table / quantize_table); these tests pin both tables
to torch's own ops bit for bit, the calibration on u8 batches to the fp32-fed
one, the new C entries' argument checks (no device needed) and the input
validation."""
import ctypes as C

import numpy as np
import pytest
import torch

from qconvnet import data
from qconvnet import quant as Q

CIFAR = (data.CIFAR_MEAN, data.CIFAR_STD)
IMAGENET = (data.IMAGENET_MEAN, data.IMAGENET_STD)


def u8_images(n, hw, seed):
    """PCG64 u8 NHWC images holding all 256 codes in every channel."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)
    if hw * hw >= 256:
        x[0].reshape(-1, 3)[:256] = np.arange(256, dtype=np.uint8)[:, None]
    return torch.from_numpy(x)


def restated(x, mean, std):
    """ToTensor + Normalize of u8 NHWC, restated: fp32 NCHW."""
    m = torch.tensor(mean, dtype=torch.float32).reshape(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).reshape(1, 3, 1, 1)
    return x.permute(0, 3, 1, 2).float().div(255).sub(m).div(s).contiguous()


@pytest.mark.parametrize("consts,hw", [(CIFAR, 32), (IMAGENET, 224)])
def test_table_expansion_equals_totensor_normalize(consts, hw):
    x = u8_images(2, hw, 7)
    for c in range(3):
        assert len(np.unique(x[..., c].numpy())) == 256
    tab = Q.normalize_table(*consts)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (3, 256)
    got = Q.expand_u8(x, tab)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, hw, hw)
    assert np.array_equal(got.numpy(), restated(x, *consts).numpy())


def _fixture_qparams():
    import netfix
    z = netfix.load()
    return float(np.float32(z["qm_in_scale"])), int(z["qm_in_zp"])


QPARAMS = [(0.0203, 120), (0.02, 0), (0.01, 255), (0.005, 77), "fixture"]


@pytest.mark.parametrize("consts", [CIFAR, IMAGENET])
@pytest.mark.parametrize("qp", QPARAMS)
def test_quantized_lookup_equals_quantize_per_tensor(consts, qp):
    s, zp = _fixture_qparams() if qp == "fixture" else qp
    x = u8_images(2, 32, 11)
    tab = Q.normalize_table(*consts)
    qlut = Q.quantize_table(tab, s, zp)
    assert qlut.dtype == torch.uint8 and tuple(qlut.shape) == (3, 256)
    idx = x.permute(0, 3, 1, 2).long()
    got = torch.stack([qlut[c][idx[:, c]] for c in range(3)], dim=1)
    want = torch.quantize_per_tensor(restated(x, *consts), float(np.float32(s)), zp, torch.quint8).int_repr()
    assert torch.equal(got, want)
    if qp in ((0.02, 0), (0.005, 77)):      # saturates at 0
        assert (qlut == 0).any()
    if qp in ((0.01, 255), (0.005, 77)):    # saturates at 255
        assert (qlut == 255).any()


@pytest.mark.parametrize("observer,mode", [("minmax", None), ("minmax", "static"), ("histogram", "static"),
                                           ("histogram", "qdq")])
def test_calibration_on_u8_equals_fp32_expansion(observer, mode):
    import netfix
    from qconvnet import qmodel
    z = netfix.load()
    folded = qmodel.fold_state_dict(netfix.state_dict(z))
    xs = [u8_images(8, 32, 21), u8_images(5, 32, 22)]
    tab = Q.normalize_table(*CIFAR)
    r_u8 = qmodel.calibrate(folded, xs, "cpu", observer=observer, mode=mode)
    r_f32 = qmodel.calibrate(folded, [Q.expand_u8(x, tab) for x in xs], "cpu", observer=observer, mode=mode)
    assert sorted(r_u8) == sorted(r_f32) and len(r_u8) >= 8
    for k in r_f32:
        a, b = np.asarray(r_u8[k], np.float32), np.asarray(r_f32[k], np.float32)
        assert a.tobytes() == b.tobytes(), k


def test_calibration_batches_pass_u8_through():
    x = u8_images(4, 32, 3)
    assert data.calibration_batches(x)[0] is x
    out = data.calibration_batches([(x, torch.zeros(4)), (x, torch.zeros(4))], max_batches=1)
    assert len(out) == 1 and out[0].dtype == torch.uint8


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


def _conv12_args(img, nimg, qlut, in_zp, p):
    return [img, nimg, qlut, in_zp, p, p, p, p, p, 0, 1, None, 0, p, p, p, p, p, 0, 1, None, p, None]


def test_conv12_u8_argument_checks(lib):
    from qconvnet._lib import QCN_ERR_ARG
    keep, p = _buf(64)
    f = lib.qcn_conv12_fused_u8_nhwc
    assert f(*_conv12_args(None, 1, p, 0, p)) == QCN_ERR_ARG
    assert f(*_conv12_args(p, 1, None, 0, p)) == QCN_ERR_ARG
    assert f(*_conv12_args(p, 1, p, 0, None)) == QCN_ERR_ARG
    for nimg in (0, -3):
        assert f(*_conv12_args(p, nimg, p, 0, p)) == QCN_ERR_ARG
    for zp in (-1, 256):
        assert f(*_conv12_args(p, 1, p, zp, p)) == QCN_ERR_ARG
    for off in (1, 2, 3):
        keep2, q = _buf(64, off)
        assert f(*_conv12_args(q, 1, p, 0, p)) == QCN_ERR_ARG
    del keep


def test_convnet_convs_u8_argument_checks(lib):
    from qconvnet import _lib
    from qconvnet._lib import QCN_ERR_ARG
    keep, p = _buf(64)
    layers = (_lib.ConvLayer * 6)()
    for i in range(6):
        layers[i] = _lib.ConvLayer(p, p, p, p, p, 0, 0, 1, None)
    f = lib.qcn_convnet_convs_u8_nhwc
    assert f(None, 1, p, 0, layers, p, p, p, 1, None) == QCN_ERR_ARG
    assert f(p, 1, None, 0, layers, p, p, p, 1, None) == QCN_ERR_ARG
    assert f(p, 1, p, 0, None, p, p, p, 1, None) == QCN_ERR_ARG
    assert f(p, 1, p, 0, layers, None, p, p, 1, None) == QCN_ERR_ARG
    for nimg in (0, -1):
        assert f(p, nimg, p, 0, layers, p, p, p, 1, None) == QCN_ERR_ARG
    for zp in (-1, 256):
        assert f(p, 1, p, zp, layers, p, p, p, 1, None) == QCN_ERR_ARG
    assert f(p, 1, p, 7, layers, p, p, p, 1, None) == QCN_ERR_ARG   # in_zp != layers[0].x_zp
    for off in (1, 2, 3):
        keep2, q = _buf(64, off)
        assert f(q, 1, p, 0, layers, p, p, p, 1, None) == QCN_ERR_ARG
    del keep


def test_normalize_argument_checks(lib):
    from qconvnet._lib import QCN_ERR_ARG
    keep, p = _buf(64)
    f = lib.qcn_u8img_normalize_f32_nchw
    assert f(None, 1, 1, 1, p, p, None) == QCN_ERR_ARG
    assert f(p, 1, 1, 1, None, p, None) == QCN_ERR_ARG
    assert f(p, 1, 1, 1, p, None, None) == QCN_ERR_ARG
    for n, h, w in ((0, 1, 1), (1, 0, 1), (1, 1, -2)):
        assert f(p, n, h, w, p, p, None) == QCN_ERR_ARG
    del keep


# ------------------------------------------------------------ input validation
@pytest.mark.parametrize("shape", [(4, 3, 32, 32), (4, 32, 32), (4, 32, 32, 4), (4, 16, 16, 3)])
def test_wrong_shaped_u8_raises(shape):
    x = torch.zeros(shape, dtype=torch.uint8)
    with pytest.raises(ValueError, match="NHWC"):
        Q.check_u8_images(x, 32)


def test_u8_nchw_is_rejected_by_the_host_paths():
    """No path casts raw bytes to float: calibration and the host expansion
    reject an NCHW u8 batch instead of reading it as values in 0..255."""
    import netfix
    from qconvnet import qmodel
    x = torch.zeros((2, 3, 32, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match="NHWC"):
        Q.expand_u8(x, Q.normalize_table(*CIFAR))
    folded = qmodel.fold_state_dict(netfix.state_dict(netfix.load()))
    with pytest.raises(ValueError, match="NHWC"):
        qmodel.calibrate(folded, [x], "cpu")
    Q.check_u8_images(torch.zeros((2, 32, 32, 3), dtype=torch.uint8), 32)   # the accepted layout
