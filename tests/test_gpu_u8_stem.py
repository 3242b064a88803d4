"""GPU: raw uint8 NHWC images straight into the ResNet stem kernels.

The method is that of tests/test_gpu_u8_input.py: every comparison is exact
equality against the fp32 entry fed with the table-expanded input
(qconvnet.quant.expand_u8 on the CPU, pinned to ToTensor + Normalize by
tests/test_u8_input_cpu.py).  The fp32 stem path is pinned to the torch.ao
fixtures by tests/test_gpu_resnet.py, so it is the oracle here.  Inputs are
PCG64 u8 images holding all 256 codes in every channel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SYNTHETIC_QP = (0.005, 77)   # saturates the table at both 0 and 255


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def u8_images(n, h, w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if h * w >= 256:
        x[0].reshape(-1, 3)[:256] = np.arange(256, dtype=np.uint8)[:, None]
    return torch.from_numpy(x)


def ntab():
    import resnetfix
    from qconvnet import quant as Q
    return Q.normalize_table(**resnetfix.IMAGENET)


_CACHE = {}


def image_pair(n, h, w, dev):
    """(u8 NHWC images, their fp32 NCHW expansion), both on the device;
    computed once per shape and never written to."""
    from qconvnet import quant as Q
    key = (n, h, w)
    if key not in _CACHE:
        x = u8_images(n, h, w, 1000 * h + w + n)
        _CACHE[key] = (x.to(dev), Q.expand_u8(x, ntab()).to(dev))
    return _CACHE[key]


def offset_view(x, offset):
    """The same bytes at data_ptr() % 4 == offset."""
    flat = torch.zeros(x.numel() + 8, dtype=torch.uint8, device=x.device)
    flat[offset:offset + x.numel()] = x.reshape(-1)
    xo = flat[offset:offset + x.numel()].view(x.shape)
    assert xo.data_ptr() % 4 == offset
    return xo


@pytest.fixture(scope="module")
def nets(dev):
    """The fixture nets (hw 64, batch 8): the static executor and the
    live-stub (QDQ) one."""
    import resnetfix
    from qconvnet.resnet import QuantizedResNet
    from qconvnet.resnet_qdq import QuantizedResNetQDQ
    z = resnetfix.load()
    zq = resnetfix.load_qdq()
    assert int(z["hw"]) == 64 and int(z["batch"]) == 8
    return {"static": QuantizedResNet(resnetfix.spec(z), dev),
            "qdq": QuantizedResNetQDQ(resnetfix.qdq_spec(zq, fixture_qparams=True), dev)}


def in_qparams(m):
    return (m.in_scale, m.in_zp) if hasattr(m, "in_scale") else (m.stem.s_x, m.stem.z_x)


def qparams_and_table(m, qp):
    from qconvnet import quant as Q
    s, zp = in_qparams(m) if qp == "fixture" else (np.float32(qp[0]), qp[1])
    qlut = Q.quantize_table(ntab(), s, zp)
    if qp != "fixture":
        assert (qlut == 0).any() and (qlut == 255).any()
    return s, zp, qlut


# ------------------------------------------------------------ stem_fused_u8
# S = 64: 8 bands per image, so ncu/8 + 1 images are ncu + 8 bands on ncu
# workgroups: some run two bands, some runs cross an image boundary.
# S = 224: 14 bands per image, ceil((ncu + 1) / 14) images for the same reason.
@pytest.mark.parametrize("qp", ["fixture", SYNTHETIC_QP])
@pytest.mark.parametrize("s,nimg", [(64, 1), (64, 3), (64, "ncu/8+1"), (224, 1), (224, "(ncu+1)/14")])
def test_stem_fused_u8(dev, ncu, nets, s, nimg, qp):
    from qconvnet import ops
    m = nets["static"]
    n = {"ncu/8+1": ncu // 8 + 1, "(ncu+1)/14": -(-(ncu + 1) // 14)}.get(nimg, nimg)
    x, xf = image_pair(n, s, s, dev)
    scale, zp, qlut = qparams_and_table(m, qp)
    want = ops.stem_fused(xf, scale, zp, m.stem)
    got = ops.stem_fused_u8(x, qlut.to(dev), zp, m.stem)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, s // 4, s // 4, 64)
    assert torch.equal(got, want)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_stem_fused_u8_moves_a_misaligned_batch(dev, nets, offset):
    from qconvnet import ops
    m = nets["static"]
    x, xf = image_pair(3, 64, 64, dev)
    got = ops.stem_fused_u8(offset_view(x, offset), m.qlut, m.in_zp, m.stem)
    assert torch.equal(got, ops.stem_fused(xf, m.in_scale, m.in_zp, m.stem))


# ------------------------------------------------------------- stem_pack_u8
@pytest.mark.parametrize("qp", ["fixture", SYNTHETIC_QP])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 7, 5), (1, 64, 64), (1, 9, 257)])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_stem_pack_u8(dev, nets, n, h, w, offset, qp):
    from qconvnet import ops
    x, xf = image_pair(n, h, w, dev)
    scale, zp, qlut = qparams_and_table(nets["static"], qp)
    want = ops.stem_pack(xf, scale, zp)
    got = ops.stem_pack_u8(offset_view(x, offset), qlut.to(dev), zp)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, h, (w - 1) // 2 + 1, 32)
    assert torch.equal(got, want)


# ------------------------------------------------- the C entries' arguments
def _stem_rc(lib, m, img_ptr, n, h, w, qlut_ptr, cout, y):
    d = m.stem
    return lib.qcn_resnet_stem_fused_u8_nhwc(img_ptr, n, h, w, qlut_ptr, m.in_zp, d.w.data_ptr(), cout,
                                             d.u.data_ptr(), d.v.data_ptr(), d.mult.data_ptr(),
                                             d.corr.data_ptr(), d.z_y, 1, y.data_ptr(), None)


def test_stem_fused_u8_argument_errors(dev, nets):
    from qconvnet import _lib
    lib = _lib.load()
    m = nets["static"]
    x, _ = image_pair(3, 64, 64, dev)
    y = torch.empty((3, 16, 16, 64), dtype=torch.uint8, device=dev)
    q = m.qlut.data_ptr()
    for offset in (1, 2, 3):   # the image rows are dword loads
        assert _stem_rc(lib, m, offset_view(x, offset).data_ptr(), 3, 64, 64, q, 64, y) == _lib.QCN_ERR_ARG
    assert _stem_rc(lib, m, x.data_ptr(), 3, 64, 32, q, 64, y) == _lib.QCN_ERR_UNSUPPORTED
    assert _stem_rc(lib, m, x.data_ptr(), 3, 32, 32, q, 64, y) == _lib.QCN_ERR_UNSUPPORTED
    assert _stem_rc(lib, m, x.data_ptr(), 3, 64, 64, q, 128, y) == _lib.QCN_ERR_UNSUPPORTED
    assert _stem_rc(lib, m, x.data_ptr(), 3, 64, 64, None, 64, y) == _lib.QCN_ERR_ARG
    assert _stem_rc(lib, m, None, 3, 64, 64, q, 64, y) == _lib.QCN_ERR_ARG
    # the zero points are bytes
    d = m.stem
    rc = lib.qcn_resnet_stem_fused_u8_nhwc(x.data_ptr(), 3, 64, 64, q, 256, d.w.data_ptr(), 64,
                                           d.u.data_ptr(), d.v.data_ptr(), d.mult.data_ptr(),
                                           d.corr.data_ptr(), d.z_y, 1, y.data_ptr(), None)
    assert rc == _lib.QCN_ERR_ARG
    rows = torch.empty((3, 64, 32, 32), dtype=torch.uint8, device=dev)
    assert lib.qcn_stem_pack_u8_nhwc(x.data_ptr(), 3, 64, 64, None, 0, rows.data_ptr(), None) == _lib.QCN_ERR_ARG
    assert lib.qcn_stem_pack_u8_nhwc(x.data_ptr(), 3, 64, 64, q, 256, rows.data_ptr(), None) == _lib.QCN_ERR_ARG
    assert lib.qcn_stem_pack_u8_nhwc(x.data_ptr(), 0, 64, 64, q, 0, rows.data_ptr(), None) == _lib.QCN_ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------- the executors
@pytest.fixture()
def no_normalize(monkeypatch):
    """ops.normalize_u8 raises: nothing on the path under test may expand the
    images to fp32."""
    from qconvnet import ops

    def boom(*a, **k):
        raise AssertionError("normalize_u8 called on the int8 inference path")
    monkeypatch.setattr(ops, "normalize_u8", boom)


@pytest.mark.parametrize("kind", ["static", "qdq"])
def test_executor_u8_skips_normalize(dev, nets, kind, no_normalize):
    m = nets[kind]
    x, xf = image_pair(8, 64, 64, dev)
    want = m.run(xf).clone()
    got = m.run(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # the model call on a host batch
    host = m(x.cpu())
    assert not host.is_cuda and torch.equal(host, want.cpu())
    assert torch.equal(m(x), want)
    if hasattr(m, "run_streams"):
        got = m.run_streams(x, 2).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    # every kept activation
    _, wi = m.run(xf, keep=True)
    wi = {k: v.clone() for k, v in wi.items()}
    _, gi = m.run(x, keep=True)
    torch.cuda.synchronize()
    assert sorted(gi) == sorted(wi)
    for k, v in wi.items():
        assert torch.equal(gi[k], v), k


@pytest.mark.parametrize("kind", ["static", "qdq"])
def test_executor_u8_layouts(dev, nets, kind, no_normalize):
    m = nets[kind]
    x, xf = image_pair(8, 64, 64, dev)
    want = m.run(xf).clone()
    # a u8 batch that is not NHWC raises instead of being cast to float
    with pytest.raises(ValueError, match="NHWC"):
        m(x.cpu().permute(0, 3, 1, 2))
    with pytest.raises(ValueError, match="NHWC"):
        m.run(x.permute(0, 3, 1, 2).contiguous())
    # a non-contiguous NHWC view (stored NCHW) is made contiguous first
    nchw = x.permute(0, 3, 1, 2).contiguous()
    assert torch.equal(m.run(nchw.permute(0, 2, 3, 1)).clone(), want)


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("kind", ["static", "qdq"])
def test_executor_misaligned_u8(dev, nets, kind, offset, no_normalize):
    m = nets[kind]
    x, xf = image_pair(8, 64, 64, dev)
    want = m.run(xf).clone()
    xo = offset_view(x, offset)
    assert torch.equal(m.run(xo).clone(), want)
    assert torch.equal(m(xo), want)
    if hasattr(m, "run_streams"):
        assert torch.equal(m.run_streams(xo, 2).clone(), want)


def test_executor_graph_replay_u8(dev, nets, no_normalize):
    m = nets["static"]
    x, xf = image_pair(8, 64, 64, dev)
    x2, xf2 = image_pair(9, 64, 64, dev)
    want, want2 = m.run(xf).clone(), m.run(xf2[:8].contiguous()).clone()
    static = x.clone()
    m.capture_graph(static)
    out = m.replay(8).clone()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # new bytes in the static input, the same graph
    static.copy_(x2[:8])
    out = m.replay(8).clone()
    torch.cuda.synchronize()
    assert torch.equal(out, want2)


@pytest.mark.parametrize("kind", ["static", "qdq"])
def test_executor_unfused_size_u8(dev, nets, kind, no_normalize):
    """96 x 96 is outside the fused stem's sizes: the row pack reads the bytes
    (launch names as for fp32 input)."""
    m = nets[kind]
    x, xf = image_pair(2, 96, 96, dev)
    if kind == "static":
        assert not m._stem_fusable(x) and not m._stem_fusable(xf)
        mu, mf = [], []
        want = m.run(xf, marks=mf).clone()
        got = m.run(x, marks=mu).clone()
        assert [n for n, _ in mu] == [n for n, _ in mf] and mu[1][0] == "stem_pack"
    else:
        want, got = m.run(xf).clone(), m.run(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(m(offset_view(x, 1)), want)


def test_fused_launch_names_u8(dev, nets):
    m = nets["static"]
    x, xf = image_pair(8, 64, 64, dev)
    mu, mf = [], []
    m.run(xf, marks=mf)
    m.run(x, marks=mu)
    torch.cuda.synchronize()
    assert [n for n, _ in mu] == [n for n, _ in mf] and mu[1][0] == "conv"
