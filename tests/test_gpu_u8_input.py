"""GPU: raw uint8 NHWC image input.

Every comparison is exact equality against the existing fp32 path fed with
the table-expanded input (qconvnet.quant.expand_u8 on the CPU — pinned to
ToTensor + Normalize by tests/test_u8_input_cpu.py).  The fp32 path is pinned
to the golden vectors elsewhere, so it is the oracle here.  Inputs are PCG64
u8 images holding all 256 codes in every channel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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


_CACHE = {}


def cifar_pair(n, dev):
    """(u8 NHWC images, their fp32 NCHW expansion), both on the device;
    computed once per batch size and never written to."""
    from qconvnet import data, quant as Q
    if n not in _CACHE:
        x = u8_images(n, 32, 32, 100 + n)
        xf = Q.expand_u8(x, Q.normalize_table(data.CIFAR_MEAN, data.CIFAR_STD))
        _CACHE[n] = (x.to(dev), xf.to(dev))
    return _CACHE[n]


@pytest.fixture(scope="module")
def models(dev):
    """The fixture's static (fast epilogue, EM 1) and per-layer QDQ (one-fma
    hand-off, EM 2) nets."""
    import netfix
    from qconvnet.qmodel import QuantizedConvNet
    z = netfix.load()
    return {"static": QuantizedConvNet(netfix.static_spec(z)[0], dev),
            "qdq": QuantizedConvNet(netfix.qdq_spec(z), dev)}


# ------------------------------------------------------------- normalize_u8
# (1,4,257): 257 quads, one 256-thread workgroup's worth plus one; (1,1,257)
# the same for the one-pixel-per-lane form (h*w not a multiple of 4)
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (3, 7, 5), (2, 32, 32), (1, 224, 224), (1, 4, 257), (1, 1, 257)])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_normalize_u8(dev, n, h, w, offset):
    from qconvnet import data, ops, quant as Q
    consts = (data.IMAGENET_MEAN, data.IMAGENET_STD) if h == 224 else (data.CIFAR_MEAN, data.CIFAR_STD)
    ntab = Q.normalize_table(*consts)
    x = u8_images(n, h, w, 5)
    want = Q.expand_u8(x, ntab)
    flat = torch.zeros(x.numel() + 8, dtype=torch.uint8, device=dev)
    flat[offset:offset + x.numel()] = x.reshape(-1).to(dev)
    xd = flat[offset:offset + x.numel()].view(n, h, w, 3)
    assert xd.data_ptr() % 4 == offset
    got = ops.normalize_u8(xd, ntab.to(dev))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3, h, w)
    assert np.array_equal(got.cpu().numpy(), want.numpy())


def test_normalize_u8_into_unaligned_output(dev):
    """An output that is only 4-byte aligned takes the one-pixel-per-lane
    form; the elements around it stay untouched."""
    from qconvnet import data, ops, quant as Q
    ntab = Q.normalize_table(data.CIFAR_MEAN, data.CIFAR_STD)
    x = u8_images(2, 32, 32, 6)
    buf = torch.full((x.numel() + 2,), -7.0, dtype=torch.float32, device=dev)
    out = buf[1:1 + x.numel()].view(2, 3, 32, 32)
    ops.normalize_u8(x.to(dev), ntab.to(dev), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), Q.expand_u8(x, ntab).numpy())
    assert buf[0].item() == -7.0 and buf[-1].item() == -7.0


# ---------------------------------------------------------- conv12_fused_u8
@pytest.mark.parametrize("qp", ["fixture", (0.005, 77)])
@pytest.mark.parametrize("nimg", [1, 3, "ncu+1"])
def test_conv12_fused_u8(dev, ncu, models, nimg, qp):
    from qconvnet import ops, quant as Q
    m = models["static"]
    n = ncu + 1 if nimg == "ncu+1" else nimg
    x, xf = cifar_pair(n, dev)
    s, zp = (m.in_scale, m.in_zp) if qp == "fixture" else (np.float32(qp[0]), qp[1])
    qlut = Q.quantize_table(m.ntab.cpu(), s, zp)
    if qp != "fixture":   # the synthetic pair saturates at both ends
        assert (qlut == 0).any() and (qlut == 255).any()
    want = ops.conv12_fused(xf, s, zp, m.L[0], m.L[1])
    got = ops.conv12_fused_u8(x, qlut.to(dev), zp, m.L[0], m.L[1])
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# --------------------------------------------------------- convnet_convs_u8
def _convs(m, x, u8, kmajor, dev):
    from qconvnet import ops
    n = x.shape[0]
    layers = ops.conv_layers(m.L, m.in_zp)
    a2 = torch.zeros((n, 16, 16, 64), dtype=torch.uint8, device=dev)
    a4 = torch.zeros((n, 8, 8, 128), dtype=torch.uint8, device=dev)
    a6 = torch.zeros(n * 4096, dtype=torch.uint8, device=dev)
    if u8:
        ok = ops.convnet_convs_u8(x, m.qlut, m.in_zp, layers, a2, a4, a6, kmajor=kmajor)
    else:
        ok = ops.convnet_convs(x, m.in_scale, m.in_zp, layers, a2, a4, a6, kmajor=kmajor)
    torch.cuda.synchronize()
    return ok, (a2, a4, a6)


@pytest.mark.parametrize("kmajor", [True, False])
@pytest.mark.parametrize("mode", ["static", "qdq"])
@pytest.mark.parametrize("nimg", [1, 5, "4ncu", "4ncu+3"])
def test_convnet_convs_u8(dev, ncu, models, nimg, mode, kmajor):
    from qconvnet import ops
    m = models[mode]
    n = {"4ncu": 4 * ncu, "4ncu+3": 4 * ncu + 3}.get(nimg, nimg)
    form = ops.convnet_convs_form(n, m.in_scale, m.in_zp, ops.conv_layers(m.L, m.in_zp), kmajor)
    assert form == (1 if n <= ncu else 2)
    x, xf = cifar_pair(n, dev)
    ok_f, want = _convs(m, xf, False, kmajor, dev)
    ok_u, got = _convs(m, x, True, kmajor, dev)
    assert ok_f and ok_u
    for name, g, w in zip(("a2", "a4", "a6"), got, want):
        assert torch.equal(g, w), name


@pytest.mark.parametrize("mode", ["static", "qdq"])
def test_convnet_convs_band_is_unsupported_for_both_inputs(dev, ncu, models, mode):
    m = models[mode]
    x, xf = cifar_pair(ncu + 1, dev)
    assert _convs(m, xf, False, True, dev)[0] is False
    assert _convs(m, x, True, True, dev)[0] is False


# --------------------------------------------------------- QuantizedConvNet
@pytest.mark.parametrize("mode", ["static", "qdq"])
@pytest.mark.parametrize("nimg", [64, "ncu+1", "4ncu"])
def test_model_run_u8_equals_expanded(dev, ncu, models, mode, nimg):
    m = models[mode]
    n = {"ncu+1": ncu + 1, "4ncu": 4 * ncu}.get(nimg, nimg)
    x, xf = cifar_pair(n, dev)
    assert m.kernel_names(x.shape) == m.kernel_names(xf.shape)
    want = m.run(xf).clone()
    got = m.run(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # every kept activation (conv12 on the bytes, then per layer)
    w_logits, wb = m.run(xf, keep=True)
    want_acts = {k: wb[k].clone() for k in ("a2", "a3", "a4", "a5", "a6", "f1")}
    w_logits = w_logits.clone()
    g_logits, gb = m.run(x, keep=True)
    torch.cuda.synchronize()
    for k, w in want_acts.items():
        assert torch.equal(gb[k], w), k
    assert torch.equal(g_logits, w_logits)


def test_model_forward_host_u8(dev, models):
    m = models["static"]
    x, xf = cifar_pair(64, dev)
    want = m(xf.cpu())
    got = m(x.cpu())
    assert not got.is_cuda and torch.equal(got, want)
    # a u8 batch that is not NHWC raises instead of being cast to float
    with pytest.raises(ValueError, match="NHWC"):
        m(x.cpu().permute(0, 3, 1, 2))
    with pytest.raises(ValueError, match="NHWC"):
        m.run(x.permute(0, 3, 1, 2).contiguous())
    # a non-contiguous NHWC view (stored NCHW) is made contiguous first
    nchw = x.permute(0, 3, 1, 2).contiguous()
    assert torch.equal(m.run(nchw.permute(0, 2, 3, 1)).clone(), want.to(dev))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_model_run_misaligned_u8(dev, models, offset):
    """The conv entries want a 4-byte aligned image pointer (and say so with
    QCN_ERR_ARG); the Python layer moves a misaligned batch first."""
    from qconvnet import _lib, ops
    m = models["static"]
    x, xf = cifar_pair(64, dev)
    flat = torch.zeros(x.numel() + 8, dtype=torch.uint8, device=dev)
    flat[offset:offset + x.numel()] = x.reshape(-1)
    xo = flat[offset:offset + x.numel()].view(x.shape)
    assert xo.data_ptr() % 4 == offset
    a2 = torch.empty((64, 16, 16, 64), dtype=torch.uint8, device=dev)
    def ptrs(d):
        return [t.data_ptr() for t in (d.w, d.u, d.v, d.mult, d.corr)]

    rc = _lib.load().qcn_conv12_fused_u8_nhwc(
        xo.data_ptr(), 64, m.qlut.data_ptr(), m.in_zp, *ptrs(m.L[0]), m.L[0].z_y, 1, None,
        m.L[1].z_x, *ptrs(m.L[1]), m.L[1].z_y, 1, None, a2.data_ptr(), None)
    assert rc == _lib.QCN_ERR_ARG
    want = m.run(xf).clone()
    assert torch.equal(m.run(xo).clone(), want)
    assert torch.equal(ops.conv12_fused_u8(xo, m.qlut, m.in_zp, m.L[0], m.L[1]),
                       ops.conv12_fused(xf, m.in_scale, m.in_zp, m.L[0], m.L[1]))


@pytest.mark.parametrize("nimg", [64, "4ncu"])
def test_model_graph_replay_u8(dev, ncu, models, nimg):
    m = models["static"]
    n = 4 * ncu if nimg == "4ncu" else nimg
    x, xf = cifar_pair(n, dev)
    want = m.run(xf).clone()
    static = x.clone()
    m.capture_graph(static)
    out = m.replay(n)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # new bytes in the static input, the same graph
    x2, xf2 = cifar_pair(n + 1, dev)
    static.copy_(x2[:n])
    out = m.replay(n).clone()
    torch.cuda.synchronize()
    assert torch.equal(out, m.run(xf2[:n].contiguous()))


@pytest.mark.parametrize("mode", ["static", "qdq"])
def test_model_fallbacks_u8(dev, ncu, mode):
    """fuse_convs=False (conv12 on the bytes + the pair launches) and
    fuse12=False (normalize_u8 + the stand-alone conv1, per layer)."""
    import netfix
    from qconvnet.qmodel import QuantizedConvNet
    z = netfix.load()
    spec = netfix.static_spec(z)[0] if mode == "static" else netfix.qdq_spec(z)
    x, xf = cifar_pair(64, dev)
    three = QuantizedConvNet(spec, dev)
    three.fuse_convs = False
    assert three.kernel_names(x.shape)[0] == "conv12"
    assert torch.equal(three.run(x).clone(), three.run(xf).clone())
    layered = QuantizedConvNet(spec, dev, fuse12=False)
    assert layered.kernel_names(x.shape)[0] == "conv1"
    want, wb = layered.run(xf, keep=True)
    want, a1 = want.clone(), wb["a1"].clone()
    got, gb = layered.run(x, keep=True)
    torch.cuda.synchronize()
    assert torch.equal(gb["a1"], a1)
    assert torch.equal(got, want)


def test_model_run_pipelined_u8(dev, models):
    m = models["static"]
    pairs = [cifar_pair(n, dev) for n in (64, 65)]
    want = [m.run(xf[:64].contiguous()).clone() for _, xf in pairs]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    got = [o.clone() for o in m.run_pipelined([x[:64].contiguous() for x, _ in pairs], streams)]
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_gpu_calibration_on_u8(dev):
    """device="cuda" calibration normalises through normalize_u8: the input
    observer's range is that of the table-expanded batch exactly (the later
    observers sit behind MIOpen's fp32 convs, the same for both inputs)."""
    import netfix
    from qconvnet import qmodel
    folded = qmodel.fold_state_dict(netfix.state_dict(netfix.load()))
    x, xf = cifar_pair(64, dev)
    r_u8 = qmodel.calibrate(folded, [x.cpu()], dev, mode="static")
    r_f32 = qmodel.calibrate(folded, [xf.cpu()], dev, mode="static")
    assert r_u8["x"] == r_f32["x"] == (xf.min().item(), xf.max().item())
    assert sorted(r_u8) == sorted(r_f32)


# ------------------------------------------------------------ models.* surface
def test_static_ptq_wrapper_on_u8(dev):
    """StaticPTQModel.quantize on a raw u8 calibration set builds the model
    the fp32-fed quantize builds (same spec), and the model takes u8 batches."""
    import netfix
    from models.static_ptq_model import StaticPTQModel
    x, xf = cifar_pair(64, dev)
    built = []
    for calib in (x.cpu(), xf.cpu()):
        ptq = StaticPTQModel(device=dev)
        ptq.load_state_dict(netfix.state_dict(netfix.load()))
        built.append(ptq.quantize(calib))
    a, b = (m.spec for m in built)
    assert a["in"] == b["in"]
    for name in [f"conv{i}" for i in range(1, 7)] + ["fc1", "fc2"]:
        assert (a[name]["s_y"], a[name]["z_y"]) == (b[name]["s_y"], b[name]["z_y"]), name
    assert torch.equal(built[0](x), built[1](xf))


def test_dynamic_model_on_u8(dev):
    """The fp32-conv + dynamic-int8 model normalises u8 input through
    normalize_u8: the same logits as for the expanded batch."""
    import netfix
    from models.dynamic_ptq_model import DynamicPTQModel
    x, xf = cifar_pair(64, dev)
    m = DynamicPTQModel(device=dev)
    m.load_state_dict(netfix.state_dict(netfix.load()))
    q = m.quantize()
    assert torch.equal(q(x), q(xf))
    with pytest.raises(ValueError, match="NHWC"):
        q(x.permute(0, 3, 1, 2))


# ----------------------------------------------------------- QuantizedResNet
def test_resnet_u8_equals_expanded(dev):
    import resnetfix
    from qconvnet import quant as Q
    from qconvnet.resnet import QuantizedResNet
    z = resnetfix.load()
    qm = QuantizedResNet(resnetfix.spec(z), dev)
    hw = int(z["hw"])
    x = u8_images(int(z["batch"]), hw, hw, 9)
    xf = Q.expand_u8(x, Q.normalize_table(**resnetfix.IMAGENET))
    want = qm.run(xf.to(dev)).clone()
    got = qm.run(x.to(dev)).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(qm(x), qm(xf))
    with pytest.raises(ValueError, match="NHWC"):
        qm(x.permute(0, 3, 1, 2))
