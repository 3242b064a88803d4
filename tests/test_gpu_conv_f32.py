"""GPU: the deterministic fp32 3x3 conv (ops.conv3x3_f32, csrc/conv_f32.hip)
against F.conv2d in float64 on the CPU, its batch invariance as bits, and the
dynamic models with body="hip"."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (nimg, cin, cout, h, w, pool): the six SimpleConvNet layers and the smallest
# shapes that cross each tail (K granule, N tile, band tile, odd sizes)
SHAPES = [(1, 1, 1, 1, 1, 0), (2, 3, 5, 4, 6, 1), (2, 5, 7, 5, 7, 0), (1, 4, 16, 3, 70, 0),
          (1, 68, 33, 9, 3, 0), (1, 8, 8, 2, 2, 1), (3, 3, 64, 32, 32, 0), (2, 64, 64, 32, 32, 1),
          (2, 64, 128, 16, 16, 0), (2, 128, 128, 16, 16, 1), (1, 128, 256, 8, 8, 0),
          (1, 256, 256, 8, 8, 1)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def run(dev, x, w, cout, bias=None, affine=None, x_nchw=True, y_nchw=True, packed=None, **kw):
    """ops.conv3x3_f32 on NCHW host tensors; the result back as NCHW on the host."""
    from qconvnet import ops
    if packed is None:
        packed = torch.from_numpy(ops.pack_conv3x3_f32(w)).to(dev)
    xd = (x if x_nchw else x.permute(0, 2, 3, 1)).contiguous().to(dev)
    y = ops.conv3x3_f32(xd, packed, cout, bias=None if bias is None else bias.to(dev),
                        affine=None if affine is None else tuple(a.to(dev) for a in affine),
                        x_nchw=x_nchw, y_nchw=y_nchw, **kw).cpu()
    return y if y_nchw else y.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exact_on_integers(dev, shape):
    """Integer-valued inputs in [-8, 8]: every partial sum is exact in fp32, so
    the kernel must equal the float64 conv and epilogue bit for bit."""
    n, cin, cout, h, w, pool = shape
    g = torch.Generator().manual_seed(sum(shape))
    ri = lambda *s: torch.randint(-8, 9, s, generator=g).float()
    x, wt, b, al, be = ri(n, cin, h, w), ri(cout, cin, 3, 3), ri(cout), ri(cout), ri(cout)
    conv = F.conv2d(x.double(), wt.double(), None, padding=1)
    for x_nchw, y_nchw, (relu, bias, affine) in itertools.product(
            (False, True) if cin <= 4 else (False,), (False, True),
            ((True, True, False), (False, False, True), (True, True, True), (False, True, False))):
        t = conv + b.double().view(1, -1, 1, 1) if bias else conv
        if affine:
            t = t * al.double().view(1, -1, 1, 1) + be.double().view(1, -1, 1, 1)
        t = F.relu(t) if relu else t
        t = F.max_pool2d(t, 2, 2) if pool else t
        got = run(dev, x, wt, cout, b if bias else None, (al, be) if affine else None, x_nchw, y_nchw,
                  relu=relu, pool=bool(pool))
        assert torch.equal(bits(got), bits(t.float())), (x_nchw, y_nchw, relu, bias, affine)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_rounding_level_on_reals(dev, shape):
    """|y - y64| <= 2 (9 cin + 2) 2^-24 S, S = conv(|x|, |w|) + |bias|: twice the
    forward error bound gamma_{K+1} sum|x||w| of any order of correctly rounded
    fp32 operations (the factor covers MFMA-internal adds that are not
    individually round-to-nearest).  Derived, not measured."""
    n, cin, cout, h, w, pool = shape
    g = torch.Generator().manual_seed(sum(shape) + 1)
    x, wt, b = (torch.randn(n, cin, h, w, generator=g), 0.1 * torch.randn(cout, cin, 3, 3, generator=g),
                torch.randn(cout, generator=g))
    y64 = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    S = F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), padding=1)
    got = run(dev, x, wt, cout, b, x_nchw=False, y_nchw=False)
    ratio = ((got.double() - y64).abs() / (2 * (9 * cin + 2) * 2.0 ** -24 * S)).max().item()
    print(f"{shape}: max error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    if pool:
        pooled = run(dev, x, wt, cout, b, x_nchw=False, y_nchw=False, pool=True)
        assert torch.equal(bits(pooled), bits(F.max_pool2d(got, 2, 2)))


@pytest.mark.parametrize("cin,cout,hw,pool", [(64, 64, 32, True), (128, 256, 8, False)])
def test_batch_invariance_bits(dev, cin, cout, hw, pool):
    from qconvnet import ops
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(33, hw, hw, cin, generator=g).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    pk = torch.from_numpy(ops.pack_conv3x3_f32(0.1 * torch.randn(cout, cin, 3, 3, generator=g))).to(dev)
    f = lambda t: ops.conv3x3_f32(t.contiguous(), pk, cout, bias=b, relu=True, pool=pool)
    whole = bits(f(x))
    assert torch.equal(bits(torch.cat([f(x[i:i + 1]) for i in range(33)])), whole)
    assert torch.equal(bits(torch.cat([f(x[:5]), f(x[5:32]), f(x[32:])])), whole)
    assert torch.equal(bits(f(x.flip(0)).flip(0)), whole)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        y = f(x)
    side.synchronize()
    assert torch.equal(bits(y), whole) and torch.equal(bits(f(x)), whole)


@pytest.fixture(scope="module")
def sd(dev):
    import netfix
    return netfix.state_dict(netfix.load(False))   # as tests/test_gpu_models.py builds it


@pytest.mark.parametrize("fold", [True, False])
def test_model_batch_invariant_images_to_logits(dev, sd, fold):
    from models.dynamic_ptq_model import DynamicQuantConvNet
    from oracle import torch_ref
    m = DynamicQuantConvNet(sd, fold=fold, device=dev, granularity="sample", body="hip")
    u8 = torch.randint(0, 256, (33, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    for x in (torch.from_numpy(torch_ref.synthetic_images(33, 7)), u8):   # fp32 NCHW, raw u8 NHWC
        x = x.to(dev)
        whole = bits(m(x))
        assert torch.equal(bits(torch.cat([m(x[:1]), m(x[1:6]), m(x[6:])])), whole)
        assert torch.equal(bits(torch.cat([m(x[i:i + 1]) for i in range(33)])), whole)


# tests/test_gpu_models.py:110-116: end to end the GPU features differ from the
# CPU model's in the last bits, which moves a few dynamic-quantized fc inputs by
# one step; the project's stated bound on the logits is 1 % of max|logit|.
REF_MODE_REL_TOL = 1e-2


@pytest.mark.parametrize("kind", ["static_ptq", "dynamic_ptq"])
def test_model_against_cpu_reference(dev, sd, kind):
    from models.dynamic_ptq_model import DynamicPTQModel
    from models.static_ptq_model import StaticPTQModel
    from oracle import torch_ref
    fp = torch_ref.SimpleConvNetRef()
    fp.load_state_dict(sd)
    fp.eval()
    ref = torch_ref.build_static_ptq_cpu(fp) if kind == "static_ptq" else torch_ref.build_dynamic_ptq_cpu(fp)
    m = StaticPTQModel(mode="reference") if kind == "static_ptq" else DynamicPTQModel()
    m.load_state_dict(sd)
    q = m.quantize(body="hip")
    assert q.body == "hip"
    x = torch.from_numpy(torch_ref.synthetic_images(256, 41))
    with torch.no_grad():
        want = ref(x).numpy()
    got = q(x).numpy()
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"{kind}: max rel diff {rel:.3e}")
    assert rel <= REF_MODE_REL_TOL


def test_body_argument(dev, sd, monkeypatch):
    from models.dynamic_ptq_model import DynamicPTQModel, DynamicQuantConvNet
    from models.static_ptq_model import StaticPTQModel
    from oracle import torch_ref
    from qconvnet import ops
    with pytest.raises(ValueError):
        DynamicQuantConvNet(sd, device=dev, body="nope")
    with pytest.raises(ValueError):
        DynamicPTQModel().quantize(body="nope")
    with pytest.raises(ValueError):
        StaticPTQModel(mode="static").quantize(None, body="hip")

    def boom(*a, **k):
        raise AssertionError("the default body reached ops.conv3x3_f32")
    monkeypatch.setattr(ops, "conv3x3_f32", boom)
    m = DynamicQuantConvNet(sd, device=dev)
    assert m.body == "torch" and m.packed is None
    assert m(torch.from_numpy(torch_ref.synthetic_images(4, 3)).to(dev)).shape == (4, 10)


def test_status_codes_with_a_gpu(dev):
    from test_conv_f32_cpu import status_cases
    assert [(lbl, got) for lbl, want, got in status_cases() if got != want] == []
