"""GPU: the bf16 3x3 conv (ops.conv3x3_bf16, csrc/conv_bf16.hip) against
F.conv2d in float64 on the CPU with t.bfloat16().float() as the rounding, its
free bf16 hand-off and its batch invariance as bits, and the dynamic models
with body="bf16"."""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (nimg, cin, cout, h, w, pool): the smallest map, odd channels and sizes, the
# 8-channel K unit with w past two blocks, Cin off the step with a second band,
# a second Cin chunk and channel tile, and one shape per wave arrangement
SHAPES = [(1, 1, 1, 1, 1, 0), (2, 3, 5, 4, 6, 1), (2, 5, 7, 5, 7, 0), (1, 9, 16, 3, 70, 0),
          (1, 68, 33, 9, 3, 0), (1, 264, 65, 8, 8, 1), (2, 64, 64, 32, 32, 1), (2, 128, 128, 16, 16, 1),
          (1, 256, 256, 8, 8, 1)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def run(dev, x, w, cout, bias=None, affine=None, x_fmt="nhwc", y_fmt="nhwc", **kw):
    """ops.conv3x3_bf16 on NCHW fp32 host tensors, x handed over as x_fmt and y
    asked for as y_fmt ("nchw", "nhwc" or "bf16"); the result back as NCHW."""
    from qconvnet import ops
    packed = torch.from_numpy(ops.pack_conv3x3_bf16(w)).to(dev)
    xd = (x if x_fmt == "nchw" else x.permute(0, 2, 3, 1)).contiguous()
    xd = (xd.bfloat16() if x_fmt == "bf16" else xd).to(dev)
    y = ops.conv3x3_bf16(xd, packed, cout, bias=None if bias is None else bias.to(dev),
                         affine=None if affine is None else tuple(a.to(dev) for a in affine),
                         x_nchw=x_fmt == "nchw", y_nchw=y_fmt == "nchw", y_bf16=y_fmt == "bf16", **kw).cpu()
    return y if y_fmt == "nchw" else y.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exact_on_integers(dev, shape):
    """Integers in [-8, 8] are exact in bf16 and every partial sum is exact in
    fp32: the kernel must equal the float64 conv and epilogue bit for bit (a
    bf16 result: its bf16 rounding)."""
    n, cin, cout, h, w, pool = shape
    g = torch.Generator().manual_seed(sum(shape))
    ri = lambda *s: torch.randint(-8, 9, s, generator=g).float()
    x, wt, b, al, be = ri(n, cin, h, w), ri(cout, cin, 3, 3), ri(cout), ri(cout), ri(cout)
    conv = F.conv2d(x.double(), wt.double(), None, padding=1)
    for x_fmt, y_fmt, (relu, bias, affine) in itertools.product(
            ("nchw", "nhwc", "bf16") if cin <= 4 else ("nhwc", "bf16"), ("nhwc", "nchw", "bf16"),
            ((True, True, False), (False, False, True), (True, True, True), (False, True, False))):
        t = conv + b.double().view(1, -1, 1, 1) if bias else conv
        if affine:
            t = t * al.double().view(1, -1, 1, 1) + be.double().view(1, -1, 1, 1)
        t = F.relu(t) if relu else t
        t = (F.max_pool2d(t, 2, 2) if pool else t).float()
        got = run(dev, x, wt, cout, b if bias else None, (al, be) if affine else None, x_fmt, y_fmt,
                  relu=relu, pool=bool(pool))
        assert torch.equal(bits(got), bits(t.bfloat16() if y_fmt == "bf16" else t)), (x_fmt, y_fmt, relu, bias, affine)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_rounding_level_on_reals(dev, shape):
    """With xb, wb the bf16-rounded operands (their products are exact in fp32):
    |y - y64| <= 2 (9 cin + 2) 2^-24 S, S = conv(|xb|, |wb|) + |bias|: twice the
    forward error bound gamma_{K+1} sum|x||w| of any order of correctly rounded
    fp32 additions (the factor covers MFMA-internal adds that are not
    individually round-to-nearest).  Derived, not measured."""
    n, cin, cout, h, w, pool = shape
    g = torch.Generator().manual_seed(sum(shape) + 1)
    x, wt, b = (torch.randn(n, cin, h, w, generator=g), 0.1 * torch.randn(cout, cin, 3, 3, generator=g),
                torch.randn(cout, generator=g))
    xb, wb = x.bfloat16().double(), wt.bfloat16().double()
    y64 = F.conv2d(xb, wb, b.double(), padding=1)
    S = F.conv2d(xb.abs(), wb.abs(), b.double().abs(), padding=1)
    got = run(dev, x, wt, cout, b)
    ratio = ((got.double() - y64).abs() / (2 * (9 * cin + 2) * 2.0 ** -24 * S)).max().item()
    print(f"{shape}: max error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    if pool:
        assert torch.equal(bits(run(dev, x, wt, cout, b, pool=True)), bits(F.max_pool2d(got, 2, 2)))


@pytest.mark.parametrize("cin,cout,hw", [(64, 64, 32), (128, 128, 16)])
def test_handoff_is_free(dev, cin, cout, hw):
    """A bf16 result is the fp32 result rounded, and the next layer computes
    the same bits from either."""
    from qconvnet import ops
    g = torch.Generator().manual_seed(cout)
    x = torch.randn(3, hw, hw, cin, generator=g).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    pk = [torch.from_numpy(ops.pack_conv3x3_bf16(0.1 * torch.randn(co, ci, 3, 3, generator=g))).to(dev)
          for co, ci in ((cout, cin), (32, cout))]
    y32, y16 = (ops.conv3x3_bf16(x, pk[0], cout, bias=b, relu=True, pool=True, y_bf16=f) for f in (False, True))
    assert y16.dtype == torch.bfloat16 and torch.equal(bits(y16), bits(y32.bfloat16()))
    assert torch.equal(bits(ops.conv3x3_bf16(y16, pk[1], 32)), bits(ops.conv3x3_bf16(y32, pk[1], 32)))


def test_batch_invariance_bits(dev):
    from qconvnet import ops
    cin, cout, hw = 64, 64, 32
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(33, hw, hw, cin, generator=g).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    pk = torch.from_numpy(ops.pack_conv3x3_bf16(0.1 * torch.randn(cout, cin, 3, 3, generator=g))).to(dev)
    f = lambda t: ops.conv3x3_bf16(t.contiguous(), pk, cout, bias=b, relu=True, pool=True, y_bf16=True)
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
    from models.baseline_model import CONV_TABLE
    from models.dynamic_ptq_model import DynamicQuantConvNet
    from oracle import torch_ref
    from qconvnet import ops
    m = DynamicQuantConvNet(sd, fold=fold, device=dev, granularity="sample", body="bf16")
    u8 = torch.randint(0, 256, (33, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    for x in (torch.from_numpy(torch_ref.synthetic_images(33, 7)), u8):   # fp32 NCHW, raw u8 NHWC
        x = x.to(dev)
        whole = bits(m(x))
        assert torch.equal(bits(torch.cat([m(x[:1]), m(x[1:6]), m(x[6:])])), whole)
        assert torch.equal(bits(torch.cat([m(x[i:i + 1]) for i in range(33)])), whole)
    # features(): bf16 hand-offs; the same six calls with fp32 hand-offs give the same bits
    x = torch.from_numpy(torch_ref.synthetic_images(5, 9)).to(dev)
    y = x
    for i, (wp, b, affine) in enumerate(m.bconvs):
        y = ops.conv3x3_bf16(y, wp, CONV_TABLE[i][1], bias=b, affine=affine, relu=True,
                             pool=bool(CONV_TABLE[i][2]), x_nchw=i == 0, y_nchw=i == 5)
    assert torch.equal(bits(m.features(x)), bits(y.reshape(5, -1)))


def test_model_error_against_fp32_no_worse_than_int8(dev, sd):
    """The logits' max error against the fp32 CPU model, relative to max|logit|,
    for body="bf16" and body="int8" in the same run: bf16's reason to exist is
    that it is the smaller one."""
    from models.dynamic_ptq_model import DynamicQuantConvNet
    from oracle import torch_ref
    fp = torch_ref.SimpleConvNetRef()
    fp.load_state_dict(sd)
    fp.eval()
    x = torch.from_numpy(torch_ref.synthetic_images(256, 41))
    with torch.no_grad():
        want = fp(x)
    rel = {}
    for body in ("bf16", "int8"):
        got = DynamicQuantConvNet(sd, device=dev, granularity="sample", body=body)(x.to(dev)).cpu()
        rel[body] = ((got - want).abs().max() / want.abs().max()).item()
        print(f"{body}: max |logit error| / max |logit| = {rel[body]:.3e}")
    assert rel["bf16"] <= rel["int8"]


def test_quantize_passes_body_through(dev, sd):
    from models.dynamic_ptq_model import DynamicPTQModel
    from models.static_ptq_model import StaticPTQModel
    for m in (DynamicPTQModel(), StaticPTQModel(mode="reference")):
        m.load_state_dict(sd)
        q = m.quantize(body="bf16")
        assert q.body == "bf16" and len(q.bconvs) == 6 and q.bconvs[0][0].dtype == torch.int16
