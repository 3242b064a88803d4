"""GPU: the dynamically quantized int8 3x3 conv (ops.conv3x3_dyn,
csrc/conv_dyn.hip) as bits against the numpy contract composed from
oracle.qref, its batch invariance, and the dynamic models with body="int8"."""
import itertools

import numpy as np
import pytest
import torch

import opedge as E
from oracle import qref
from qconvnet import quant as Q

pytestmark = pytest.mark.gpu
F32 = np.float32

# (nimg, h, w, cin, cout): 1x1 map (all taps but the centre are padding), cin 3, cout 1; 2x2 with
# pool; odd h, w, cin % 16 != 0, cout one past a 64-channel tile; two bands x three blocks across
# with channel tiles past cout; two blocks across of the 4-wave-wide block; the 2 x 2 wave block with
# idle channel waves; several K steps; a second cin chunk; then the six layers
SHAPES = [(2, 1, 1, 3, 1), (2, 2, 2, 8, 5), (5, 5, 7, 20, 65), (2, 9, 19, 16, 130), (1, 4, 40, 4, 8),
          (1, 6, 12, 36, 70), (1, 8, 8, 128, 16), (1, 8, 8, 256, 16), (2, 2, 2, 272, 4),
          (2, 32, 32, 3, 64), (2, 32, 32, 64, 64), (2, 16, 16, 64, 128), (2, 16, 16, 128, 128),
          (2, 8, 8, 128, 256), (2, 8, 8, 256, 256)]
# neighbouring images need qparams orders of magnitude apart (tests/dynrows.py)
KINDS = ("normal", "huge", "negative", "constant", "zero")
# (bias, affine, relu, pool)
FORMS = ((True, False, False, False), (True, True, False, False), (True, False, True, True),
         (False, False, False, False))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()
    return torch.device("cuda:0")


def mixed_images(n, h, w, c, seed):
    return np.stack([E.dyn_input(KINDS[i % len(KINDS)], 1, h * w * c, seed + i).reshape(h, w, c)
                     for i in range(n)])


def acc_ref(x, wq, rr=False):
    """Contract steps 1-3 per image: (acc [n, h, w, cout] int32, scales, zero points)."""
    ohwi = np.ascontiguousarray(wq.transpose(0, 2, 3, 1))
    acc, ss, zs = [], [], []
    for xi in x:
        s, z = qref.choose_qparams_dynamic(xi.min(), xi.max(), reduce_range=rr)
        acc.append(qref.conv3x3_acc_nhwc(qref.quantize_legacy_fma(xi, s, z)[None], z, ohwi)[0])
        ss.append(s)
        zs.append(z)
    return np.stack(acc), np.array(ss, F32), np.array(zs, np.int32)


def epilogue_ref(acc, ss, s_w, bias, affine, relu, pool):
    """Contract steps 4-5 in float32 on [n, h, w, cout]."""
    a = acc.astype(F32)
    sc = np.broadcast_to((ss.reshape(-1, 1, 1, 1) * s_w.reshape(1, 1, 1, -1)).astype(F32), a.shape)
    t = Q.fmaf_host(a, sc, np.broadcast_to(np.zeros(1, F32) if bias is None else bias, a.shape))
    if affine is not None:
        t = Q.fmaf_host(t, np.broadcast_to(affine[0], a.shape), np.broadcast_to(affine[1], a.shape))
    if relu:
        t = np.maximum(t, F32(0))
    return qref.maxpool2x2_nhwc(t) if pool else t


def run(dev, x, pk, s_w, cout, bias, affine, relu, pool, x_nchw=False, y_nchw=False, **kw):
    """ops.image_minmax + ops.conv3x3_dyn on NHWC host data -> (y NHWC, stats, qparams) on the host."""
    from qconvnet import ops
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xd = t(x.transpose(0, 3, 1, 2) if x_nchw else x)
    y, st, qp = ops.conv3x3_dyn(xd, ops.image_minmax(xd), pk[0], pk[1], t(s_w), cout, bias=t(bias),
                                affine=None if affine is None else (t(affine[0]), t(affine[1])),
                                relu=relu, pool=pool, x_nchw=x_nchw, y_nchw=y_nchw, qparams=True, **kw)
    y = y.cpu().numpy()
    return (y.transpose(0, 2, 3, 1) if y_nchw else y), st.cpu().numpy(), (qp[0].cpu().numpy(), qp[1].cpu().numpy())


def packed(dev, wq):
    from qconvnet import ops
    return tuple(torch.from_numpy(a).to(dev) for a in ops.pack_conv3x3_dyn(wq))


def check(got, ref, zs_ss, label):
    y, st, (gs, gz) = got
    ss, zs = zs_ss
    assert np.array_equal(E.bits(y), E.bits(ref)), label
    assert np.array_equal(E.bits(gs), E.bits(ss)) and np.array_equal(gz, zs), label
    n = ref.shape[0]
    assert np.array_equal(st[:, :, 0].min(1), ref.reshape(n, -1).min(1)), label
    assert np.array_equal(st[:, :, 1].max(1), ref.reshape(n, -1).max(1)), label


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_against_contract(dev, shape):
    n, h, w, cin, cout = shape
    rng = np.random.default_rng(sum(shape))
    x = mixed_images(n, h, w, cin, sum(shape))
    wq = rng.integers(-128, 128, (cout, cin, 3, 3), dtype=np.int8)
    s_pc = rng.uniform(0.002, 0.01, cout).astype(F32)
    bias, al, be = (rng.standard_normal(cout).astype(F32) for _ in range(3))
    acc, ss, zs = acc_ref(x, wq)
    assert E.distinct_ok(acc)
    pk = packed(dev, wq)
    for s_w, (hb, ha, relu, pool) in itertools.product((s_pc[:1], s_pc), FORMS):
        pool = pool and h % 2 == 0 and w % 2 == 0
        b, aff = (bias if hb else None), ((al, be) if ha else None)
        ref = epilogue_ref(acc, ss, s_w, b, aff, relu, pool)
        for x_nchw, y_nchw in itertools.product((False, True), (False, True)):
            check(run(dev, x, pk, s_w, cout, b, aff, relu, pool, x_nchw, y_nchw), ref, (ss, zs),
                  (s_w.size, hb, ha, relu, pool, x_nchw, y_nchw))


def test_reduce_range_flag(dev):
    n, h, w, cin, cout = 3, 4, 6, 16, 8
    rng = np.random.default_rng(2)
    x = mixed_images(n, h, w, cin, 2)
    wq = rng.integers(-128, 128, (cout, cin, 3, 3), dtype=np.int8)
    s_w, bias = np.array([0.004], F32), rng.standard_normal(cout).astype(F32)
    acc, ss, zs = acc_ref(x, wq, rr=True)
    assert zs.max() <= 127
    check(run(dev, x, packed(dev, wq), s_w, cout, bias, None, True, True, reduce_range=True),
          epilogue_ref(acc, ss, s_w, bias, None, True, True), (ss, zs), "reduce_range")


def test_full_range_accumulator(dev):
    """cin = 256, codes 0 and 255 only, weights +-127: |acc| reaches 9 * 256 * 255 * 127."""
    cin, cout = 256, 20
    rng = np.random.default_rng(3)
    x = np.ones((3, 8, 8, cin), F32)                        # z = 0: every pixel is code 255
    x[1] = rng.integers(0, 2, x[1].shape).astype(F32)       # codes 0 and 255
    x[2] = -rng.integers(0, 2, x[2].shape).astype(F32)      # z = 255: q - z is 0 or -255
    x[2, 3:6, 3:6] = -1.0
    wq = (rng.integers(0, 2, (cout, cin, 3, 3)) * 254 - 127).astype(np.int8)
    wq[0], wq[1] = 127, -127
    acc, ss, zs = acc_ref(x, wq)
    assert list(zs) == [0, 0, 255] and acc.max() == 9 * 256 * 255 * 127 == -acc.min()
    s_w, bias = np.full(cout, 0.003, F32), rng.standard_normal(cout).astype(F32)
    check(run(dev, x, packed(dev, wq), s_w, cout, bias, None, False, False),
          epilogue_ref(acc, ss, s_w, bias, None, False, False), (ss, zs), "full range")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_batch_invariance_bits(dev):
    from qconvnet import ops
    cin, cout, hw = 64, 128, 16
    rng = np.random.default_rng(4)
    x = torch.from_numpy(mixed_images(33, hw, hw, cin, 4)).to(dev)
    pk = packed(dev, rng.integers(-128, 128, (cout, cin, 3, 3), dtype=np.int8))
    s_w = torch.from_numpy(rng.uniform(0.002, 0.01, cout).astype(F32)).to(dev)
    b = torch.from_numpy(rng.standard_normal(cout).astype(F32)).to(dev)

    def f(t):
        t = t.contiguous()
        y, st = ops.conv3x3_dyn(t, ops.image_minmax(t), pk[0], pk[1], s_w, cout, bias=b, relu=True, pool=True)
        return torch.cat([y.reshape(len(t), -1), st.amin(1)[:, :1], st.amax(1)[:, 1:]], 1)
    whole = bits(f(x))
    assert torch.equal(bits(torch.cat([f(x[:1]), f(x[1:6]), f(x[6:])])), whole)
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
    return netfix.state_dict(netfix.load(False))


def model_ref(sd, fold, x):
    """The whole-model contract on NCHW images: the layer reference chained
    (per-channel conv weights, full 8 bits), then the per-sample dynamic head."""
    from models.baseline_model import CONV_TABLE
    from qconvnet.qmodel import fold_state_dict
    g = {k: v.numpy() for k, v in sd.items()}
    f = fold_state_dict(sd)
    bn = lambda i: Q.bn_eval_affine(*(g[f"bn{i}.{k}"] for k in ("running_mean", "running_var", "weight", "bias")))
    t = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    for i in range(1, 7):
        w, b = (f[f"conv{i}.w"], f[f"conv{i}.b"]) if fold else (g[f"conv{i}.weight"], g[f"conv{i}.bias"])
        flat = w.reshape(w.shape[0], -1)
        s_w = Q.qparams_symmetric(flat.min(1), flat.max(1))
        acc, ss, _ = acc_ref(t, Q.quantize_weight(w, s_w))
        t = epilogue_ref(acc, ss, s_w, b, None if fold else bn(i), True, CONV_TABLE[i - 1][2])
    t = np.ascontiguousarray(t.transpose(0, 3, 1, 2)).reshape(len(x), -1)
    for name in ("fc1", "fc2"):
        w, b = (f["fc1.w"], f["fc1.b"]) if fold and name == "fc1" else (g[name + ".weight"], g[name + ".bias"])
        s_w = Q.qparams_symmetric(w.min(), w.max())
        t = np.concatenate([qref.linear_dynamic(r[None], Q.quantize_weight(w, s_w), s_w, b) for r in t])
        if name == "fc1":
            t = np.maximum(t if fold else Q.fmaf_host(t, *(np.broadcast_to(a, t.shape) for a in bn(7))), F32(0))
    return t


@pytest.mark.parametrize("fold", [True, False])
def test_model_batch_invariant_and_exact(dev, sd, fold):
    from models.dynamic_ptq_model import DynamicQuantConvNet
    from oracle import torch_ref
    m = DynamicQuantConvNet(sd, fold=fold, device=dev, granularity="sample", body="int8")
    xh = torch_ref.synthetic_images(33, 7)
    x = torch.from_numpy(xh).to(dev)
    whole = m(x)
    assert torch.equal(bits(torch.cat([m(x[:1]), m(x[1:6]), m(x[6:])])), bits(whole))
    rows = [1, 32]   # the reference of an image does not depend on the others: two rows of the 33
    assert np.array_equal(E.bits(whole[rows].cpu().numpy()), E.bits(model_ref(sd, fold, xh[rows])))


def test_interface(dev, sd):
    from models.dynamic_ptq_model import DynamicPTQModel
    from models.static_ptq_model import StaticPTQModel
    for m in (DynamicPTQModel(), StaticPTQModel(mode="reference")):
        m.load_state_dict(sd)
        q = m.quantize(body="int8", granularity="sample")
        assert q.body == "int8" and len(q.qconvs) == 6 and q.qconvs[0][0].dtype == torch.int8
    d = DynamicPTQModel()
    d.load_state_dict(sd)
    d.quantize(body="int8")
    size_int8 = d.get_model_size()
    d.quantize(body="hip")
    assert size_int8 > d.get_model_size() + 1.0   # the int8 conv weights are counted (~1.1 MB)
    with pytest.raises(ValueError):
        StaticPTQModel(mode="static").quantize(None, body="int8")
    from test_conv_dyn_cpu import status_cases
    assert [(lbl, got) for lbl, want, got in status_cases() if got != want] == []
