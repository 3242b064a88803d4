"""GPU: the per-sample dynamic Linear (qcn_linear_dynamic_rows_f32,
ops.linear_dynamic_rows, granularity="sample" of the dynamic models).  Row i of
its result is quantized::linear_dynamic of x[i] alone: the kernels are
compared with dynrows.rows_ref (pinned against torch in
test_dynamic_rows_cpu.py) as fp32 bit patterns, the per-row scale and zero
point exactly; there is no tolerance anywhere.  NaN and inf are outside the
contract."""
import ctypes as C

import numpy as np
import pytest
import torch

import dynrows as D
import opedge as E
from oracle import qref

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _T(dev):
    return lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_bits(got, want):
    return np.array_equal(E.bits(got.cpu().numpy() if torch.is_tensor(got) else got), E.bits(want))


def _wsum(w):
    return w.astype(np.int64).sum(1).astype(np.int32)


@pytest.fixture(scope="module")
def c33(dev):
    """The (33, 384, 65) case on the device with its row reference (per-channel, bias)."""
    x, w, s_pt, s_pc, b = D.case(33, 384, 65)
    T = _T(dev)
    return dict(x=x, w=w, s=s_pc, b=b, args=(T(w), T(s_pc), T(_wsum(w)), T(b)),
                ref=D.rows_ref(x, w, s_pc, b))


@pytest.mark.parametrize("m,k,n", D.SHAPES)
def test_rows_kernel_vs_reference(dev, m, k, n):
    from qconvnet import ops
    x, w, s_pt, s_pc, b = D.case(m, k, n)
    T = _T(dev)
    xt, wt, wsum = T(x), T(w), T(_wsum(w))
    for s_w in (s_pt, s_pc):
        st = T(s_w)
        for bias in (b, None):
            for rr in (True, False):
                want = D.rows_ref(x, w, s_w, bias, rr)
                ws, wz = D.rows_qparams(x, rr)
                got, (gs, gz) = ops.linear_dynamic_rows(xt, wt, st, wsum, T(bias), reduce_range=rr,
                                                        qparams=True)
                what = (s_w.size, bias is None, rr)
                assert gz.dtype == torch.int32 and np.array_equal(gz.cpu().numpy(), wz), what
                assert _same_bits(gs, ws), what
                bad = (E.bits(got.cpu().numpy()) != E.bits(want)).any(axis=1)
                assert not bad.any(), (what, "rows", np.flatnonzero(bad).tolist())


def test_input_not_16_byte_aligned(dev):
    """k % 4 == 0 but x starts 4 bytes past a 16-byte boundary (a view): the
    quantize kernel must not use its 16-byte loads."""
    from qconvnet import ops
    x, w, s_pt, s_pc, b = D.case(7, 96, 33)
    T = _T(dev)
    xt = T(np.concatenate([np.zeros(1, F32), x.ravel()]))[1:].view(7, 96)
    assert xt.data_ptr() % 16 == 4 and xt.is_contiguous()
    got = ops.linear_dynamic_rows(xt, T(w), T(s_pc), T(_wsum(w)), T(b))
    assert _same_bits(got, D.rows_ref(x, w, s_pc, b))


def test_batch_invariance(dev, c33):
    from qconvnet import ops
    xt = _T(dev)(c33["x"])

    def run(t):
        return ops.linear_dynamic_rows(t.contiguous(), *c33["args"]).cpu().numpy()

    whole = run(xt)
    assert _same_bits(whole, c33["ref"])
    assert _same_bits(np.concatenate([run(xt[i:i + 1]) for i in range(33)]), whole)
    assert _same_bits(np.concatenate([run(xt[:5]), run(xt[5:32]), run(xt[32:])]), whole)
    assert _same_bits(run(xt.flip(0))[::-1], whole)


def test_differs_from_the_batch_form(dev, c33):
    from qconvnet import ops
    xt = _T(dev)(c33["x"])
    rows = ops.linear_dynamic_rows(xt, *c33["args"]).cpu().numpy()
    batch = ops.linear_dynamic(xt, *c33["args"]).cpu().numpy()
    assert (E.bits(rows) != E.bits(batch)).any(axis=1).any()
    alone = ops.linear_dynamic(xt[:1].contiguous(), *c33["args"]).cpu().numpy()
    assert _same_bits(rows[:1], alone)


def test_one_outlier_leaves_the_other_rows_alone(dev, c33):
    """One element of 40.0 in row 5: the batch form gives every row the
    outlier's range; here every row keeps its own."""
    from qconvnet import ops
    x = E.dyn_input("normal", 33, 384, 12)
    x[5, 7] = 40.0
    got = ops.linear_dynamic_rows(_T(dev)(x), *c33["args"])
    assert _same_bits(got, D.rows_ref(x, c33["w"], c33["s"], c33["b"]))
    batch = qref.linear_dynamic(x, c33["w"], c33["s"], c33["b"])
    assert not _same_bits(got, batch)


def test_workspace_and_stream(dev, c33):
    from qconvnet import ops
    m, k = c33["x"].shape
    xt = _T(dev)(c33["x"])
    need = ops.lib().qcn_linear_dynamic_rows_workspace_size(m, k)
    assert need == (16 * m + 63) // 64 * 64 + m * k
    # exactly the size: used (the records of the rows are in it afterwards)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device=dev)
    got, (s, z) = ops.linear_dynamic_rows(xt, *c33["args"], workspace=ws, qparams=True)
    assert _same_bits(got, c33["ref"])
    rec = ws[:16 * m].view(torch.float32).view(m, 4)
    assert torch.equal(rec[:, 0], s) and torch.equal(rec[:, 3].contiguous().view(torch.int32), z)
    ws_s, ws_z = D.rows_qparams(c33["x"])
    assert _same_bits(s, ws_s) and np.array_equal(z.cpu().numpy(), ws_z)
    # one byte short: the binding allocates its own and leaves this one alone
    short = torch.full((need - 1,), 0xAB, dtype=torch.uint8, device=dev)
    got = ops.linear_dynamic_rows(xt, *c33["args"], workspace=short)
    assert _same_bits(got, c33["ref"])
    assert bool((short == 0xAB).all())
    # a non-default stream
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = ops.linear_dynamic_rows(xt, *c33["args"])
    side.synchronize()
    assert _same_bits(got, c33["ref"])


def test_bad_arguments_return_status(dev):
    from qconvnet import _lib
    lib = _lib.load()
    m, k, n = 4, 8, 3
    buf = {"x": torch.zeros(m, k, device=dev), "w": torch.zeros(n, k, dtype=torch.int8, device=dev),
           "w_scale": torch.ones(1, device=dev), "wsum": torch.zeros(n, dtype=torch.int32, device=dev),
           "bias": None, "y": torch.zeros(m, n, device=dev),
           "workspace": torch.zeros(lib.qcn_linear_dynamic_rows_workspace_size(m, k), dtype=torch.uint8,
                                    device=dev)}

    def call(m=m, k=k, n=n, **null):
        p = {name: None if t is None or name in null else C.c_void_p(t.data_ptr())
             for name, t in buf.items()}
        return lib.qcn_linear_dynamic_rows_f32(p["x"], m, k, p["w"], n, p["w_scale"], 0, p["wsum"],
                                               p["bias"], 1, p["y"], p["workspace"], None)

    assert call() == _lib.QCN_OK     # bias is optional
    torch.cuda.synchronize()
    for name in ("x", "w", "w_scale", "wsum", "y", "workspace"):
        assert call(**{name: True}) == _lib.QCN_ERR_ARG, name
    for dim in ("m", "k", "n"):
        for val in (0, -1):
            assert call(**{dim: val}) == _lib.QCN_ERR_ARG, (dim, val)


# ------------------------------------------------------------------- models
def _host_fc(fc):
    w, s, _, b = (t.cpu().numpy() for t in fc)
    return w, s, b


def _raise(*a, **kw):
    raise AssertionError("sample granularity consulted _range")


def test_convnet_sample_granularity(dev, monkeypatch):
    from models.baseline_model import SimpleConvNet
    from models.dynamic_ptq_model import DynamicQuantConvNet
    from qconvnet import ops
    torch.manual_seed(0)
    sd = SimpleConvNet().eval().state_dict()
    # "huge" and "subnormal" rows would leave fp32's range in the fc1 -> ReLU -> fc2 chain
    order = tuple("normal" if c in ("huge", "subnormal") else c for c in D.ORDER)
    feats = D.mixed_rows(33, 4096, 3, order)
    ft = _T(dev)(feats)

    model = DynamicQuantConvNet(sd, device=dev, granularity="sample")
    model.sharded = True
    monkeypatch.setattr(model, "_range", _raise)
    got = model.classify(ft).cpu().numpy()
    alone = np.concatenate([model.classify(ft[i:i + 1].contiguous()).cpu().numpy() for i in range(33)])
    assert _same_bits(alone, got)
    h = qref.relu_f32(D.rows_ref(feats, *_host_fc(model.fc[0])))
    want = D.rows_ref(h, *_host_fc(model.fc[1]))
    assert _same_bits(got, want) and E.distinct_ok(want)

    # the default is what the class has always computed
    batch = DynamicQuantConvNet(sd, device=dev)
    assert batch.granularity == "batch"
    h = torch.relu(ops.linear_dynamic(ft, *batch.fc[0])).contiguous()
    chain = ops.linear_dynamic(h, *batch.fc[1]).cpu().numpy()
    assert _same_bits(batch.classify(ft), chain)
    assert not _same_bits(got, chain)


def test_resnet_fc_sample_granularity(dev):
    from models.optimized_custom_quantization import DynamicFcResNet
    from models.resnet import resnet50
    from qconvnet import ops
    torch.manual_seed(0)
    fp = resnet50().eval()
    feats = D.mixed_rows(9, 2048, 5)
    ft = _T(dev)(feats)
    model = DynamicFcResNet(fp, dev, granularity="sample")
    got = model.classify(ft).cpu().numpy()
    alone = np.concatenate([model.classify(ft[i:i + 1].contiguous()).cpu().numpy() for i in range(9)])
    assert _same_bits(alone, got)
    assert _same_bits(got, D.rows_ref(feats, *_host_fc(model.fc)))
    model.granularity = "batch"      # the default: one ops.linear_dynamic call
    chain = ops.linear_dynamic(ft, *model.fc).cpu().numpy()
    assert _same_bits(model.classify(ft), chain)
    assert not _same_bits(got, chain)
