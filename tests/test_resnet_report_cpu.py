"""CPU: histogram calibration of both ResNet executors against torch.ao's
HistogramObserver (bit for bit), the numpy restatement of the fp32-against-
fp32 error statistics (cmpref.py) against torch, qconvnet.qerror.summarize_f32
on hand-made counts, and the host half of qcn_qerror_f32_f32 (argument checks,
workspace size) — no device."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.ao.quantization as tq

import cmpref as R
from oracle import torch_ref

IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
HW = 64


# ------------------------------------------------------- histogram calibration
def _qconfig():
    return tq.QConfig(
        activation=tq.HistogramObserver.with_args(reduce_range=False),
        weight=tq.PerChannelMinMaxObserver.with_args(dtype=torch.qint8,
                                                     qscheme=torch.per_channel_symmetric))


@pytest.fixture(scope="module")
def fp32():
    m = torch_ref.ResNetRef((1, 1, 1, 1), 10)
    m.load_state_dict(torch_ref.resnet_state_dict(m, 0))
    return m.eval()


@pytest.fixture(scope="module", params=("fp32", "u8"))
def batches(request):
    """(what the calibration is fed, the fp32 NCHW tensors torch.ao is fed):
    two batches of 4 images."""
    from qconvnet import quant as Q
    from qconvnet.qmodel import normalized_input
    if request.param == "fp32":
        b = [torch.from_numpy(torch_ref.synthetic_images(4, s, hw=HW, **IMAGENET)) for s in (1, 2)]
        return b, b
    rng = np.random.default_rng(3)
    raw = [torch.from_numpy(rng.integers(0, 256, (4, HW, HW, 3), dtype=np.uint8)) for _ in range(2)]
    ntab = Q.normalize_table(IMAGENET["mean"], IMAGENET["std"])
    return raw, [normalized_input(r, "cpu", ntab) for r in raw]


def _same_qparams(ranges, observers):
    from qconvnet import quant as Q
    assert sorted(ranges) == sorted(observers)
    for name, obs in observers.items():
        assert isinstance(obs, tq.HistogramObserver), name
        s, z = obs.calculate_qparams()
        got = Q.qparams_affine(*ranges[name])
        assert (np.float32(got[0]), int(got[1])) == (np.float32(s.item()), int(z.item())), name


def test_static_histogram_calibration_is_torch_ao(fp32, batches):
    from qconvnet.resnet import calibrate, fold_state_dict
    fed, as_fp32 = batches
    torch.backends.quantized.engine = "fbgemm"
    net = copy.deepcopy(fp32).eval()
    net = tq.fuse_modules(net, torch_ref.resnet_fuse_list(net), inplace=False)
    net.qconfig = _qconfig()
    tq.prepare(net, inplace=True)
    with torch.no_grad():
        for xb in as_fp32:
            net(xb)
    obs = {"x": net.quant.activation_post_process, "stem": net.conv1.activation_post_process,
           "fc": net.fc.activation_post_process}
    for i in range(4):
        blk = getattr(net, f"layer{i + 1}")[0]
        obs.update({f"b{i}.c1": blk.conv1.activation_post_process,
                    f"b{i}.c2": blk.conv2.activation_post_process,
                    f"b{i}.c3": blk.conv3.activation_post_process,
                    f"b{i}.ds": blk.downsample[0].activation_post_process,
                    f"b{i}.out": blk.q_out.activation_post_process})
    assert len(obs) == 23
    assert sum(isinstance(m, tq.HistogramObserver) for m in net.modules()) == 23
    ranges = calibrate(fold_state_dict(fp32.state_dict()), fed, "cpu", observer="histogram")
    _same_qparams(ranges, obs)


def test_reference_histogram_calibration_is_torch_ao(fp32, batches):
    from qconvnet.resnet_qdq import calibrate, unfolded_state
    fed, as_fp32 = batches
    torch.backends.quantized.engine = "fbgemm"
    net = torch_ref.RefQDQResNet(copy.deepcopy(fp32).eval()).eval()
    for m in net.modules():
        if isinstance(m, torch_ref._QDQConv):
            m.qconfig = _qconfig()
    tq.prepare(net, inplace=True)
    with torch.no_grad():
        for xb in as_fp32:
            net(xb)
    obs = {}

    def put(name, m):
        obs[name + ".in"] = m.quant.activation_post_process
        obs[name + ".out"] = m.op.activation_post_process

    put("stem", net.conv1)
    put("fc", net.fc)
    for i in range(4):
        blk = getattr(net, f"layer{i + 1}")[0]
        for k, m in (("c1", blk.conv1), ("c2", blk.conv2), ("c3", blk.conv3), ("ds", blk.downsample[0])):
            put(f"b{i}.{k}", m)
    assert len(obs) == 36
    assert sum(isinstance(m, tq.HistogramObserver) for m in net.modules()) == 36
    ranges = calibrate(unfolded_state(fp32.state_dict()), fed, "cpu", observer="histogram")
    _same_qparams(ranges, obs)


def test_minmax_default_is_unchanged_and_unknown_observer_raises(fp32, batches):
    from qconvnet import resnet, resnet_qdq
    fed, _ = batches
    for mod, net in ((resnet, resnet.fold_state_dict(fp32.state_dict())),
                     (resnet_qdq, resnet_qdq.unfolded_state(fp32.state_dict()))):
        today = mod.calibrate(net, fed)
        named = mod.calibrate(net, fed, "cpu", observer="minmax")
        assert list(named) == list(today)
        for n in today:
            assert named[n] == today[n], n
        hist = mod.calibrate(net, fed[:1], "cpu", observer="histogram")
        assert list(hist) == list(today)
        with pytest.raises(ValueError):
            mod.calibrate(net, fed, "cpu", observer="nope")
    # the running min/max computed directly on the same inputs
    from qconvnet import quant as Q
    from qconvnet.qmodel import normalized_input
    ntab = Q.normalize_table(IMAGENET["mean"], IMAGENET["std"])
    lo, hi = torch.aminmax(torch.cat([normalized_input(b, "cpu", ntab) for b in fed]))
    assert today["stem.in"] == (np.float32(lo.item()), np.float32(hi.item()))


# ------------------------------------------------------------- restatement
@pytest.mark.parametrize("count", (1, 37, 1024, 4096))
def test_sqnr_is_compute_sqnr(count):
    """Within 0.01 dB at <= 4,096 elements: torch's fp32 norms carry a relative
    error of at most about n * 2^-24 ~ 2.4e-4, i.e. 2e-3 dB; 0.01 dB is x5."""
    from torch.ao.ns.fx.utils import compute_sqnr
    rng = np.random.default_rng(count)
    x = rng.standard_normal(count).astype(np.float32)
    y = (x + (0.05 * rng.standard_normal(count)).astype(np.float32)).astype(np.float32)
    ref = float(compute_sqnr(torch.from_numpy(x), torch.from_numpy(y)))
    got = R.sqnr_db(x, y)
    assert abs(got - ref) <= 0.01, (got, ref)


@pytest.mark.parametrize("shape", ((3, 5, 3, 7), (2, 64, 16, 16), (130, 10), (4, 1, 9, 9)))
def test_differ_and_max_are_torch(shape):
    x, y = R.make_case(np.random.default_rng(len(shape)), shape)
    y[0, 0] = np.float32(-0.0)      # -0.0 == +0.0
    x[0, 0] = np.float32(0.0)
    counts, sums = R.stats(x, y)
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    ch = [d for d in range(tx.dim()) if d != 1]
    assert np.array_equal(counts[:, 0], np.full(shape[1], x.size // shape[1]))
    assert np.array_equal(counts[:, 1], (tx != ty).sum(ch).numpy())
    mx = (tx - ty).abs().amax(ch).numpy()
    assert np.array_equal(counts[:, 2].astype(np.uint32).view(np.float32), mx)
    e = tx.double() - ty.double()
    ref = torch.stack([(tx.double() ** 2).sum(ch), (e * e).sum(ch), e.abs().sum(ch), e.sum(ch)], 1)
    assert R.close(sums, ref.numpy(), x.size // shape[1])


def test_close_is_the_derived_bound():
    ref = np.array([[4.0, 2.0, 3.0, -1.0], [0.0, 0.0, 0.0, 0.0]])
    eps = 4.0 * 100 * 2.0 ** -53
    assert R.close(ref, ref, 100)
    assert R.close(ref * np.array([1 + eps / 2, 1, 1, 1]), ref, 100)
    assert not R.close(ref * np.array([1 + 3 * eps, 1, 1, 1]), ref, 100)
    row0 = np.array([[1.0], [0.0]])
    assert R.close(ref + row0 * np.array([0, 0, 0, 2 * eps]), ref, 100)   # bound: eps * sum|e| = 3 eps
    assert not R.close(ref + row0 * np.array([0, 0, 0, 4 * eps]), ref, 100)
    assert not R.close(ref + np.array([[0, 0, 0, 0], [0, 0, 0, 1e-300]]), ref, 100)   # no |e|, no sum e
    assert not R.close(ref + np.array([[0, 0, 0, 0], [0, 1e-300, 0, 0]]), ref, 100)   # zero stays zero


def test_summarize_f32_fields_and_special_cases():
    from qconvnet.qerror import DERIVED_F32, RAW_F32, summarize_f32
    bits = lambda v: int(np.float32(v).view(np.uint32))
    counts = np.array([[10, 3, bits(0.5)],     # ordinary
                       [10, 0, bits(0.0)],     # no error: +inf
                       [10, 4, bits(0.25)],    # no signal: -inf
                       [10, 0, bits(0.0)]],    # neither: nan
                      np.int64)
    sums = np.array([[100.0, 1.0, 2.0, -1.5], [50.0, 0.0, 0.0, 0.0], [0.0, 4.0, 5.0, 5.0],
                     [0.0, 0.0, 0.0, 0.0]])
    r = summarize_f32(counts, sums)
    assert RAW_F32 == ("count", "differ", "max_abs_err", "sum_x2", "sum_e2", "sum_abs_e", "sum_e")
    assert DERIVED_F32 == ("sqnr_db", "mse", "mean_abs_err", "mean_err", "differ_frac")
    assert set(RAW_F32) | set(DERIVED_F32) | {"tensor"} == set(r)
    assert np.array_equal(r["count"], [10, 10, 10, 10]) and np.array_equal(r["differ"], [3, 0, 4, 0])
    assert r["max_abs_err"].dtype == np.float32
    assert np.array_equal(r["max_abs_err"], np.array([0.5, 0, 0.25, 0], np.float32))
    for i, k in enumerate(("sum_x2", "sum_e2", "sum_abs_e", "sum_e")):
        assert np.array_equal(r[k], sums[:, i]), k
    assert r["sqnr_db"][0] == 10.0 * np.log10(100.0)
    assert r["sqnr_db"][1] == np.inf and r["sqnr_db"][2] == -np.inf and np.isnan(r["sqnr_db"][3])
    assert np.array_equal(r["mse"], sums[:, 1] / 10) and np.array_equal(r["mean_abs_err"], sums[:, 2] / 10)
    assert np.array_equal(r["mean_err"], sums[:, 3] / 10)
    assert np.array_equal(r["differ_frac"], [0.3, 0, 0.4, 0])
    t = r["tensor"]
    assert set(RAW_F32) | set(DERIVED_F32) == set(t)
    assert (t["count"], t["differ"]) == (40, 7) and t["max_abs_err"] == np.float32(0.5)
    assert (t["sum_x2"], t["sum_e2"], t["sum_abs_e"], t["sum_e"]) == (150.0, 5.0, 7.0, 3.5)
    assert t["sqnr_db"] == 10.0 * np.log10(150.0 / 5.0)
    assert t["mse"] == 5.0 / 40 and t["mean_abs_err"] == 7.0 / 40 and t["mean_err"] == 3.5 / 40
    assert t["differ_frac"] == 7 / 40
    assert summarize_f32(counts[1:2], sums[1:2])["tensor"]["sqnr_db"] == np.inf
    assert summarize_f32(counts[2:3], sums[2:3])["tensor"]["sqnr_db"] == -np.inf
    assert np.isnan(summarize_f32(counts[3:4], sums[3:4])["tensor"]["sqnr_db"])
    with pytest.raises(ValueError):
        summarize_f32(counts, sums[:3])


# ---------------------------------------------------------- ABI, host half
@pytest.fixture(scope="module")
def lib():
    from qconvnet import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libqconvnet.so missing — run __graft_entry__.build()")
    return _lib.load()


def test_bad_arguments_before_any_device_call(lib):
    """Host addresses stand in for the device pointers: every call below must
    return before it could touch them."""
    x = np.zeros(8, np.float32)
    y = np.zeros(8, np.float32)
    counts = np.zeros(3, np.int64)
    sums = np.zeros(4, np.float64)
    ws = np.zeros(64, np.float64)
    P = lambda a: C.c_void_p(a.ctypes.data)

    def call(x=x, y=y, n=1, c=1, h=2, w=2, counts=counts, sums=sums, ws=ws):
        return lib.qcn_qerror_f32_f32(P(x) if x is not None else None, P(y) if y is not None else None,
                                      n, c, h, w, 1, P(counts) if counts is not None else None,
                                      P(sums) if sums is not None else None,
                                      P(ws) if ws is not None else None, None)

    for kw in (dict(x=None), dict(y=None), dict(counts=None), dict(sums=None), dict(ws=None),
               dict(n=-1), dict(c=0), dict(h=0), dict(w=0)):
        assert call(**kw) == -1, kw
    assert call(c=1 << 20) == -2
    assert call(n=1 << 16, h=1 << 8, w=1 << 8) == -2   # n * h * w >= 2^31
    assert call(n=0) == 0            # nothing to launch
    assert not counts.any() and not sums.any()


def test_workspace_size(lib):
    size = lib.qcn_qerror_f32_workspace_size
    for shape in ((-1, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert size(*shape) == -1, shape
    assert size(1, 1 << 20, 1, 1) == -2
    assert size(1 << 16, 1, 1 << 8, 1 << 8) == -2      # n * h * w >= 2^31
    assert size(0, 64, 8, 8) == 0
    # room for at least one record (4 doubles, 2 uint32) per channel, never
    # shrinking as c grows, and proportional to c over whole channel groups
    for n, h, w in ((1, 1, 1), (2, 16, 16), (1024, 32, 32)):
        prev = 0
        for c in (1, 2, 3, 4, 5, 16, 17, 64, 65, 128, 257, 2048):
            s = size(n, c, h, w)
            assert s >= 40 * c and s >= prev, (n, c, h, w, s)
            prev = s
        base = size(n, 64, h, w)
        for k in (2, 4, 32):
            assert size(n, 64 * k, h, w) == k * base


def test_python_surface_is_exported():
    from qconvnet import ops, qerror, resnet, resnet_qdq
    for name in ("qerror_f32_workspace_size", "qerror_f32_buffers", "qerror_f32"):
        assert callable(getattr(ops, name)), name
    for name in ("summarize_f32", "FloatErrorStats", "score_pairs"):
        assert callable(getattr(qerror, name)), name
    for mod in (resnet, resnet_qdq):
        for name in ("layer_names", "layer_pairs", "layer_report"):
            assert callable(getattr(mod, name)), (mod.__name__, name)
    assert ops.qerror_f32_workspace_size(2, 64, 16, 16) == ops.qerror_workspace_size(2, 64, 16, 16)
    with pytest.raises(ValueError):
        ops.qerror_f32_workspace_size(1, 0, 1, 1)
