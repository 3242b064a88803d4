"""GPU: qcn_histc_f32 against torch.histc on the CPU copy (counts equal
exactly; every bin stays below 2^24, where torch's fp32 counts are exact too),
ops.HistogramObserver against torch.ao's HistogramObserver on the CPU, and
quantize(observer="histogram") with calibration on the device."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BINS = 2048


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()
    return torch.device("cuda:0")


def _randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _device_counts(x_cpu, lo, hi, dev, bins=BINS, out=None, view_from=0):
    """ops.histc of x_cpu[view_from:] over the device range [lo, hi]."""
    from qconvnet import ops
    xd = x_cpu.to(dev)[view_from:]
    mm = torch.tensor([lo, hi], dtype=torch.float32).to(dev)
    out = ops.histc(xd, mm, bins, out=out)
    return out, out.cpu().numpy().view(np.uint32).astype(np.int64)


def _torch_counts(x_cpu, lo, hi, bins=BINS):
    ref = torch.histc(x_cpu, bins, min=lo, max=hi)
    assert float(ref.max()) < 2 ** 24
    return ref.numpy().astype(np.int64)


def _check(x_cpu, dev, lo=None, hi=None, bins=BINS, view_from=0):
    x_ref = x_cpu[view_from:]
    lo = float(x_ref.min()) if lo is None else lo
    hi = float(x_ref.max()) if hi is None else hi
    _, got = _device_counts(x_cpu, lo, hi, dev, bins, view_from=view_from)
    ref = _torch_counts(x_ref, lo, hi, bins)
    assert got.sum() == ref.sum()
    assert np.array_equal(got, ref), f"{np.count_nonzero(got != ref)} bins differ"


@pytest.mark.parametrize("count", [1, 3, 4, 255, 1027, 300001])
def test_histc_counts(dev, count):
    _check(_randn(count, count), dev)


def test_histc_unaligned_view(dev):
    x = _randn(300001, 1)
    for k in (1, 2, 3):
        _check(x, dev, view_from=k)
    _check(x[:3], dev, view_from=1)      # fewer elements than the way to the 16-byte boundary
    _check(x[:8], dev, view_from=3)      # head, one float4, no tail


def test_histc_normal(dev):
    _check(_randn(64 * 16 * 16 * 16, 2), dev)


def test_histc_post_relu_hot_bin(dev):
    _check(F.relu(_randn(64 * 16 * 16 * 16, 3)), dev)


def test_histc_all_equal(dev):
    x = torch.full((70001,), 0.375)
    _check(x, dev)                       # lo == hi -> [lo - 1, hi + 1]
    _check(torch.zeros(4099), dev)


def test_histc_range_narrower_than_data(dev):
    x = _randn(300001, 4) * 3.0
    _check(x, dev, lo=-1.25, hi=2.5)
    ref = _torch_counts(x, -1.25, 2.5)
    assert ref.sum() < x.numel()         # some elements were skipped


def test_histc_bin_edges_and_neighbours(dev):
    for lo, hi in ((-3.7, 5.1), (0.0, 6.3), (-1.0, 1.0)):
        edges = torch.linspace(lo, hi, BINS + 1)
        x = torch.cat([edges, torch.nextafter(edges, torch.tensor(float("inf"))),
                       torch.nextafter(edges, torch.tensor(float("-inf"))), _randn(5000, 5)])
        _check(x, dev, lo=float(edges[0]), hi=float(edges[-1]))


def test_histc_denormals_and_negative_zero(dev):
    tiny = torch.tensor([1e-45, -1e-45, 1e-40, -1e-40, 5.9e-39, -0.0, 0.0, 1.1754944e-38])
    _check(torch.cat([tiny, _randn(1000, 6)]), dev)
    _check(tiny, dev)                                  # a denormal-wide range
    _check(tiny, dev, lo=0.0, hi=1.1754944e-38)
    _check(F.relu(_randn(1000, 7)) * -1.0, dev)        # hi == -0.0 -> range [lo, 0]


@pytest.mark.parametrize("bins", [16, 4096])
def test_histc_other_bin_counts(dev, bins):
    _check(_randn(100003, bins), dev, bins=bins)
    _check(F.relu(_randn(100003, bins + 1)), dev, bins=bins)


def test_histc_adds_into_hist(dev):
    a, b = _randn(50001, 8), F.relu(_randn(70003, 9))
    out, first = _device_counts(a, -4.0, 4.0, dev)
    assert np.array_equal(first, _torch_counts(a, -4.0, 4.0))
    _, both = _device_counts(b, -4.0, 4.0, dev, out=out)
    assert np.array_equal(both, _torch_counts(a, -4.0, 4.0) + _torch_counts(b, -4.0, 4.0))


def test_histc_reset_range_counts_nothing(dev):
    from qconvnet import ops
    obs = ops.MinMaxObserver(dev)          # reset: [+inf, -inf]
    out = ops.histc(_randn(10007, 10).to(dev), obs.state)
    assert int(out.cpu().abs().sum()) == 0


def test_histc_argument_statuses(dev):
    from qconvnet import _lib
    lib = _lib.load()
    x = torch.zeros(64, device=dev)
    mm = torch.tensor([0.0, 1.0], device=dev)
    h = torch.zeros(BINS, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.qcn_histc_f32(None, 64, p(mm), BINS, p(h), None) == _lib.QCN_ERR_ARG
    assert lib.qcn_histc_f32(p(x), 64, None, BINS, p(h), None) == _lib.QCN_ERR_ARG
    assert lib.qcn_histc_f32(p(x), 64, p(mm), BINS, None, None) == _lib.QCN_ERR_ARG
    assert lib.qcn_histc_f32(p(x), -1, p(mm), BINS, p(h), None) == _lib.QCN_ERR_ARG
    assert lib.qcn_histc_f32(p(x), 1 << 32, p(mm), BINS, p(h), None) == _lib.QCN_ERR_ARG
    for bins in (1000, 8, 8192, 0):
        assert lib.qcn_histc_f32(p(x), 64, p(mm), bins, p(h), None) == _lib.QCN_ERR_UNSUPPORTED
    assert lib.qcn_histc_f32(p(x), 0, p(mm), BINS, p(h), None) == _lib.QCN_OK
    torch.cuda.synchronize()
    assert int(h.cpu().abs().sum()) == 0


@pytest.mark.parametrize("first", ["scaled", "constant"])
def test_histogram_observer_matches_torch(dev, first):
    import torch.ao.quantization as tq
    from qconvnet import ops
    from qconvnet import quant as Q
    base = [F.relu(torch.randn(64, 16, 16, 16, generator=torch.Generator().manual_seed(20 + i)))
            for i in range(3)]
    seq = [base[0] * 1.0, base[1] * 2.0, base[2] * 0.5]
    if first == "constant":
        seq[0] = torch.full((64, 16, 16, 16), 0.5)
    ref, obs = tq.HistogramObserver(reduce_range=False), ops.HistogramObserver(dev)
    for x in seq:
        ref(x)
        obs(x.to(dev))
        assert torch.equal(obs.histogram, ref.histogram)
        assert torch.equal(obs.min_val, ref.min_val) and torch.equal(obs.max_val, ref.max_val)
    scale, zp = Q.qparams_affine(*obs.values())
    rs, rz = ref.calculate_qparams()
    assert scale == np.float32(rs.item()) and zp == int(rz.item())


def test_static_ptq_quantize_histogram_on_device(dev):
    """Calibration on the device builds a model whose forward runs and agrees
    with the CPU-calibrated histogram model (MIOpen's fp32 convs are not
    bit-stable against the CPU's, so this is a smoke check; the parity gates
    are the histc and observer tests above).

    The net is a briefly trained one on the synthetic 10-class task, and the
    images come from that task: an argmax comparison needs decision margins.
    The logits are u8 steps of fc2's scale, and an image whose two best logits
    lie within one step of each other changes its argmax with the last bit of
    any scale.  Measured with random-init weights on noise images: 3 to 13 of
    256 images have such a margin, the device- and host-calibrated ranges
    agree to 3e-6 relative, and the 3 (histogram; MinMax on the golden
    weights: 5) disagreeing images all had a margin of 0 or 1 step — 98.8 %,
    a property of that net, not of the calibration."""
    from models.baseline_model import trained_synthetic_model
    from models.static_ptq_model import StaticPTQModel
    from qconvnet import data
    sd = trained_synthetic_model(0, steps=100, batch=128, device=dev).state_dict()
    # most of this test's seconds are first-use costs in the process: the first
    # training step (~2.5 s) and MIOpen's first run of each fp32 conv shape (~3 s)
    calib = torch.from_numpy(data.synthetic_task(256, 1)[0])
    loader = [calib[:128], calib[128:]]
    x = torch.from_numpy(data.synthetic_task(256, 2)[0]).to(dev)
    logits = {}
    for where in ("cuda", "cpu"):
        m = StaticPTQModel(device=dev)
        m.load_state_dict(sd)
        q = m.quantize(loader, observer="histogram", calibration_device=where)
        logits[where] = q(x).cpu().numpy()
    assert logits["cuda"].shape == (256, 10) and np.isfinite(logits["cuda"]).all()
    agree = np.mean(logits["cuda"].argmax(1) == logits["cpu"].argmax(1))
    top2 = np.sort(logits["cpu"], 1)[:, -2:]
    step = float(q.spec["fc2"]["s_y"])
    print("argmax agreement", agree, "images within one fc2 step of a tie:",
          int(((top2[:, 1] - top2[:, 0]) <= 1.5 * step).sum()))
    assert agree >= 0.99
