"""CPU: histogram-observer calibration against torch.ao's own
HistogramObserver(reduce_range=False) on this host — the host combine and
search (qconvnet.quant), calibrate(observer="histogram") end to end against
torch's observers and against a torch.ao-converted net, and the unchanged
MinMax default."""
import numpy as np
import pytest
import torch
import torch.ao.quantization as tq
import torch.nn.functional as F

from qconvnet import quant as Q
from qconvnet import qmodel


def _torch_observer():
    return tq.HistogramObserver(reduce_range=False)


def _seq(kind):
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)
    if kind == "growing":        # the range grows at both ends
        return [r(4000), r(4000) * 2.0 - 0.5, r(4000) * 3.0 + 1.0]
    if kind == "unchanged":      # later batches stay inside the first range
        a = r(4000)
        return [a, a[:3000] * 0.5, torch.cat([a[:10], a.min().reshape(1), a.max().reshape(1)])]
    if kind == "constant_first":  # orig_min == orig_max on the first combine
        return [torch.full((512,), 0.75), r(4000), r(4000) * 1.5]
    if kind == "post_relu":
        return [F.relu(r(8, 16, 12, 12)), F.relu(r(8, 16, 12, 12) * 2.0),
                F.relu(r(8, 16, 12, 12) * 0.5)]
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["growing", "unchanged", "constant_first", "post_relu"])
def test_combine_and_search_match_torch(kind):
    ref, st = _torch_observer(), Q.HistogramState()
    for x in _seq(kind):
        ref(x)
        st.observe_host(x)
        assert torch.equal(st.histogram, ref.histogram)
        assert torch.equal(st.min_val, ref.min_val) and torch.equal(st.max_val, ref.max_val)
    lo, hi = st.search()
    rlo, rhi = ref._non_linear_param_search()
    assert lo == np.float32(rlo.item()) and hi == np.float32(rhi.item())
    scale, zp = Q.qparams_affine(lo, hi)
    rs, rz = ref.calculate_qparams()
    assert scale == np.float32(rs.item()) and zp == int(rz.item())


def test_update_takes_integer_counts():
    """The device path hands exact integer counts over the running range to
    HistogramState.update; that equals observing the same data on the host."""
    a, b = _seq("growing")[:2]
    ref, st = Q.HistogramState(), Q.HistogramState()
    lo, hi = torch.tensor(float("inf")), torch.tensor(float("-inf"))
    for x in (a, b):
        ref.observe_host(x)
        lo, hi = torch.min(lo, x.min()), torch.max(hi, x.max())
        counts = torch.histc(x, 2048, min=lo, max=hi).numpy().astype(np.uint32)
        st.update(float(lo), float(hi), torch.from_numpy(counts.astype(np.float32)))
    assert torch.equal(st.histogram, ref.histogram)
    assert torch.equal(st.min_val, ref.min_val) and torch.equal(st.max_val, ref.max_val)


# ------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def net():
    from models.baseline_model import synthetic_model
    from qconvnet import data
    calib = torch.from_numpy(data.synthetic_images(64, 1))
    fp = synthetic_model(0, calib)
    folded = qmodel.fold_state_dict(fp.state_dict())
    batches = [calib[:32], calib[32:] * 1.5]
    ranges = qmodel.calibrate(folded, batches, "cpu", observer="histogram", mode="static")
    return fp, folded, batches, ranges


def test_calibrate_histogram_matches_torch_observers(net):
    _, folded, batches, ranges = net
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in folded.items()}
    names = ["x"] + [f"conv{i}_out" for i in range(1, 7)] + ["fc1_out", "fc2_out"]
    obs = {n: _torch_observer() for n in names}
    with torch.no_grad():
        for x in batches:
            obs["x"](x)
            for i, (_, _, pool) in enumerate(qmodel.CONV_TABLE, start=1):
                x = F.relu(F.conv2d(x, t[f"conv{i}.w"], t[f"conv{i}.b"], padding=1))
                obs[f"conv{i}_out"](x)
                if pool:
                    x = F.max_pool2d(x, 2, 2)
            x = F.relu(F.linear(x.reshape(x.shape[0], -1), t["fc1.w"], t["fc1.b"]))
            obs["fc1_out"](x)
            obs["fc2_out"](F.linear(x, t["fc2.w"], t["fc2.b"]))
    assert sorted(ranges) == sorted(names)
    for n in names:
        rlo, rhi = obs[n]._non_linear_param_search()
        assert ranges[n] == (np.float32(rlo.item()), np.float32(rhi.item())), n


def test_qspec_matches_torch_ao_histogram_net(net):
    """A net calibrated the torch-default way (HistogramObserver activations)
    and converted by torch.ao has the qparams build_qspec derives here."""
    from oracle import torch_ref
    fp, folded, batches, ranges = net
    torch.backends.quantized.engine = "fbgemm"
    ao = torch_ref._FusedInt8Net(fp).eval()
    fuse = [[f"conv{i}", f"bn{i}", f"relu{i}"] for i in range(1, 7)] + [["fc1", "relu7"]]
    ao = tq.fuse_modules(ao, fuse, inplace=False)
    ao.qconfig = tq.QConfig(
        activation=tq.HistogramObserver.with_args(reduce_range=False),
        weight=tq.MinMaxObserver.with_args(dtype=torch.qint8, qscheme=torch.per_tensor_symmetric))
    tq.prepare(ao, inplace=True)
    with torch.no_grad():
        for xb in batches:
            ao(xb)
    tq.convert(ao, inplace=True)
    ref = qmodel.qspec_from_torch_ao(ao)
    spec = qmodel.build_qspec(folded, ranges, "static")
    assert spec["in"] == ref["in"]
    for name in [f"conv{i}" for i in range(1, 7)] + ["fc1", "fc2"]:
        assert spec[name]["s_y"] == ref[name]["s_y"], name
        assert spec[name]["z_y"] == ref[name]["z_y"], name


def test_histogram_qdq_observes_inputs_and_pre_relu_outputs(net):
    _, folded, batches, _ = net
    ranges = qmodel.calibrate(folded, batches[:1], "cpu", observer="histogram", mode="qdq")
    assert sorted(ranges) == sorted([f"conv{i}_{s}" for i in range(1, 7) for s in ("in", "out")]
                                    + ["fc1_in", "fc1_out"])
    ref = _torch_observer()
    ref(batches[0])
    rlo, rhi = ref._non_linear_param_search()
    assert ranges["conv1_in"] == (np.float32(rlo.item()), np.float32(rhi.item()))
    assert ranges["conv1_out"][0] < 0          # the pre-ReLU output
    qmodel.build_qspec(folded, ranges, "qdq")


def test_minmax_default_is_unchanged_and_unknown_observer_raises(net):
    _, folded, batches, _ = net
    today = qmodel.calibrate(folded, batches, "cpu")
    named = qmodel.calibrate(folded, batches, "cpu", observer="minmax")
    assert list(named) == list(today) and len(today) == 16
    for n in today:
        assert named[n] == today[n]
    # the running min/max computed directly on the same inputs
    x = torch.cat(batches)
    lo, hi = torch.aminmax(x)
    assert today["x"] == (np.float32(lo.item()), np.float32(hi.item()))
    assert today["conv1_in"] == today["x"]
    static = qmodel.calibrate(folded, batches, "cpu", observer="minmax", mode="static")
    assert all(static[n] == today[n] for n in static) and len(static) == 9
    with pytest.raises(ValueError):
        qmodel.calibrate(folded, batches, "cpu", observer="nope")
    with pytest.raises(ValueError):
        qmodel.calibrate(folded, batches, "cpu", observer="histogram")   # needs a mode
    with pytest.raises(ValueError):
        qmodel.calibrate(folded, batches, "cpu", observer="minmax", mode="nope")
