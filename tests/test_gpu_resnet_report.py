"""GPU: the per-layer error report of both ResNet executors
(qconvnet.resnet / qconvnet.resnet_qdq: run(keep="layers"), layer_names,
layer_pairs, layer_report; CustomQuantizedResNet50.quantization_report and its
observer / calibration_device keywords) on the fixture nets of resnetfix.py:
layers (1,1,1,1), 64 x 64, 8 images, fixture qparams.

The reports are compared with the numpy restatements (qerrref.py for the u8
hand-offs, cmpref.py for the fp32 ones) applied to the very tensors
layer_pairs yielded, copied to the host as they pass: counts equal, sums within
the derived bounds of test_gpu_qerror.py / test_gpu_qerror_f32.py."""
import numpy as np
import pytest
import torch

import cmpref
import qerrref
import resnetfix

pytestmark = pytest.mark.gpu

BATCH = 6   # 8 images: a batch of 6 and a ragged one of 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nets(dev):
    """{mode: (executor, its report module, the fp32 weights its walk reads, images fp32 NCHW)}"""
    from qconvnet import resnet, resnet_qdq
    z = resnetfix.load()
    sp = resnetfix.spec(z)
    assert resnetfix.check_weights(sp, z) == []
    zq = resnetfix.load_qdq()
    spq = resnetfix.qdq_spec(zq, fixture_qparams=True)
    assert resnetfix.check_qdq_spec(spq, zq) == []
    return {
        "static": (resnet.QuantizedResNet(sp, dev), resnet,
                   resnet.fold_state_dict(resnetfix.fp32_model(z).state_dict()),
                   torch.from_numpy(resnetfix.images(z))),
        "reference": (resnet_qdq.QuantizedResNetQDQ(spq, dev), resnet_qdq,
                      resnet_qdq.unfolded_state(resnetfix.fp32_model(zq).state_dict()),
                      torch.from_numpy(resnetfix.images(zq))),
    }


@pytest.fixture(scope="module")
def u8_images():
    return torch.from_numpy(np.random.default_rng(11).integers(0, 256, (8, 64, 64, 3), dtype=np.uint8))


def _same(a, b):
    assert list(a) == list(b)
    for name in a:
        assert set(a[name]) == set(b[name]), name
        for k, v in a[name].items():
            if k == "tensor":
                for kk, vv in v.items():
                    assert np.array_equal(vv, b[name]["tensor"][kk], equal_nan=True), (name, kk)
            else:
                assert np.array_equal(v, b[name][k], equal_nan=True), (name, k)


def test_inspection_mode_gives_the_default_forward(dev, nets):
    qm, _, _, x = nets["static"]
    x = x.to(dev)
    assert qm._stem_fusable(x)      # so the default forward and the inspection mode differ in the stem too
    before, kept = qm.run(x, keep=True)
    before, kept = before.clone(), {k: v.clone() for k, v in kept.items()}
    plain = qm.run(x).clone()
    logits, inter = qm.run(x, keep="layers")
    assert torch.equal(plain, before) and torch.equal(logits, before)
    for k, v in kept.items():       # stem, block{i}, pool
        assert torch.equal(inter[k], v), k
    want = {"stem", "stem.conv", "pool", "fc.q"}
    for i, b in enumerate(qm.blocks):
        want |= {f"block{i}", f"block{i}.c1", f"block{i}.c2", f"block{i}.c3"}
        want |= {f"block{i}.ds"} if b["ds"] is not None else set()
    assert set(inter) == want
    assert inter["stem.conv"].shape == (8, 32, 32, 64) and inter["fc.q"].dtype == torch.uint8
    assert set(qm.run(x, keep=True)[1]) == set(kept)
    assert torch.equal(qm.run(x), before)
    with pytest.raises(ValueError):
        qm.run(x, keep="everything")
    # raw u8 images: the same inspection mode, the same bits as the default forward of them
    u8 = torch.from_numpy(np.random.default_rng(12).integers(0, 256, (3, 64, 64, 3), dtype=np.uint8)).to(dev)
    assert torch.equal(qm.run(u8, keep="layers")[0], qm.run(u8).clone())


def _restate(seen):
    """{name: (counts, sums)} of the recorded pairs, batches combined."""
    ref = {}
    for name, xh, yh, scale, zp, nhwc in seen:
        assert nhwc
        if yh.ndim == 4:
            yh = yh.transpose(0, 3, 1, 2)
        assert yh.shape == xh.shape, name
        if yh.dtype == np.uint8:
            c, s = qerrref.stats(xh, yh, scale, zp)
        else:
            assert scale is None and zp is None
            c, s = cmpref.stats(xh, yh)
        if name in ref:
            pc, ps = ref[name]
            mx = np.maximum(c[:, -1], pc[:, -1])
            c, s = c + pc, s + ps
            c[:, -1] = mx
        ref[name] = (c, s)
    return ref


@pytest.mark.parametrize("mode", ("static", "reference"))
def test_layer_report_matches_restatement(dev, nets, mode, monkeypatch):
    """Every name's SQNR over the channels combined is finite; a single
    channel's may be nan or infinite (a ReLU output that is zero on every
    image)."""
    from qconvnet.qerror import summarize, summarize_f32
    qm, mod, weights, x = nets[mode]
    before = qm.run(x.to(dev)).clone()
    seen = []
    pairs = mod.layer_pairs

    def recording(*args, **kw):
        for item in pairs(*args, **kw):
            name, xf, y, scale, zp, nhwc = item
            seen.append((name, xf.cpu().numpy(), y.cpu().numpy(), scale, zp, nhwc))
            yield item

    monkeypatch.setattr(mod, "layer_pairs", recording)
    report = mod.layer_report(qm, weights, x, batch=BATCH)
    names = mod.layer_names(qm)
    if mode == "static":
        want = ["x", "stem"] + [f"b{i}.{k}" for i in range(4) for k in ("c1", "c2", "c3", "ds", "out")] \
            + ["pool", "fc"]
    else:
        want = ["stem", "stem.pool"] + [f"b{i}{k}" for i in range(4) for k in (".c1", ".c2", ".c3", ".ds", "")] \
            + ["pool", "fc"]
    assert list(report) == names == want
    assert [s[0] for s in seen] == names * 2
    f32_names = {"stem.pool", "pool"} | {f"b{i}" for i in range(4)} if mode == "reference" else set()
    ref = _restate(seen)
    for name in names:
        got, (c, s) = report[name], ref[name]
        n_c = int(c[0, 0])
        if name in f32_names:
            assert c.shape[1] == 3, name
            wantr = summarize_f32(c, s)
            for k in ("count", "differ", "max_abs_err"):
                assert np.array_equal(got[k], wantr[k]), (name, k)
                assert got["tensor"][k] == wantr["tensor"][k], (name, k)
            gs = np.stack([got[k] for k in ("sum_x2", "sum_e2", "sum_abs_e", "sum_e")], 1)
            print(mode, name, "excess", cmpref.excess(gs, s, n_c))
            assert cmpref.close(gs, s, n_c), name
        else:
            assert c.shape[1] == 5, name
            wantr = summarize(c, s)
            for k in ("count", "below", "above", "differ", "max_abs_err"):
                assert np.array_equal(got[k], wantr[k]), (name, k)
                assert got["tensor"][k] == wantr["tensor"][k], (name, k)
            for k in ("sum_x2", "sum_e2", "sum_abs_e"):
                assert qerrref.close(got[k], wantr[k], n_c), (name, k)
        print(mode, name, "sqnr", got["tensor"]["sqnr_db"], "non-finite channels",
              int((~np.isfinite(got["sqnr_db"])).sum()))
        assert np.isfinite(got["tensor"]["sqnr_db"]), name
        assert got["tensor"]["count"] == c[:, 0].sum()
    if "x" in report:
        assert not report["x"]["differ"].any()
        assert report["x"]["tensor"]["count"] == 8 * 3 * 64 * 64
    assert torch.equal(qm.run(x.to(dev)), before)


@pytest.mark.parametrize("mode", ("static", "reference"))
def test_u8_images_give_the_same_report(dev, nets, mode, u8_images):
    from qconvnet.qmodel import normalized_input
    qm, mod, weights, _ = nets[mode]
    fp = normalized_input(u8_images, qm.device, qm.ntab)
    _same(mod.layer_report(qm, weights, u8_images, batch=BATCH),
          mod.layer_report(qm, weights, fp, batch=BATCH))


@pytest.mark.parametrize("mode", ("static", "reference"))
def test_repeated_report_is_bit_identical(dev, nets, mode):
    qm, mod, weights, x = nets[mode]
    _same(mod.layer_report(qm, weights, x, batch=BATCH), mod.layer_report(qm, weights, x, batch=BATCH))


@pytest.mark.parametrize("mode", ("static", "reference"))
def test_model_surface(dev, mode, monkeypatch, u8_images):
    from models.custom_quantization_model import CustomQuantizedResNet50
    from models.resnet import synthetic_images, synthetic_resnet
    from qconvnet import qmodel, resnet, resnet_qdq
    from qconvnet import quant as Q

    made = []

    class Recording(qmodel._HistRange):
        """The device histogram observer, and beside it the host one fed the
        same activations copied to the host."""

        def __init__(self, device):
            super().__init__(device)
            assert torch.device(device).type == "cuda"
            self.host = Q.HistogramState()
            made.append(self)

        def __call__(self, x):
            super().__call__(x)
            self.host.observe_host(x.detach().cpu())

    monkeypatch.setitem(qmodel._OBSERVERS, "histogram", Recording)
    m = synthetic_resnet(1, (1, 1, 1, 1), num_classes=10, hw=64, calib_images=8, device=dev)
    calib = [torch.from_numpy(synthetic_images(4, s, 64)) for s in (5, 6)]
    w = CustomQuantizedResNet50(m, calibration_batches=calib, device=dev, mode=mode,
                                observer="histogram", calibration_device="cuda")
    assert len(made) == (23 if mode == "static" else 36)
    for i, r in enumerate(made):
        assert r.values() == r.host.search(), i
    with pytest.raises(ValueError):
        CustomQuantizedResNet50(m, calibration_batches=calib, device=dev, mode=mode, observer="nope")
    assert w.fp32_model is m and "fp32_model" not in dict(w.named_children())
    qm = w.quantized_model
    got = w.quantization_report(u8_images[:6], batch=4)
    if mode == "static":
        ref = resnet.layer_report(qm, resnet.fold_state_dict(m.state_dict()), u8_images[:6], batch=4)
        assert got["x"]["tensor"]["count"] == 6 * 3 * 64 * 64
    else:
        ref = resnet_qdq.layer_report(qm, resnet_qdq.unfolded_state(m.state_dict()), u8_images[:6], batch=4)
        assert "sum_e" in got["b0"] and "below" in got["b0.c1"]
    _same(got, ref)
    out = w(torch.from_numpy(synthetic_images(2, 9, 64)))
    assert out.shape == (2, 10)
