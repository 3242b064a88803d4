"""GPU: qcn_qerror_u8_f32 and what is built on it (ops.qerror,
qerror.QuantErrorStats / layer_pairs / layer_report, the models'
quantization_report) against the numpy restatement in qerrref.py.

counts are compared for equality in every field, the bit pattern of the max
included.  Each sums entry must lie within relative 4 * N_c * 2^-53 of the
restatement (N_c: the channel's element count), a zero on one side a zero on
the other.  The bound is derived, not measured: the terms are identical in
both (every operation is the same IEEE operation and nothing is contracted),
only the order of the N_c non-negative additions differs, which costs at most
(N_c - 1) * 2^-53 per side.

Inputs (qerrref.make_case): q uniform with 5 % of the codes forced to 0 and
5 % to 255; x = d + scale * noise, N(0, 0.35) on interior codes, N(0, 3) on
the end codes.  Asserted on the restatement alone, for every shape of at least
500 elements, before the device is asked: below, above and differ each cover
at least 1 % of the tensor."""
import numpy as np
import pytest
import torch

import qerrref as R

pytestmark = pytest.mark.gpu

SLICES, TILE = 512, 4096   # qcn::kQerrSlices, qcn::kQerrTile
# 64 channels are one group of 64 x 64-pixel tiles; one image more than
# SLICES tiles' worth of pixels, so some workgroups walk two tiles
OVER_CAP = (SLICES * (TILE // 64) // (32 * 32) + 1, 64, 32, 32)
SHAPES = ((3, 5, 3, 7), (1, 3, 32, 32), (2, 64, 16, 16), (2, 257, 2, 2), (130, 10, 1, 1),
          (5, 512, 1, 1), (1, 1, 1, 1), (4, 1, 9, 9), OVER_CAP)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


_CASES = {}


def _case(shape):
    """(x NCHW, q NCHW, scale, zp, counts, sums), made once per shape."""
    if shape not in _CASES:
        k = SHAPES.index(shape)
        scale, zp = R.QPARAMS[k % len(R.QPARAMS)]
        x, q = R.make_case(np.random.default_rng(7000 + k), shape, scale, zp)
        counts, sums = R.stats(x, q, scale, zp)
        for a in (x, q, counts, sums):
            a.setflags(write=False)
        _CASES[shape] = (x, q, scale, zp, counts, sums)
    return _CASES[shape]


def _place(a, dev, offset):
    """A device copy of ``a`` that starts ``offset`` elements into its allocation."""
    t = torch.from_numpy(np.array(a))
    flat = torch.zeros(t.numel() + offset, dtype=t.dtype, device=dev)
    flat[offset:] = t.to(dev).reshape(-1)
    return flat[offset:].view(t.shape)


def _run(dev, x, q_nchw, scale, zp, nhwc, offset=False, bufs=None):
    from qconvnet import ops
    n, c = x.shape[:2]
    q = np.ascontiguousarray(q_nchw.transpose(0, 2, 3, 1)) if nhwc else q_nchw
    xd = _place(x, dev, 1 if offset else 0)     # 4 bytes in
    qd = _place(q, dev, 1 if offset else 0)     # 1 byte in
    if offset:
        assert xd.data_ptr() % 16 == 4 and qd.data_ptr() % 16 == 1
    counts, sums = bufs if bufs is not None else ops.qerror_buffers(c, dev)
    ops.qerror(xd, qd, scale, zp, counts, sums, nhwc=nhwc)
    return counts, sums


def test_inputs_cover_every_field():
    for shape in SHAPES:
        x, q, scale, zp, counts, _ = _case(shape)
        if x.size < 500:
            continue
        tot = counts.sum(0)
        frac = tot[1:4] / tot[0]
        assert (frac >= 0.01).all(), (shape, frac)


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("nhwc", (0, 1), ids=("nchw", "nhwc"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_restatement(dev, shape, nhwc, offset):
    x, q, scale, zp, rc, rs = _case(shape)
    counts, sums = _run(dev, x, q, scale, zp, nhwc, offset)
    counts, sums = counts.cpu().numpy(), sums.cpu().numpy()
    n_c = x.size // shape[1]
    print(shape, nhwc, offset, "max rel", np.max(np.abs(sums - rs) / np.maximum(np.abs(rs), 1e-300)),
          "bound", 4.0 * n_c * 2.0 ** -53)
    assert np.array_equal(counts, rc)
    assert R.close(sums, rs, n_c)


@pytest.mark.parametrize("scale,zp", R.QPARAMS)
def test_every_qparam_pair(dev, scale, zp):
    shape = (2, 64, 16, 16)
    x, q = R.make_case(np.random.default_rng(zp), shape, scale, zp)
    rc, rs = R.stats(x, q, scale, zp)
    counts, sums = _run(dev, x, q, scale, zp, 1)
    assert np.array_equal(counts.cpu().numpy(), rc)
    assert R.close(sums.cpu().numpy(), rs, x.size // shape[1])


@pytest.mark.parametrize("shape", ((37, 5, 3, 7), (130, 10, 1, 1)), ids=("tile", "direct"))
def test_ragged_slices_accumulate(dev, shape):
    from qconvnet import ops
    scale, zp = R.QPARAMS[0]
    x, q = R.make_case(np.random.default_rng(5), shape, scale, zp)
    whole_c, whole_s = _run(dev, x, q, scale, zp, 1)
    bufs = ops.qerror_buffers(shape[1], dev)
    cut = (0, 1, shape[0] // 3 + 2, shape[0])
    for a, b in zip(cut[:-1], cut[1:]):
        _run(dev, x[a:b], q[a:b], scale, zp, 1, bufs=bufs)
    assert np.array_equal(bufs[0].cpu().numpy(), whole_c.cpu().numpy())
    assert R.close(bufs[1].cpu().numpy(), whole_s.cpu().numpy(), x.size // shape[1])
    rc, rs = R.stats(x, q, scale, zp)
    assert np.array_equal(bufs[0].cpu().numpy(), rc)
    assert R.close(bufs[1].cpu().numpy(), rs, x.size // shape[1])


@pytest.mark.parametrize("shape", ((2, 64, 16, 16), OVER_CAP, (5, 512, 1, 1)),
                         ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bit_identical(dev, shape):
    x, q, scale, zp, _, _ = _case(shape)
    a = _run(dev, x, q, scale, zp, 1)
    b = _run(dev, x, q, scale, zp, 1)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))


@pytest.mark.parametrize("shape", ((2, 64, 16, 16), (3, 5, 3, 7), (130, 10, 1, 1)),
                         ids=lambda s: "x".join(map(str, s)))
def test_exact_dequantized_input_has_no_error(dev, shape):
    from qconvnet.qerror import summarize
    _, q, scale, zp, _, _ = _case(shape)
    x = R.dequant(q, scale, zp)
    counts, sums = _run(dev, x, q, scale, zp, 1)
    r = summarize(counts.cpu().numpy(), sums.cpu().numpy())
    assert not r["sum_e2"].any() and not r["sum_abs_e"].any() and not r["differ"].any()
    assert not r["max_abs_err"].any() and not r["below"].any() and not r["above"].any()
    assert (r["sqnr_db"] == np.inf).all() and r["tensor"]["sqnr_db"] == np.inf


def test_no_rows_leaves_the_buffers_untouched(dev):
    from qconvnet import _lib, ops
    import ctypes as C
    counts, sums = ops.qerror_buffers(4, dev)
    counts.fill_(7)
    sums.fill_(1.5)
    x = torch.zeros((0, 4, 3, 3), dtype=torch.float32, device=dev)
    q = torch.zeros((0, 3, 3, 4), dtype=torch.uint8, device=dev)
    ops.qerror(x, q, 0.1, 3, counts, sums)
    # and the entry itself, with real addresses
    keep = torch.zeros(64, dtype=torch.uint8, device=dev)
    rc = _lib.load().qcn_qerror_u8_f32(C.c_void_p(keep.data_ptr()), C.c_void_p(keep.data_ptr()), 0, 4,
                                       3, 3, 1, C.c_float(0.1), 3, C.c_void_p(counts.data_ptr()),
                                       C.c_void_p(sums.data_ptr()), C.c_void_p(keep.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert (counts == 7).all() and (sums == 1.5).all()


def test_stats_object_one_copy(dev):
    from qconvnet.qerror import QuantErrorStats, summarize
    shape = (3, 5, 3, 7)
    x, q, scale, zp, rc, rs = _case(shape)
    st = QuantErrorStats(5, dev)
    xd = torch.from_numpy(np.array(x)).to(dev)
    qd = torch.from_numpy(np.ascontiguousarray(q.transpose(0, 2, 3, 1))).to(dev)
    st.update(xd, qd, scale, zp).update(xd, qd, scale, zp)
    r = st.result()
    ref = summarize(2 * rc * np.array([1, 1, 1, 1, 0]) + rc * np.array([0, 0, 0, 0, 1]), 2 * rs)
    for k in ("count", "below", "above", "differ", "max_abs_err"):
        assert np.array_equal(r[k], ref[k]), k
    assert np.allclose(r["sqnr_db"], ref["sqnr_db"], rtol=0, atol=1e-9)
    assert st.reset().result()["tensor"]["count"] == 0


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def net(dev):
    import netfix
    from qconvnet.qmodel import QuantizedConvNet
    z = netfix.load(False)
    spec, folded = netfix.static_spec(z)
    models = {"static": QuantizedConvNet(spec, dev), "qdq": QuantizedConvNet(netfix.qdq_spec(z), dev)}
    u8 = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (9, 32, 32, 3), dtype=np.uint8))
    return models, folded, u8, netfix.state_dict(z)


def _fp32(model, u8):
    from qconvnet.qmodel import normalized_input
    return normalized_input(u8, model.device, model.ntab)


def _same(a, b):
    assert list(a) == list(b)
    for name in a:
        for k, v in a[name].items():
            if k == "tensor":
                for kk, vv in v.items():
                    assert np.array_equal(vv, b[name]["tensor"][kk], equal_nan=True), (name, kk)
            else:
                assert np.array_equal(v, b[name][k], equal_nan=True), (name, k)


@pytest.mark.parametrize("mode", ("static", "qdq"))
@pytest.mark.parametrize("count", (6, 9))
def test_layer_report_matches_restatement(dev, net, mode, count, monkeypatch):
    """layer_report against the restatement applied to the very tensors
    layer_pairs yielded to it, copied to the host as they pass.  Every layer's
    SQNR (the channels combined) is finite; a single channel's may be nan — a
    ReLU output that is zero on every image, with every code on the zero point
    (2 to 7 of fc1's 512 channels on these images)."""
    from qconvnet import qerror
    from qconvnet.qerror import layer_names, layer_report, summarize
    models, folded, u8, _ = net
    m = models[mode]
    x = _fp32(m, u8[:count])
    before = m.run(x).clone()
    seen = []
    pairs = qerror.layer_pairs

    def recording(*args, **kw):
        for item in pairs(*args, **kw):
            name, xf, q, scale, zp, nhwc = item
            seen.append((name, xf.cpu().numpy(), q.cpu().numpy(), scale, zp, nhwc))
            yield item

    monkeypatch.setattr(qerror, "layer_pairs", recording)
    report = layer_report(m, folded, x, batch=6)
    names = ["x"] + [f"conv{i}" for i in range(1, 7)] + ["fc1"] + (["fc2"] if mode == "static" else [])
    assert list(report) == names == layer_names(mode)
    assert [s[0] for s in seen] == names * (-(-count // 6))
    ref = {}
    for name, xh, qh, scale, zp, nhwc in seen:
        assert nhwc
        if qh.ndim == 4:
            qh = qh.transpose(0, 3, 1, 2)
        assert qh.shape == xh.shape
        c, s = R.stats(xh, qh, scale, zp)
        pc, ps = ref.get(name, (0, 0))
        mx = np.maximum(c[:, 4], pc[:, 4]) if name in ref else c[:, 4]
        c = c + pc
        c[:, 4] = mx
        ref[name] = (c, s + ps)
    for name in names:
        got, (c, s) = report[name], ref[name]
        want = summarize(c, s)
        for k in ("count", "below", "above", "differ", "max_abs_err"):
            assert np.array_equal(got[k], want[k]), (name, k)
            assert got["tensor"][k] == want["tensor"][k], (name, k)
        n_c = int(c[0, 0])
        for k in ("sum_x2", "sum_e2", "sum_abs_e"):
            assert R.close(got[k], want[k], n_c), (name, k)
        print(mode, count, name, "sqnr", got["tensor"]["sqnr_db"], "non-finite channels",
              int((~np.isfinite(got["sqnr_db"])).sum()))
        assert np.isfinite(got["tensor"]["sqnr_db"]), name
        assert got["tensor"]["count"] == want["tensor"]["count"] == c[:, 0].sum()
    assert not report["x"]["differ"].any()
    assert torch.equal(m.run(x), before)


@pytest.mark.parametrize("mode", ("static", "qdq"))
def test_u8_images_give_the_same_report(dev, net, mode):
    from qconvnet.qerror import layer_report
    models, folded, u8, _ = net
    m = models[mode]
    _same(layer_report(m, folded, u8[:6], batch=6), layer_report(m, folded, _fp32(m, u8[:6]), batch=6))


def test_model_surface(dev, net):
    from models.custom_quantization_model import CustomQuantizationModel
    from models.static_ptq_model import StaticPTQModel
    from qconvnet import data
    from qconvnet.qerror import layer_report
    from qconvnet.qmodel import fold_state_dict
    _, _, u8, sd = net
    for cls, mode in ((StaticPTQModel, "static"), (CustomQuantizationModel, "qdq")):
        m = cls()
        m.load_state_dict(sd)
        with pytest.raises(RuntimeError):
            m.quantization_report(u8[:6])
        qm = m.quantize(data.SyntheticLoader(32, 32, seed=1), calibration_device="cuda")
        assert qm.mode == mode
        fp = m.fp32_model if mode == "static" else m.model
        got = m.quantization_report(u8[:6], batch=6)
        _same(got, layer_report(qm, fold_state_dict(fp.state_dict()), u8[:6], batch=6))
        assert got["x"]["tensor"]["count"] == 6 * 3 * 32 * 32
