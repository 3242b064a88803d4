"""CPU: the numpy restatement of the quantization-error statistics
(qerrref.py) against torch, qconvnet.qerror.summarize on hand-made counts, and
the host half of the C ABI (argument checks, workspace size) — no device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import qerrref as R


@pytest.mark.parametrize("scale,zp", R.QPARAMS)
def test_qref_is_quantize_per_tensor(scale, zp):
    """Odd and even zero points; 512 inputs sit at or next to a tie (x * inv near k + 0.5)."""
    rng = np.random.default_rng(zp)
    x, _ = R.make_case(rng, (4096,), scale, zp)
    x[:512] = (np.float32(scale) * (np.arange(512, dtype=np.float32) - 128.5)).astype(np.float32)
    ref = torch.quantize_per_tensor(torch.from_numpy(x), scale, zp, torch.quint8).int_repr().numpy()
    assert np.array_equal(R.qref(x, scale, zp), ref)


@pytest.mark.parametrize("count", (1, 37, 1024, 4096))
@pytest.mark.parametrize("scale,zp", R.QPARAMS)
def test_sqnr_is_compute_sqnr(count, scale, zp):
    """Within 0.01 dB at <= 4,096 elements: torch's fp32 norms carry a relative
    error of at most about n * 2^-24 ~ 2.4e-4, i.e. 2e-3 dB; 0.01 dB is x5."""
    from torch.ao.ns.fx.utils import compute_sqnr
    rng = np.random.default_rng(100 * zp + count)
    x, q = R.make_case(rng, (count,), scale, zp)
    d = torch.from_numpy(R.dequant(q, scale, zp))
    ref = float(compute_sqnr(torch.from_numpy(x), d))
    got = R.sqnr_db(x, q, scale, zp)
    assert abs(got - ref) <= 0.01, (got, ref)


def test_summarize_fields_and_special_cases():
    from qconvnet.qerror import DERIVED, RAW, summarize
    bits = lambda v: int(np.float32(v).view(np.uint32))
    counts = np.array([[10, 1, 2, 3, bits(0.5)],     # ordinary
                       [10, 0, 0, 0, bits(0.0)],     # no error: +inf
                       [10, 0, 0, 4, bits(0.25)],    # no signal: -inf
                       [10, 0, 0, 0, bits(0.0)]],    # neither: nan
                      np.int64)
    sums = np.array([[100.0, 1.0, 2.0], [50.0, 0.0, 0.0], [0.0, 4.0, 5.0], [0.0, 0.0, 0.0]])
    r = summarize(counts, sums)
    assert set(RAW) | set(DERIVED) | {"tensor"} == set(r)
    assert np.array_equal(r["count"], [10, 10, 10, 10])
    assert np.array_equal(r["below"], [1, 0, 0, 0]) and np.array_equal(r["above"], [2, 0, 0, 0])
    assert np.array_equal(r["differ"], [3, 0, 4, 0])
    assert r["max_abs_err"].dtype == np.float32
    assert np.array_equal(r["max_abs_err"], np.array([0.5, 0, 0.25, 0], np.float32))
    assert np.array_equal(r["sum_x2"], sums[:, 0]) and np.array_equal(r["sum_e2"], sums[:, 1])
    assert np.array_equal(r["sum_abs_e"], sums[:, 2])
    assert r["sqnr_db"][0] == 10.0 * np.log10(100.0)
    assert r["sqnr_db"][1] == np.inf and r["sqnr_db"][2] == -np.inf and np.isnan(r["sqnr_db"][3])
    assert np.array_equal(r["mse"], sums[:, 1] / 10) and np.array_equal(r["mean_abs_err"], sums[:, 2] / 10)
    assert np.array_equal(r["below_frac"], [0.1, 0, 0, 0]) and np.array_equal(r["above_frac"], [0.2, 0, 0, 0])
    assert np.array_equal(r["differ_frac"], [0.3, 0, 0.4, 0])
    t = r["tensor"]
    assert set(RAW) | set(DERIVED) == set(t)
    assert (t["count"], t["below"], t["above"], t["differ"]) == (40, 1, 2, 7)
    assert t["max_abs_err"] == np.float32(0.5)
    assert (t["sum_x2"], t["sum_e2"], t["sum_abs_e"]) == (150.0, 5.0, 7.0)
    assert t["sqnr_db"] == 10.0 * np.log10(150.0 / 5.0)
    assert t["mse"] == 5.0 / 40 and t["mean_abs_err"] == 7.0 / 40 and t["differ_frac"] == 7 / 40
    # combined special cases
    assert summarize(counts[1:2], sums[1:2])["tensor"]["sqnr_db"] == np.inf
    assert summarize(counts[2:3], sums[2:3])["tensor"]["sqnr_db"] == -np.inf
    assert np.isnan(summarize(counts[3:4], sums[3:4])["tensor"]["sqnr_db"])


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
    q = np.zeros(8, np.uint8)
    counts = np.zeros(5, np.int64)
    sums = np.zeros(3, np.float64)
    ws = np.zeros(64, np.float64)
    P = lambda a: C.c_void_p(a.ctypes.data)

    def call(x=x, q=q, n=1, c=1, h=2, w=2, scale=0.1, zp=3, counts=counts, sums=sums, ws=ws):
        return lib.qcn_qerror_u8_f32(P(x) if x is not None else None, P(q) if q is not None else None,
                                     n, c, h, w, 1, C.c_float(scale), zp,
                                     P(counts) if counts is not None else None,
                                     P(sums) if sums is not None else None,
                                     P(ws) if ws is not None else None, None)

    for kw in (dict(x=None), dict(q=None), dict(counts=None), dict(sums=None), dict(ws=None),
               dict(n=-1), dict(c=0), dict(h=0), dict(w=0), dict(zp=-1), dict(zp=256),
               dict(scale=0.0), dict(scale=-0.1), dict(scale=float("inf")), dict(scale=float("nan"))):
        assert call(**kw) == -1, kw
    assert call(c=1 << 20) == -2
    assert call(n=0) == 0            # nothing to launch
    assert not counts.any() and not sums.any()


def test_workspace_size(lib):
    size = lib.qcn_qerror_workspace_size
    for shape in ((-1, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert size(*shape) == -1, shape
    assert size(1, 1 << 20, 1, 1) == -2
    assert size(1 << 16, 1, 1 << 8, 1 << 8) == -2      # n * h * w >= 2^31
    assert size(0, 64, 8, 8) == 0
    # room for at least one record (3 doubles, 4 uint32) per channel, never
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
