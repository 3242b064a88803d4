"""GPU: qcn_qerror_f32_f32 and what is built on it (ops.qerror_f32,
qerror.FloatErrorStats) against the numpy restatement in cmpref.py.

counts are compared for equality in every field, the bit pattern of the max
included.  The sums' bounds are derived, not measured (cmpref.close): the
terms are identical in both (every operation is the same IEEE operation and
nothing is contracted), only the order of the N_c additions differs, which
costs at most (N_c - 1) * 2^-53 per side relative to the sum of the terms'
magnitudes.  So sum x^2, sum e^2 and sum |e| (non-negative terms) lie within
relative 4 * N_c * 2^-53, a zero on one side a zero on the other, and the
signed sum e within absolute 4 * N_c * 2^-53 * sum |e|.

Inputs (cmpref.make_case): x ~ N(0, 1); y = x + N(0, 0.05) with 10 % of the
elements set equal to x; with three channels or more one channel wholly equal
and one with x = 0 and y != 0.  Asserted on the restatement alone, for every
shape of at least 500 elements, before the device is asked: differ lies
strictly between 5 % and 95 % of the tensor."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmpref as R

pytestmark = pytest.mark.gpu

SLICES, TILE = 512, 4096   # qcn::kQerrSlices, qcn::kQerrTile
# one image more than SLICES tiles' worth of pixels of a 64-channel group, so
# some workgroups walk two tiles
OVER_CAP = (SLICES * (TILE // 64) // (32 * 32) + 1, 64, 32, 32)
SHAPES = ((3, 5, 3, 7), (1, 3, 32, 32), (2, 64, 16, 16), (2, 257, 2, 2), (130, 10, 1, 1),
          (5, 512, 1, 1), (1, 1, 1, 1), (4, 1, 9, 9), OVER_CAP)
assert OVER_CAP == (33, 64, 32, 32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


_CASES = {}


def _case(shape):
    """(x NCHW, y NCHW, counts, sums), made once per shape."""
    if shape not in _CASES:
        x, y = R.make_case(np.random.default_rng(8000 + SHAPES.index(shape)), shape)
        counts, sums = R.stats(x, y)
        for a in (x, y, counts, sums):
            a.setflags(write=False)
        _CASES[shape] = (x, y, counts, sums)
    return _CASES[shape]


def _place(a, dev, offset):
    """A device copy of ``a`` that starts ``offset`` elements into its allocation."""
    t = torch.from_numpy(np.array(a))
    flat = torch.zeros(t.numel() + offset, dtype=t.dtype, device=dev)
    flat[offset:] = t.to(dev).reshape(-1)
    return flat[offset:].view(t.shape)


def _run(dev, x, y_nchw, nhwc, offset=False, bufs=None):
    from qconvnet import ops
    c = x.shape[1]
    y = np.ascontiguousarray(y_nchw.transpose(0, 2, 3, 1)) if nhwc else y_nchw
    xd = _place(x, dev, 1 if offset else 0)     # 4 bytes in
    yd = _place(y, dev, 1 if offset else 0)
    if offset:
        assert xd.data_ptr() % 16 == 4 and yd.data_ptr() % 16 == 4
    counts, sums = bufs if bufs is not None else ops.qerror_f32_buffers(c, dev)
    ops.qerror_f32(xd, yd, counts, sums, nhwc=nhwc)
    return counts, sums


def test_inputs_cover_every_field():
    for shape in SHAPES:
        x, y, counts, sums = _case(shape)
        if shape[1] >= 3:
            assert counts[-1, 1] == 0 and counts[-1, 2] == 0         # a channel wholly equal
            assert sums[0, 0] == 0 and counts[0, 1] == counts[0, 0]  # a channel with x = 0, y != 0
        if x.size < 500:
            continue
        frac = counts[:, 1].sum() / counts[:, 0].sum()
        assert 0.05 < frac < 0.95, (shape, frac)


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("nhwc", (0, 1), ids=("nchw", "nhwc"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_restatement(dev, shape, nhwc, offset):
    x, y, rc, rs = _case(shape)
    counts, sums = _run(dev, x, y, nhwc, offset)
    counts, sums = counts.cpu().numpy(), sums.cpu().numpy()
    n_c = x.size // shape[1]
    rel, sgn, bound = R.excess(sums, rs, n_c)
    print(shape, nhwc, offset, "max rel", rel, "max |d sum e| / sum |e|", sgn, "bound", bound)
    assert np.array_equal(counts, rc)
    assert R.close(sums, rs, n_c)


@pytest.mark.parametrize("nhwc", (0, 1), ids=("nchw", "nhwc"))
@pytest.mark.parametrize("shape", ((37, 5, 3, 7), (130, 10, 1, 1)), ids=("tile", "direct"))
def test_ragged_slices_accumulate(dev, shape, nhwc):
    from qconvnet import ops
    x, y = R.make_case(np.random.default_rng(5), shape)
    whole_c, whole_s = _run(dev, x, y, nhwc)
    bufs = ops.qerror_f32_buffers(shape[1], dev)
    cut = (0, 1, shape[0] // 3 + 2, shape[0])
    for a, b in zip(cut[:-1], cut[1:]):
        _run(dev, x[a:b], y[a:b], nhwc, bufs=bufs)
    n_c = x.size // shape[1]
    assert np.array_equal(bufs[0].cpu().numpy(), whole_c.cpu().numpy())
    assert R.close(bufs[1].cpu().numpy(), whole_s.cpu().numpy(), n_c)
    rc, rs = R.stats(x, y)
    assert np.array_equal(bufs[0].cpu().numpy(), rc)
    assert R.close(bufs[1].cpu().numpy(), rs, n_c)


@pytest.mark.parametrize("nhwc", (0, 1), ids=("nchw", "nhwc"))
@pytest.mark.parametrize("shape", ((2, 64, 16, 16), OVER_CAP, (5, 512, 1, 1)),
                         ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bit_identical(dev, shape, nhwc):
    x, y, _, _ = _case(shape)
    a = _run(dev, x, y, nhwc)
    b = _run(dev, x, y, nhwc)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))


@pytest.mark.parametrize("shape", ((2, 64, 16, 16), (3, 5, 3, 7), (130, 10, 1, 1)),
                         ids=lambda s: "x".join(map(str, s)))
def test_equal_input_has_no_error(dev, shape):
    from qconvnet.qerror import summarize_f32
    x, _, _, _ = _case(shape)
    x = np.array(x)
    x[:, 0] = 1.0       # (the recipe's zero channel would have no signal either)
    for nhwc in (0, 1):
        counts, sums = _run(dev, x, x, nhwc)
        r = summarize_f32(counts.cpu().numpy(), sums.cpu().numpy())
        assert not r["sum_e2"].any() and not r["sum_abs_e"].any() and not r["sum_e"].any()
        assert not r["differ"].any() and not r["max_abs_err"].any()
        assert (r["count"] == x.size // shape[1]).all()
        assert (r["sqnr_db"] == np.inf).all() and r["tensor"]["sqnr_db"] == np.inf


def test_signed_zero_is_equal(dev):
    x = np.zeros((2, 3, 4, 4), np.float32)
    y = np.full((2, 3, 4, 4), -0.0, np.float32)
    counts, sums = _run(dev, x, y, 1)
    assert not counts.cpu().numpy()[:, 1:].any() and not sums.cpu().numpy().any()


def test_no_rows_leaves_the_buffers_untouched(dev):
    from qconvnet import _lib, ops
    counts, sums = ops.qerror_f32_buffers(4, dev)
    counts.fill_(7)
    sums.fill_(1.5)
    x = torch.zeros((0, 4, 3, 3), dtype=torch.float32, device=dev)
    y = torch.zeros((0, 3, 3, 4), dtype=torch.float32, device=dev)
    ops.qerror_f32(x, y, counts, sums)
    # and the entry itself, with real addresses
    keep = torch.zeros(64, dtype=torch.uint8, device=dev)
    rc = _lib.load().qcn_qerror_f32_f32(C.c_void_p(keep.data_ptr()), C.c_void_p(keep.data_ptr()), 0, 4,
                                        3, 3, 1, C.c_void_p(counts.data_ptr()),
                                        C.c_void_p(sums.data_ptr()), C.c_void_p(keep.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert (counts == 7).all() and (sums == 1.5).all()


def test_stats_object_one_copy(dev):
    from qconvnet.qerror import FloatErrorStats, summarize_f32
    shape = (3, 5, 3, 7)
    x, y, rc, rs = _case(shape)
    st = FloatErrorStats(5, dev)
    xd = torch.from_numpy(np.array(x)).to(dev)
    yd = torch.from_numpy(np.ascontiguousarray(y.transpose(0, 2, 3, 1))).to(dev)
    st.update(xd, yd).update(xd, yd)
    r = st.result()
    ref = summarize_f32(2 * rc * np.array([1, 1, 0]) + rc * np.array([0, 0, 1]), 2 * rs)
    for k in ("count", "differ", "max_abs_err"):
        assert np.array_equal(r[k], ref[k]), k
    assert R.close(np.stack([r[k] for k in ("sum_x2", "sum_e2", "sum_abs_e", "sum_e")], 1),
                   2 * rs, 2 * x.size // shape[1])
    assert st.reset().result()["tensor"]["count"] == 0
    with pytest.raises(ValueError):
        st.update(xd[:, :4], yd[..., :4])
