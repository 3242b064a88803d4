"""GPU: the dynamic int8 convs (ops.conv3x3_dyn, ops.conv3x3_dyn_pair,
ops.conv3x3_dyn_pair32, ops.image_minmax) where the model's own shapes and
random inputs do not reach: exact rounding ties in the input and in the u8
hand-off, every input class of tests/dynconv.py with the ranges chained into a
following conv, every channel-group count and the deepest K the entries
accept, inputs and outputs off the 16-byte boundary, and reduce_range on the
pairs.  Everything is compared as bits with the numpy contract of
tests/test_gpu_conv_dyn.py; tests/test_conv_dyn_edges_cpu.py shows that the
inputs are the edges they claim to be."""
import itertools

import numpy as np
import pytest
import torch

import dynconv as D
import opedge as E
from oracle import qref
from test_gpu_conv_dyn import acc_ref, bits, check, dev, epilogue_ref, mixed_images, packed, run  # noqa: F401
from test_gpu_conv_dyn_pair import dyn_layer, to_dev

pytestmark = pytest.mark.gpu
F32 = np.float32
PAIR_OPS = ("conv3x3_dyn_pair", "conv3x3_dyn_pair32")


def layer_params(rng, c):
    """(per-channel scales, bias) of a layer with c output channels."""
    return rng.uniform(0.002, 0.01, c).astype(F32), rng.standard_normal(c).astype(F32)


def weights(rng, cout, cin):
    return rng.integers(-128, 128, (cout, cin, 3, 3), dtype=np.int8)


def pair_ref(x, ws, epi, pool, rr=False):
    """The contract applied twice; epi[i] = (s_w, bias, affine, relu) of layer i.
    Returns (y, mid, qparams of x, qparams of mid, B's accumulators)."""
    acc_a, ss_a, zs_a = acc_ref(x, ws[0], rr)
    mid = epilogue_ref(acc_a, ss_a, *epi[0], False)
    acc_b, ss_b, zs_b = acc_ref(mid, ws[1], rr)
    ref = epilogue_ref(acc_b, ss_b, *epi[1], pool)
    assert np.isfinite(ref).all()
    return ref, mid, (ss_a, zs_a), (ss_b, zs_b), acc_b


def single(dev, xd, st, layer, pool=False, rr=False, x_nchw=False, **kw):
    from qconvnet import ops
    return ops.conv3x3_dyn(xd, st, layer.packed, layer.wsum, layer.w_scale, layer.channels, bias=layer.bias,
                           affine=layer.affine, relu=layer.relu, pool=pool, reduce_range=rr, x_nchw=x_nchw, **kw)


def run_pair(dev, name, x, ws, epi, pool=False, rr=False, x_nchw=False):
    """The pair op ``name`` on NHWC host data -> its device results (y NHWC, y_stats,
    qparams of x, qparams of mid), after asserting that y has the bits of the two single calls."""
    from qconvnet import ops
    la, lb = (dyn_layer(dev, w, *e) for w, e in zip(ws, epi))
    xd = to_dev(dev, x.transpose(0, 3, 1, 2) if x_nchw else x)
    st = ops.image_minmax(xd)
    got = getattr(ops, name)(xd, st, la, lb, pool=pool, reduce_range=rr, x_nchw=x_nchw, qparams=True)
    t, tst = single(dev, xd, st, la, rr=rr, x_nchw=x_nchw)
    two = single(dev, t, tst, lb, pool=pool, rr=rr, want_stats=False)[0]
    assert torch.equal(bits(got[0]), bits(two)), (name, "two single calls")
    return got


def check_pair(got, ref, qa, qb, label):
    y, ys, qx, qm = got
    assert np.array_equal(E.bits(y.cpu().numpy()), E.bits(ref)), label
    for (gs, gz), (s, z) in ((qx, qa), (qm, qb)):
        assert np.array_equal(E.bits(gs.cpu().numpy()), E.bits(s)) and np.array_equal(gz.cpu().numpy(), z), label
    ys, n = ys.cpu().numpy(), len(ref)
    assert ys.shape == (n, 1, 2), label
    assert np.array_equal(ys[:, 0, 0], ref.reshape(n, -1).min(1)), label
    assert np.array_equal(ys[:, 0, 1], ref.reshape(n, -1).max(1)), label


def host(got):
    """conv3x3_dyn's device results with qparams as check() takes them."""
    y, st, qp = got
    return y.cpu().numpy(), st.cpu().numpy(), (qp[0].cpu().numpy(), qp[1].cpu().numpy())


# ----------------------------------------------------------------------- ties
@pytest.mark.parametrize("shift,zp", D.TIE_SHIFTS)
@pytest.mark.parametrize("shape", D.TIE_SHAPES, ids=str)
def test_input_ties(dev, shape, shift, zp):
    """About half of the staged values are exact k + 0.5: rounding them half
    away changes more than a tenth of the accumulators (shown on the CPU)."""
    n, h, w, cin, cout = shape
    x = D.tie_images(n, h, w, cin, shift, sum(shape))
    rng = np.random.default_rng(sum(shape))
    wq = weights(rng, cout, cin)
    s_w, bias = layer_params(rng, cout)
    acc, ss, zs = acc_ref(x, wq)
    assert np.array_equal(E.bits(ss), E.bits(np.ones(n, F32))) and list(zs) == [zp] * n and E.distinct_ok(acc)
    ref = epilogue_ref(acc, ss, s_w, bias, None, False, False)
    pk = packed(dev, wq)
    for x_nchw in (False, True):
        check(run(dev, x, pk, s_w, cout, bias, None, False, False, x_nchw), ref, (ss, zs), x_nchw)


@pytest.mark.parametrize("name", D.MID_MAPS)
def test_mid_ties(dev, name):
    """More than a tenth of the values that the pair kernels quantize in LDS are
    exact ties (s_mid = 0.5 on integers / 4)."""
    h, w = D.MID_MAPS[name]
    x, wa, wb = D.mid_tie_case(h, w, h + w)
    s_b, bias = layer_params(np.random.default_rng(h), D.MID_COUT)
    epi = [(D.MID_S_W, None, None, False), (s_b, bias, None, False)]
    ref, mid, qa, qb, acc_b = pair_ref(x, (wa, wb), epi, False)
    assert np.array_equal(E.bits(qb[0]), E.bits(np.full(len(x), 0.5, F32))) and E.distinct_ok(acc_b)
    assert min(D.tie_share(m, 0.5, 0) for m in mid) >= 0.10
    op = "conv3x3_dyn_pair32" if name == "pair32" else "conv3x3_dyn_pair"
    for x_nchw in (False, True):
        check_pair(run_pair(dev, op, x, (wa, wb), epi, x_nchw=x_nchw), ref, qa, qb, x_nchw)


# -------------------------------------------------------------------- classes
def class_forms(rng, c):
    """(bias, affine, relu) of the first layer: nothing (an all-zero image gives
    an all-zero output), ReLU alone and with a bias (zeros and the range
    [0, hi] reach the next layer), and an affine with negative slopes and -0.0
    shifts (+0.0 and -0.0 side by side in the next layer's range)."""
    bias, beta = (rng.standard_normal(c).astype(F32) for _ in range(2))
    alpha = rng.uniform(0.5, 1.5, c).astype(F32)
    alpha[1::3] *= F32(-1)
    beta[1:3] = -0.0
    return (None, None, False), (None, None, True), (bias, None, True), (None, (alpha, beta), False)


def class_case(name):
    h, w, cin, cmid, cout = D.CLASS_SHAPE
    kinds = D.BATCHES[name]
    x = D.class_batch(kinds, h, w, cin, 40)
    rng = np.random.default_rng(40)
    ws = [weights(rng, cmid, cin), weights(rng, cout, cmid), weights(rng, 8, cout)]
    par = [layer_params(rng, c) for c in (cmid, cout, 8)]
    acc = acc_ref(x, ws[0])[0]
    # the single-code classes are the only inputs allowed to give degenerate accumulators
    assert all(E.distinct_ok(a) for k, a in zip(kinds, acc) if k not in D.SINGLE_CODE)
    return x, ws, par, class_forms(rng, cmid)


@pytest.mark.parametrize("name", D.BATCHES)
def test_classes_single_chained(dev, name):
    """conv3x3_dyn on three images of a class (and on one of each), then a
    second conv3x3_dyn on its output and range slots: a degenerate range is
    written and consumed."""
    from qconvnet import ops
    x, ws, par, forms = class_case(name)
    xd = to_dev(dev, x)
    l2 = dyn_layer(dev, ws[1], par[1][0], par[1][1], None, False)
    for bias, affine, relu in forms:
        acc1, ss1, zs1 = acc_ref(x, ws[0])
        ref1 = epilogue_ref(acc1, ss1, par[0][0], bias, affine, relu, False)
        acc2, ss2, zs2 = acc_ref(ref1, ws[1])
        ref2 = epilogue_ref(acc2, ss2, par[1][0], par[1][1], None, False, False)
        assert np.isfinite(ref2).all()
        if affine is not None and "zero" in D.BATCHES[name]:
            z0 = E.bits(ref1[D.BATCHES[name].index("zero")])
            assert (z0 == 0x80000000).any() and (z0 == 0).any()      # -0.0 and +0.0 in one image's range
        l1 = dyn_layer(dev, ws[0], par[0][0], bias, affine, relu)
        got1 = single(dev, xd, ops.image_minmax(xd), l1, qparams=True)
        got2 = single(dev, got1[0], got1[1], l2, qparams=True)
        label = (bias is not None, affine is not None, relu)
        check(host(got1), ref1, (ss1, zs1), label + (1,))
        check(host(got2), ref2, (ss2, zs2), label + (2,))


@pytest.mark.parametrize("op", PAIR_OPS)
@pytest.mark.parametrize("name", D.BATCHES)
def test_classes_pairs_chained(dev, name, op):
    """The same batches through the pair kernels (the mid range is reduced and
    consumed in LDS), then a conv3x3_dyn on the pair's output and its one slot."""
    x, ws, par, forms = class_case(name)
    l3 = dyn_layer(dev, ws[2], par[2][0], par[2][1], None, False)
    for bias, affine, relu in forms:
        epi = [(par[0][0], bias, affine, relu), (par[1][0], par[1][1], None, relu)]
        ref, _, qa, qb, _ = pair_ref(x, ws[:2], epi, False)
        acc3, ss3, zs3 = acc_ref(ref, ws[2])
        ref3 = epilogue_ref(acc3, ss3, par[2][0], par[2][1], None, False, False)
        assert np.isfinite(ref3).all()
        got = run_pair(dev, op, x, ws[:2], epi)
        label = (bias is not None, affine is not None, relu)
        check_pair(got, ref, qa, qb, label)
        check(host(single(dev, got[0], got[1], l3, qparams=True)), ref3, (ss3, zs3), label + (3,))


# -------------------------------------------------------------------- K depth
# cin of conv3x3_dyn: 5, 6, 7, 9, 11, 13 and 15 channel groups in one chunk on a 3 x 5 map; two full
# chunks, two and a group, three and a group on 2 x 2
SINGLE_K = [(3, 5, c) for c in (80, 96, 112, 144, 176, 208, 240)] + [(2, 2, c) for c in (512, 528, 784)]


def check_single_k(dev, x, wq, rng):
    cout = wq.shape[0]
    s_w, bias = layer_params(rng, cout)
    acc, ss, zs = acc_ref(x, wq)
    ref = epilogue_ref(acc, ss, s_w, bias, None, False, False)
    assert np.isfinite(ref).all() and E.distinct_ok(acc)
    pk = packed(dev, wq)
    for x_nchw in (False, True):
        check(run(dev, x, pk, s_w, cout, bias, None, False, False, x_nchw), ref, (ss, zs), x_nchw)
    return acc


@pytest.mark.parametrize("h,w,cin", SINGLE_K)
def test_single_k_depth(dev, h, w, cin):
    rng = np.random.default_rng(cin)
    check_single_k(dev, mixed_images(3, h, w, cin, cin), weights(rng, 20, cin), rng)


def test_single_deepest_k_full_range(dev):
    """cin = 7310 (29 chunks), codes 0 and 255, weights +-127: the centre pixel's
    accumulators are +-9 * 7310 * 255 * 127, the extreme the entries accept."""
    x, wq = D.deep_k_case(3)
    acc = check_single_k(dev, x, wq, np.random.default_rng(1)).astype(np.int64)
    assert acc.max() == D.DEEP_PEAK == -acc.min()


# (h, w, cin, cmid) of conv3x3_dyn_pair, cout = 20: 2, 3, 6, 7, 9, 13 and 15 channel groups of cmid in
# the 4-wave class; two full chunks and three chunks and a group of cin
PAIR_K = [(5, 7, 20, c) for c in (17, 40, 96, 112, 144, 208, 240)] + [(2, 2, c, 24) for c in (512, 784)]
# (cin, cmid) of conv3x3_dyn_pair32 on a 9 x 10 map: 3 groups of cin, 2 and 3 of cmid
PAIR32_K = [(48, 17), (33, 32), (64, 48)]


def check_pair_k(dev, op, x, ws, rng):
    epi = [layer_params(rng, w.shape[0]) + (None, False) for w in ws]
    ref, _, qa, qb, acc_b = pair_ref(x, ws, epi, False)
    assert E.distinct_ok(acc_b)
    check_pair(run_pair(dev, op, x, ws, epi), ref, qa, qb, op)


@pytest.mark.parametrize("h,w,cin,cmid", PAIR_K)
def test_pair_k_depth(dev, h, w, cin, cmid):
    rng = np.random.default_rng(cin + cmid)
    check_pair_k(dev, "conv3x3_dyn_pair", mixed_images(3, h, w, cin, cin + cmid),
                 (weights(rng, cmid, cin), weights(rng, 20, cmid)), rng)


def test_pair_deepest_k_full_range(dev):
    """The cin = 7310 full-range case as layer A (cmid = 4) of the pair."""
    x, wa = D.deep_k_case(4)
    rng = np.random.default_rng(2)
    check_pair_k(dev, "conv3x3_dyn_pair", x, (wa, weights(rng, 5, 4)), rng)


@pytest.mark.parametrize("cin,cmid", PAIR32_K)
def test_pair32_k_depth(dev, cin, cmid):
    rng = np.random.default_rng(cin + cmid)
    check_pair_k(dev, "conv3x3_dyn_pair32", mixed_images(3, 9, 10, cin, cin + cmid),
                 (weights(rng, cmid, cin), weights(rng, 20, cmid)), rng)


# ------------------------------------------------------------------ alignment
OFFSETS = [(ox, oy) for ox, oy in itertools.product(range(4), range(4)) if ox == 0 or oy == 0 or ox == oy][1:]


def at_offset(dev, shape, off, src=None):
    """A contiguous fp32 device tensor that starts ``off`` floats past a 16-byte boundary."""
    n = int(np.prod(shape))
    buf = torch.zeros(n + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v if src is None else v.copy_(src)


def flat_bits(*ts):
    return torch.cat([bits(t).reshape(-1) for t in ts])


def test_alignment_single(dev):
    """NHWC with cin % 4 == 0 off the 16-byte boundary (the scalar staging loads
    where the aligned call takes float4) and y off it: the aligned call's bits."""
    from qconvnet import ops
    n, h, w, cin, cout = 2, 5, 7, 24, 20
    rng = np.random.default_rng(5)
    x, wq = mixed_images(n, h, w, cin, 5), weights(rng, cout, cin)
    s_w, bias = layer_params(rng, cout)
    acc, ss, zs = acc_ref(x, wq)
    layer = dyn_layer(dev, wq, s_w, bias, None, True)
    xd = to_dev(dev, x)
    base = single(dev, xd, ops.image_minmax(xd), layer, qparams=True)
    check(host(base), epilogue_ref(acc, ss, s_w, bias, None, True, False), (ss, zs), "aligned")
    for ox, oy in OFFSETS:
        xo = at_offset(dev, xd.shape, ox, xd)
        y, st, qp = single(dev, xo, ops.image_minmax(xo), layer, qparams=True, out=at_offset(dev, base[0].shape, oy))
        assert y.data_ptr() % 16 == 4 * oy
        assert torch.equal(flat_bits(y, st, *qp), flat_bits(base[0], base[1], *base[2])), (ox, oy)


@pytest.mark.parametrize("op,h,w", [("conv3x3_dyn_pair", 5, 7), ("conv3x3_dyn_pair", 10, 12),
                                    ("conv3x3_dyn_pair32", 18, 9)])
def test_alignment_pairs(dev, op, h, w):
    from qconvnet import ops
    n, cin, cmid, cout = 2, 24, 20, 12
    rng = np.random.default_rng(h)
    x, ws = mixed_images(n, h, w, cin, h), (weights(rng, cmid, cin), weights(rng, cout, cmid))
    epi = [layer_params(rng, c) + (None, True) for c in (cmid, cout)]
    ref, _, qa, qb, _ = pair_ref(x, ws, epi, False)
    base = run_pair(dev, op, x, ws, epi)
    check_pair(base, ref, qa, qb, "aligned")
    la, lb = (dyn_layer(dev, wq, *e) for wq, e in zip(ws, epi))
    xd = to_dev(dev, x)
    for ox, oy in OFFSETS:
        xo = at_offset(dev, xd.shape, ox, xd)
        y, ys, qx, qm = getattr(ops, op)(xo, ops.image_minmax(xo), la, lb, qparams=True,
                                         out=at_offset(dev, base[0].shape, oy))
        assert y.data_ptr() % 16 == 4 * oy
        assert torch.equal(flat_bits(y, ys, *qx, *qm), flat_bits(base[0], base[1], *base[2], *base[3])), (ox, oy)


@pytest.mark.parametrize("count", D.MINMAX_COUNTS)
def test_image_minmax_strided_loop(dev, count):
    """More than 256 elements per image with a count % 4 tail, from aligned and
    offset bases (count 1024: the float4 kernel aligned, the scalar one else),
    extremes in the first element and in the tail, against numpy."""
    from qconvnet import ops
    x = D.minmax_images(count, count)
    shape = (4, 7, 7, 7) if count == 343 else (4, count)
    ref = np.stack([x.min(1), x.max(1)], 1).reshape(4, 1, 2)
    for off in range(4):
        got = ops.image_minmax(at_offset(dev, shape, off, to_dev(dev, x.reshape(shape))))
        assert np.array_equal(E.bits(got.cpu().numpy()), E.bits(ref)), off


# --------------------------------------------------------------- reduce_range
@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("op,h,w", [("conv3x3_dyn_pair", 6, 8), ("conv3x3_dyn_pair", 10, 12),
                                    ("conv3x3_dyn_pair32", 18, 10)])
def test_reduce_range_pairs(dev, op, h, w, pool):
    """reduce_range=True quantizes x and the mid hand-off to [0, 127]."""
    cin, cmid, cout = 20, 24, 20
    rng = np.random.default_rng(h + w)
    x, ws = mixed_images(5, h, w, cin, h + w), (weights(rng, cmid, cin), weights(rng, cout, cmid))
    epi = [layer_params(rng, c) + (None, True) for c in (cmid, cout)]
    ref, mid, qa, qb, acc_b = pair_ref(x, ws, epi, pool, rr=True)
    assert qa[1].max() <= 127 and qb[1].max() <= 127 and E.distinct_ok(acc_b)
    assert max(qref.quantize_legacy_fma(m, s, z).max() for m, s, z in zip(mid, *qb)) <= 127
    got = run_pair(dev, op, x, ws, epi, pool=pool, rr=True)
    check_pair(got, ref, qa, qb, (op, pool))
    assert int(got[2][1].max()) <= 127 and int(got[3][1].max()) <= 127
