"""CPU: the constructions of tests/dynconv.py do what they claim, shown with
oracle.qref alone at the shapes test_gpu_conv_dyn_edges.py runs: the tie sets
hold exact ties that a half-away rounding would turn into other accumulators,
the input classes reach the qparams branches they are there for, and the
deep-K case drives the int32 accumulator to its extreme inside the bound."""
import numpy as np
import pytest
import torch

import dynconv as D
import opedge as E
from oracle import qref

F32 = np.float32


def qparams(xi, rr=False):
    return qref.choose_qparams_dynamic(xi.min(), xi.max(), reduce_range=rr)


# ------------------------------------------------------------------ input ties
@pytest.mark.parametrize("shift,zp", D.TIE_SHIFTS)
@pytest.mark.parametrize("shape", D.TIE_SHAPES, ids=str)
def test_input_ties(shape, shift, zp):
    n, h, w, cin, cout = shape
    x = D.tie_images(n, h, w, cin, shift, sum(shape))
    for xi in x:
        s, z = qparams(xi)
        assert E.bits(s) == E.bits(F32(1.0)) and z == zp
        assert D.tie_share(xi, s, z) >= 0.25
        codes, away = qref.quantize_legacy_fma(xi, s, z), D.quantize_half_away(xi, s, z)
        assert {0, 255} <= set(np.unique(codes)) and np.mean(codes != away) >= 0.15
    wq = np.random.default_rng(sum(shape)).integers(-128, 128, (cout, cin, 3, 3), dtype=np.int8)
    acc = D.acc_with(qref.quantize_legacy_fma, x, wq)
    assert E.distinct_ok(acc)
    assert np.mean(acc != D.acc_with(D.quantize_half_away, x, wq)) >= 0.10


# -------------------------------------------------------------------- mid ties
def mid_of(x, wa):
    """Layer A of the mid-tie case in float32: fmaf(acc, s_x * s_w, 0)."""
    ohwi = np.ascontiguousarray(wa.transpose(0, 2, 3, 1))
    out = []
    for xi in x:
        s, z = qparams(xi)
        a = qref.conv3x3_acc_nhwc(qref.quantize_legacy_fma(xi, s, z)[None], z, ohwi)[0].astype(F32)
        out.append(qref.fmaf(a, np.full(a.shape, F32(s) * D.MID_S_W[0], F32), np.zeros(a.shape, F32)))
    return np.stack(out)


@pytest.mark.parametrize("name", D.MID_MAPS)
def test_mid_ties(name):
    h, w = D.MID_MAPS[name]
    x, wa, wb = D.mid_tie_case(h, w, h + w)
    for xi in x:
        assert qparams(xi) == (F32(1.0), 0)
    mid = mid_of(x, wa)
    assert np.array_equal(mid[..., 0], x[..., 0] / 2) and np.array_equal(mid[..., 1:], x[..., 1:] / 8)
    for mi in mid:
        s, z = qparams(mi)
        assert E.bits(s) == E.bits(F32(0.5)) and z == 0
        assert D.tie_share(mi, s, z) >= 0.10
    acc = D.acc_with(qref.quantize_legacy_fma, mid, wb)
    assert E.distinct_ok(acc)
    assert np.mean(acc != D.acc_with(D.quantize_half_away, mid, wb)) >= 0.10


# --------------------------------------------------------------------- classes
def test_small_takes_the_floor_branch():
    h, w, c = D.CLASS_SHAPE[:3]
    for seed in range(40, 43):
        x = D.class_image("small", h, w, c, seed)
        assert x.min() < 0 < x.max()
        for rr in (False, True):
            s, z = qparams(x, rr)
            ts, tz = torch._choose_qparams_per_tensor(torch.from_numpy(x), rr)
            assert (float(s), z) == (float(F32(ts)), int(tz))
            # the scale before the floor is below it: the range is amplified, both ends non-zero
            assert (float(x.max()) - float(x.min())) / (127 if rr else 255) < float(D.SMALL_SCALE)
            assert E.bits(s) == E.bits(D.SMALL_SCALE)
            assert np.unique(qref.quantize_legacy_fma(x, s, z)).size > 8


@pytest.mark.parametrize("name", D.BATCHES)
def test_class_batches(name):
    """The classes whose every element quantizes to the zero point are exactly
    SINGLE_CODE; every other image gives non-degenerate accumulators;
    "positive" has its range extended to 0."""
    h, w, cin, cmid, _ = D.CLASS_SHAPE
    kinds = D.BATCHES[name]
    x = D.class_batch(kinds, h, w, cin, 40)
    wq = np.random.default_rng(40).integers(-128, 128, (cmid, cin, 3, 3), dtype=np.int8)
    acc = D.acc_with(qref.quantize_legacy_fma, x, wq)
    for kind, xi, ai in zip(kinds, x, acc):
        s, z = qparams(xi)
        only_zp = bool((qref.quantize_legacy_fma(xi, s, z) == z).all())
        assert only_zp == (kind in D.SINGLE_CODE), kind
        assert E.distinct_ok(ai) != (kind in D.SINGLE_CODE), kind
        if kind in D.SINGLE_CODE:
            assert not ai.any(), kind
        if kind == "positive":
            assert xi.min() > 0 and z == 0 and E.bits(s) == E.bits(F32(float(xi.max()) / 255))
    if name == "mixed":
        scales = np.array([float(qparams(xi)[0]) for xi in x])
        assert set(kinds) == set(E.DYN_CLASSES) | {"small"} and scales.max() / scales.min() > 1e30


# --------------------------------------------------------------------- deep K
def test_deep_k_reaches_the_accumulator_bound():
    x, wq = D.deep_k_case(3)
    assert x.shape == (3, 3, 3, D.DEEP_CIN) and D.DEEP_PEAK == 9 * 7310 * 255 * 127 < 2 ** 31
    assert 9 * (D.DEEP_CIN + 1) * 255 * 128 > 2 ** 31 - 1      # and it is the bound of csrc/conv_dyn.hpp
    assert [qparams(xi)[1] for xi in x] == [0, 0, 255]
    for xi in x:
        assert set(np.unique(qref.quantize_legacy_fma(xi, *qparams(xi)))) <= {0, 255}
    acc = D.acc_with(qref.quantize_legacy_fma, x, wq).astype(np.int64)
    assert acc.max() == D.DEEP_PEAK == -acc.min()
    assert acc[0, 1, 1, 0] == D.DEEP_PEAK and acc[2, 1, 1, 0] == -D.DEEP_PEAK    # the centre pixel, all nine taps


# ---------------------------------------------------------------- image_minmax
@pytest.mark.parametrize("count", D.MINMAX_COUNTS)
def test_minmax_extremes_sit_at_the_ends(count):
    x = D.minmax_images(count, count)
    assert x[0].argmax() == 0 and x[0].argmin() == count - 1
    assert x[1].argmin() == 0 and x[1].argmax() == count - 1
    assert x[2].argmax() == count - 1 and (count % 4 < 2 or x[2].argmin() == count - count % 4)
    assert np.abs(x[3]).max() < 100
