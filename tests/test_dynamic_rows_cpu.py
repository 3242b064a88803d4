"""CPU: the reference of the per-sample dynamic Linear (dynrows.rows_ref, the
row-by-row qref.linear_dynamic) pinned against torch's dynamic Linear run on
each [1, k] row, the conditions on it that test_gpu_dynamic_rows.py relies on,
and the ``granularity`` argument's errors.  Everything is compared as bits."""
import numpy as np
import pytest
import torch

import dynrows as D
import opedge as E
from oracle import qref
from test_op_edges_cpu import _torch_dynamic_linear


@pytest.mark.parametrize("m,k,n", D.SHAPES)
def test_rows_ref_matches_torch_row_by_row(m, k, n):
    torch.backends.quantized.engine = "fbgemm"
    x, w, s_pt, s_pc, b = D.case(m, k, n)
    for s_w, pc in ((s_pt, False), (s_pc, True)):
        for bias in (b, None):
            got = D.rows_ref(x, w, s_w, bias)
            want = np.concatenate([_torch_dynamic_linear(x[i:i + 1], w, s_w, bias, pc) for i in range(m)])
            assert np.array_equal(E.bits(got), E.bits(want)), (pc, bias is None)


@pytest.mark.parametrize("m,k,n", D.SHAPES)
def test_reference_output_conditions(m, k, n):
    """Finite, not degenerate, and (m >= 2: rows 0 and 1 are "normal" and
    "huge") different from the per-batch form in at least one row — what lets
    the GPU test tell the two forms apart."""
    x, w, s_pt, s_pc, b = D.case(m, k, n)
    for s_w in (s_pt, s_pc):
        for bias in (b, None):
            for rr in (True, False):
                y = D.rows_ref(x, w, s_w, bias, rr)
                assert np.isfinite(y).all()
                assert E.distinct_ok(y)
                if m >= 2:
                    batch = qref.linear_dynamic(x, w, s_w, bias, reduce_range=rr)
                    assert (E.bits(y) != E.bits(batch)).any(axis=1).any()


def test_rows_qparams_differ_by_orders_of_magnitude():
    s, z = D.rows_qparams(D.mixed_rows(10, 96, 11))
    assert s.max() / s.min() > 1e20 and np.unique(z).size > 2


def test_unknown_granularity_raises():
    """Checked before anything touches a device or a state dict."""
    from models.dynamic_ptq_model import DynamicPTQModel, DynamicQuantConvNet
    from models.optimized_custom_quantization import DynamicFcResNet
    from models.static_ptq_model import StaticPTQModel
    with pytest.raises(ValueError):
        DynamicQuantConvNet({}, granularity="row")
    with pytest.raises(ValueError):
        DynamicFcResNet(None, granularity="tensor")
    with pytest.raises(ValueError):
        DynamicPTQModel().quantize(granularity="image")
    for mode in ("static", "reference"):
        with pytest.raises(ValueError):
            StaticPTQModel(mode=mode).quantize(granularity="rows")


def test_static_mode_refuses_sample_granularity():
    from models.static_ptq_model import StaticPTQModel
    with pytest.raises(ValueError):
        StaticPTQModel(mode="static").quantize(granularity="sample")
