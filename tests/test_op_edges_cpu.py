"""CPU: the references test_gpu_op_edges.py compares the kernels with, pinned
against torch CPU ops at every edge that file adds, so that a mismatch on the
GPU points at the kernel and not at the oracle.  Everything is compared
exactly; fp32 maps as bit patterns."""
import numpy as np
import pytest
import torch
import torch.nn.functional as tF

import opedge as E
from oracle import qref

F32 = np.float32


# ------------------------------------------------------------ dynamic Linear
@pytest.mark.parametrize("kind", [k for k in E.DYN_CLASSES])
def test_choose_qparams_matches_torch(kind):
    x = E.dyn_input(kind, 5, 40, 3)
    for rr in (False, True):
        s, z = qref.choose_qparams_dynamic(x.min(), x.max(), reduce_range=rr)
        ts, tz = torch._choose_qparams_per_tensor(torch.from_numpy(x), rr)
        assert (float(s), int(z)) == (float(F32(ts)), int(tz)), (kind, rr)


def _torch_dynamic_linear(x, w, s_w, b, per_channel):
    """quantized::linear_dynamic through torch.ao's module (reduce_range is
    the fbgemm engine's default, True)."""
    import torch.ao.nn.quantized.dynamic as nnqd
    n, k = w.shape
    wt = torch.from_numpy(w)
    if per_channel:
        qw = torch._make_per_channel_quantized_tensor(wt, torch.from_numpy(s_w.astype(np.float64)),
                                                      torch.zeros(n, dtype=torch.int64), 0)
    else:
        qw = torch._make_per_tensor_quantized_tensor(wt, float(s_w[0]), 0)
    mod = nnqd.Linear(k, n, bias_=b is not None, dtype=torch.qint8)
    mod.set_weight_bias(qw, torch.from_numpy(b) if b is not None else None)
    return mod(torch.from_numpy(x)).numpy()


@pytest.mark.parametrize("m,k,n", [(1, 1, 1), (3, 40, 7), (5, 96, 33), (33, 128, 65)])
def test_linear_dynamic_matches_torch(m, k, n):
    torch.backends.quantized.engine = "fbgemm"
    w, s_pt, s_pc, b = E.dyn_weights(k, n, k + n)
    for kind in E.DYN_CLASSES:
        x = E.dyn_input(kind, m, k, 11)
        for s_w, pc in ((s_pt, False), (s_pc, True)):
            for bias in (b, None):
                want = _torch_dynamic_linear(x, w, s_w, bias, pc)
                got = qref.linear_dynamic(x, w, s_w, bias, reduce_range=True)
                assert np.array_equal(E.bits(got), E.bits(want)), (kind, pc, bias is None)
    assert E.distinct_ok(qref.linear_dynamic(E.dyn_input("normal", m, k, 11), w, s_pc, b)) or m * n < 16


# ------------------------------------------------------ fp32 hand-offs (ResNet)
N, H, W, C = 2, 5, 6, 12


def _t_dq_bn(y_nhwc, s, z, stats):
    """torch.dequantize -> F.batch_norm(training=False) on a channels-last map."""
    t = torch.from_numpy(y_nhwc).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
    x = torch.dequantize(torch._make_per_tensor_quantized_tensor(t, float(s), int(z)))
    x = x.contiguous(memory_format=torch.channels_last)
    mean, var, gamma, bias = (torch.from_numpy(a) for a in stats)
    return tF.batch_norm(x, mean, var, gamma, bias, training=False, eps=1e-5)


def _t_quant(x_nchw, s, z):
    q = torch.quantize_per_tensor(x_nchw.contiguous(memory_format=torch.channels_last), float(s), int(z),
                                  torch.quint8)
    return q.int_repr().permute(0, 2, 3, 1).contiguous().numpy()


def _nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous().numpy()


@pytest.fixture(scope="module")
def maps():
    rng = np.random.default_rng(21)
    y = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
    yd = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
    y.reshape(-1)[::5] = 30      # q == z: signed zeros out of the BN, in every pool window
    return y, yd


@pytest.mark.parametrize("relu", [False, True])
def test_dq_bn_q_composition_matches_torch(maps, relu):
    y, _ = maps
    stats = E.bn_stats(C, 1)
    alpha, beta = qref.bn_eval_constants(*stats)
    for s, z, s_next, z_next in ((F32(0.05), 30, F32(0.1), 7), (F32(0.25), 0, F32(0.5), 255)):
        t = _t_dq_bn(y, s, z, stats)
        if relu:
            t = torch.relu(t)
        want = _t_quant(t, s_next, z_next)
        got = E.ref_dq_bn_q(y, s, z, alpha, beta, relu, s_next, z_next)
        assert np.array_equal(got, want)
        f = qref.bn_eval_nhwc(qref.dequantize(y, s, z), alpha, beta)
        f = qref.relu_f32(f) if relu else f
        assert np.array_equal(E.bits(f), E.bits(_nhwc(t)))
        # (a ReLU'd map quantized at zero point 255 is 255 everywhere)
        assert E.distinct_ok(f) and (E.distinct_ok(got) or (relu and z_next == 255))


def test_dq_bn_q_ties_match_torch(maps):
    """alpha = 1, beta = 0, s_next = 2 s: every odd q - z is an exact .5 tie."""
    y, _ = maps
    s, z, alpha, beta, s_next, z_next = E.handoff_params(C, len(E.HANDOFF_SETS) - 1)
    t = torch.from_numpy(y).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
    x = torch.dequantize(torch._make_per_tensor_quantized_tensor(t, float(s), int(z)))
    want = _t_quant(x, s_next, z_next)
    got = E.ref_dq_bn_q(y, s, z, alpha, beta, False, s_next, z_next)
    assert np.array_equal(got, want) and E.distinct_ok(got)


def test_stem_composition_matches_torch(maps):
    y = maps[0].copy()
    y[0, :, :, 1], y[1, ::2, :, 1] = 30, 30     # q == z in the negative-gamma channel
    stats = E.bn_stats(C, 2)
    stats[0][1], stats[3][1] = -0.0, -0.0       # its shift is -0.0: fma(+0, alpha < 0, -0.0) = -0.0
    alpha, beta = qref.bn_eval_constants(*stats)
    s, z, s_next, z_next = F32(0.05), 30, F32(0.1), 7
    t = tF.max_pool2d(torch.relu(_t_dq_bn(y, s, z, stats)), 3, 2, 1)
    f, q = E.ref_stem(y, s, z, alpha, beta, s_next, z_next)
    assert np.array_equal(E.bits(f), E.bits(_nhwc(t)))
    assert np.array_equal(q, _t_quant(t, s_next, z_next))
    assert E.distinct_ok(f) and E.distinct_ok(q)
    zeros = E.bits(f)[f == 0]
    assert (zeros == 0).any() and (zeros == 0x80000000).any()     # both signs of zero win windows


@pytest.mark.parametrize("downsample", [False, True])
def test_join_composition_matches_torch(maps, downsample):
    y3, yd = maps
    st3, std = E.bn_stats(C, 3), E.bn_stats(C, 4)
    a3, b3 = qref.bn_eval_constants(*st3)
    ad, bd = qref.bn_eval_constants(*std)
    s3, z3, sd, zd, s_next, z_next = F32(0.05), 30, F32(0.04), 200, F32(0.1), 7
    if downsample:
        ident, t_id = (yd, sd, zd, ad, bd), _t_dq_bn(yd, sd, zd, std)
    else:
        ident = E.wide_range_map((N, H, W, C), 5)
        ident[0, 0, 0, :] = -0.0
        t_id = torch.from_numpy(ident).permute(0, 3, 1, 2)
    t = torch.relu(_t_dq_bn(y3, s3, z3, st3) + t_id)
    f, q = E.ref_join(y3, s3, z3, a3, b3, ident, s_next, z_next)
    assert np.array_equal(E.bits(f), E.bits(_nhwc(t)))
    assert np.array_equal(q, _t_quant(t, s_next, z_next))
    assert E.distinct_ok(f) and E.distinct_ok(q)


@pytest.mark.parametrize("shape", [(3, 2, 2, 64), (3, 7, 7, 64), (2, 5, 8, 128), (1, 19, 17, 64)])
def test_avgpool_f32_matches_torch(shape):
    """2x2: the sequential sum; 7x7 and 5x8: full 16-pixel blocks and a
    remainder; 19x17: a second cascade level.  C % 64 == 0: ATen's 4-vector
    column blocks whatever the host's vector width (see qref)."""
    x = E.wide_range_map(shape, 6)
    t = torch.from_numpy(x).permute(0, 3, 1, 2)     # channels-last strides
    assert t.is_contiguous(memory_format=torch.channels_last)
    want = tF.adaptive_avg_pool2d(t, 1).reshape(shape[0], shape[3]).numpy()
    got = qref.avgpool_f32_nhwc(x)
    assert np.array_equal(E.bits(got), E.bits(want)) and E.distinct_ok(got)


# ----------------------------------------------------------- channel_affine
@pytest.mark.parametrize("relu", [False, True])
def test_channel_affine_reference_matches_torch(relu):
    from qconvnet import quant as Q
    rows, cols = 5, 512
    x, stats = E.channel_affine_case(rows, cols)
    alpha, beta = Q.bn_eval_affine(*stats)
    got = Q.fmaf_host(x, alpha[None, :], beta[None, :])
    if relu:
        got = qref.relu_f32(got)
    want = E.channel_affine_torch(x, stats, relu)
    assert np.array_equal(E.bits(got), E.bits(want)) and E.distinct_ok(got)
    assert (alpha < 0).any() and (E.bits(got) == 0x80000000).any()


# ------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("shape", [(2, 7, 5, 16), (1, 2, 2, 48), (3, 3, 9, 5), (3, 8, 6, 3)])
def test_maxpool2x2_floor_mode_matches_torch(shape):
    q = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    t = torch.from_numpy(q).permute(0, 3, 1, 2).float()
    want = tF.max_pool2d(t, 2, 2).permute(0, 2, 3, 1).numpy().astype(np.uint8)
    got = qref.maxpool2x2_nhwc(q)
    assert np.array_equal(got, want) and E.distinct_ok(got)
