"""GPU: the dynamic int8 conv pair for maps up to 32 x 32 (ops.conv3x3_dyn_pair32,
csrc/conv_dyn_pair32.hip) as bits against the numpy contract of
tests/test_gpu_conv_dyn.py applied twice and against the two single calls,
its batch invariance, and the dynamic models with pairs="all"."""
import itertools

import numpy as np
import pytest
import torch

import opedge as E
from test_gpu_conv_dyn import acc_ref, bits, dev, epilogue_ref, mixed_images, sd  # noqa: F401
from test_gpu_conv_dyn_pair import dyn_layer, problem, to_dev

pytestmark = pytest.mark.gpu
F32 = np.float32

# (h, w, cin, cmid, cout, pool): one position and one channel; pool with cin past 16 and cmid past
# 32; the first maps past the register-resident classes, a second pixel group down / across; both
# owned groups partial; the largest cin at an even non-multiple of 8; 31 rows; the model pair
CASES = [(1, 1, 3, 1, 1, 0), (2, 2, 20, 33, 64, 1), (17, 8, 3, 8, 8, 0), (8, 17, 3, 8, 8, 0),
         (9, 25, 16, 64, 1, 0), (26, 30, 64, 64, 64, 1), (31, 32, 3, 64, 64, 0), (32, 32, 3, 64, 64, 1)]


@pytest.mark.parametrize("full", [False, True], ids=["bias", "bias_affine_relu"])
@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_pair32_against_contract(dev, case, per_channel, full):
    from qconvnet import ops
    pool = bool(case[5])
    x, ws, par, (acc_a, ss_a, zs_a) = problem(case)
    epi = [(p[0] if per_channel else p[0][:1], p[1], (p[2], p[3]) if full else None, full) for p in par]
    mid = epilogue_ref(acc_a, ss_a, *epi[0], False)
    acc_b, ss_b, zs_b = acc_ref(mid, ws[1])
    ref = epilogue_ref(acc_b, ss_b, *epi[1], pool)
    assert np.isfinite(ref).all() and E.distinct_ok(acc_b)
    n = len(x)
    la, lb = (dyn_layer(dev, w, *e) for w, e in zip(ws, epi))
    xd = {False: to_dev(dev, x), True: to_dev(dev, x.transpose(0, 3, 1, 2))}
    t, st = ops.conv3x3_dyn(xd[False], ops.image_minmax(xd[False]), la.packed, la.wsum, la.w_scale, la.channels,
                            bias=la.bias, affine=la.affine, relu=full)
    two = ops.conv3x3_dyn(t, st, lb.packed, lb.wsum, lb.w_scale, lb.channels, bias=lb.bias, affine=lb.affine,
                          relu=full, pool=pool, want_stats=False)[0].cpu().numpy()
    for x_nchw, y_nchw in itertools.product((False, True), (False, True)):
        y, ys, qx, qm = ops.conv3x3_dyn_pair32(xd[x_nchw], ops.image_minmax(xd[x_nchw]), la, lb, pool=pool,
                                               x_nchw=x_nchw, y_nchw=y_nchw, qparams=True)
        y = y.cpu().numpy()
        y = y.transpose(0, 2, 3, 1) if y_nchw else y
        label = (x_nchw, y_nchw)
        assert np.array_equal(E.bits(y), E.bits(ref)), label
        assert np.array_equal(E.bits(y), E.bits(two)), label
        for (gs, gz), (s, z) in ((qx, (ss_a, zs_a)), (qm, (ss_b, zs_b))):
            assert np.array_equal(E.bits(gs.cpu().numpy()), E.bits(s)) and np.array_equal(gz.cpu().numpy(), z), label
        ys = ys.cpu().numpy()
        assert ys.shape == (n, 1, 2), label
        assert np.array_equal(ys[:, 0, 0], ref.reshape(n, -1).min(1)), label
        assert np.array_equal(ys[:, 0, 1], ref.reshape(n, -1).max(1)), label


def test_full_range_mid_codes(dev):
    """The mid codes are 0 and 255 only and B's weights +-127 at cmid = 64 on a
    24 x 8 map (a wave's second pixel group): B's |acc| reaches 9 * 64 * 255 * 127."""
    from oracle import qref
    from qconvnet import ops
    h, w, cin, cmid, cout = 24, 8, 4, 64, 20
    rng = np.random.default_rng(5)
    x = np.ones((3, h, w, cin), F32)                                       # mid constant > 0: code 255, z = 0
    x[1] = rng.integers(0, 2, (h, w, 1)).astype(F32)                       # mid 0 or > 0: codes 0 and 255
    x[1, 18:21, 3:6] = 1.0
    x[2] = -x[1]                                                           # mid < 0 or 0: z = 255
    wa = np.zeros((cmid, cin, 3, 3), np.int8)
    wa[:, :, 1, 1] = 127                                                   # A copies the pixel's sum to every channel
    wb = (rng.integers(0, 2, (cout, cmid, 3, 3)) * 254 - 127).astype(np.int8)
    wb[0], wb[1] = 127, -127
    s_a, s_b, bias = np.array([0.003], F32), np.full(cout, 0.003, F32), rng.standard_normal(cout).astype(F32)
    acc_a, ss_a, _ = acc_ref(x, wa)
    mid = epilogue_ref(acc_a, ss_a, s_a, None, None, False, False)
    acc_b, ss_b, zs_b = acc_ref(mid, wb)
    codes = [qref.quantize_legacy_fma(m, s, z) for m, s, z in zip(mid, ss_b, zs_b)]
    assert list(zs_b) == [0, 0, 255] and all(set(np.unique(c)) <= {0, 255} for c in codes)
    assert {0, 255} <= set(np.unique(codes[1])) and acc_b.max() == 9 * 64 * 255 * 127 == -acc_b.min()
    assert acc_b[1:, 16:].max() == 9 * 64 * 255 * 127                      # reached in the second pixel group too
    ref = epilogue_ref(acc_b, ss_b, s_b, bias, None, False, False)
    xd = to_dev(dev, x)
    y, _, _, (gs, gz) = ops.conv3x3_dyn_pair32(xd, ops.image_minmax(xd), dyn_layer(dev, wa, s_a, None, None, False),
                                               dyn_layer(dev, wb, s_b, bias, None, False), qparams=True)
    assert np.array_equal(E.bits(y.cpu().numpy()), E.bits(ref))
    assert np.array_equal(E.bits(gs.cpu().numpy()), E.bits(ss_b)) and np.array_equal(gz.cpu().numpy(), zs_b)


def test_batch_invariance_bits(dev):
    from qconvnet import ops
    hw, cin, cmid, cout = 32, 3, 64, 64
    rng = np.random.default_rng(hw)
    x = to_dev(dev, mixed_images(33, hw, hw, cin, hw))
    la, lb = (dyn_layer(dev, rng.integers(-128, 128, (co, ci, 3, 3), dtype=np.int8),
                        rng.uniform(0.002, 0.01, co).astype(F32), rng.standard_normal(co).astype(F32), None, True)
              for ci, co in ((cin, cmid), (cmid, cout)))

    def f(t):
        t = t.contiguous()
        y, st = ops.conv3x3_dyn_pair32(t, ops.image_minmax(t), la, lb, pool=True)
        return torch.cat([y.reshape(len(t), -1), st[:, 0]], 1)
    whole = bits(f(x))
    assert torch.equal(bits(torch.cat([f(x[:1]), f(x[1:6]), f(x[6:])])), whole)
    assert torch.equal(bits(f(x.flip(0)).flip(0)), whole)


@pytest.mark.parametrize("fold", [True, False])
def test_model_pairs_all_bit_equal(dev, sd, fold):
    from models.dynamic_ptq_model import DynamicQuantConvNet
    from oracle import torch_ref
    x = torch.from_numpy(torch_ref.synthetic_images(9, 11)).to(dev)
    m = [DynamicQuantConvNet(sd, fold=fold, device=dev, granularity="sample", body="int8", pairs=p)
         for p in (False, "all")]
    assert m[1].pairs == "all" and m[0].pairs is False
    assert torch.equal(bits(m[1](x)), bits(m[0](x)))
    assert torch.equal(bits(m[1](x[:2])), bits(m[0](x))[:2])


@pytest.mark.parametrize("shape,pool,status", [((33, 8, 3, 8, 8), False, "unsupported"),
                                               ((8, 8, 3, 65, 8), False, "unsupported"),
                                               ((8, 8, 65, 8, 8), False, "unsupported"),
                                               ((7, 8, 3, 8, 8), True, "invalid argument")], ids=str)
def test_op_refuses(dev, shape, pool, status):
    from qconvnet import _lib, ops
    h, w, cin, cmid, cout = shape
    assert ops.conv3x3_dyn_pair32_supported(*shape) == (status != "unsupported")
    x = torch.zeros((2, h, w, cin), device=dev)
    la, lb = (dyn_layer(dev, np.zeros((co, ci, 3, 3), np.int8), np.ones(1, F32), None, None, False)
              for ci, co in ((cin, cmid), (cmid, cout)))
    with pytest.raises(_lib.QcnError, match=status):
        ops.conv3x3_dyn_pair32(x, ops.image_minmax(x), la, lb, pool=pool)
