"""GPU: the 16x16 pair main loop (pipe_job16: weight fragments requested two
K-steps ahead, refilled in place) against the unfused per-layer launches
(ops.conv3x3), byte for byte.

The batches are the smallest that reach the persistent wave-specialised body
(ncu = the device's CU count): conv3+4 shapes from 2 ncu images, conv5+6
shapes from 4 ncu, the one launch from 4 ncu.  At 2 ncu + 1 images (one per
tile) workgroup 0 of conv3+4 runs a tile more than the others, so in the
same period a job's hand-over of the next job's first weight chunk is
followed by another job there and by nothing elsewhere; 4 ncu + 3 leaves
ragged last tiles (phantom segments) in conv5+6.

Inputs: random u8 activations with random s8 weights; all-255 activations with
+127 / -128 / mixed weights (|acc| up to 255 * 128 * 9 Cin); an all-zero
image inside the random batch.  Epilogues: the fast form (z_y == 0 + ReLU) and
the one-fma QDQ hand-off form, the two the 16x16 body is built for."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import convchain as CC

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = {"conv34": (16, 64, 128, 2), "conv56": (8, 128, 256, 4)}   # hw, cin, cout, images per CU
EXTRA = {"conv34": (0, 1), "conv56": (0, 3)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()
    return torch.device("cuda:0")


def _ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _weights(rng, cout, cin, kind):
    if kind == "random":
        return rng.integers(-128, 128, (cout, cin, 3, 3), dtype=np.int8)
    # accumulator range: channel c % 4 == 0 all +127, 1 all -128, 2 +127 / -128
    # alternating along cin, 3 a random choice of the two
    w = np.empty((cout, cin, 3, 3), np.int8)
    w[0::4] = 127
    w[1::4] = -128
    w[2::4] = np.where(np.arange(cin) % 2 == 0, 127, -128).astype(np.int8)[None, :, None, None]
    w[3::4] = rng.choice(np.array([127, -128], np.int8), (len(w[3::4]), cin, 3, 3))
    return w


def _layer(dev, w, z_x, mode, nxt, pool):
    """A conv layer in the form ops.conv3x3 / ops.conv_pair take.  Per-channel
    multipliers put +-3 sigma of a random-input accumulator (or, for a
    constant-sign channel, its full range) across the u8 output range."""
    from qconvnet import _lib, ops
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    cout, cin = w.shape[:2]
    packed, wsum = ops.pack_conv3x3(w)
    w64 = w.astype(np.int64).reshape(cout, -1)
    spread = np.maximum(3.0 * 74.0 * np.sqrt((w64 ** 2).sum(1)), 255.0 * np.abs(w64.sum(1)))
    z_y = 0 if mode == 1 else 37
    mult = ((255.0 - z_y) / spread).astype(F32)
    u = (np.arange(cout) % 5 - 2).astype(F32) * F32(1000.0)   # bias / (s_x s_w), per channel
    d = NS(w=T(packed), cout=cout, u=T(u), v=T(np.ones(cout, F32)), mult=T(mult),
           corr=T(((128 - z_x) * wsum.astype(np.int64)).astype(np.int32)), z_x=z_x, z_y=z_y,
           relu=True, pool=pool, qdq=None)
    if mode == 2:
        s_y = F32(0.05)
        d.qdq = ops.qdq_struct(s_y, z_y, F32(CC.FOUND_RATIO) * s_y, nxt)
        out = (C.c_float * 4)()
        assert _lib.load().qcn_qdq_affine(C.byref(d.qdq), z_y, z_y, out) == 1, "no one-fma form"
    return d


def _unfused(x, la, lb):
    from qconvnet import ops
    a = ops.conv3x3(x, la.z_x, la.w, la.cout, la.u, la.v, la.mult, la.corr, la.z_y, la.relu, False, la.qdq)
    return ops.conv3x3(a, lb.z_x, lb.w, lb.cout, lb.u, lb.v, lb.mult, lb.corr, lb.z_y, lb.relu, True, lb.qdq)


@pytest.mark.parametrize("mode", [1, 2], ids=["fast", "qdq"])
@pytest.mark.parametrize("data", ["random", "range"])
@pytest.mark.parametrize("extra", [0, 1], ids=["full", "ragged"])
@pytest.mark.parametrize("block", list(SHAPES))
def test_pair_launch_equals_unfused_layers(dev, block, extra, data, mode):
    from qconvnet import ops
    hw, cin, cout, per_cu = SHAPES[block]
    n = per_cu * _ncu(dev) + EXTRA[block][extra]
    rng = np.random.default_rng([hw, extra, mode, int(data == "range")])
    # conv A's input zero point: 0 at full range (255 - z_x as large as it gets)
    z_xa, z_hand = (0, 7) if data == "range" else (113, 12)
    la = _layer(dev, _weights(rng, cout, cin, data), z_xa, mode, z_hand, False)
    # conv B reads A's output: its zero point is A's z_y, or the hand-off's z2
    lb = _layer(dev, _weights(rng, cout, cout, data), z_hand if mode == 2 else la.z_y, mode, 3, True)
    if data == "range":
        x = torch.full((n, hw, hw, cin), 255, dtype=torch.uint8, device=dev)
    else:
        x = torch.randint(0, 256, (n, hw, hw, cin), dtype=torch.uint8, device=dev)
        x[1] = 0          # an all-zero image, and one at the very end
        x[n - 1] = 0
    want = _unfused(x, la, lb)
    assert want.min().item() < want.max().item()   # (not one saturated constant)
    got = torch.full_like(want, 0xA5)
    assert ops.conv_pair(x, la, lb, got) is True
    torch.cuda.synchronize()
    bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, f"{block} n={n}: {len(bad)} images differ, first {bad[:8]}"
    if block == "conv56" and n % 128 == 0:   # conv6's chunk-major output for the head
        gk = torch.full((4 * 4 * cout // 32, n, 32), 0xA5, dtype=torch.uint8, device=dev)
        assert ops.conv_pair(x, la, lb, gk, kmajor=True) is True
        assert torch.equal(ops.from_kmajor(gk).reshape(n, 4, 4, cout), want)


@pytest.mark.parametrize("profile", ["fast", "qdq"])
def test_one_launch_equals_unfused_layers(dev, profile):
    """conv1 .. conv6 in one launch at 4 ncu + 3 images against the per-layer
    launches of the same model: a2, a4, a6 and the logits."""
    from qconvnet.qmodel import QuantizedConvNet
    n = 4 * _ncu(dev) + 3
    model = QuantizedConvNet(CC.make_spec(profile), dev)
    idx = torch.from_numpy(CC.batch(n, seed=3)).to(dev)
    x = torch.from_numpy(CC.pool_images(model.spec)).to(dev)[idx].contiguous()
    x[2] = 0.0        # an all-zero image
    x[5] = 1e9        # every QuantStub output 255
    x[n - 1] = 0.0
    runs = {}
    for path in ("layers", "default"):
        model.fuse12 = path != "layers"
        model.fuse_convs = path == "default"
        model.convs_w4 = False
        try:   # nothing the second path leaves unwritten may hold the first path's result
            for t in model.buffers(n).values():
                t.fill_(0xA5) if t.dtype == torch.uint8 else t.zero_()
        except KeyError:
            pass
        model.run(x, keep=path == "layers")
        torch.cuda.synchronize()
        names = model.kernel_names(x.shape, keep=path == "layers")
        assert names[0] == ("conv1" if path == "layers" else "conv1_6"), names
        b = model.buffers(n)
        runs[path] = {k: b[k].clone() for k in ("a2", "a4", "a6", "logits")}
    for k in ("a2", "a4", "a6", "logits"):
        assert torch.equal(runs["default"][k], runs["layers"][k]), k
