"""GPU: conv2 of the fused conv1+conv2 pipeline on the 16x16x64 MFMA
(conv_mainloop_res16: the Cin + 32 patch, the padding row the two half-image
patches share, the re-swizzled resident weights, the pooled 16x16 epilogue).

Expected values: the unfused per-layer launches (conv1_f32, then conv3x3 with
its pool) on the same device, byte for byte; for the images of the
tests/convchain.py pool also the numpy oracle.

Shapes, the smallest at which the pipeline can still go wrong:

  1         top half, then the bottom half with its two copied conv1 rows,
            both against the shared padding row
  ncu + 1   one workgroup runs a second image: the patches, the shared row
            and the column halos are reused after a full image
  2ncu + 3  workgroups with three and with two images
  3         the one-image-per-workgroup launch of conv1 .. conv6
  4ncu + 3  the persistent launch of conv1 .. conv6, ragged last round

Inputs are the full-range profiles of tests/convchain.py (every epilogue
form conv2 has: fast, per-channel constants, general, one-fma QDQ hand-off,
declined QDQ hand-off) with two more images, every byte 0 and every byte
255 (fp32: the values the QuantStub saturates to 0 and 255), and a spec whose
conv1 / conv2 weights are only -128, -127 and 127 with whole output channels
of one value."""
import copy

import numpy as np
import pytest
import torch

import convchain as CC

pytestmark = pytest.mark.gpu

PROFILES = ("fast", "fast_pc", "general", "qdq", "qdq_declined", "extreme")
# profiles whose conv3 .. conv6 share one epilogue form: the persistent launch takes them
PERSISTENT = ("fast", "fast_pc", "qdq", "extreme")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def extreme_spec():
    """The fast profile with conv1's and conv2's weights at the ends of int8:
    random -128 / -127 / 127, and output channels 0 .. 2 all 127, all -128 and
    all -127."""
    spec = copy.deepcopy(CC.make_spec("fast"))
    rng = np.random.default_rng(1234)
    for name in ("conv1", "conv2"):
        e = spec[name]
        w = rng.choice(np.array([-128, -127, 127], np.int8), size=e["w"].shape)
        w[0], w[1], w[2] = 127, -128, -127
        e["w"] = w.astype(np.int8)
    return spec


_CACHE = {}


def model(profile, dev):
    if ("m", profile) not in _CACHE:
        from qconvnet.qmodel import QuantizedConvNet
        spec = extreme_spec() if profile == "extreme" else CC.make_spec(profile)
        _CACHE["m", profile] = QuantizedConvNet(spec, dev)
    return _CACHE["m", profile]


def pool(profile, u8, dev):
    """The POOL images of convchain plus an all-0 and an all-255 image, on the
    device; made once and never written to."""
    key = ("pool", profile, u8)
    if key not in _CACHE:
        m = model(profile, dev)
        if u8:
            x = CC.pool_images_u8()
            ext = np.stack([np.zeros_like(x[0]), np.full_like(x[0], 255)])
        else:
            x = CC.pool_images(m.spec)
            s, z = float(m.in_scale), int(m.in_zp)
            ext = np.stack([np.full_like(x[0], (0 - z) * s), np.full_like(x[0], (255 - z) * s)])
        _CACHE[key] = torch.from_numpy(np.concatenate([x, ext])).to(dev)
    return _CACHE[key]


def index(n):
    """Pool positions of a batch of n: the pool in order, then the two
    constant images, then convchain's neighbour-differing sequence."""
    head = np.arange(min(n, CC.POOL + 2))
    if n <= head.size:
        return head
    return np.concatenate([head, CC.batch(n - head.size, seed=3)])


def unfused_a2(profile, u8, dev):
    """conv1_f32 + conv3x3 (pooled) per image of the pool: the expected a2."""
    key = ("want", profile, u8)
    if key not in _CACHE:
        from qconvnet import ops
        m = model(profile, dev)
        x = pool(profile, u8, dev)
        xf = ops.normalize_u8(x, m.ntab) if u8 else x
        l1, l2 = m.L[0], m.L[1]
        a1 = ops.conv1_f32(xf, m.in_scale, m.in_zp, l1.w, l1.u, l1.v, l1.mult, l1.corr, l1.z_y, l1.relu, l1.qdq)
        a2 = ops.conv3x3(a1, l2.z_x, l2.w, l2.cout, l2.u, l2.v, l2.mult, l2.corr, l2.z_y, l2.relu, True, l2.qdq)
        torch.cuda.synchronize()
        _CACHE[key] = a2
    return _CACHE[key]


def conv12(profile, u8, x, dev, out=None):
    from qconvnet import ops
    m = model(profile, dev)
    if u8:
        return ops.conv12_fused_u8(x, m.qlut, m.in_zp, m.L[0], m.L[1], out=out)
    return ops.conv12_fused(x, m.in_scale, m.in_zp, m.L[0], m.L[1], out=out)


def check(label, got, want, idx):
    msg = CC.mismatch(label, got.cpu().numpy(), want.cpu().numpy(), idx)
    assert msg is None, msg


def test_unfused_reference_equals_oracle(dev):
    """The expected values themselves: the per-layer launches against the
    numpy oracle on the pool, for the two input kinds of one profile each."""
    for profile, u8 in (("general", False), ("qdq", True)):
        m = model(profile, dev)
        o = CC.pool_oracle(profile, u8=True, mean=m.mean, std=m.std) if u8 else CC.pool_oracle(profile)
        want = torch.from_numpy(np.ascontiguousarray(o["a2"]))
        check(f"{profile} unfused a2", unfused_a2(profile, u8, dev)[:CC.POOL], want, np.arange(CC.POOL))


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("size", ["1", "ncu+1", "2ncu+3"])
@pytest.mark.parametrize("profile", PROFILES)
def test_conv12_equals_unfused(dev, ncu, profile, size, u8):
    n = {"1": 1, "ncu+1": ncu + 1, "2ncu+3": 2 * ncu + 3}[size]
    idx = index(n)
    idx_dev = torch.from_numpy(idx).to(dev)
    # one image: each of the pool's kinds in turn (a pool image, all 0, all 255)
    starts = (0, CC.POOL, CC.POOL + 1) if n == 1 else (0,)
    for s in starts:
        sel = idx_dev + s if n == 1 else idx_dev
        x = pool(profile, u8, dev)[sel].contiguous()
        got = conv12(profile, u8, x, dev)
        torch.cuda.synchronize()
        check(f"{profile} n={n} first image {s} a2", got, unfused_a2(profile, u8, dev)[sel], idx + (s if n == 1 else 0))


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_same_buffers_twice(dev, ncu, u8):
    """Two launches in a row on the same input and output buffers: nothing a
    launch leaves behind changes the next one."""
    n = ncu + 1
    idx = index(n)
    idx_dev = torch.from_numpy(idx).to(dev)
    x = pool("fast", u8, dev)[idx_dev].contiguous()
    want = unfused_a2("fast", u8, dev)[idx_dev]
    out = torch.full((n, 16, 16, 64), 0xA5, dtype=torch.uint8, device=dev)
    for rep in range(2):
        conv12("fast", u8, x, dev, out=out)
        torch.cuda.synchronize()
        check(f"launch {rep} a2", out, want, idx)
        out.fill_(0xA5)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("size", ["3", "4ncu+3"])
@pytest.mark.parametrize("profile", PROFILES)
def test_one_launch_a2_equals_unfused(dev, ncu, profile, size, u8):
    """a2 of the conv1 .. conv6 launches: one image per workgroup at batch 3
    (every profile), persistent at 4 ncu + 3 (the profiles it takes; the
    others must be declined, not run some other way)."""
    from qconvnet import ops
    n = 3 if size == "3" else 4 * ncu + 3
    m = model(profile, dev)
    idx = index(n)
    if n == 3:   # a pool image and the two constant ones
        idx = np.array([0, CC.POOL, CC.POOL + 1])
    idx_dev = torch.from_numpy(idx).to(dev)
    x = pool(profile, u8, dev)[idx_dev].contiguous()
    layers = ops.conv_layers(m.L, m.in_zp)
    a2 = torch.full((n, 16, 16, 64), 0xA5, dtype=torch.uint8, device=dev)
    a4 = torch.empty((n, 8, 8, 128), dtype=torch.uint8, device=dev)
    a6 = torch.empty(n * 4096, dtype=torch.uint8, device=dev)
    if u8:
        ok = ops.convnet_convs_u8(x, m.qlut, m.in_zp, layers, a2, a4, a6, kmajor=False)
    else:
        ok = ops.convnet_convs(x, m.in_scale, m.in_zp, layers, a2, a4, a6, kmajor=False)
    torch.cuda.synchronize()
    assert ok == (n == 3 or profile in PERSISTENT)
    if ok:
        check(f"{profile} n={n} a2", a2, unfused_a2(profile, u8, dev)[idx_dev], idx)
