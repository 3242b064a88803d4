"""GPU: Resize -> CenterCrop of raw u8 images of mixed sizes on the device
(qcn_resize_crop_u8_hwc, qconvnet.preprocess).

Every comparison is exact equality: the output bytes against the numpy
restatement (tests/resizeref.py) and against Pillow's bytes in the fixture
(tests/golden/ops_resize.npz; tests/test_resize_cpu.py pins the restatement to
both), and the tap tables the device computed in double, read back from the
workspace, against the restatement's.  All sources of one (R, C) go in a
single mixed batch, packed back to back (the (32, 32) batch has images at
odd offsets; test_misaligned_source moves whole batches) and repeated to
more than twice the device's CU count in images.  PIL is not imported here."""
import numpy as np
import pytest
import torch

import resizeref as R

pytestmark = pytest.mark.gpu

GROUPS = [rc for rc, _ in R.MATRIX]
GROUP_IDS = [f"r{r}_c{c}" for r, c in GROUPS]


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


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(R.GOLDEN))


_BATCH = {}


def batch(rc, ncu, dev):
    """The mixed batch of one (R, C), made once and never written to: its
    sources, repeat count, plan, and the packed bytes on the device at byte
    offsets 0..3 of a buffer (index 0 is the allocation's own alignment)."""
    from qconvnet import preprocess as P
    if rc not in _BATCH:
        sources = dict(R.MATRIX)[rc]
        reps = (2 * ncu) // len(sources) + 1
        assert reps * len(sources) > 2 * ncu
        packed, sizes = P.pack([R.case(*rc, h, w)["src"] for h, w in sources] * reps)
        desc = P.plan(sizes, *rc)
        if rc == (32, 32):   # its odd-sized sources put later images on odd addresses
            assert any(int(o) % 2 for o in desc["offset"])
        buf = torch.zeros(packed.numel() + 8, dtype=torch.uint8, device=dev)
        _BATCH[rc] = dict(sources=sources, reps=reps, desc=desc, packed=packed.to(dev), buf=buf)
    return _BATCH[rc]


def at_offset(b, offset):
    """The batch's bytes at data_ptr() % 4 == offset."""
    if offset == 0:
        return b["packed"]
    n = b["packed"].numel()
    b["buf"][offset:offset + n] = b["packed"]
    v = b["buf"][offset:offset + n]
    assert v.data_ptr() % 4 == offset
    return v


def expected_tables(k, c, stride):
    """(int32 [2 c, stride], bool mask of the words a record defines) of one case."""
    want = np.zeros((2 * c, stride), np.int32)
    mask = np.zeros((2 * c, stride), bool)
    for j, (xmin, taps) in enumerate(k["htab"] + k["vtab"]):
        assert 2 + len(taps) <= stride
        want[j, :2 + len(taps)] = [xmin, len(taps)] + taps
        mask[j, :2 + len(taps)] = True
    return want, mask


def check_batch(b, rc, out, workspace, stride, golden):
    r, c = rc
    ns, reps = len(b["sources"]), b["reps"]
    assert out.dtype == torch.uint8 and tuple(out.shape) == (ns * reps, c, c, 3)
    got = out.cpu().numpy().reshape(reps, ns, c, c, 3)
    tab = workspace[:ns * reps * 2 * c * stride * 4].cpu().numpy().view(np.int32)
    tab = tab.reshape(reps, ns, 2 * c, stride)
    for j, (h, w) in enumerate(b["sources"]):
        k = R.case(r, c, h, w)
        want, mask = expected_tables(k, c, stride)
        bad = [i for i in range(reps) if not np.array_equal(tab[i, j][mask], want[mask])]
        assert bad == [], f"{h}x{w}: tap tables differ in repeats {bad[:8]}"
        bad = [i for i in range(reps) if not np.array_equal(got[i, j], k["out"])]
        assert bad == [], (f"{h}x{w}: bytes differ in repeats {bad[:8]}, "
                           f"{int((got[bad[0], j] != k['out']).sum())} in the first")
        assert np.array_equal(got[0, j], golden[R.case_name(r, c, h, w) + ".out"]), f"{h}x{w} vs Pillow"


@pytest.mark.parametrize("rc", GROUPS, ids=GROUP_IDS)
def test_bytes_and_tap_tables(dev, ncu, golden, rc):
    from qconvnet import ops, preprocess as P
    b = batch(rc, ncu, dev)
    need, stride = ops.resize_crop_workspace_size(b["desc"], rc[1], rc[1])
    out, ws = P.resize_center_crop_packed(b["packed"], b["desc"], rc[1])
    torch.cuda.synchronize()
    assert ws.numel() >= need
    check_batch(b, rc, out, ws, stride, golden)


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("rc", [(32, 32), (40, 25)], ids=["r32_c32", "r40_c25"])
def test_misaligned_source(dev, ncu, golden, rc, offset):
    """The same launch with src moved by 1, 2 and 3 bytes, into an output that
    itself starts off a 4-byte boundary, with the caller's workspace."""
    from qconvnet import ops, preprocess as P
    b = batch(rc, ncu, dev)
    n, c = len(b["desc"]), rc[1]
    need, stride = ops.resize_crop_workspace_size(b["desc"], c, c)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    flat = torch.full((n * c * c * 3 + 8,), 0xA5, dtype=torch.uint8, device=dev)
    out = flat[offset:offset + n * c * c * 3].view(n, c, c, 3)
    got, ws2 = P.resize_center_crop_packed(at_offset(b, offset), b["desc"], c, out=out, workspace=ws)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and ws2.data_ptr() == ws.data_ptr()
    check_batch(b, rc, out, ws, stride, golden)
    assert bool((flat[:offset] == 0xA5).all()) and bool((flat[offset + n * c * c * 3:] == 0xA5).all())


def test_list_entry_mixed_inputs(dev):
    """resize_center_crop on a list of numpy arrays and tensors, and on nothing."""
    from qconvnet import preprocess as P
    sizes = [(75, 100), (100, 75), (40, 30)]
    imgs = [R.case(73, 64, h, w)["src"] for h, w in sizes]
    out = P.resize_center_crop([imgs[0], torch.from_numpy(imgs[1].copy()), imgs[2]], 73, 64, device=dev)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (3, 64, 64, 3)
    for i, (h, w) in enumerate(sizes):
        assert np.array_equal(out[i].cpu().numpy(), R.case(73, 64, h, w)["out"])
    empty = P.resize_center_crop([], 73, 64, device=dev)
    assert empty.is_cuda and tuple(empty.shape) == (0, 64, 64, 3)


def test_outside_the_envelope_launches_nothing(dev, monkeypatch):
    """(1025, 1025) at R = 32 needs 67 taps: the Python entry raises naming the
    image before anything is uploaded, and the C entry returns its status with
    the output untouched."""
    from qconvnet import _lib, ops, preprocess as P

    def boom(*a, **k):
        raise AssertionError("resize_crop reached the launch")
    small = R.case(32, 32, 24, 31)["src"]
    big = np.zeros((1025, 1025, 3), np.uint8)
    with monkeypatch.context() as m:
        m.setattr(ops, "resize_crop", boom)
        with pytest.raises(ValueError, match="image 1"):
            P.resize_center_crop([small, big], 32, 32, device=dev)
    packed, sizes = P.pack([small, big])
    desc = P.plan(sizes, 32, 32)
    src = packed.to(dev)
    desc_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    with pytest.raises(ValueError):
        ops.resize_crop(src, desc, desc_dev, 32, 32)
    y = torch.full((2, 32, 32, 3), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device=dev)
    import ctypes as C
    rc = _lib.load().qcn_resize_crop_u8_hwc(src.data_ptr(), src.numel(),
                                            desc.ctypes.data_as(C.POINTER(_lib.ResizeImg)),
                                            desc_dev.data_ptr(), 2, 32, 32, y.data_ptr(), ws.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == _lib.QCN_ERR_UNSUPPORTED
    assert bool((y == 0xA5).all()) and bool((ws == 0xA5).all())


def test_resnet_logits_from_resized_images(dev):
    """End to end: the fixture ResNet (hw 64) on resize_center_crop(list, 73, 64)
    gives the logits of the same model fed the restatement's u8 batch."""
    import resnetfix
    from qconvnet import preprocess as P
    from qconvnet.resnet import QuantizedResNet
    z = resnetfix.load()
    assert int(z["hw"]) == 64
    m = QuantizedResNet(resnetfix.spec(z), dev)
    sizes = [(75, 100), (100, 75), (40, 30), (100, 75), (40, 30), (75, 100), (75, 100), (40, 30)]
    want_u8 = np.stack([R.case(73, 64, h, w)["out"] for h, w in sizes])
    want = m.run(torch.from_numpy(want_u8).to(dev)).clone()
    x = P.resize_center_crop([R.case(73, 64, h, w)["src"] for h, w in sizes], 73, 64, device=dev)
    assert x.dtype == torch.uint8 and tuple(x.shape) == (8, 64, 64, 3)
    got = m.run(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.from_numpy(want_u8))
    assert torch.equal(got, want)
    assert torch.equal(m(x), want)
