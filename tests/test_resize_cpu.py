"""CPU: the numpy restatement of Resize -> CenterCrop (resizeref.py) against
the Pillow fixture (tests/golden/ops_resize.npz) and, where PIL imports,
against live Pillow; qconvnet.preprocess's host half; and the host half of the
C ABI (argument checks, workspace size, the tap envelope) — no device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import resizeref as R

CASES = [(r, c, h, w) for (r, c), srcs in R.MATRIX for h, w in srcs]
IDS = [R.case_name(*k) for k in CASES]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(R.GOLDEN))


@pytest.mark.parametrize("r,c,h,w", CASES, ids=IDS)
def test_restatement_is_the_fixture(golden, r, c, h, w):
    name = R.case_name(r, c, h, w)
    k = R.case(r, c, h, w)
    assert R.sha(k["src"]) == str(golden[name + ".src_sha"]), "source generator drifted"
    if name + ".src" in golden:
        assert np.array_equal(golden[name + ".src"], k["src"])
    else:
        assert k["src"].nbytes > R.STORED_SOURCE_BYTES
    assert np.array_equal(k["out"], golden[name + ".out"])


@pytest.mark.parametrize("r,c,h,w", CASES, ids=IDS)
def test_coverage_conditions(r, c, h, w):
    """A window that could not show a wrong tap proves nothing: both extremes
    and at least 64 distinct bytes, wherever the source's short side is >= 16."""
    if min(h, w) < 16:
        return
    out = R.case(r, c, h, w)["out"]
    assert out.min() == 0 and out.max() == 255
    assert len(np.unique(out)) >= 64


def test_tap_counts_of_the_matrix():
    """The matrix reaches the tap counts it is there for: 7, 33 and 64 at
    R = 32 (a scale of exactly 32 has windows of 64 in records sized for 65),
    5 at (40, 25), at most 3 when upscaling, and a border-clipped window."""
    def most(r, c, h, w):
        k = R.case(r, c, h, w)
        return max(len(t[1]) for t in k["htab"] + k["vtab"])
    assert most(32, 32, 97, 129) == 7
    assert most(32, 32, 700, 513) >= 33 and most(32, 32, 513, 1100) >= 33
    assert most(32, 32, 1024, 1024) == 64
    assert most(40, 25, 100, 83) == 5
    assert most(32, 32, 7, 5) <= 3 and most(32, 32, 1, 1) == 1
    k = R.case(32, 32, 24, 31)
    assert k["vtab"][0][0] == 0 and len(k["vtab"][0][1]) < len(k["vtab"][5][1])


@pytest.mark.parametrize("r,c,h,w", CASES, ids=IDS)
def test_restatement_is_live_pillow(r, c, h, w):
    pytest.importorskip("PIL")
    from PIL import Image
    k = R.case(r, c, h, w)
    oh, ow = R.resized_size(h, w, r)
    top, left = R.crop_offset(oh, c), R.crop_offset(ow, c)
    im = Image.fromarray(k["src"], "RGB").resize((ow, oh), Image.BILINEAR)
    assert np.array_equal(np.asarray(im.crop((left, top, left + c, top + c))), k["out"])


# ------------------------------------------------------------ preprocess.plan
def test_plan_sizes_and_bankers_offsets():
    from qconvnet import preprocess as P
    from qconvnet import _lib
    assert P.DESC.itemsize == C.sizeof(_lib.ResizeImg) == 32
    # oh - C = 117 -> 58 (58.5 to even), 119 -> 60 (59.5 to even), 118 -> 59
    assert P.crop_offset(224 + 117, 224) == 58 and P.crop_offset(224 + 119, 224) == 60
    assert P.crop_offset(224 + 118, 224) == 59 and P.crop_offset(224, 224) == 0
    assert P.crop_offset(256 + 1, 256) == 0 and P.crop_offset(256 + 3, 256) == 2
    # Resize(256): short side 256, long side truncated
    assert P.resized_size(375, 500, 256) == (256, 341)      # 341.33
    assert P.resized_size(500, 375, 256) == (341, 256)
    assert P.resized_size(333, 500, 256) == (256, 384)      # 384.38
    assert P.resized_size(256, 256, 256) == (256, 256)
    assert P.resized_size(100, 341, 256) == (256, 872)      # 872.96
    sizes = [(375, 500), (500, 333), (7, 5), (256, 256)]
    d = P.plan(sizes, 256, 224)
    assert d.dtype == P.DESC and len(d) == 4
    off = 0
    for e, (h, w) in zip(d, sizes):
        oh, ow = R.resized_size(h, w, 256)
        assert (e["h"], e["w"], e["oh"], e["ow"]) == (h, w, oh, ow)
        assert (e["top"], e["left"]) == (R.crop_offset(oh, 224), R.crop_offset(ow, 224))
        assert e["offset"] == off
        off += h * w * 3
    assert d[0]["left"] == 58 and d[0]["top"] == 16           # 341 - 224 = 117 -> 58
    e = P.plan([(343, 256)], 256, 224)[0]                     # 343 - 224 = 119 -> 60
    assert (e["oh"], e["top"]) == (343, 60)
    assert len(P.plan([], 256, 224)) == 0
    with pytest.raises(ValueError, match="crop"):
        P.plan(sizes, 224, 256)
    with pytest.raises(ValueError):
        P.plan([(0, 5)], 32, 32)


def test_pack_and_argument_errors():
    from qconvnet import preprocess as P
    a = R.source(7, 5)
    b = torch.from_numpy(R.source(24, 31).copy())
    nc = torch.from_numpy(R.source(9, 6).copy()).permute(1, 0, 2)      # a non-contiguous [6, 9, 3]
    packed, sizes = P.pack([a, b, nc])
    assert sizes == [(7, 5), (24, 31), (6, 9)] and packed.dtype == torch.uint8 and packed.dim() == 1
    want = np.concatenate([a.reshape(-1), b.numpy().reshape(-1), nc.contiguous().numpy().reshape(-1)])
    assert np.array_equal(packed.numpy(), want)
    for bad in (a.astype(np.float32), a[..., :2], a[0], torch.zeros((3, 4, 4), dtype=torch.uint8), [[1]]):
        with pytest.raises(ValueError, match="image 1"):
            P.pack([a, bad])
    # refused on the host, whatever the device: crop > resize, and the envelope by name
    with pytest.raises(ValueError, match="crop"):
        P.resize_center_crop([a], 32, 33, device="cpu")
    big = np.zeros((1025, 1025, 3), np.uint8)
    with pytest.raises(ValueError, match="image 2"):
        P.resize_center_crop([a, a, big], 32, 32, device="cpu")
    # the long side's truncation counts: 2000 -> int(62.5) = 62 is 32.26 source samples per output
    assert P.outside_envelope(P.plan([(1024, 1024), (1025, 1025), (1024, 2000), (1024, 1984)], 32, 32)) == [1, 2]


# ------------------------------------------------------- the C ABI, host half
@pytest.fixture(scope="module")
def lib():
    from qconvnet import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libqconvnet.so missing — run __graft_entry__.build()")
    return _lib.load()


def _descp(desc):
    from qconvnet import _lib
    return desc.ctypes.data_as(C.POINTER(_lib.ResizeImg))


def test_bad_arguments_before_any_device_call(lib):
    """Host addresses stand in for the device pointers: every call below must
    return before it could touch them."""
    from qconvnet import preprocess as P
    sizes = [(24, 31), (97, 129)]
    good = P.plan(sizes, 32, 32)
    nbytes = sum(h * w * 3 for h, w in sizes)
    src = np.zeros(nbytes, np.uint8)
    y = np.zeros(2 * 32 * 32 * 3, np.uint8)
    raw = np.zeros((1 << 16) + 16, np.uint8)
    ws = raw[(-raw.ctypes.data) % 16:]
    V = lambda a: C.c_void_p(a.ctypes.data)

    def call(desc=good, src=src, src_bytes=nbytes, dev=good, n=2, ch=32, cw=32, y=y, ws=ws):
        return lib.qcn_resize_crop_u8_hwc(V(src) if src is not None else None, src_bytes,
                                          _descp(desc) if desc is not None else None,
                                          V(dev) if dev is not None else None, n, ch, cw,
                                          V(y) if y is not None else None,
                                          V(ws) if ws is not None else None, None)

    def edit(i, **kw):
        d = good.copy()
        for k, v in kw.items():
            d[i][k] = v
        return d

    for kw in (dict(src=None), dict(desc=None), dict(dev=None), dict(y=None), dict(ws=None),
               dict(n=-1), dict(ch=0), dict(cw=0), dict(ch=-3), dict(src_bytes=-1),
               dict(desc=edit(0, h=0)), dict(desc=edit(1, w=0)), dict(desc=edit(0, oh=0)),
               dict(desc=edit(1, ow=-1)), dict(desc=edit(1, offset=-1)),
               dict(desc=edit(0, top=-1)), dict(desc=edit(1, left=-1)),
               dict(desc=edit(0, top=1)),                       # 32 rows from row 1 of 32
               dict(desc=edit(1, left=good[1]["ow"] - 31)),     # one column past the right edge
               dict(ch=33),                                     # a window taller than oh = 32
               dict(src_bytes=nbytes - 1),                      # the last image runs past the buffer
               dict(desc=edit(1, offset=good[1]["offset"] + 1)),
               dict(ws=ws[4:])):                                # workspace off its 16-byte boundary
        assert call(**kw) == -1, kw
    # more than 65 taps on either axis
    assert call(desc=edit(1, h=1025, oh=32, top=0), src_bytes=1 << 40) == -2
    assert call(desc=edit(1, w=33 * 42 + 1, ow=42, left=0), src_bytes=1 << 40) == -2
    assert call(n=0) == 0            # nothing to launch
    assert not y.any() and not ws.any()


def test_workspace_size_and_envelope_edge(lib):
    from qconvnet import preprocess as P
    size, stride = lib.qcn_resize_crop_workspace_size, lib.qcn_resize_crop_tap_stride
    d = P.plan([(24, 31), (97, 129)], 32, 32)
    for f in (size, stride):
        assert f(None, 2, 32, 32) == -1 and f(_descp(d), -1, 32, 32) == -1
        assert f(_descp(d), 2, 0, 32) == -1 and f(_descp(d), 2, 32, 0) == -1
        assert f(_descp(d), 2, 33, 32) == -1                 # window outside (oh, ow)
    assert size(_descp(d), 0, 32, 32) == 0
    # a record holds xmin, the count and the most taps of the batch: 97 -> 32 has 7
    assert stride(_descp(d), 2, 32, 32) >= 2 + 7
    assert stride(_descp(d[:1]), 1, 32, 32) >= 2 + 3
    # room for every record and for the rows of the intermediate each image needs
    for sizes, r, c in (([(24, 31), (97, 129)], 32, 32), ([(375, 500), (500, 333)], 256, 224),
                        ([(1024, 1024)], 32, 32), ([(100, 83)], 40, 25)):
        d = P.plan(sizes, r, c)
        n, s = len(d), stride(_descp(d), len(d), c, c)
        taps = rows = 0
        for e in d:
            vt = R.coeffs(int(e["h"]), int(e["oh"]), int(e["top"]), c)
            ht = R.coeffs(int(e["w"]), int(e["ow"]), int(e["left"]), c)
            taps = max([taps] + [len(k) for _, k in vt + ht])
            rows = max(rows, vt[-1][0] + len(vt[-1][1]) - vt[0][0])
        assert s >= 2 + taps
        total = size(_descp(d), n, c, c)
        assert total >= n * 2 * c * s * 4 + n * rows * c * 3, (sizes, total)
        assert total <= n * 2 * c * s * 4 + n * ((rows + 3) * c * 3 + 16), (sizes, total)
    # the envelope: a square of side 32 R is accepted, 32 R + 1 refused
    for r in (32, 73, 256):
        c = min(r, 224)
        ok, bad = P.plan([(32 * r, 32 * r)], r, c), P.plan([(32 * r + 1, 32 * r + 1)], r, c)
        assert size(_descp(ok), 1, c, c) > 0 and stride(_descp(ok), 1, c, c) >= 2 + 65
        assert size(_descp(bad), 1, c, c) == -2 and stride(_descp(bad), 1, c, c) == -2
    # one image outside the envelope refuses the batch
    mixed = P.plan([(24, 31), (1025, 1025)], 32, 32)
    assert size(_descp(mixed), 2, 32, 32) == -2
    from qconvnet import ops
    with pytest.raises(ValueError):
        ops.resize_crop_workspace_size(mixed, 32, 32)
    d = P.plan([(24, 31), (97, 129)], 32, 32)
    assert ops.resize_crop_workspace_size(d, 32, 32) == (size(_descp(d), 2, 32, 32), stride(_descp(d), 2, 32, 32))
