"""CPU: the C-ABI library loads, exports every symbol include/qconvnet.h
declares, and its host-side (packing) entry points are correct.  No device
compute is called here."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qconvnet.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(qcn_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from qconvnet import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libqconvnet.so missing — run __graft_entry__.build()")
    return _lib.load()


def test_every_declared_symbol_is_exported(lib):
    names = _declared()
    assert len(names) >= 15
    missing = [n for n in names if not hasattr(lib, n)]
    assert missing == []


def test_binding_covers_header():
    from qconvnet import _lib
    assert set(_declared()) == set(_lib.SIGNATURES)


def test_version(lib):
    assert lib.qcn_version() >= 100


def test_pack_conv3x3_layout(lib):
    from qconvnet import ops
    rng = np.random.default_rng(0)
    for cin, cout in ((64, 64), (128, 256), (3, 64), (48, 32)):
        w = rng.integers(-128, 128, (cout, cin, 3, 3)).astype(np.int8)
        packed, wsum = ops.pack_conv3x3(w)
        assert np.array_equal(wsum, w.reshape(cout, -1).astype(np.int64).sum(1))
        ohwi = w.transpose(0, 2, 3, 1).reshape(cout, 9, cin)
        if cin % 64 == 0 and cout % 64 == 0:
            # [chunk = tap*(cin/64) + cb][cout][64]
            p = packed.reshape(9, cin // 64, cout, 64)
            ref = ohwi.reshape(cout, 9, cin // 64, 64).transpose(1, 2, 0, 3)
            assert np.array_equal(p, ref)
        else:
            assert np.array_equal(packed.reshape(cout, 9, cin), ohwi)


def test_pack_conv1_layout(lib):
    from qconvnet import ops
    w = np.random.default_rng(1).integers(-128, 128, (64, 3, 3, 3)).astype(np.int8)
    packed, wsum = ops.pack_conv1(w)
    p = packed.reshape(64, 32)
    assert np.all(p[:, 27:] == 0)
    ref = w.transpose(0, 2, 3, 1).reshape(64, 27)  # k = tap*3 + c
    assert np.array_equal(p[:, :27], ref)
    assert np.array_equal(wsum, ref.astype(np.int64).sum(1))


def test_bad_arguments_return_status(lib):
    import ctypes as C
    assert lib.qcn_pack_conv3x3_weight(None, 64, 64, None, None) == -1
    assert lib.qcn_conv3x3_u8s8_nhwc(None, 1, 8, 8, 64, 0, None, 64, None, None, None, None, 0, 1,
                                     0, None, None, None) == -1
    assert lib.qcn_quantize_f32_u8(None, None, 1, 1, 1, 1, 0, C.c_float(1.0), 0, None) == -1
    assert lib.qcn_linear_u8s8(None, 1, 1, 0, None, 1, None, None, None, None, 0, 0, None, None,
                               C.c_float(1.0), None) == -1


def _conv_status_cases(lib):
    """(label, status) of every SimpleConvNet conv entry for arguments it must
    refuse on the host: every call here returns before the first HIP call, so
    the table holds with and without a GPU.  The pointers are never read."""
    import ctypes as C
    from qconvnet import _lib
    buf = np.zeros(64, np.uint8)
    P = buf.ctypes.data + (-buf.ctypes.data % 16)   # any aligned non-null address
    BIG = (1 << 19) + 1                             # nimg * 4096 > 2^31 - 1
    one = C.c_float(1.0)
    cases = []

    def add(label, rc):
        cases.append((label, int(rc)))

    def bad_zps(name, call, zps):
        """call(**{zp: value}) for -1 and 256 in each zero-point argument."""
        for zp in zps:
            for val in (-1, 256):
                add(f"{name} {zp}={val}", call(**{zp: val}))

    # ---- conv3+4 / conv5+6 pair (hw 5: no kernel, so a case the checks let
    # through would still stop at the shape)
    def pair(x=P, nimg=4, x_zp=1, wa=P, zmid=2, y_zp=3, y=P, kmajor=0):
        return lib.qcn_conv3x3_pair_u8s8(x, nimg, 5, 64, x_zp, wa, 128, P, P, P, P, zmid, 1, None, P, 128,
                                         P, P, P, P, y_zp, 1, None, kmajor, y, None)
    add("pair x=null", pair(x=None))
    add("pair wa=null", pair(wa=None))
    add("pair y=null", pair(y=None))
    add("pair nimg=0", pair(nimg=0))
    bad_zps("pair", pair, ("x_zp", "zmid", "y_zp"))
    add("pair kmajor nimg=big", pair(nimg=BIG, kmajor=1))
    add("pair kmajor nimg=big y_zp=256", pair(nimg=BIG, kmajor=1, y_zp=256))

    # ---- chunk-major conv6
    def km(x=P, nimg=4, h=8, w=8, x_zp=1, y_zp=3, pool=1, y=P):
        return lib.qcn_conv3x3_u8s8_kmajor(x, nimg, h, w, 128, x_zp, P, 256, P, P, P, P, y_zp, 1, pool, y,
                                           None)
    add("kmajor x=null", km(x=None))
    add("kmajor y=null", km(y=None))
    add("kmajor nimg=0", km(nimg=0))
    bad_zps("kmajor", km, ("x_zp", "y_zp"))
    add("kmajor pool odd", km(h=7, w=7))
    add("kmajor 16x16", km(h=16, w=16))
    add("kmajor 16x16 y_zp=-1", km(h=16, w=16, y_zp=-1))
    add("kmajor nimg=big", km(nimg=BIG))

    # ---- conv1+conv2, fp32 and raw-u8 input
    def c12(x=P, nimg=4, in_scale=1.0, in_zp=1, w1=P, z1=2, x2_zp=2, y_zp=3, y=P):
        return lib.qcn_conv12_fused_f32_nchw(x, nimg, C.c_float(in_scale), in_zp, w1, P, P, P, P, z1, 1, None,
                                             x2_zp, P, P, P, P, P, y_zp, 1, None, y, None)

    def c12u(x=P, nimg=4, qlut=P, in_zp=1, w1=P, z1=2, x2_zp=2, y_zp=3, y=P):
        return lib.qcn_conv12_fused_u8_nhwc(x, nimg, qlut, in_zp, w1, P, P, P, P, z1, 1, None, x2_zp, P, P, P,
                                            P, P, y_zp, 1, None, y, None)
    for name, f in (("conv12", c12), ("conv12_u8", c12u)):
        add(f"{name} x=null", f(x=None))
        add(f"{name} w1=null", f(w1=None))
        add(f"{name} y=null", f(y=None))
        add(f"{name} nimg=0", f(nimg=0))
        bad_zps(name, f, ("in_zp", "z1", "x2_zp", "y_zp"))
    add("conv12 in_scale=0", c12(in_scale=0.0))
    add("conv12 in_scale=nan", c12(in_scale=float("nan")))
    add("conv12_u8 qlut=null", c12u(qlut=None))
    add("conv12_u8 img misaligned", c12u(x=P + 1))

    # ---- stand-alone conv1 (hw 7: no kernel)
    def c1(x=P, nimg=4, in_scale=1.0, in_zp=1, y_zp=3, y=P):
        return lib.qcn_conv1_f32_nchw(x, nimg, 7, C.c_float(in_scale), in_zp, P, P, P, P, P, y_zp, 1, None, y,
                                      None, None)
    add("conv1 x=null", c1(x=None))
    add("conv1 y=null", c1(y=None))
    add("conv1 nimg=0", c1(nimg=0))
    add("conv1 in_scale=0", c1(in_scale=0.0))
    bad_zps("conv1", c1, ("in_zp", "y_zp"))

    # ---- the layer-array entries
    def layers(k, first_zp=1, edit=None, qdq_at=None):
        """k chained layers (x_zp first_zp, 11, 12, ...); edit(arr) breaks one."""
        arr = (_lib.ConvLayer * k)()
        keep = []
        for i in range(k):
            arr[i] = _lib.ConvLayer(P, P, P, P, P, first_zp if i == 0 else 10 + i, 11 + i, 1, None)
        if qdq_at is not None:   # the next layer then reads z2 = 77, not y_zp
            q = _lib.QDQ(1.0, arr[qdq_at].y_zp, 1.0, 77)
            keep.append(q)
            arr[qdq_at].qdq = C.pointer(q)
        if edit:
            edit(arr)
        return arr, keep

    def setf(i, field, val):
        def edit(arr):
            setattr(arr[i], field, val)
        return edit

    def form(nimg=4, in_scale=1.0, in_zp=1, L=None, **kw):
        arr, keep = layers(6, **kw) if L is None else (L, None)
        return lib.qcn_convnet_convs_form(nimg, C.c_float(in_scale), in_zp, arr, 1)

    def convs(x=P, nimg=4, in_scale=1.0, in_zp=1, a2=P, a6=P, L=None, **kw):
        arr, keep = layers(6, **kw) if L is None else (L, None)
        return lib.qcn_convnet_convs_f32_nchw(x, nimg, C.c_float(in_scale), in_zp, arr, a2, P, a6, 1, None)

    def convsu(x=P, nimg=4, qlut=P, in_zp=1, a2=P, a6=P, L=None, **kw):
        arr, keep = layers(6, **kw) if L is None else (L, None)
        return lib.qcn_convnet_convs_u8_nhwc(x, nimg, qlut, in_zp, arr, a2, P, a6, 1, None)

    def c36(x=P, nimg=4, a4=P, a6=P, L=None, **kw):
        arr, keep = layers(4, **kw) if L is None else (L, None)
        return lib.qcn_convs36_u8s8(x, nimg, arr, a4, a6, 1, None)

    null_layers = C.POINTER(_lib.ConvLayer)()
    for name, f, k in (("form", form, 6), ("convs", convs, 6), ("convs_u8", convsu, 6), ("convs36", c36, 4)):
        add(f"{name} layers=null", f(L=null_layers))
        add(f"{name} nimg=0", f(nimg=0))
        add(f"{name} layer0.w=null", f(edit=setf(0, "w", None)))
        add(f"{name} layer3.corr=null", f(edit=setf(3, "corr", None)))
        add(f"{name} layer{k - 1}.mult=null", f(edit=setf(k - 1, "mult", None)))
        for val in (-1, 256):
            add(f"{name} layer0.x_zp={val}", f(first_zp=val))
            add(f"{name} layer2.x_zp={val}", f(edit=setf(2, "x_zp", val)))
            add(f"{name} layer1.y_zp={val}", f(edit=setf(1, "y_zp", val)))
            add(f"{name} layer{k - 1}.y_zp={val}", f(edit=setf(k - 1, "y_zp", val)))
        add(f"{name} chain broken at 2", f(edit=setf(2, "x_zp", 99)))
        add(f"{name} chain ignores qdq.z2", f(qdq_at=1))
        add(f"{name} nimg=big", f(nimg=BIG))
        add(f"{name} nimg=big chain broken", f(nimg=BIG, edit=setf(3, "x_zp", 99)))
        if name != "convs36":
            add(f"{name} in_zp != layer0.x_zp", f(in_zp=2))
            bad_zps(name, f, ("in_zp",))
        if name in ("form", "convs"):
            add(f"{name} in_scale=0", f(in_scale=0.0))
    add("convs x=null", convs(x=None))
    add("convs a2=null", convs(a2=None))
    add("convs a6=null", convs(a6=None))
    add("convs_u8 x=null", convsu(x=None))
    add("convs_u8 qlut=null", convsu(qlut=None))
    add("convs_u8 a6=null", convsu(a6=None))
    add("convs_u8 img misaligned", convsu(x=P + 1))
    add("convs36 a2=null", c36(x=None))
    add("convs36 a4=null", c36(a4=None))
    add("convs36 a6=null", c36(a6=None))
    # layers 0, 1 on the fast epilogue (y_zp 0), 2, 3 general: mixed forms
    mixed, _ = layers(4, edit=lambda a: [setf(0, "y_zp", 0)(a), setf(1, "x_zp", 0)(a), setf(1, "y_zp", 0)(a),
                                         setf(2, "x_zp", 0)(a)])
    add("convs36 mixed forms", c36(L=mixed))
    add("convs36 mixed forms nimg=big", c36(L=mixed, nimg=BIG))
    return cases


# QCN_ERR_UNSUPPORTED (-2) where listed, QCN_ERR_ARG (-1) everywhere else
CONV_STATUS_UNSUPPORTED = {
    "pair kmajor nimg=big", "kmajor 16x16", "kmajor nimg=big",
    "conv1 y_zp=-1", "conv1 y_zp=256",   # conv1's output zero point is not range-checked: the shape refuses
    "form nimg=big", "convs nimg=big", "convs_u8 nimg=big", "convs36 nimg=big",
    "convs36 mixed forms", "convs36 mixed forms nimg=big",
}


def test_conv_entries_bad_argument_statuses(lib):
    """The status of every SimpleConvNet conv entry for null pointers, an empty
    batch, zero points of -1 and 256 in each zero-point argument, a layer
    with a null field, a broken x_zp chain, in_zp != layers[0].x_zp, mixed
    epilogue forms and batches past the 32-bit offsets (and, where two
    defects meet, which check comes first)."""
    cases = _conv_status_cases(lib)
    assert len(cases) == len(set(label for label, _ in cases))
    got = {label for label, rc in cases if rc == -2}
    wrong = [(label, rc) for label, rc in cases if rc not in (-1, -2)]
    assert wrong == []
    assert got == CONV_STATUS_UNSUPPORTED


def test_product_fails_loudly_without_library(monkeypatch, tmp_path):
    """The int8 path has no CPU fallback: a missing .so raises.  (monkeypatch
    puts LIB_PATH and the loaded handle back; reloading the module here would
    leave that handle declared with the previous module's ctypes classes, and
    every later test in the same process that passes a struct would fail.)"""
    from qconvnet import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.QcnError):
        _lib.load()
