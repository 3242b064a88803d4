"""CPU: the synthetic ResNet conv cases of tests/resnetops.py are what they
claim to be, and the library's form queries (qcn_conv_gemm_form,
qcn_conv1x1_join_reduce_form: the launch's own dispatch, recording instead of
launching) pick the kernel family and instantiation the case matrix expects.

* coverage: every case the GPU file uses is built here once; the builder
  asserts the DESIGN section 3 conditions on the oracle's bytes (both clamps,
  the levels between, the joined and the reduced output, .5 ties);
* determinism: a case rebuilt from its seed is the same bytes;
* forms: every host-decidable field of the reported form against
  resnetops.expected_form, with zo1 / zo2 agreeing with qcn_join_affine;
* oracle: conv_q -> add_relu_q -> conv_q against a direct int64 / float64
  evaluation of one join-reduce case.
Host-only: no device work is called."""
import os

import numpy as np
import pytest

import resnetops as R
from oracle import qref

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from qconvnet import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libqconvnet.so missing — run __graft_entry__.build()")
    return _lib.load()


def _conv_form(c, join=None):
    from qconvnet import ops
    e = c["e"]
    resid = None if join is None else (None, join["s_r"], join["z_r"], join["s_o"], join["z_o"])
    return ops.conv_gemm_form(c["qx"].shape, e["z_x"], R.host_layer(e), resid=resid)


def _check_conv(c, join=None):
    f = _conv_form(c, join)
    streams = f["family"] in ("stream", "stream_s2")
    assert (f["nchunk"], f["per"]) == ((-1, -1) if streams else (0, 0))     # asked without the device
    want = R.expected_form(c["qx"].shape, c["e"], None if join is None else join["zo"])
    assert R.host_fields(f) == want, (c["key"], f, want)
    if f["family"] in ("stream", "stream_s2"):
        assert f["nstrip"] == -(-c["ref"][..., 0].size // 32)
    return f


# ---------------------------------------------------------------- coverage
def _levels(c, lo):
    at_lo, at_hi, levels, distinct = R.coverage(c["ref"], lo)
    assert at_lo >= 0.02 and at_hi >= 0.02 and levels >= 0.90 and distinct >= 64
    return at_lo, at_hi


@pytest.mark.parametrize("group", ["STREAM", "STREAM_S2", "TILED", "IMG", "PATCH"])
def test_conv_cases_cover_and_dispatch(lib, group):
    """Per conv case: the coverage conditions (asserted by the builder and
    again here), full-range weights, the scale spread, and the form the
    dispatch reports."""
    seen = set()
    for key in getattr(R, group):
        c = R.conv_case(*key)
        e = c["e"]
        at_lo, at_hi = _levels(c, R.lo_of(e))
        print(f"{group} {key}: z_y {e['z_y']} at_lo {at_lo:.3f} at_255 {at_hi:.3f}")
        assert e["w"].min() == -128 and e["w"].max() == 127 and e["z_x"] == key[-1]
        if key[9]:
            assert e["s_w"].max() / e["s_w"].min() >= 7.9
        if group == "PATCH":      # qcn_conv3x3_u8s8_nhwc is an entry of its own
            continue
        f = _check_conv(c)
        seen.add((f["family"], f["bn"], f["nw"], f["k"], f["rq"]))
    if group == "STREAM":
        assert seen == {("stream", 0, nw, k, rq) for k in (64, 128, 256, 512) for nw in (4, 2)
                        if nw == 4 or k <= 256 for rq in (0, 1, 2)}
    if group == "STREAM_S2":
        assert seen == {("stream_s2", 0, 4, k, rq) for k in (256, 512) for rq in (0, 1)}
    if group == "TILED":
        assert seen == {("tiled", bn, 8 if bn == 256 else 4, 0, rq) for bn in (64, 128, 256) for rq in (0, 1, 2)}
    if group == "IMG":
        assert seen == {("img", 0, 8, 0, 2)}


def test_join_cases_cover_and_dispatch(lib):
    """Joined outputs saturate at both ends; zo1 / zo2 are what
    qcn_join_affine answers, and the streaming dispatch reports them (the tiled
    kernel has no one-fma form: 1 for both)."""
    seen = set()
    for key, zo, z_r in R.STREAM_JOIN + R.TILED_JOIN:
        j = R.join_case(lib, key, zo, z_r)
        _levels(j, j["z_o"])
        assert (j["z_o"] != 0) == (zo == "zo0") and j["z_r"] == z_r
        if zo != "zo0":
            assert (j["affine"] is not None) == (zo == "zo2")
        f = _check_conv(j["conv"], j)
        seen.add((f["family"], f["k"], f["bn"], f["rq"], f["zo"]))
    assert {s for s in seen if s[0] == "stream"} == \
        {("stream", k, 0, rq, zo) for k in (64, 128, 256, 512) for rq in (0, 1) for zo in (0, 1, 2)}
    assert {s[2:] for s in seen if s[0] == "tiled"} >= {(bn, 1, zo) for bn in (64, 128) for zo in (0, 1)}
    assert len({z for _, _, z in R.STREAM_JOIN}) >= 6     # the identity zero point varies


def test_join_affine_constants_reproduce_the_join(lib):
    """The one-fma constants of every zo2 case, over all 256 x 256 byte pairs:
    sat(rne(fma(y, a, fma(r, b, c)))) equals the join's op sequence as
    qref.add_relu_q evaluates it."""
    y, r = (t.astype(np.uint8) for t in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    done = set()
    for key, zo, z_r in R.STREAM_JOIN:
        if zo != "zo2":
            continue
        j = R.join_case(lib, key, zo, z_r)
        e = j["conv"]["e"]
        qp = (e["s_y"], e["z_y"], j["s_r"], j["z_r"], j["s_o"])
        a, b, c = (F32(t) for t in j["affine"])
        v = qref.fmaf(y.astype(F32), a, qref.fmaf(r.astype(F32), b, np.full(y.shape, c, F32)))
        got = np.clip(np.rint(v), 0, 255).astype(np.uint8)
        assert np.array_equal(got, qref.add_relu_q(y, qp[0], qp[1], r, qp[2], qp[3], qp[4], 0)), qp
        done.add(qp)
    assert len(done) == 8


def test_join_reduce_cases_cover_and_dispatch(lib):
    from qconvnet import ops
    seen = set()
    for key, zo, z_r, cr, form in R.JOIN_REDUCE:
        c = R.reduce_case(lib, key, zo, z_r, cr, form)
        j, e = c["join"], c["e"]
        _levels(c, R.lo_of(e))
        assert (e["z_x"], e["s_x"]) == (j["z_o"], j["s_o"])
        assert (e["relu"], e["z_y"] == 0) == {"relu_z0": (True, True), "relu_z": (True, False),
                                              "norelu_z": (False, False)}[form]
        resid = (None, j["s_r"], j["z_r"], j["s_o"], j["z_o"])
        f = ops.conv_join_reduce_form(j["conv"]["qx"].shape, j["conv"]["e"]["z_x"], R.host_layer(j["conv"]["e"]),
                                      resid, R.host_layer(e))
        assert R.host_fields(f) == R.expected_reduce_form(j["conv"]["e"], j["zo"], cr)
        assert f["nstrip"] == 6
        seen.add((cr, f["rq"], f["zo"], form))
    assert len(seen) == 36
    # outside the envelope the query answers what the launch would
    j = R.join_case(lib, R.STREAM_JOIN[3][0], "zo0", R.STREAM_JOIN[3][2])
    other = R.host_layer(R.conv_case(*R.STREAM[0])["e"])      # 256 output channels: no fused reduce
    assert ops.conv_join_reduce_form(j["conv"]["qx"].shape, 5, R.host_layer(j["conv"]["e"]),
                                     (None, j["s_r"], j["z_r"], j["s_o"], j["z_o"]), other) is None


def test_ties_and_stem_cases(lib):
    for args in R.TIES_STREAM + R.TIES_TILED:
        c = R.ties_case(*args)
        assert c["ties"] >= 0.01
        print(f"ties {args}: share of unclamped outputs on an exact .5: {c['ties']:.3f}")
        _levels(c, R.lo_of(c["e"]))
        _check_conv(c)
    for kind, pc in R.STEM:
        c = R.stem_case(kind, pc)
        f = _check_conv(dict(key=c["key"], qx=c["rows"], e=c["e"], ref=c["conv"]))
        assert (f["family"], f["bn"]) == ("tiled", 64)
        assert np.unique(c["q"]).size == 256
    for kind in R.TIES_STEM:
        R.stem_case(kind, False, True)


def test_long_cases(lib):
    """The steady-state cases: an 8-image pool each, one per streaming
    instantiation family; the strip plan itself needs the device."""
    fams = set()
    for key, zo, red in R.LONG:
        z_r = R.zr(key[3], zo)
        if red:
            c = R.reduce_case(lib, key, zo, z_r, *red)
            fams.add(("join_reduce", red[0]))
        elif zo:
            j = R.join_case(lib, key, zo, z_r)
            f = _check_conv(j["conv"], j)
            fams.add((f["family"], f["k"], f["rq"], f["zo"]))
        else:
            f = _check_conv(R.conv_case(*key))
            fams.add((f["family"], f["k"], f["rq"], f["zo"]))
        assert key[0] == R.POOL
    assert len(fams) == len(R.LONG)
    ncu = 256
    for cg, p in ((2, 4), (2, 3), (1, 4)):
        strips = R.strips_for(ncu, cg, p)
        n = R.long_batch(strips)
        nstrip = -(-n * 196 // 32)
        nchunk = (ncu * 4 // cg) & ~7
        per = -(-nstrip // nchunk)
        assert per >= p + 2 and nstrip % per != 0


def test_form_query_arguments(lib):
    """The query runs the launch's own argument checks."""
    import ctypes as C
    from qconvnet import _lib
    f = _lib.ConvForm()
    q = lambda *a: lib.qcn_conv_gemm_form(*a, C.byref(f))  # noqa: E731
    #           n  h  w  cin zx cout kh kw sy sx py px zy relu resid
    assert q(3, 7, 9, 64, 5, 256, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0.0, 0.0, 0, 0.0, 0, 0) == 0
    assert (f.family, f.k, f.nw, f.rq, f.zo, f.p, f.nstrip, f.per) == (1, 64, 4, 0, -1, 4, 6, -1)
    assert q(3, 7, 9, 64, 5, 256, 1, 1, 1, 1, 0, 0, 300, 1, 0, 0.0, 0.0, 0, 0.0, 0, 0) == _lib.QCN_ERR_ARG
    assert q(3, 7, 9, 48, 5, 256, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0.0, 0.0, 0, 0.0, 0, 0) == _lib.QCN_ERR_UNSUPPORTED
    # a join rejects a ReLU of the conv's own, and needs its scales
    assert q(3, 7, 9, 64, 5, 256, 1, 1, 1, 1, 0, 0, 0, 1, 1, 0.1, 0.1, 0, 0.1, 0, 0) == _lib.QCN_ERR_ARG
    assert q(3, 7, 9, 64, 5, 256, 1, 1, 1, 1, 0, 0, 0, 0, 1, 0.1, 0.0, 0, 0.1, 0, 0) == _lib.QCN_ERR_ARG
    assert lib.qcn_conv_gemm_form(3, 7, 9, 64, 5, 256, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0.0, 0.0, 0, 0.0, 0, 0,
                                  None) == _lib.QCN_ERR_ARG
    # the probe does not outlive the query: a launch with missing tensors is still refused
    assert lib.qcn_conv_gemm_u8s8_nhwc(None, 3, 7, 9, 64, 5, None, 256, 1, 1, 1, 1, 0, 0, None, None, None, None,
                                       0, 1, None, 0.0, 0.0, 0, 0.0, 0, None, None) == _lib.QCN_ERR_ARG


def test_cases_are_deterministic(lib):
    key, zo, z_r, cr, form = R.JOIN_REDUCE[7]
    first = R.reduce_case(lib, key, zo, z_r, cr, form)
    for fn in (R.conv_case, R._join_walk, R.join_case, R.reduce_case):
        fn.cache_clear()
    again = R.reduce_case(lib, key, zo, z_r, cr, form)
    assert again is not first
    for a, b in ((first["ref"], again["ref"]), (first["join"]["ref"], again["join"]["ref"]),
                 (first["join"]["r"], again["join"]["r"]), (first["join"]["conv"]["qx"], again["join"]["conv"]["qx"]),
                 (first["e"]["w"], again["e"]["w"]), (first["e"]["b"], again["e"]["b"])):
        assert np.array_equal(a, b)
    assert (first["join"]["s_r"], first["join"]["s_o"], first["e"]["s_y"]) == \
        (again["join"]["s_r"], again["join"]["s_o"], again["e"]["s_y"])
    t = R.ties_case(*R.TIES_STREAM[0])
    R.ties_case.cache_clear()
    assert np.array_equal(t["qx"], R.ties_case(*R.TIES_STREAM[0])["qx"])


def _requant_direct(acc, e):
    """clamp(rne(fp32(fp32(acc) + u v) * mult) + z_y) with the fma evaluated in
    float64 (exact for these magnitudes up to the one rounding to fp32)."""
    u, v, m = (a.astype(np.float64) for a in R.consts(e))
    t = (acc.astype(np.float64) + u * v).astype(F32)           # |acc + u v| < 2^53: one rounding
    ab = (t.astype(np.float64) * m).astype(F32)
    r = np.rint(ab.astype(np.float64)).astype(np.int64) + e["z_y"]
    return np.clip(r, R.lo_of(e), 255).astype(np.uint8)


def test_join_reduce_oracle_against_direct_evaluation(lib):
    """qref.conv_q -> add_relu_q -> conv_q, as the GPU tests compose them,
    against int64 sums and float64 arithmetic written out here."""
    key, zo, z_r, cr, form = R.JOIN_REDUCE[4]     # rq0n, zo1, norelu_z
    c = R.reduce_case(lib, key, zo, z_r, cr, form)
    j, e2 = c["join"], c["e"]
    e1, qx = j["conv"]["e"], j["conv"]["qx"]
    w1 = e1["w"][:, :, 0, 0].astype(np.int64)
    acc1 = (qx.astype(np.int64) - e1["z_x"]) @ w1.T
    y3 = _requant_direct(acc1, e1)
    assert np.array_equal(y3, j["conv"]["ref"])
    a = ((y3.astype(np.float64) - e1["z_y"]) * float(e1["s_y"])).astype(F32)      # exact product, one rounding
    b = ((j["r"].astype(np.float64) - j["z_r"]) * float(j["s_r"])).astype(F32)
    s = np.maximum((a.astype(np.float64) + b.astype(np.float64)).astype(F32), F32(0))
    inv = F32(1.0) / F32(j["s_o"])
    qj = np.clip(np.rint((s.astype(np.float64) * float(inv)).astype(F32)).astype(np.int64) + j["z_o"], 0, 255)
    assert np.array_equal(qj.astype(np.uint8), j["ref"])
    acc2 = (qj - j["z_o"]) @ e2["w"][:, :, 0, 0].astype(np.int64).T
    assert np.array_equal(_requant_direct(acc2, e2), c["ref"])
    # and the composition the GPU file calls
    u, v, m = R.consts(e1)
    y = qref.conv_q(qx, e1["z_x"], e1["w"], u, v, m, e1["z_y"], False)
    q = qref.add_relu_q(y, e1["s_y"], e1["z_y"], j["r"], j["s_r"], j["z_r"], j["s_o"], j["z_o"])
    u, v, m = R.consts(e2)
    assert np.array_equal(qref.conv_q(q, j["z_o"], e2["w"], u, v, m, e2["z_y"], e2["relu"]), c["ref"])
