"""GPU: the ResNet conv kernels at full range, in every epilogue and join form,
bit for bit against oracle.qref on the synthetic cases of tests/resnetops.py
(full-range weights, outputs that saturate at both clamps, identity zero
points that vary, exact .5 ties).  Every case first asserts the form the
library reports for it (qcn_conv_gemm_form / qcn_conv1x1_join_reduce_form, the
launch's own dispatch), so that no case passes on another kernel than the one
it names.

Short cases run 3 x 7 x 9 = 189 pixels (a ragged last strip / tile) unless the
kernel fixes the map.  Long cases gather a batch from an 8-image pool on the
device (convchain.batch's index rule), sized from the device's CU count so
that every chunk of the streaming kernel walks at least P + 2 strips (its
counted-vmcnt ring past the first round) and the last chunk is shorter; only
the pool crosses PCIe, and the expected result is oracle[idx]."""
import numpy as np
import pytest
import torch

import convchain as CC
import resnetops as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from qconvnet import _lib
    return _lib.load()


def _T(dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)    # a copy: the cases' arrays are read-only


def _layer(dev, e):
    """Device-side layer of an entry: k-major weights, requant constants."""
    from qconvnet import ops
    d = R.host_layer(e)
    packed, wsum = ops.pack_conv_kmajor(e["w"])
    u, v, mult = R.consts(e)
    d.w, d.u, d.v, d.mult = _T(dev, packed), _T(dev, u), _T(dev, v), _T(dev, mult)
    d.corr = _T(dev, ((128 - int(e["z_x"])) * wsum.astype(np.int64)).astype(np.int32))
    return d


def _resid(dev, j):
    return (None if dev is None else _T(dev, j["r"]), j["s_r"], j["z_r"], j["s_o"], j["z_o"])


def _same(label, got, want):
    msg = CC.mismatch(label, got.cpu().numpy(), np.asarray(want), np.arange(got.shape[0]))
    assert msg is None, msg


def _conv(dev, c, d, impl="gemm", join=None, x=None):
    """One launch into a poisoned output buffer; on the GEMM path the form the
    library reports is asserted first."""
    from qconvnet import ops
    e = c["e"]
    x = _T(dev, c["qx"]) if x is None else x
    resid = None if join is None else _resid(dev, join)
    if impl == "gemm":
        f = ops.conv_gemm_form(x.shape, e["z_x"], d, resid=resid, device=True)
        want = R.expected_form(tuple(x.shape), e, None if join is None else join["zo"])
        assert R.host_fields(f) == want, (f, want)
        if f["family"] in ("stream", "stream_s2"):
            assert f["per"] >= 1 and (f["nchunk"] - 1) * f["per"] < f["nstrip"] <= f["nchunk"] * f["per"], f
    n, h, w, _ = x.shape
    oh, ow = (h + 2 * d.py - d.kh) // d.sy + 1, (w + 2 * d.px - d.kw) // d.sx + 1
    out = torch.full((n, oh, ow, d.cout), 0xA5, dtype=torch.uint8, device=dev)
    ops.conv(x, e["z_x"], d, out=out, resid=resid, impl=impl)
    torch.cuda.synchronize()
    return out


def _ids(cases):
    def one(c):
        if isinstance(c, str):
            return c
        key, rest = (c, ()) if isinstance(c[0], int) else (c[0], c[1:])
        n, h, w, cin, cout, k, s = key[:7]
        name = f"{n}x{h}x{w}x{cin}-{cout}-{k[0]}x{k[1]}s{s[0]}-{key[8]}-{'pc' if key[9] else 'pt'}"
        for r in rest:
            if isinstance(r, tuple):
                name += "-" + "-".join(str(t) for t in r)
            elif r is not None:
                name += f"-{r}"
        return name
    return [one(c) for c in cases]


# ------------------------------------------------------------------ stream
@pytest.mark.parametrize("key", R.STREAM + R.STREAM_S2, ids=_ids(R.STREAM + R.STREAM_S2))
def test_stream(dev, key):
    """conv1x1_stream_kernel without a join: K x NW x RQ, per-channel and
    per-tensor, and the stride-2 form."""
    c = R.conv_case(*key)
    _same("y", _conv(dev, c, _layer(dev, c["e"])), c["ref"])


@pytest.mark.parametrize("case", R.STREAM_JOIN, ids=_ids(R.STREAM_JOIN))
def test_stream_join(dev, lib, case):
    """K x RQ {0, 1} x ZO {0, 1, 2}: the joined bytes saturate at both ends."""
    key, zo, z_r = case
    j = R.join_case(lib, key, zo, z_r)
    _same("joined", _conv(dev, j["conv"], _layer(dev, j["conv"]["e"]), join=j), j["ref"])


@pytest.mark.parametrize("case", R.JOIN_REDUCE, ids=_ids(R.JOIN_REDUCE))
def test_join_reduce(dev, lib, case):
    """The expand + join + fused reduce against the oracle and against the
    two separate launches."""
    from qconvnet import ops
    key, zo, z_r, cr, form = case
    c = R.reduce_case(lib, key, zo, z_r, cr, form)
    j = c["join"]
    e3, e1 = j["conv"]["e"], c["e"]
    d3, d1 = _layer(dev, e3), _layer(dev, e1)
    x, resid = _T(dev, j["conv"]["qx"]), _resid(dev, j)
    f = ops.conv_join_reduce_form(x.shape, e3["z_x"], d3, resid, d1, device=True)
    assert R.host_fields(f) == R.expected_reduce_form(e3, j["zo"], cr), f
    out = torch.full(j["ref"].shape, 0xA5, dtype=torch.uint8, device=dev)
    out2 = torch.full(c["ref"].shape, 0xA5, dtype=torch.uint8, device=dev)
    got = ops.conv_join_reduce(x, e3["z_x"], d3, resid, d1, out=out, out2=out2)
    assert got is not None, "the library declined a supported shape"
    torch.cuda.synchronize()
    _same("joined", out, j["ref"])
    _same("reduced", out2, c["ref"])
    q_sep = ops.conv(x, e3["z_x"], d3, resid=resid)
    y2_sep = ops.conv(q_sep, j["z_o"], d1)
    assert torch.equal(q_sep, out) and torch.equal(y2_sep, out2)


# ------------------------------------------------------------------- tiled
@pytest.mark.parametrize("impl", ["gemm", "gen"])
@pytest.mark.parametrize("key", R.TILED, ids=_ids(R.TILED))
def test_tiled(dev, key, impl):
    """conv_gemm_kernel at BN 64 / 128 / 256 in its three requant branches over
    3x3 s1, 3x3 s2, 1x1 K = 1024 and the 7x1 stem-row conv; the same cases on
    the register-direct kernel (impl gen)."""
    c = R.conv_case(*key)
    _same("y", _conv(dev, c, _layer(dev, c["e"]), impl=impl), c["ref"])


@pytest.mark.parametrize("case", R.TILED_JOIN, ids=_ids(R.TILED_JOIN))
def test_tiled_join(dev, lib, case):
    key, zo, z_r = case
    j = R.join_case(lib, key, zo, z_r)
    _same("joined", _conv(dev, j["conv"], _layer(dev, j["conv"]["e"]), join=j), j["ref"])


@pytest.mark.parametrize("key", R.IMG, ids=_ids(R.IMG))
def test_whole_image(dev, key):
    """conv3x3_img_kernel: 14 x 14 x 256 and 7 x 7 x 512, one and two channel groups."""
    c = R.conv_case(*key)
    _same("y", _conv(dev, c, _layer(dev, c["e"])), c["ref"])


@pytest.mark.parametrize("key", R.PATCH, ids=_ids(R.PATCH))
def test_patch_ring(dev, key):
    """qcn_conv3x3_u8s8_nhwc at the ResNet maps (56 x 56 x 64, 28 x 28 x 128)."""
    from qconvnet import ops
    c = R.conv_case(*key)
    e = c["e"]
    cout = e["w"].shape[0]
    packed, wsum = ops.pack_conv3x3(e["w"])
    u, v, m = R.consts(e)
    corr = ((128 - e["z_x"]) * wsum.astype(np.int64)).astype(np.int32)
    out = torch.full(c["ref"].shape, 0xA5, dtype=torch.uint8, device=dev)
    ops.conv3x3(_T(dev, c["qx"]), e["z_x"], _T(dev, packed), cout, _T(dev, u), _T(dev, v), _T(dev, m),
                _T(dev, corr), e["z_y"], e["relu"], False, out=out)
    torch.cuda.synchronize()
    _same("y", out, c["ref"])


# -------------------------------------------------------------------- stem
def _stem(dev, c, entry):
    from qconvnet import ops
    e = c["e"]
    d = _layer(dev, e)
    out = torch.full(c["ref"].shape, 0xA5, dtype=torch.uint8, device=dev)
    if entry == "f32":
        x = _T(dev, c["x"])
        ops.stem_fused(x, c["s_in"], R.STEM_ZP, d, out=out)
        rows = ops.stem_pack(x, c["s_in"], R.STEM_ZP)
    else:
        img, qlut = _T(dev, c["img"]), _T(dev, R.stem_qlut())
        ops.stem_fused_u8(img, qlut, R.STEM_ZP, d, out=out)
        rows = ops.stem_pack_u8(img, qlut, R.STEM_ZP)
    torch.cuda.synchronize()
    _same("rows", rows, c["rows"])
    _same("pooled", out, c["ref"])
    # the three launches it replaces, against the oracle's own stages
    conv = ops.conv(rows, R.STEM_ZP, d)
    _same("conv", conv, c["conv"])
    assert torch.equal(ops.maxpool3x3s2(conv), out)


@pytest.mark.parametrize("entry", ["f32", "u8"])
@pytest.mark.parametrize("kind,pc", R.STEM)
def test_stem_fused(dev, kind, pc, entry):
    """The fused stem (fp32 and raw-byte entry) against qref.stem_pack ->
    conv_q -> maxpool3x3s2_nhwc, in the three requant forms."""
    _stem(dev, R.stem_case(kind, pc), entry)


# -------------------------------------------------------------------- ties
@pytest.mark.parametrize("impl", ["gemm", "gen"])
@pytest.mark.parametrize("args", R.TIES_STREAM + R.TIES_TILED, ids=_ids(
    [a + (False, 0) for a in R.TIES_STREAM + R.TIES_TILED]))
def test_requant_ties(dev, args, impl):
    """About half of the unclamped requant inputs are exact .5 ties: round to
    nearest even in the pack-only and the rint forms."""
    c = R.ties_case(*args)
    _same("y", _conv(dev, c, _layer(dev, c["e"]), impl=impl), c["ref"])


@pytest.mark.parametrize("entry", ["f32", "u8"])
@pytest.mark.parametrize("kind", R.TIES_STEM)
def test_stem_ties(dev, kind, entry):
    _stem(dev, R.stem_case(kind, False, True), entry)


# ------------------------------------------------------------ steady state
def _plan(query, n0, p):
    """Batch and reported form with per >= p + 2 and a shorter last chunk: the
    batch sized from the CU count (occupancy <= 4) is grown only if the device
    plans more chunks than that, and by single images until the strip count is
    no multiple of ``per``."""
    n = n0
    f = query(n)
    if f["per"] < p + 2:
        n = max(n, R.long_batch(f["nchunk"] * (p + 1) + 1))
    for n in range(n, n + 8):
        f = query(n)
        if f["per"] >= p + 2 and f["nstrip"] % f["per"] != 0:
            break
    return n, f


@pytest.mark.parametrize("case", R.LONG, ids=_ids(R.LONG))
def test_stream_steady_state(dev, lib, case):
    """Every streaming instantiation family past its first ring round, with
    saturating outputs: per >= P + 2 strips per chunk, last chunk shorter,
    196-pixel images drifting against the 32-pixel strips."""
    from qconvnet import ops
    key, zo, red = case
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    z_r = R.zr(key[3], zo) if zo else None
    if red:
        c = R.reduce_case(lib, key, zo, z_r, *red)
        j = c["join"]
    else:
        c = None
        j = R.join_case(lib, key, zo, z_r) if zo else None
    conv = j["conv"] if j else R.conv_case(*key)
    e = conv["e"]
    d = _layer(dev, e)
    dn = _layer(dev, c["e"]) if red else None
    h, w, cin = conv["qx"].shape[1:]
    nw = 8 if red else 4
    p = 4 if red else R.STREAM_P[(cin, 4)]
    resid0 = _resid(None, j) if j else None

    def query(n):
        if red:
            return ops.conv_join_reduce_form((n, h, w, cin), e["z_x"], d, resid0, dn, device=True)
        return ops.conv_gemm_form((n, h, w, cin), e["z_x"], d, resid=resid0, device=True)

    n, f = _plan(query, R.long_batch(R.strips_for(ncu, 256 // (32 * nw), p)), p)
    print(f"n {n} form {f}")
    assert f["family"] == ("join_reduce" if red else "stream_s2" if e["stride"] == (2, 2) else "stream")
    assert (f["k"], f["p"], f["rq"], f["zo"]) == (cin, p, R.rq_of(e), j["zo"] if j else -1)
    assert f["per"] >= p + 2, f
    last = f["nstrip"] - (f["nchunk"] - 1) * f["per"]
    assert 0 < last < f["per"], f
    assert f["nstrip"] == -(-n * 196 // 32)

    idx = torch.from_numpy(CC.batch(n)).to(dev)
    x = _T(dev, conv["qx"])[idx].contiguous()
    if j:
        resid = (_T(dev, j["r"])[idx].contiguous(),) + resid0[1:]
        want = _T(dev, j["ref"])[idx]
    else:
        resid, want = None, _T(dev, conv["ref"])[idx]
    out = torch.full(want.shape, 0xA5, dtype=torch.uint8, device=dev)
    if red:
        out2 = torch.full((n, h, w, red[0]), 0xA5, dtype=torch.uint8, device=dev)
        assert ops.conv_join_reduce(x, e["z_x"], d, resid, dn, out=out, out2=out2) is not None
        torch.cuda.synchronize()
        assert torch.equal(out2, _T(dev, c["ref"])[idx]), "reduced"
    else:
        ops.conv(x, e["z_x"], d, out=out, resid=resid)
        torch.cuda.synchronize()
    if not torch.equal(out, want):
        bad = torch.nonzero((out != want).reshape(n, -1).any(1)).flatten()
        pytest.fail(f"{bad.numel()} of {n} images differ; first at batch pos {int(bad[0])} "
                    f"(pool image {int(idx[bad[0]])}, strip {int(bad[0]) * 196 // 32}, per {f['per']})")
