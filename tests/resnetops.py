"""Synthetic cases for the ResNet conv kernels (csrc/convgemm.hip, convgen.hip,
resnet_stem.hip and the patch-ring qcn_conv3x3_u8s8_nhwc), the counterpart of
tests/convchain.py: test_resnet_ops_cpu.py pins the cases and their coverage
on the host, test_gpu_resnet_ops.py drives every launch form with them.  Host
only: nothing here touches a device (qcn_join_affine and the form queries are
host calls of the library).

Per-conv case: full-range random int8 weights (-128 included), uniform input
bytes, a given input zero point, per-tensor or per-channel weight scales spread
over 8x, and output qparams derived from the oracle's own accumulators by
convchain's recipe (F: z_y = 0, s_y = p97 / 255; G: p4 / p96, z_y != 0).  The
epilogue kinds, named for the requant form the streaming kernel compiles in:

  rq0   F with ReLU         rq0n  F without ReLU     (the saturating pack alone)
  rq1   G without ReLU      (rint + z_y, then the saturating pack)
  rq2   G with ReLU         (the general clamp, floor z_y)

Join case: a conv case without ReLU (rq0n / rq1) plus uniform identity bytes
with their own zero point and the join's output qparams derived by percentile
from the oracle's real-valued sum s_y (y3 - z_y) + s_r (r - z_r): kind zo0 the
G recipe (z_o != 0: with the join's ReLU the floor is z_o), zo1 / zo2 the F
recipe (z_o = 0), where a fixed seeded sequence of identity scales within a
factor sqrt(2) of s_y is walked until qcn_join_affine declines (zo1) or
returns its one-fma form (zo2).  A reduce case adds the next block's 1x1 conv
on the joined bytes.

Ties case: per-tensor, bias 0, s_x s_w / s_y = 2^-shift, weights multiples of
2^a and centred inputs multiples of 2^b with a + b = shift - 1: every
accumulator is a multiple of 2^(shift - 1), so every requant input fp32(acc) *
2^-shift is a multiple of 0.5 and about half of them are exact .5 ties.

Every case asserts the coverage conditions of DESIGN section 3 on the oracle's
bytes before it is handed out (assert_coverage)."""
import ctypes as C
import functools
import types
import zlib

import numpy as np

import convchain
from convchain import F32, POOL, SEED
from oracle import qref

S_X = F32(0.02)
KINDS = {"rq0": ("F", True), "rq0n": ("F", False), "rq1": ("G", False), "rq2": ("G", True)}
JOIN_KINDS = ("zo0", "zo1", "zo2")
# the fused reduce's three forms
REDUCE_KINDS = {"relu_z0": "rq0", "relu_z": "rq2", "norelu_z": "rq1"}
# identity scales tried for a zo1 / zo2 pair: the solver declines about one
# scale in 25 (measured on the host), so 400 tries miss a decline with
# probability 1e-7; a try costs a few milliseconds
MAX_WALK = 400


def _rng(*key):
    return np.random.default_rng([SEED, zlib.crc32(repr(key).encode())])


# ---------------------------------------------------------------- coverage
def coverage(y, lo):
    """(share at the lower clamp, share at 255, share of the integers of
    [lo, 255] that occur, distinct stored values)."""
    y = np.asarray(y)
    vals = np.unique(y)
    return float(np.mean(y == lo)), float(np.mean(y == 255)), vals.size / (256.0 - lo), int(vals.size)


def assert_coverage(y, lo, what):
    """>= 2 % of the outputs at each clamp, >= 90 % of the
    integers between the clamps occur, >= 64 distinct stored values."""
    at_lo, at_hi, levels, distinct = coverage(y, lo)
    assert int(np.min(y)) >= lo, (what, int(np.min(y)), lo)
    assert at_lo >= 0.02 and at_hi >= 0.02, (what, at_lo, at_hi)
    assert levels >= 0.90, (what, levels)
    assert distinct >= 64, (what, distinct)
    return at_lo, at_hi, levels, distinct


# ------------------------------------------------------------------- convs
def consts(e):
    return qref.requant_constants(e["s_x"], e["s_w"], e["s_y"], e["b"])


def conv_ref(qx, e):
    u, v, m = consts(e)
    return qref.conv_q(qx, e["z_x"], e["w"], u, v, m, e["z_y"], e["relu"], e["stride"], e["pad"])


def lo_of(e):
    return e["z_y"] if e["relu"] else 0


@functools.lru_cache(maxsize=None)
def conv_case(n, h, w, cin, cout, kernel=(1, 1), stride=(1, 1), pad=(0, 0), kind="rq0", pc=True, z_x=77):
    """dict(qx u8 [n,h,w,cin], e the layer entry (convchain.layer_entry's
    fields plus stride / pad / kernel), ref the oracle's output bytes)."""
    key = (n, h, w, cin, cout, kernel, stride, pad, kind, pc, z_x)
    rng = _rng("conv", *key)
    qx = rng.integers(0, 256, (n, h, w, cin), dtype=np.uint8)
    fg, relu = KINDS[kind]
    e, acc = convchain.layer_entry(rng, lambda wq: qref.conv_acc_nhwc(qx, z_x, wq, stride, pad),
                                   (cout, cin) + tuple(kernel), S_X, z_x, fg, relu, pc, full=True)
    e.update(stride=tuple(stride), pad=tuple(pad), kernel=tuple(kernel))
    ref = qref.requantize(acc, *consts(e), e["z_y"], e["relu"])
    assert (e["z_y"] == 0) == (fg == "F"), (key, e["z_y"])
    assert e["w"].min() == -128 and e["w"].max() == 127
    assert_coverage(ref, lo_of(e), key)
    for a in (qx, ref, e["w"]):
        a.setflags(write=False)
    return dict(key=key, qx=qx, e=e, ref=ref)


@functools.lru_cache(maxsize=None)
def ties_case(n, h, w, cin, cout, kernel=(1, 1), stride=(1, 1), pad=(0, 0), kind="rq0", z_x=128, wstep=16,
              xstep=8, extra=0):
    """Per-tensor, bias 0, power-of-two requant multiplier 2^-shift with
    shift = log2(wstep xstep) + 1 + extra: weights multiples of wstep, centred
    inputs multiples of xstep.  z_y: 0 for rq0 / rq0n, else 101."""
    key = (n, h, w, cin, cout, kernel, stride, pad, kind, z_x, wstep, xstep, extra)
    rng = _rng("ties", *key)
    nx = 256 // xstep
    i0 = -(z_x // xstep)                 # smallest step with z_x + xstep i >= 0
    qx = (z_x + xstep * rng.integers(i0, i0 + nx, (n, h, w, cin))).astype(np.int64)
    assert qx.min() >= 0 and qx.max() <= 255
    qx = qx.astype(np.uint8)
    wq = (wstep * rng.integers(-128 // wstep, 128 // wstep, (cout, cin) + tuple(kernel))).astype(np.int8)
    shift = int(np.log2(wstep * xstep)) + 1 + extra
    fg, relu = KINDS[kind]
    s_w, s_y = F32(2.0 ** -9), F32(2.0 ** -6)
    s_x = F32(2.0 ** (9 - 6 - shift))
    e = dict(w=wq, b=np.zeros(cout, F32), s_w=s_w, s_x=s_x, z_x=int(z_x), s_y=s_y,
             z_y=0 if fg == "F" else 101, relu=relu, stride=tuple(stride), pad=tuple(pad), kernel=tuple(kernel))
    u, v, m = consts(e)
    assert np.all(m == F32(2.0 ** -shift)) and np.all(u == 0)
    acc = qref.conv_acc_nhwc(qx, z_x, wq, stride, pad)
    ref = qref.requantize(acc, u, v, m, e["z_y"], relu)
    t = acc.astype(np.float64) * 2.0 ** -shift       # exact: the requant's input
    assert np.all(np.abs(acc) < 2 ** 24)
    r = np.rint(t) + e["z_y"]
    inside = (r > lo_of(e)) & (r < 255)
    ties = np.abs(t - np.floor(t)) == 0.5
    share = float(np.mean(ties[inside]))
    assert share >= 0.01, (key, share)
    assert_coverage(ref, lo_of(e), key)
    for a in (qx, ref, wq):
        a.setflags(write=False)
    return dict(key=key, qx=qx, e=e, ref=ref, ties=share)


# ------------------------------------------------------------------- joins
def join_affine(lib, s_y, z_y, s_r, z_r, s_o):
    """qcn_join_affine (host): the one-fma form's constants, or None."""
    out = (C.c_float * 3)()
    rc = lib.qcn_join_affine(float(s_y), int(z_y), float(s_r), int(z_r), float(s_o), out)
    assert rc in (0, 1), rc
    return tuple(out) if rc == 1 else None


def _join_qparams(real, kind):
    """s_o, z_o from the real-valued sum: zo0 the G recipe, else the F recipe."""
    return convchain._qparams(real, "G" if kind == "zo0" else "F", False)


def _real_sum(y3, e, r, s_r, z_r):
    return (qref.dequantize(y3, e["s_y"], e["z_y"]).astype(np.float64) +
            qref.dequantize(r, s_r, z_r).astype(np.float64))


@functools.lru_cache(maxsize=None)
def _join_walk(lib, conv_key, z_r):
    """The identity scales of the zo1 (declined) and zo2 (one-fma form found)
    cases of a conv case: the first of each kind along a seeded sequence of
    s_r = s_y 2^t, t uniform in [-1/2, 1/2]."""
    c = conv_case(*conv_key)
    e = c["e"]
    rng = _rng("walk", conv_key, z_r)
    r = identity_bytes(conv_key)
    found = {}
    for _ in range(MAX_WALK):
        s_r = F32(float(e["s_y"]) * 2.0 ** rng.uniform(-0.5, 0.5))
        s_o, z_o = _join_qparams(_real_sum(c["ref"], e, r, s_r, z_r), "zo1")
        form = join_affine(lib, e["s_y"], e["z_y"], s_r, z_r, s_o)
        found.setdefault("zo2" if form is not None else "zo1", (s_r, s_o))
        if len(found) == 2:
            break
    assert len(found) == 2, f"{conv_key}: only {sorted(found)} along the identity-scale sequence"
    return found


def identity_bytes(conv_key):
    c = conv_case(*conv_key)
    return _rng("identity", conv_key).integers(0, 256, c["ref"].shape, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def join_case(lib, conv_key, zo_kind, z_r):
    """A conv case without ReLU plus the join: dict(conv, r identity bytes,
    s_r, z_r, s_o, z_o, ref the joined bytes, affine what qcn_join_affine
    answers for the join's qparams)."""
    c = conv_case(*conv_key)
    e = c["e"]
    assert not e["relu"], "the joined conv takes no ReLU of its own"
    r = identity_bytes(conv_key)
    if zo_kind == "zo0":
        s_r = F32(float(e["s_y"]) * 2.0 ** _rng("s_r", conv_key, z_r).uniform(-0.5, 0.5))
        s_o, z_o = _join_qparams(_real_sum(c["ref"], e, r, s_r, z_r), "zo0")
        assert z_o != 0
    else:
        s_r, s_o = _join_walk(lib, conv_key, z_r)[zo_kind]
        z_o = 0
    ref = qref.add_relu_q(c["ref"], e["s_y"], e["z_y"], r, s_r, z_r, s_o, z_o)
    affine = join_affine(lib, e["s_y"], e["z_y"], s_r, z_r, s_o)
    if zo_kind != "zo0":
        assert (affine is not None) == (zo_kind == "zo2")
    assert_coverage(ref, z_o, (conv_key, zo_kind, z_r))
    r.setflags(write=False)
    ref.setflags(write=False)
    return dict(conv=c, r=r, s_r=F32(s_r), z_r=int(z_r), s_o=F32(s_o), z_o=int(z_o), ref=ref, affine=affine,
                zo=JOIN_KINDS.index(zo_kind))


@functools.lru_cache(maxsize=None)
def reduce_case(lib, conv_key, zo_kind, z_r, cr, form, pc=True):
    """A join case plus the next block's reduce conv (1x1, 256 -> cr) on the
    joined bytes, in one of REDUCE_KINDS: dict(join, e the reduce's entry,
    ref its output bytes)."""
    j = join_case(lib, conv_key, zo_kind, z_r)
    qj = j["ref"]
    rng = _rng("reduce", conv_key, zo_kind, z_r, cr, form, pc)
    fg, relu = KINDS[REDUCE_KINDS[form]]
    e, acc = convchain.layer_entry(rng, lambda wq: qref.conv_acc_nhwc(qj, j["z_o"], wq), (cr, qj.shape[-1], 1, 1),
                                   j["s_o"], j["z_o"], fg, relu, pc, full=True)
    e.update(stride=(1, 1), pad=(0, 0), kernel=(1, 1))
    ref = qref.requantize(acc, *consts(e), e["z_y"], e["relu"])
    assert_coverage(ref, lo_of(e), (conv_key, zo_kind, z_r, cr, form))
    ref.setflags(write=False)
    return dict(join=j, e=e, ref=ref)


# ------------------------------------------------------------- long batches
def long_batch(strips, hw=14):
    """Images of hw x hw pixels for at least ``strips`` 32-pixel strips plus
    half an image, so that the strip count is no round number."""
    return int(np.ceil(strips * 32 / (hw * hw))) + 1


def strips_for(ncu, cg, p, occupancy=4):
    """Strips after which every chunk of launch_stream's plan (at most
    ncu * occupancy / cg chunks) walks at least p + 2 of them."""
    return (ncu * occupancy // cg) * (p + 1) + 1


# ------------------------------------------------------------------- forms
def host_layer(e):
    """The fields ops.conv_gemm_form / ops.conv() read off a layer, without
    device tensors."""
    cout = e["w"].shape[0]
    return types.SimpleNamespace(cout=cout, kh=e["kernel"][0], kw=e["kernel"][1], sy=e["stride"][0],
                                 sx=e["stride"][1], py=e["pad"][0], px=e["pad"][1], z_y=int(e["z_y"]),
                                 s_y=e["s_y"], relu=bool(e["relu"]))


def rq_of(e):
    """The requant form an entry selects (qcn_conv_form_t.rq)."""
    return 0 if e["z_y"] == 0 else (2 if e["relu"] else 1)


STREAM_P = {(64, 4): 4, (128, 4): 4, (256, 4): 4, (512, 4): 3, (64, 2): 4, (128, 2): 3, (256, 2): 4}


def expected_form(shape, e, zo=None):
    """The host-decidable fields of the form the dispatch must pick for a
    conv of ``e`` on an input of ``shape`` (n, h, w, cin), with a join of kind
    ``zo`` (0 / 1 / 2) or none: the table the tests hold the library to."""
    n, h, w, cin = shape
    cout = e["w"].shape[0]
    k, s, p = e["kernel"], e["stride"], e["pad"]
    resid = zo is not None
    plain = k == (1, 1) and p == (0, 0)
    f = dict(bn=0, rq=rq_of(e), zo=-1 if zo is None else zo, k=0, p=0, bl=0, cr=0)
    if plain and s == (1, 1) and cin in (64, 128, 256, 512) and \
            (cout % 128 == 0 or (not resid and cout % 64 == 0 and cin <= 256)):
        nw = 4 if cout % 128 == 0 else 2
        f.update(family="stream", nw=nw, k=cin, p=STREAM_P[(cin, nw)],
                 bl=int(cin >= 128 if nw == 4 else cin == 256))
    elif not resid and k == (3, 3) and s == (1, 1) and p == (1, 1) and cout % 256 == 0 and \
            (h, w, cin) in ((14, 14, 256), (7, 7, 512)):
        f.update(family="img", nw=8, rq=2)
    elif not resid and plain and s == (2, 2) and cin in (256, 512) and cout % 128 == 0 and not e["relu"]:
        f.update(family="stream_s2", nw=4, k=cin, p=STREAM_P[(cin, 4)], bl=1)
    else:
        bn = 256 if cout % 256 == 0 and not resid and (k != (1, 1) or cin >= 2048) else \
            (128 if cout % 128 == 0 else 64)
        f.update(family="tiled", bn=bn, nw=8 if bn == 256 else 4, zo=-1 if zo is None else min(zo, 1))
    return f


def expected_reduce_form(e, zo, cr):
    return dict(family="join_reduce", bn=0, nw=8, rq=rq_of(e), zo=zo, k=64, p=4, bl=0, cr=cr)


def host_fields(form):
    """A reported form without the device-dependent strip plan."""
    return {k: v for k, v in form.items() if k not in ("nstrip", "nchunk", "per")}


# -------------------------------------------------------------------- stem
STEM_ZP = 120


def stem_qlut():
    """QuantStub table [3][256] of the u8 entry: a permutation of the bytes per
    channel (the kernels look it up byte by byte and assume nothing else)."""
    b = np.arange(256)
    return np.stack([(b * 7 + 3) % 256, (b * 37 + 101) % 256, (255 - b)]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def stem_case(kind, pc=True, ties=False, n=2, hw=64):
    """The fused stem (QuantStub -> 7x7/2 conv -> 3x3/2 max-pool) on raw bytes
    img (u8 NHWC) through stem_qlut(), and on the fp32 NCHW images x that
    quantize to the same bytes: dict(img, x, q the QuantStub output, s_in,
    e the 7x1 row conv's entry (e["w7"] the 7x7 weights), rows, conv the conv
    output, ref the pooled output), by qref.stem_pack -> conv_q ->
    maxpool3x3s2_nhwc."""
    from qconvnet import ops
    key = (kind, pc, ties, n, hw)
    rng = _rng("stem", *key)
    fg, relu = KINDS[kind]
    if ties:
        s_in = F32(2.0 ** -5)
        want = STEM_ZP + 8 * rng.integers(-15, 16, (n, hw, hw, 3))     # centred multiples of 8
        inv = [np.argsort(t) for t in stem_qlut()]                      # byte whose table entry is want
        img = np.stack([inv[c][want[..., c]] for c in range(3)], -1).astype(np.uint8)
    else:
        s_in = S_X
        img = rng.integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)
    q = np.stack([stem_qlut()[c][img[..., c]] for c in range(3)], -1)
    x = np.ascontiguousarray(qref.dequantize(q, s_in, STEM_ZP).transpose(0, 3, 1, 2))
    assert np.array_equal(qref.quantize_per_tensor(qref.nchw_to_nhwc(x), s_in, STEM_ZP), q)
    rows = qref.stem_pack(x, s_in, STEM_ZP)
    acc_of = lambda w7: qref.conv_acc_nhwc(rows, STEM_ZP, ops.stem_weight_rows(w7), (2, 1), (3, 0))  # noqa: E731
    if ties:
        w7 = (16 * rng.integers(-8, 8, (64, 3, 7, 7))).astype(np.int8)
        e = dict(w=w7, b=np.zeros(64, F32), s_w=F32(2.0 ** -9), s_x=s_in, z_x=STEM_ZP, s_y=F32(2.0 ** -6),
                 z_y=0 if fg == "F" else 101, relu=relu)
        acc = acc_of(w7)
        t = acc.astype(np.float64) * 2.0 ** -8
        assert np.all(consts(e)[2] == F32(2.0 ** -8))
        r = np.rint(t) + e["z_y"]
        inside = (r > lo_of(e)) & (r < 255)
        share = float(np.mean((np.abs(t - np.floor(t)) == 0.5)[inside]))
        assert share >= 0.01, (key, share)
    else:
        e, acc = convchain.layer_entry(rng, acc_of, (64, 3, 7, 7), s_in, STEM_ZP, fg, relu, pc, full=True)
    e["w7"] = e["w"]
    e["w"] = ops.stem_weight_rows(e["w7"])
    e.update(stride=(2, 1), pad=(3, 0), kernel=(7, 1))
    conv = qref.requantize(acc, *consts(e), e["z_y"], e["relu"])
    assert np.array_equal(conv, conv_ref(rows, e))
    ref = qref.maxpool3x3s2_nhwc(conv)
    assert_coverage(conv, lo_of(e), key)
    # the max-pool moves mass off the lower clamp: the stored map keeps the
    # upper clamp and the level count
    assert np.mean(ref == 255) >= 0.02 and np.unique(ref).size >= 64, key
    for a in (img, x, rows, conv, ref):
        a.setflags(write=False)
    return dict(key=key, img=img, x=x, q=q, s_in=s_in, e=e, rows=rows, conv=conv, ref=ref)


# ------------------------------------------------------------------ matrix
# the cases of test_gpu_resnet_ops.py (test_resnet_ops_cpu.py walks the same
# lists); a conv key is conv_case's argument tuple
PIX = (3, 7, 9)                  # 189 pixels: five full strips and a ragged one
ZX = {32: 131, 64: 5, 128: 130, 256: 0, 512: 255, 1024: 77}
ZR = {32: 9, 64: 17, 128: 131, 256: 90, 512: 200, 1024: 60}


def ck(n, h, w, cin, cout, kernel=(1, 1), stride=(1, 1), pad=(0, 0), kind="rq0", pc=True):
    return (n, h, w, cin, cout, kernel, stride, pad, kind, pc, ZX[cin])


def zr(k, zo):
    """Identity zero point of a join on a K-deep conv: near mid-range for zo0,
    so that the real-valued sum has the negative share a non-zero z_o needs."""
    return 128 + ZR[k] % 64 if zo == "zo0" else ZR[k]


def _kinds(pc):
    return ("rq0", "rq1", "rq2") if pc else ("rq0n", "rq1", "rq2")


STREAM = [ck(*PIX, k, cout, kind=kind, pc=pc)
          for k in (64, 128, 256, 512) for cout in (256, 192) if cout == 256 or k <= 256
          for pc in (True, False) for kind in _kinds(pc)]
# (conv key, join kind, identity zero point)
STREAM_JOIN = [(ck(*PIX, k, 256, kind=kind), zo, zr(k, zo))
               for k in (64, 128, 256, 512) for kind in ("rq0n", "rq1") for zo in JOIN_KINDS]
STREAM_S2 = [ck(5, 13, 11, k, 256, stride=(2, 2), kind=kind) for k in (256, 512) for kind in ("rq0n", "rq1")]
# (conv key, join kind, identity zero point, reduce cout, reduce form)
JOIN_REDUCE = [(ck(*PIX, 64, 256, kind=kind), zo, zr(64, zo), cr, form)
               for cr in (64, 128) for kind in ("rq0n", "rq1") for zo in JOIN_KINDS for form in REDUCE_KINDS]
TILED_GEOM = {
    "3x3s1": lambda cout, kind, pc: ck(5, 7, 9, 32, cout, (3, 3), (1, 1), (1, 1), kind, pc),
    "3x3s2": lambda cout, kind, pc: ck(7, 13, 11, 32, cout, (3, 3), (2, 2), (1, 1), kind, pc),
    "1x1k1024": lambda cout, kind, pc: ck(5, 7, 9, 1024, cout, kind=kind, pc=pc),
    "stemrow": lambda cout, kind, pc: ck(3, 20, 11, 32, cout, (7, 1), (2, 1), (3, 0), kind, pc),
}
# cout 64 / 128 / 256: BN 64 / 128 / 256 (the 1x1 conv takes BN 256 from K = 2048 on: BN 128 at cout 256)
TILED = [TILED_GEOM[g](cout, kind, cout != 128) for g in TILED_GEOM for cout in (64, 128, 256)
         for kind in ("rq0", "rq1", "rq2")]
TILED_JOIN = [(TILED_GEOM[g](cout, "rq1", True), zo, zr(32, zo)) for g in ("3x3s1", "1x1k1024") for cout in (64, 128)
              for zo in ("zo0", "zo1")]
# a join on K <= 128 and 64 output channels has no streaming form: the tiled
# kernel's early identity loads (one and two stages)
TILED_JOIN += [(ck(*PIX, k, 64, kind=kind), zo, zr(k, zo)) for k, kind in ((64, "rq0n"), (128, "rq1"))
               for zo in ("zo0", "zo1")]
IMG = [ck(2, hw, hw, cin, cout, (3, 3), (1, 1), (1, 1), kind, cout == 256)
       for hw, cin in ((14, 256), (7, 512)) for cout in (256, 512) for kind in ("rq0", "rq1", "rq2")]
PATCH = [ck(2, hw, hw, c, c, (3, 3), (1, 1), (1, 1), kind, kind != "rq1")
         for hw, c in ((56, 64), (28, 128)) for kind in ("rq0", "rq1", "rq2")]
STEM = [(kind, kind != "rq1") for kind in ("rq0", "rq1", "rq2")]
# ties_case argument tuples, at each family's shallowest K
TIES_STREAM = [(*PIX, 64, 256, (1, 1), (1, 1), (0, 0), kind) for kind in ("rq0", "rq1")]
TIES_TILED = [(5, 7, 9, 32, 128, (3, 3), (1, 1), (1, 1), kind) for kind in ("rq0", "rq1")] + \
             [(3, 20, 11, 32, 64, (7, 1), (2, 1), (3, 0), kind) for kind in ("rq0", "rq1")]
TIES_STEM = ["rq0", "rq1"]
# steady state: (conv key on the 14 x 14 pool, join kind or None, reduce (cr, form) or None)
LONG = [(ck(POOL, 14, 14, k, 256, kind="rq2"), None, None) for k in (64, 128, 256, 512)] + \
       [(ck(POOL, 14, 14, k, 256, kind=kind), zo, None) for k in (64, 128, 256, 512)
        for kind, zo in (("rq1", "zo0"), ("rq0n", "zo2"))] + \
       [(ck(POOL, 27, 27, k, 256, stride=(2, 2), kind=kind), None, None)
        for k, kind in ((256, "rq1"), (512, "rq0n"))] + \
       [(ck(POOL, 14, 14, 64, 256, kind="rq0n"), "zo2", (64, "relu_z0")),
        (ck(POOL, 14, 14, 64, 256, kind="rq1"), "zo0", (128, "relu_z"))]
