"""Synthetic conv chains for the fused conv launches (test_conv_chain_cpu.py
pins the specs and this oracle on the host; test_gpu_conv_chain.py drives
every fused launch form with them).  Host only: nothing here touches a device.

A *profile* is a product qspec (the dict netfix.static_spec / netfix.qdq_spec
return) that the harness owns: full-range random int8 weights and qparams
derived, layer by layer, from the numpy oracle run on a pool of POOL images,
so that every conv's requantized output spans [lower clamp, 255] and saturates
at both ends.  The profiles differ in the epilogue form the dispatch code
(conv_epi.hpp epi_mode) sees per layer:

  fast          every conv z_y == 0 + ReLU (mode 1), per-tensor weight scales
  fast_pc       the same with per-channel weight scales spread over 8x
  general       every conv z_y != 0 (mode 0); ReLU on conv2/4/6 only; the input
                zero point is neither 0 nor 128
  mixed_a       conv1/3/5 fast, conv2/4/6 general: pair modes (1, 0)
  mixed_b       conv1/3/5 general, conv2/4/6 fast: pair modes (0, 1)
  qdq           per-layer QDQ, every hand-off with a one-fma form: (2, 2)
  qdq_declined  per-layer QDQ, every hand-off declined (ConvEpi::qdq == 1)
  qdq_mixed     as qdq, conv3's and conv6's hand-offs declined: a lone
                one-fma layer inside each pair

qparams recipe, for a layer with real-valued output r = s_x s_w (acc + b / (s_x s_w))
over the pool: fast: z_y = 0, s_y = p97(r) / 255; general: lo, hi = p4(r),
p96(r), s_y = (hi - lo) / 255, z_y = round(-lo / s_y).  A declined hand-off
rounds s_y DOWN to a power of two (more saturation, never less) and sets the
next stub's scale to exactly 2 s_y: (q1 - z1) s1 / s2 is then exact and lands
on .5 for every odd q1 - z1, which no single fma reproduces.  Those layers
also get a positive mean bias (0.6 of the accumulator's deviation) so that
z_y sits near 85 and the halved hand-off still has more than 64 levels.
"""
import ctypes as C
import functools

import numpy as np

from oracle import qref

F32 = np.float32
PROFILES = ("fast", "fast_pc", "general", "mixed_a", "mixed_b", "qdq", "qdq_declined", "qdq_mixed")
STATIC = PROFILES[:5]
QDQ = PROFILES[5:]
PURE = ("fast", "fast_pc", "qdq")    # conv3..conv6 all mode 1 or all mode 2
POOL = 8
SEED = 0
CONV_TABLE = ((3, 64, False), (64, 64, True), (64, 128, False), (128, 128, True),
              (128, 256, False), (256, 256, True))
# QuantStub scale: a power of two, so (j + .5) * IN_SCALE are exact ties
IN_SCALE = F32(2.0 ** -6)
IN_ZP = dict(fast=128, fast_pc=114, general=77, mixed_a=128, mixed_b=99, qdq=121, qdq_declined=60,
             qdq_mixed=131)
# 'F' fast / 'G' general, conv1..conv6
KINDS = dict(fast="FFFFFF", fast_pc="FFFFFF", general="GGGGGG", mixed_a="FGFGFG", mixed_b="GFGFGF",
             qdq="GGGGGG", qdq_declined="GGGGGG", qdq_mixed="GGGGGG")
DECLINED = dict(qdq=(), qdq_declined=(1, 2, 3, 4, 5, 6), qdq_mixed=(3, 6))
# host-side epilogue modes of conv3..conv6 (conv_epi.hpp epi_mode)
PAIR_MODES = dict(fast=(1, 1, 1, 1), fast_pc=(1, 1, 1, 1), general=(0, 0, 0, 0), mixed_a=(1, 0, 1, 0),
                  mixed_b=(0, 1, 0, 1), qdq=(2, 2, 2, 2), qdq_declined=(0, 0, 0, 0),
                  qdq_mixed=(0, 2, 2, 0))
NEXT_ZP = (0, 9, 7, 0, 12, 3)    # z2 of conv1..conv6's hand-offs (conv B pads with 7 / 12)
FOUND_RATIO = 0.55               # s2 / s_y of a hand-off that has a one-fma form


# ------------------------------------------------------------------ inputs
def _pool_f32(s, z, seed):
    rng = np.random.default_rng([seed, 77])
    steps = rng.uniform(-48.0, 304.0, (POOL, 3, 32, 32))
    x = ((steps - z) * float(s)).astype(F32)
    sp = np.array([(j + 0.5 - z) * float(s) for j in (0, 1, 2, 3, 126, 127, 253, 254)] +
                  [1e9, -1e9, 0.0, -0.0], F32)
    flat = x.reshape(POOL, 3, -1)
    flat[:, :, :sp.size] = sp            # first row of every plane: the conv's padded edge
    flat[:, :, -sp.size:] = sp[::-1]
    return x


def input_qparams(spec):
    return spec["in"] if spec["mode"] == "static" else (spec["conv1"]["s_x"], spec["conv1"]["z_x"])


def pool_images(spec, seed=SEED):
    """POOL fp32 NCHW images whose QuantStub outputs cover 0..255, saturate at
    both ends (+-1e9 included) and hit exact .5 ties."""
    return _pool_f32(*input_qparams(spec), seed)


def pool_images_u8(seed=SEED):
    """POOL raw uint8 NHWC images, uniform bytes."""
    return np.random.default_rng([seed, 78]).integers(0, 256, (POOL, 32, 32, 3), dtype=np.uint8)


def u8_quantized(spec, img, mean, std):
    """The QuantStub output of raw images: quantize_table[c][byte], NHWC."""
    from qconvnet import quant as Q
    tab = Q.quantize_table(Q.normalize_table(mean, std), *input_qparams(spec)).numpy()
    return np.stack([tab[c][img[..., c]] for c in range(3)], axis=-1)


def batch(n, seed=SEED):
    """Index vector into the pool: random, neighbours differ, and every pool
    image occurs (from n = POOL on).  The device batch is pool[idx], the
    expected result of every image oracle[idx]."""
    rng = np.random.default_rng([seed, n])
    idx = np.empty(n, np.int64)
    k = min(n, POOL)
    idx[:k] = rng.permutation(POOL)[:k]
    if n > k:
        idx[k:] = (idx[k - 1] + np.cumsum(rng.integers(1, POOL, n - k))) % POOL
    return idx


# ------------------------------------------------------------------ oracle
def _consts(e):
    return qref.requant_constants(e["s_x"], e["s_w"], e["s_y"], e["b"])


def handoff(y, e):
    """DeQuantStub -> ReLU -> the next layer's QuantStub."""
    s2, z2 = e["next"]
    f = np.maximum(qref.dequantize(y, e["s_y"], e["z_y"]), F32(0.0))
    return qref.quantize_per_tensor(f, s2, z2)


def _conv_layer(q, e, pool, acc=None):
    """(requant output before pool / hand-off, activation as stored)."""
    if acc is None:
        # fp64 BLAS accumulation of the same sum as qref.conv3x3_acc_nhwc
        # (exact: |acc| < 2^53), OIHW weights as the product spec holds them
        acc = qref.conv_acc_nhwc(q, e["z_x"], e["w"], (1, 1), (1, 1))
    r = qref.requantize(acc, *_consts(e), e["z_y"], e["relu"])
    y = qref.maxpool2x2_nhwc(r) if pool else r
    if "next" in e:
        y = handoff(y, e)
    return r, y


def _fc1(flat, e):
    w = np.ascontiguousarray(e["w"][:, qref.flatten_perm_nhwc_to_nchw()])
    return qref.linear_q(flat, e["z_x"], w, *_consts(e), e["z_y"], e["relu"])


def chain_oracle(spec, q_in):
    """numpy reference of conv1..conv6 (+ fc1) of a product qspec on the
    QuantStub output q_in (u8 NHWC [n,32,32,3]): a1..a6 as the device stores
    them (pooled, after the QDQ hand-off), r1..r6 the requant outputs before
    pool and hand-off, f1 fc1's u8 output."""
    out = {}
    q = q_in
    for i, (_, _, pool) in enumerate(CONV_TABLE, 1):
        out[f"r{i}"], q = _conv_layer(q, spec[f"conv{i}"], pool)
        out[f"a{i}"] = q
    out["f1"] = _fc1(q.reshape(q.shape[0], -1), spec["fc1"])
    return out


# ------------------------------------------------------------------- specs
def _qparams(r, kind, declined):
    if kind == "F":
        return F32(np.percentile(r, 97) / 255.0), 0
    lo, hi = np.percentile(r, 4), np.percentile(r, 96)
    z_y = int(np.clip(np.rint(-lo * 255.0 / (hi - lo)), 0, 255))
    s_y = (hi - lo) / 255.0
    if declined:
        s_y = 2.0 ** np.floor(np.log2(s_y))
    return F32(s_y), z_y


def layer_entry(rng, acc_of, shape, s_x, z_x, kind, relu, per_channel, declined=False, full=False):
    """Random weights / bias and derived output qparams of one layer;
    ``acc_of(w)`` gives the exact accumulators over the pool."""
    cout = shape[0]
    w = rng.integers(-128 if full else -127, 128, shape).astype(np.int8)
    if per_channel:
        s_w = (F32(5e-4) * F32(8.0) ** np.linspace(0, 1, cout)[rng.permutation(cout)]).astype(F32)
    else:
        s_w = F32(2e-3)
    acc = acc_of(w)
    aws = (F32(s_x) * np.atleast_1d(s_w)).astype(F32).astype(np.float64)
    b = ((rng.standard_normal(cout) * 0.2 + (0.6 if declined else 0.0)) * acc.std() * aws).astype(F32)
    r = (acc + b.astype(np.float64) / aws) * aws
    s_y, z_y = _qparams(r, kind, declined)
    return dict(w=w, b=b, s_w=s_w, s_x=F32(s_x), z_x=int(z_x), s_y=s_y, z_y=z_y, relu=bool(relu)), acc


def make_spec(profile, seed=SEED):
    """Product qspec of ``profile`` (see the module docstring); fc1 / fc2
    included so QuantizedConvNet accepts it."""
    return _derive(profile, seed)[0]


@functools.lru_cache(maxsize=None)
def _derive(profile, seed):
    """(spec, the oracle's activations of the fp32 pool the qparams were
    derived on — what chain_oracle(spec, QuantStub(pool)) returns)."""
    rng = np.random.default_rng([seed, PROFILES.index(profile)])
    qdq = profile in QDQ
    pc = profile == "fast_pc"
    s_x, z_x = IN_SCALE, IN_ZP[profile]
    spec = {"mode": "qdq" if qdq else "static", "per_channel": pc}
    if not qdq:
        spec["in"] = (s_x, z_x)
    q = qref.quantize_per_tensor(qref.nchw_to_nhwc(_pool_f32(s_x, z_x, seed)), s_x, z_x)
    out = {"q_in": q}
    for i, (cin, cout, pool) in enumerate(CONV_TABLE, 1):
        kind = KINDS[profile][i - 1]
        declined = qdq and i in DECLINED[profile]
        relu = not qdq and (kind == "F" or i % 2 == 0)
        e, acc = layer_entry(rng, lambda w: qref.conv_acc_nhwc(q, z_x, w, (1, 1), (1, 1)),
                              (cout, cin, 3, 3), s_x, z_x, kind, relu, pc, declined)
        if qdq:
            s2 = F32(2.0) * e["s_y"] if declined else F32(float(e["s_y"]) * FOUND_RATIO)
            e["next"] = (F32(s2), NEXT_ZP[i - 1])
        spec[f"conv{i}"] = e
        out[f"r{i}"], q = _conv_layer(q, e, pool, acc)
        out[f"a{i}"] = q
        s_x, z_x = e["next"] if qdq else (e["s_y"], e["z_y"])
    flat = q.reshape(POOL, -1)
    perm = qref.flatten_perm_nhwc_to_nchw()
    kind = "G" if profile == "general" or qdq else "F"
    spec["fc1"], acc = layer_entry(rng, lambda w: qref.linear_acc(flat, z_x, w[:, perm]), (512, 4096),
                                    s_x, z_x, kind, not qdq, pc, full=True)
    e = spec["fc1"]
    out["f1"] = f1 = qref.requantize(acc, *_consts(e), e["z_y"], e["relu"])
    if qdq:
        spec["fc2"] = dict(w=(rng.standard_normal((10, 512)) * 0.05).astype(F32),
                           b=rng.standard_normal(10).astype(F32))
        return spec, out
    spec["fc2"], _ = layer_entry(rng, lambda w: qref.linear_acc(f1, e["z_y"], w), (10, 512), e["s_y"],
                                  e["z_y"], "G", False, pc, full=True)
    return spec, out


@functools.lru_cache(maxsize=None)
def pool_oracle(profile, seed=SEED, u8=False, mean=None, std=None):
    """chain_oracle of the profile's pool (fp32 pool, or the raw-image pool
    through the QuantStub table), computed once per profile."""
    spec, out = _derive(profile, seed)
    if not u8:    # the derivation already ran the chain on this pool
        return out
    q = u8_quantized(spec, pool_images_u8(seed), mean, std)
    out = chain_oracle(spec, q)
    out["q_in"] = q
    return out


# --------------------------------------------------------------- structure
def conv_lo(e):
    return e["z_y"] if e["relu"] else 0


def handoff_found(lib, spec):
    """Per conv with a QDQ hand-off: whether the library finds its one-fma
    form (qcn_qdq_affine, a host call)."""
    return [entry_found(lib, spec[f"conv{i}"]) for i in range(1, 7)]


def entry_found(lib, e):
    """None without a hand-off; else whether qcn_qdq_affine finds its form."""
    from qconvnet import ops
    if "next" not in e:
        return None
    q = ops.qdq_struct(e["s_y"], e["z_y"], *e["next"])
    out = (C.c_float * 4)()
    rc = lib.qcn_qdq_affine(C.byref(q), int(e["z_y"]), int(conv_lo(e)), out)
    assert rc in (0, 1), rc
    return rc == 1


def epi_modes(lib, spec):
    """conv_epi.hpp's epi_mode per conv: a found hand-off form gives 2;
    z_y == 0, lo == 0 and no hand-off gives 1; else 0."""
    found = handoff_found(lib, spec)
    modes = []
    for i in range(1, 7):
        e = spec[f"conv{i}"]
        if found[i - 1] is not None:
            modes.append(2 if found[i - 1] else 0)
        else:
            modes.append(1 if e["z_y"] == 0 and conv_lo(e) == 0 else 0)
    return modes


# ------------------------------------------------------------------ reports
def mismatch(name, got, want, idx):
    """None when got == want; else one line that locates the first mismatch:
    buffer, count, batch position, pool image, y, x, channel, got / want."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{name}: shape {got.shape}, expected {want.shape}"
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    p = tuple(bad[0])
    where = f"batch pos {p[0]} (pool image {int(idx[p[0]])})"
    if len(p) == 4:
        where += f" y {p[1]} x {p[2]} channel {p[3]}"
    else:
        where += "".join(f" [{v}]" for v in p[1:])
    return f"{name}: {len(bad)} of {got.size} differ; first at {where}: got {got[p]} want {want[p]}"
