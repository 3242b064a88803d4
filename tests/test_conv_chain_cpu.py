"""CPU: the synthetic conv-chain profiles of tests/convchain.py are what they
claim to be, and their numpy oracle is tied to the pinned one.

* coverage: on the oracle alone, every conv of every profile saturates at
  both ends and uses nearly every level between, so a wrong clamp, zero point
  or per-channel constant changes stored bytes;
* structure: the QDQ found / declined pattern (the library's own host solver),
  the host-side epilogue modes, the zero-point chain the library enforces;
* cross-check: chain_oracle on the pinned fixture spec reproduces
  qref.static_int8_forward (itself pinned against torch.ao).
Host-only: no device work is called."""
import os

import numpy as np
import pytest

import convchain as CC
import netfix
from oracle import qref


@pytest.fixture(scope="module")
def lib():
    from qconvnet import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libqconvnet.so missing — run __graft_entry__.build()")
    return _lib.load()


@pytest.mark.parametrize("profile", CC.PROFILES)
def test_coverage_conditions(profile):
    """Per conv, on the requant output before pool and hand-off: >= 2% at the
    lower clamp, >= 2% at 255, >= 90% of the integers of [lower clamp, 255]
    occur; the activation as stored has >= 64 distinct values."""
    spec = CC.make_spec(profile)
    o = CC.pool_oracle(profile)
    for i in range(1, 7):
        e = spec[f"conv{i}"]
        r, lo = o[f"r{i}"], CC.conv_lo(e)
        at_lo, at_hi = np.mean(r == lo), np.mean(r == 255)
        levels = np.unique(r).size / (256 - lo)
        stored = np.unique(o[f"a{i}"]).size
        print(f"{profile} conv{i}: z_y {e['z_y']} lo {lo} at_lo {at_lo:.3f} at_255 {at_hi:.3f} "
              f"levels {levels:.3f} stored distinct {stored}")
        assert r.min() >= lo
        assert at_lo >= 0.02 and at_hi >= 0.02, (i, at_lo, at_hi)
        assert levels >= 0.90, (i, levels)
        assert stored >= 64, (i, stored)


@pytest.mark.parametrize("profile", CC.PROFILES)
def test_profile_structure(lib, profile):
    spec = CC.make_spec(profile)
    found = CC.handoff_found(lib, spec)
    modes = CC.epi_modes(lib, spec)
    print(f"{profile}: hand-offs found {found} epilogue modes {modes}")
    convs = [spec[f"conv{i}"] for i in range(1, 7)]
    if profile in CC.QDQ:
        assert spec["mode"] == "qdq"
        assert found == [i not in CC.DECLINED[profile] for i in range(1, 7)]
        assert all(not e["relu"] and e["z_y"] != 0 for e in convs)
        for i in CC.DECLINED[profile]:   # the tie construction: s_y = 2^k, s2 = 2 s_y
            e = spec[f"conv{i}"]
            assert np.log2(float(e["s_y"])) % 1 == 0 and e["next"][0] == np.float32(2) * e["s_y"]
    else:
        assert spec["mode"] == "static" and found == [None] * 6
        # the split-K head applies
        assert spec["fc2"]["z_x"] == spec["fc1"]["z_y"] and spec["fc2"]["s_x"] == spec["fc1"]["s_y"]
    assert tuple(modes[2:]) == CC.PAIR_MODES[profile]
    # the chain the library enforces: x_zp[i] == y_zp[i-1], or the hand-off's z2
    z_in = CC.input_qparams(spec)[1]
    assert convs[0]["z_x"] == z_in
    for prev, e in zip(convs, convs[1:] + [spec["fc1"]]):
        want = prev["next"] if "next" in prev else (prev["s_y"], prev["z_y"])
        assert (e["s_x"], e["z_x"]) == want
    for i, e in enumerate(convs, 1):
        assert e["w"].min() == -127 and e["w"].max() == 127
        if CC.KINDS[profile][i - 1] == "F":
            assert e["z_y"] == 0 and e["relu"]
        else:
            assert e["z_y"] != 0
    if profile == "general":
        assert z_in not in (0, 128)
        assert [e["relu"] for e in convs] == [False, True] * 3
        assert all(e["z_x"] != 0 for e in convs[1:])   # conv B pads with a non-zero zero point
    if profile == "fast_pc":
        assert all(e["s_w"].max() / e["s_w"].min() >= 7.9 for e in convs)
        # the u = b / aws, v = 1 form of the constants
        u, v, _ = qref.requant_constants(convs[2]["s_x"], convs[2]["s_w"], convs[2]["s_y"], convs[2]["b"])
        assert np.all(v == 1) and np.unique(u).size > 100
    if profile == "qdq_mixed":   # conv B of each pair pads with its hand-off's z2
        assert convs[3]["z_x"] == CC.NEXT_ZP[2] != 0 and convs[5]["z_x"] == CC.NEXT_ZP[4] != 0


@pytest.mark.parametrize("profile", ["fast", "general", "qdq_declined"])
def test_pool_inputs(profile):
    """QuantStub outputs of the fp32 pool: every level, saturation from far
    outside at both ends, exact .5 ties; the raw-image pool uses every byte."""
    spec = CC.make_spec(profile)
    s, z = CC.input_qparams(spec)
    x = CC.pool_images(spec)
    assert x.shape == (CC.POOL, 3, 32, 32) and x.dtype == np.float32
    q = qref.quantize_per_tensor(x, s, z)
    assert np.unique(q).size == 256
    assert x.max() >= 1e9 and x.min() <= -1e9
    t = x.astype(np.float64) / float(s)
    assert np.mean(t + z < -20) > 0.02 and np.mean(t + z > 275) > 0.02
    ties = np.abs(t - np.floor(t)) == 0.5
    assert ties.sum() >= 8 * CC.POOL
    img = CC.pool_images_u8()
    assert img.shape == (CC.POOL, 32, 32, 3) and np.unique(img).size == 256


@pytest.mark.parametrize("n", [5, 8, 259, 1027])
def test_batch_index(n):
    idx = CC.batch(n)
    assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < CC.POOL
    assert np.all(idx[1:] != idx[:-1])
    assert np.unique(idx).size == min(n, CC.POOL)
    assert np.array_equal(idx, CC.batch(n))


def test_chain_oracle_equals_pinned_static_forward():
    z = netfix.load()
    spec, _ = netfix.static_spec(z)
    x = netfix.images(z)[:2]
    _, _, inter = qref.static_int8_forward(x, netfix.oracle_dict(spec), keep=True)
    o = CC.chain_oracle(spec, inter["q_in"])
    for i in range(1, 7):
        assert np.array_equal(o[f"a{i}"], inter[f"conv{i}"]), i
    assert np.array_equal(o["f1"], inter["fc1"])
    # the pre-pool requant output against the 3x3 primitive itself
    e = spec["conv2"]
    w = np.ascontiguousarray(e["w"].transpose(0, 2, 3, 1))
    u, v, m = qref.requant_constants(e["s_x"], e["s_w"], e["s_y"], e["b"])
    assert np.array_equal(o["r2"], qref.conv3x3_q(o["a1"], e["z_x"], w, u, v, m, e["z_y"], True))


def test_pool_oracle_is_chain_oracle_of_the_pool():
    """The activations kept from the qparams derivation are what chain_oracle
    computes from the finished spec (hand-offs and a declined one included)."""
    spec = CC.make_spec("qdq_mixed")
    o = CC.pool_oracle("qdq_mixed")
    x = CC.pool_images(spec)
    q = qref.quantize_per_tensor(qref.nchw_to_nhwc(x), *CC.input_qparams(spec))
    assert np.array_equal(q, o["q_in"])
    again = CC.chain_oracle(spec, q)
    for k, v in again.items():
        assert np.array_equal(v, o[k]), k


def test_mismatch_report_locates_the_element():
    want = np.zeros((3, 4, 4, 8), np.uint8)
    got = want.copy()
    assert CC.mismatch("a2", got, want, [5, 1, 7]) is None
    got[1, 2, 3, 4] = 9
    got[2, 0, 0, 0] = 1
    msg = CC.mismatch("a2", got, want, [5, 1, 7])
    assert msg == ("a2: 2 of 384 differ; first at batch pos 1 (pool image 1) y 2 x 3 channel 4: "
                   "got 9 want 0")
