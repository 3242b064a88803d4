"""GPU: every fused conv launch form against the numpy oracle, bit for bit,
on the synthetic profiles of tests/convchain.py (full-range weights, outputs
that saturate at both ends, every epilogue form the dispatch distinguishes).

The device batch is pool[idx] for a random index vector into an 8-image pool,
so every position of a batch is compared with the oracle of its own image at
the cost of 8 oracle images per profile.  The batches are the smallest that
select each form in qcn_conv3x3_pair_u8s8, convnet_convs_plan and
qcn_convs36_u8s8 (ncu = the device's CU count, 256 on the MI355X):

  5         convnet_convs_sm_kernel; fuse_convs=False: SmA3/SmB4, launch_pair_ga_split
  ncu+3     the one launch declined: conv12p, launch_pair<A3,B4>, launch_pair_ga
            with an odd last image
  2*ncu+1   conv3+4 persistent wave-specialised (16x16 for the pure profiles,
            32x32 for the others); conv5+6 launch_pair_ga
  4*ncu     everything persistent; n % 128 == 0: conv6 chunk-major for the head
  4*ncu+3   everything persistent, ragged last tiles, NHWC conv6

Each case first asserts that kernel_names() is the sequence this table
predicts for the profile (otherwise a fallback would pass silently)."""
import numpy as np
import pytest
import torch

import convchain as CC

pytestmark = pytest.mark.gpu

BATCHES = {"5": lambda ncu: 5, "ncu+3": lambda ncu: ncu + 3, "2ncu+1": lambda ncu: 2 * ncu + 1,
           "4ncu": lambda ncu: 4 * ncu, "4ncu+3": lambda ncu: 4 * ncu + 3}
LAYERS = tuple(f"conv{i}" for i in range(1, 7))
THREE = ("conv12", "conv34", "conv56")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cache():
    return {}


def _ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _model(cache, profile, dev):
    key = ("model", profile)
    if key not in cache:
        from qconvnet.qmodel import QuantizedConvNet
        cache[key] = QuantizedConvNet(CC.make_spec(profile), dev)
    return cache[key]


def _oracle(cache, profile, dev, u8=False):
    """The pool's oracle activations on the device (computed once per profile)."""
    key = ("oracle", profile, u8)
    if key not in cache:
        m = _model(cache, profile, dev)
        o = CC.pool_oracle(profile, u8=True, mean=m.mean, std=m.std) if u8 else CC.pool_oracle(profile)
        cache[key] = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in o.items()}
    return cache[key]


def _expect_names(profile, n, ncu, path):
    """The launches the dispatch rules give for this profile, batch and path."""
    static, pure = profile in CC.STATIC, profile in CC.PURE
    if path == "layers":   # per-layer QDQ has no chunk-major conv6 hand-off: no head
        return LAYERS + (("fc12",) if n % 128 == 0 and static else ("fc1", "fc2"))
    tail = ("fc12",) if n % 128 == 0 else ("fc1", "fc2")
    if path == "default" and (n <= ncu or (n >= 4 * ncu and pure)):
        return ("conv1_6",) + tail
    if path == "w4" and pure:
        return ("conv12", "conv3_6") + tail
    return THREE + tail


def _run(model, x, path):
    """One forward on ``path``; returns (kernel names, buffers cloned)."""
    from qconvnet import ops
    n = x.shape[0]
    model.fuse12 = path != "layers"
    model.fuse_convs = path in ("default", "w4")
    model.convs_w4 = path == "w4"
    keep = path == "layers"
    try:   # nothing a path leaves unwritten may still hold an earlier path's result
        for t in model.buffers(n).values():
            t.fill_(0xA5) if t.dtype == torch.uint8 else t.zero_()
    except KeyError:
        pass
    marks = []
    model.run(x, keep=keep, marks=marks)
    torch.cuda.synchronize()
    names = model.kernel_names(x.shape, keep=keep)
    assert len(marks) == len(names) + 1   # one event before the first launch, one after each
    b = model.buffers(n)
    want = ("a1", "a2", "a3", "a4", "a5", "a6") if keep else ("a2", "a4", "a6")
    got = {k: b[k].clone() for k in want + ("f1", "logits")}
    if names[-1] == "fc12" and not keep:   # conv6 wrote the head's chunk-major input
        got["a6"] = ops.from_kmajor(b["a6k"]).reshape(n, 4, 4, 256).contiguous()
    if model.mode == "static":
        got["q"] = b["q"].clone()
    return names, got


def _compare(label, got, oracle, idx, idx_dev, keys):
    """Mismatch reports (one line each) of got[k] against oracle[k][idx]."""
    bad = []
    for k in keys:
        want = oracle[k][idx_dev]
        if not torch.equal(got[k], want):
            bad.append(CC.mismatch(f"{label} {k}", got[k].cpu().numpy(), want.cpu().numpy(), idx))
    return bad


def _paths_agree(profile, runs):
    """Logits between the paths: equal for the static nets; for QDQ within
    1e-5 max|ref| (the fp32 fc2 sums in another order in the head) and the
    same argmax."""
    ref = runs["layers"]
    bad = []
    for path, got in runs.items():
        if profile in CC.STATIC:
            if not (torch.equal(got["q"], ref["q"]) and torch.equal(got["logits"], ref["logits"])):
                bad.append(f"{path}: logits differ from the per-layer path")
            continue
        tol = 1e-5 * ref["logits"].abs().max().item()
        err = (got["logits"] - ref["logits"]).abs().max().item()
        if not err <= tol or not torch.equal(got["logits"].argmax(1), ref["logits"].argmax(1)):
            bad.append(f"{path}: logits off the per-layer path by {err:.3e} (tol {tol:.3e})")
    return bad


@pytest.mark.parametrize("size", list(BATCHES))
@pytest.mark.parametrize("profile", CC.PROFILES)
def test_fused_launches_equal_oracle(dev, cache, profile, size):
    from qconvnet import ops
    ncu = _ncu(dev)
    n = BATCHES[size](ncu)
    model = _model(cache, profile, dev)
    oracle = _oracle(cache, profile, dev)
    idx = CC.batch(n)
    idx_dev = torch.from_numpy(idx).to(dev)
    pool = torch.from_numpy(CC.pool_images(model.spec)).to(dev)
    x = pool[idx_dev].contiguous()
    pure = profile in CC.PURE

    # the library's own host answers for this batch
    layers = ops.conv_layers(model.L, model.in_zp)
    form = ops.convnet_convs_form(n, model.in_scale, model.in_zp, layers, kmajor=n % 128 == 0)
    assert form == (1 if n <= ncu else (2 if n >= 4 * ncu and pure else 0))

    paths = ["default", "three"] + (["w4"] if n >= 4 * ncu else []) + ["layers"]
    runs, bad = {}, []
    for path in paths:
        want = _expect_names(profile, n, ncu, path)
        model.fuse12, model.fuse_convs, model.convs_w4 = path != "layers", path in ("default", "w4"), path == "w4"
        # right before the first forward too (the host query)
        assert model.kernel_names(x.shape, keep=path == "layers") == want, (path, "before the run")
        names, got = _run(model, x, path)
        print(f"{profile} n={n} {path}: {' '.join(names)}")
        assert names == want, path
        keys = ("a1", "a2", "a3", "a4", "a5", "a6", "f1") if path == "layers" else ("a2", "a4", "a6", "f1")
        bad += _compare(f"{profile} n={n} {path}", got, oracle, idx, idx_dev, keys)
        runs[path] = got
    if n >= 4 * ncu and not pure:   # mixed forms: the conv3..conv6 launch declines, no launch
        b = model.buffers(n)
        assert ops.convs36(b["a2"], layers, b["a4"], b["a6"], kmajor=False) is False
    bad += _paths_agree(profile, runs)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("size", ["5", "4ncu+3"])
@pytest.mark.parametrize("profile", ["fast", "general", "qdq"])
def test_raw_image_launches_equal_oracle(dev, cache, profile, size):
    """Raw uint8 NHWC images through qcn_convnet_convs_u8_nhwc (default) and
    qcn_conv12_fused_u8_nhwc (fuse_convs=False) against the oracle fed from
    the QuantStub table."""
    ncu = _ncu(dev)
    n = BATCHES[size](ncu)
    model = _model(cache, profile, dev)
    oracle = _oracle(cache, profile, dev, u8=True)
    idx = CC.batch(n, seed=1)
    idx_dev = torch.from_numpy(idx).to(dev)
    x = torch.from_numpy(CC.pool_images_u8()).to(dev)[idx_dev].contiguous()
    bad = []
    for path in ("default", "three"):
        names, got = _run(model, x, path)
        print(f"{profile} u8 n={n} {path}: {' '.join(names)}")
        assert names == _expect_names(profile, n, ncu, path), path
        bad += _compare(f"{profile} u8 n={n} {path}", got, oracle, idx, idx_dev, ("a2", "a4", "a6", "f1"))
    assert not bad, "\n".join(bad)
