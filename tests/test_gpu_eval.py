"""GPU: qcn_eval_topk_f32 and what is built on it (ops.eval_topk,
evaluate.EvalCounts / evaluate(), ModelEvaluator(counts="device")) against
the numpy restatement of the rule in evalref.py.  Every output is an integer
count or an index: everything is compared for equality.

Inputs (evalref): `quantised` logits 0.25 * (q - L // 2), `special` (the same
with NaN, +-inf and -0.0 written in) and `tiefree` (row permutations with a
NaN in 30 % of rows); about 3 % of the labels are -1, cols or 2**40 + 3.
Up to 16 columns the labels are uniform; above that half of them come from
the row's 8 leading columns (evalref.labels says why uniform labels cannot
cover hits on wide rows).

Coverage, asserted on evalref alone at 1027 rows for every cols >= 10 before
the device is asked (fewer columns cannot miss at k = 5, and a handful of rows
cannot carry percentages):
  quantised, special: at least 5 % of rows have the label's value tied across
      the k boundary at k = 1 and at k = 5; at least 2 % of rows hit and at
      least 2 % miss at both k;
  special, tiefree: at least 1 % of rows have a NaN maximum;
  every family: at least 1 % of rows have a bad label."""
import ctypes as C

import numpy as np
import pytest
import torch

import evalref as R

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 63, 64, 65, 257, 1027)
LDS_BOUND = 256           # qcn::kEvalLdsCols: LDS class bins up to here
COLS = (1, 2, 10, 31, 33, 64, 65, LDS_BOUND, LDS_BOUND + 1, 1000, 1003)
FAMILIES = ("quantised", "special", "tiefree")
TOP = ROWS[-1]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from qconvnet import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


_CASES = {}


def _case(family, cols):
    """(x [1027, cols], labels, rank, pred), made once; smaller row counts are
    leading slices of it."""
    key = (family, cols)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * FAMILIES.index(family) + cols)
        if family == "tiefree":
            x = R.tiefree(rng, TOP, cols)
        else:
            x = getattr(R, family)(rng, TOP, cols, R.levels_for(cols))
        lab = R.labels(rng, TOP, cols, x=x)
        for a in (x, lab):
            a.setflags(write=False)
        _CASES[key] = (x, lab, R.rank(x, lab), R.pred(x))
    return _CASES[key]


def _coverage(family, cols):
    x, lab, r, _ = _case(family, cols)
    ok = R.in_range(lab, cols)
    got = {"bad": (~ok).mean()}
    assert got["bad"] >= 0.01, got
    if family != "quantised":
        got["nan_max"] = np.isnan(x).any(1).mean()
        assert got["nan_max"] >= 0.01, got
    if family != "tiefree":
        for k in (1, 5):
            hit = ok & (r < k)
            got[k] = (R.tied_across(x, lab, k).mean(), hit.mean())
            assert got[k][0] >= 0.05 and got[k][1] >= 0.02 and (~hit).mean() >= 0.02, got
    return got


@pytest.mark.parametrize("cols", [c for c in COLS if c >= 10])
@pytest.mark.parametrize("family", FAMILIES)
def test_inputs_cover_the_rule(family, cols):
    print(family, cols, _coverage(family, cols))


def _launch(dev, x, lab, k, counters=None, offset=False):
    """(counters, confusion, pred) of one ops.eval_topk call as numpy."""
    from qconvnet import ops
    rows, cols = x.shape
    if offset:   # a view that starts 4 B into its allocation
        buf = torch.empty(rows * cols + 1, dtype=torch.float32, device=dev)
        xt = buf[1:].view(rows, cols)
        xt.copy_(torch.tensor(x))
        assert xt.data_ptr() % 16 == 4
    else:
        xt = torch.tensor(x, device=dev)
    conf = torch.zeros((cols, cols), dtype=torch.int64, device=dev)
    pred = torch.full((rows,), -7, dtype=torch.int64, device=dev)
    out = ops.eval_topk(xt, torch.tensor(lab, device=dev), k, counters, conf, pred)
    return out.cpu().numpy(), conf.cpu().numpy(), pred.cpu().numpy()


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("family", FAMILIES)
def test_kernel_equals_evalref(dev, family, cols):
    if cols >= 10:
        _coverage(family, cols)
    x_all, lab_all, r_all, p_all = _case(family, cols)
    for rows in ROWS:
        x, lab = np.ascontiguousarray(x_all[:rows]), np.ascontiguousarray(lab_all[:rows])
        for k in (1, 5, cols, cols + 3):
            want = R.score(x, lab, k, (r_all[:rows], p_all[:rows]))
            for offset in ((False, True) if rows in (65, TOP) else (False,)):
                got = _launch(dev, x, lab, k, offset=offset)
                for name, g, w in zip(("counters", "confusion", "pred"), got, want):
                    assert np.array_equal(g, w), (rows, k, offset, name,
                                                  int((g != w).sum()), g.ravel()[:8], w.ravel()[:8])


def test_no_optional_outputs(dev):
    """confusion and pred are nullable; a fresh zeroed counters is made."""
    from qconvnet import ops
    x, lab, r, p = _case("special", 10)
    got = ops.eval_topk(torch.tensor(x, device=dev), torch.tensor(lab, device=dev))
    assert np.array_equal(got.cpu().numpy(), R.score(x, lab, 5, (r, p))[0])


@pytest.mark.parametrize("cols", (10, LDS_BOUND + 1))
def test_updates_accumulate_in_64_bits(dev, cols):
    """Two updates (257 and 1027 rows) equal one update of the concatenation,
    and counters pre-filled with 2**33 + 7 come back increased by exactly the
    oracle's counts."""
    from qconvnet import ops
    x, lab, _, _ = _case("special", cols)
    xa, la = np.ascontiguousarray(x[:257]), np.ascontiguousarray(lab[:257])
    xc, lc = np.concatenate([xa, x]), np.concatenate([la, lab])
    want, want_conf, _ = R.score(xc, lc, 5)
    T = lambda a: torch.tensor(a, device=dev)
    base = 2 ** 33 + 7
    counters = torch.full((4 + 2 * cols,), base, dtype=torch.int64, device=dev)
    conf = torch.full((cols, cols), base, dtype=torch.int64, device=dev)
    ops.eval_topk(T(xa), T(la), 5, counters, conf)
    ops.eval_topk(T(np.ascontiguousarray(x)), T(np.ascontiguousarray(lab)), 5, counters, conf)
    assert np.array_equal(counters.cpu().numpy() - base, want)
    assert np.array_equal(conf.cpu().numpy() - base, want_conf)
    one, one_conf, _ = _launch(dev, xc, lc, 5)
    assert np.array_equal(one, want) and np.array_equal(one_conf, want_conf)


def test_bad_arguments(dev):
    from qconvnet import _lib, ops
    lib = _lib.load()
    x = torch.zeros((4, 10), dtype=torch.float32, device=dev)
    lab = torch.zeros(4, dtype=torch.int64, device=dev)
    cnt = torch.full((24,), 5, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.qcn_eval_topk_f32(p(x), 4, 10, p(lab), 0, p(cnt), None, None, None) == -1
    assert lib.qcn_eval_topk_f32(p(x), 4, 0, p(lab), 5, p(cnt), None, None, None) == -1
    assert lib.qcn_eval_topk_f32(p(x), 4, 10, p(lab), 5, None, None, None, None) == -1
    assert lib.qcn_eval_topk_f32(None, 4, 10, p(lab), 5, p(cnt), None, None, None) == -1
    assert lib.qcn_eval_topk_f32(p(x), 4, 10, None, 5, p(cnt), None, None, None) == -1
    assert lib.qcn_eval_topk_f32(p(x), -1, 10, p(lab), 5, p(cnt), None, None, None) == -1
    assert lib.qcn_eval_topk_f32(p(x), 0, 10, p(lab), 5, p(cnt), None, None, None) == 0
    out = ops.eval_topk(x[:0], lab[:0], 5, cnt)
    assert out is cnt and cnt.cpu().tolist() == [5] * 24
    with pytest.raises(_lib.QcnError):
        ops.eval_topk(x, lab, 0, cnt)
    with pytest.raises(ValueError):
        ops.eval_topk(x, lab[:3], 5, cnt)
    with pytest.raises(ValueError):
        ops.eval_topk(x, lab, 5, cnt[:23])
    with pytest.raises(TypeError):
        ops.eval_topk(x, lab.int(), 5, cnt)
    assert cnt.cpu().tolist() == [5] * 24


# ------------------------------------------------ ModelEvaluator(counts="device")
class _Fixed:
    """A model stand-in that returns a fixed logits table (on whatever device
    the table is), one batch per call."""

    def __init__(self, logits, device=None):
        self.logits = torch.from_numpy(np.ascontiguousarray(logits))
        if device is not None:
            self.logits = self.logits.to(device)
        self.i = 0

    def eval(self):
        return self

    def cpu(self):
        return self

    def to(self, device):
        return self

    def __call__(self, x):
        out = self.logits[self.i:self.i + x.shape[0]]
        self.i += x.shape[0]
        return out


def _loader(labels, bs=128):
    n = labels.shape[0]
    x = torch.zeros(n, 1)
    return [(x[i:i + bs], torch.from_numpy(labels[i:i + bs].copy())) for i in range(0, n, bs)]


CLASSES = [f"class{i}" for i in range(10)]


def test_model_evaluator_device_equals_host_on_tiefree(dev):
    from utils.model_evaluator import ModelEvaluator
    rng = np.random.default_rng(21)
    x = R.tiefree(rng, 1000, 10)
    lab = R.labels(rng, 1000, 10, bad=0)
    loader = _loader(lab)
    host, device = ModelEvaluator(loader), ModelEvaluator(loader, device=str(dev), counts="device")
    assert (device.evaluate_accuracy(_Fixed(x, dev), verbose=False)
            == host.evaluate_accuracy(_Fixed(x), verbose=False))
    got = device.evaluate_class_accuracy(_Fixed(x, dev), CLASSES, verbose=False)
    want = host.evaluate_class_accuracy(_Fixed(x), CLASSES, verbose=False)
    assert list(got.items()) == list(want.items())
    assert (device.compare_models({"m": _Fixed(x, dev)}, CLASSES)
            == host.compare_models({"m": _Fixed(x)}, CLASSES))
    assert (device.evaluate_all(_Fixed(x, dev), CLASSES, verbose=False)
            == host.evaluate_all(_Fixed(x), CLASSES, verbose=False))


def test_model_evaluator_device_equals_evalref_on_quantised(dev):
    from utils.model_evaluator import ModelEvaluator
    rng = np.random.default_rng(22)
    n = 1000
    x = R.quantised(rng, n, 10, 8)
    lab = R.labels(rng, n, 10, bad=0)
    assert R.tied_across(x, lab, 5).mean() >= 0.05 and R.tied_across(x, lab, 1).mean() >= 0.05
    ref = R.result(x, lab, 5)
    ev = ModelEvaluator(_loader(lab), device=str(dev), counts="device")
    want_acc = (100.0 * ref["top1"] / n, 100.0 * ref["topk"] / n)
    assert ev.evaluate_accuracy(_Fixed(x, dev), verbose=False) == want_acc
    per = {CLASSES[c]: 100.0 * int(ref["class_correct"][c]) / int(ref["class_total"][c])
           for c in range(10)}
    want_cls = dict(sorted(per.items(), key=lambda kv: kv[1], reverse=True))
    got_cls = ev.evaluate_class_accuracy(_Fixed(x, dev), CLASSES, verbose=False)
    assert list(got_cls.items()) == list(want_cls.items())
    # one pass answers all three
    assert ev.evaluate_all(_Fixed(x, dev), CLASSES, verbose=False) == (*want_acc, want_cls)
    res = ev.compare_models({"m": _Fixed(x, dev)}, CLASSES)
    assert res["m"]["accuracy"] == want_acc[0] and res["m"]["class_accuracies"] == want_cls


def test_model_evaluator_device_agreement_and_host_logits(dev):
    from utils.model_evaluator import ModelEvaluator
    rng = np.random.default_rng(23)
    a = R.special(rng, 1000, 10, 8)
    b = a.copy()
    b[::3] = R.special(rng, 1000, 10, 8)[::3]
    lab = R.labels(rng, 1000, 10, bad=0)
    loader = _loader(lab)
    host = ModelEvaluator(loader).agreement(_Fixed(a), _Fixed(b))
    ev = ModelEvaluator(loader, device=str(dev), counts="device")
    got = ev.agreement(_Fixed(a, dev), _Fixed(b, dev))
    assert got == host == 100.0 * int((R.pred(a) == R.pred(b)).sum()) / 1000
    assert 40.0 < got < 95.0
    with pytest.raises(ValueError):   # a model that answers with host tensors
        ev.evaluate_accuracy(_Fixed(a), verbose=False)


# -------------------------------------------------------------------- evaluate()
N_EVAL = 2 * 1024 + 37


@pytest.fixture(scope="module")
def scored(dev):
    """A calibrated static int8 model, N_EVAL random u8 images, labels, and
    evalref's result on the logits of model(x) taken batch by batch."""
    import netfix
    from models.static_ptq_model import StaticPTQModel
    rng = np.random.default_rng(31)
    img = torch.from_numpy(rng.integers(0, 256, (N_EVAL, 32, 32, 3), dtype=np.uint8))
    ptq = StaticPTQModel(device=dev)
    ptq.load_state_dict(netfix.state_dict(netfix.load()))
    model = ptq.quantize(img[:64])
    lab = R.labels(rng, N_EVAL, 10)
    logits = np.concatenate([model(img[a:a + 1024].to(dev)).cpu().numpy()
                             for a in range(0, N_EVAL, 1024)])
    assert logits.shape == (N_EVAL, 10)
    return model, img, torch.tensor(lab), R.result(logits, lab, 5, confusion=True)


@pytest.mark.parametrize("where", ("host", "device"))
@pytest.mark.parametrize("streams", (1, 2))
def test_evaluate_equals_evalref(dev, scored, streams, where):
    from qconvnet.evaluate import evaluate
    model, img, lab, want = scored
    images = img.pin_memory() if where == "host" else img.to(dev)
    labels = lab if where == "host" else lab.to(dev)
    got = evaluate(model, images, labels, batch=1024, k=5, streams=streams, confusion=True)
    assert got["rows"] == N_EVAL and got["bad_labels"] >= 1
    assert R.same_result(got, want), (got, want)
    if streams == 2:   # shared counters, two streams: the same integers every time
        again = evaluate(model, images, labels, batch=1024, k=5, streams=2, confusion=True)
        assert R.same_result(again, got)


def test_evaluate_other_models_and_counts_object(dev, scored):
    """A model without run(x, slot=) is called as model(x); EvalCounts resets,
    and its all_reduce is the identity in one process."""
    from qconvnet.evaluate import EvalCounts, evaluate
    x, lab, r, p = _case("special", 33)
    xt = torch.tensor(x, device=dev)
    rows = iter(range(0, TOP, 300))
    got = evaluate(lambda _: xt[(a := next(rows)):a + 300], torch.zeros(TOP, 1), torch.tensor(lab),
                   batch=300, k=5, streams=2, confusion=True)
    want = R.result(x, lab, 5, confusion=True)
    assert R.same_result(got, want)
    with pytest.raises(ValueError):
        evaluate(lambda _: torch.tensor(x[:300]), torch.zeros(300, 1), torch.tensor(lab[:300]),
                 batch=300)
    c = EvalCounts(33, dev, k=5, confusion=True)
    c.update(xt, torch.tensor(lab)).all_reduce()
    assert R.same_result(c.result(), want)
    c.reset()
    assert c.result()["rows"] == 0 and not c.result()["confusion"].any()
    c.update(xt[:65], torch.tensor(lab[:65], device=dev))
    assert R.same_result(c.result(), R.result(x[:65], lab[:65], 5, confusion=True))
