"""CPU: the numpy restatement of the evaluator's scoring rule (evalref) is
pinned against torch where torch defines an answer, and the host-side pieces of
the device scorer — the opt-in switch, the count all-reduce, the ABI entries —
are checked without a device."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import evalref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cols", (10, 1000))
def test_pred_is_torch_argmax_on_special(cols):
    """NaN, +-inf, +-0 and heavy ties: pred == torch.argmax == torch.max()[1]."""
    rng = np.random.default_rng(cols)
    x = R.special(rng, 4096 if cols == 10 else 512, cols, R.levels_for(cols))
    assert np.isnan(x).any(1).mean() > 0.1 and np.isinf(x).any() and np.signbit(x[x == 0]).any()
    t = torch.from_numpy(x)
    got = R.pred(x)
    assert np.array_equal(got, torch.argmax(t, 1).numpy())
    assert np.array_equal(got, torch.max(t, 1)[1].numpy())


@pytest.mark.parametrize("cols", (10, 1000))
def test_rank_is_torch_topk_membership_on_tiefree(cols):
    """Without ties torch.topk has one answer: rank < 5 is membership in it,
    rows holding a NaN included."""
    rng = np.random.default_rng(cols + 1)
    rows = 4096 if cols == 10 else 512
    x = R.tiefree(rng, rows, cols)
    lab = R.labels(rng, rows, cols, bad=0)
    assert 0.2 < np.isnan(x).any(1).mean() < 0.4
    top = torch.from_numpy(x).topk(5, 1, True, True)[1].numpy()
    member = (top == lab[:, None]).any(1)
    assert np.array_equal(R.rank(x, lab) < 5, member)
    assert np.array_equal(R.rank(x, lab) == 0, top[:, 0] == lab)


def test_rank_is_a_stable_descending_sort_on_ties():
    """On ties rank is the label's position in a stable descending sort — what
    test_models_cpu.py takes as truth for the host evaluator."""
    rng = np.random.default_rng(3)
    x = R.quantised(rng, 4096, 10, 8)
    lab = R.labels(rng, 4096, 10, bad=0)
    order = np.argsort(-x, axis=1, kind="stable")
    pos = (order == lab[:, None]).argmax(1)
    assert np.array_equal(R.rank(x, lab), pos)
    assert R.tied_across(x, lab, 5).mean() > 0.05 and R.tied_across(x, lab, 1).mean() > 0.05


def test_bad_labels_are_misses_outside_every_bin():
    x = np.array([[1, 2, 3], [3, 2, 1], [0, 0, 0], [5, 5, 1]], np.float32)
    lab = np.array([2, 3, -1, 1], np.int64)
    c, conf, p = R.score(x, lab, 2)
    assert c.tolist() == [4, 1, 2, 2, 0, 1, 1, 0, 0, 1]
    assert p.tolist() == [2, 0, 0, 0]
    assert conf.tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 1]]


def test_counts_device_needs_a_cuda_device():
    from utils.model_evaluator import ModelEvaluator
    with pytest.raises(ValueError):
        ModelEvaluator([], device="cpu", counts="device")
    with pytest.raises(ValueError):
        ModelEvaluator([], counts="gpu")
    assert ModelEvaluator([], device="cpu").counts == "host"


def test_header_and_binding_hold_the_eval_entries():
    from qconvnet import _lib
    src = open(os.path.join(ROOT, "include", "qconvnet.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("qcn_eval_topk_f32", "qcn_eval_counters_len"):
        assert re.search(r"\b" + name + r"\s*\(", src)
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["qcn_eval_topk_f32"][1]) == 9
    lib = _lib.load()
    assert lib.qcn_eval_counters_len(10) == 24 and lib.qcn_eval_counters_len(1000) == 2004
    assert lib.qcn_eval_counters_len(0) < 0


# ----------------------------------------------------- dist.sum_counts, 2 ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _shard_counts(rank, world):
    """What a rank's EvalCounts would hold for its shard (the oracle stands
    in for the device)."""
    from qconvnet.dist import shard
    rng = np.random.default_rng(5)
    x = R.special(rng, 301, 10, 8)
    lab = R.labels(rng, 301, 10)
    s, e = shard(301, world, rank)
    c, conf, _ = R.score(x[s:e], lab[s:e], 5)
    return np.concatenate([c, conf.reshape(-1)])


def _sum_worker(rank, world, port, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (os.path.join(root, "convnet-quantization_amd"), root, here):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    try:
        from qconvnet import dist as qd
        qd.init("gloo")
        t = torch.from_numpy(_shard_counts(rank, world) + (2 ** 33 if rank == 0 else 0))
        out = qd.sum_counts(t)
        q.put((rank, out.numpy()))
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    except Exception as ex:  # surface worker failures to the parent
        q.put((rank, repr(ex)))


def test_sum_counts_two_ranks_equal_the_whole_set():
    """Each rank scores its shard; the summed int64 counts (one of them past
    2^33) equal the counts of the whole set on every rank."""
    from qconvnet import dist as qd
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sum_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        assert not isinstance(res[r], str), res[r]
    whole = _shard_counts(0, 1) + 2 ** 33
    assert np.array_equal(res[0], whole) and np.array_equal(res[1], whole)
    # world size 1: the identity, and int64 only
    t = torch.arange(5)
    assert qd.sum_counts(t) is t
    with pytest.raises(TypeError):
        qd.sum_counts(torch.zeros(3))
