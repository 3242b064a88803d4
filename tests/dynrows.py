"""Shared inputs and references of the per-sample dynamic Linear tests
(test_dynamic_rows_cpu.py pins rows_ref against torch; test_gpu_dynamic_rows.py
compares the HIP kernels with it).  Host only: nothing here touches a device."""
import functools

import numpy as np

import opedge as E
from oracle import qref

F32 = np.float32

# neighbouring rows need qparams many orders of magnitude apart: a kernel that
# shares anything between rows cannot pass
ORDER = ("normal", "huge", "zero", "positive", "tiny", "negative", "onehot", "subnormal", "constant",
         "negzero")

# (m, k, n): smallest; rows 12 bytes apart (scalar loads, generic GEMM); k % 4 != 0; k % 4 == 0 but
# k % 128 != 0 (twice); MFMA with a partial feature block; a second 32-row block with 31 phantom
# rows and a second feature block of one; three row blocks with a tail of one; fc1's K; fc2's shape
SHAPES = ((1, 1, 1), (4, 3, 5), (2, 130, 9), (3, 40, 7), (7, 96, 33), (5, 128, 33), (33, 384, 65),
          (65, 128, 64), (3, 4096, 64), (33, 512, 10))


def mixed_rows(m, k, seed, order=ORDER):
    """[m, k] fp32: row i is one row of input class order[i % len(order)]."""
    return np.stack([E.dyn_input(order[i % len(order)], 1, k, seed + i)[0] for i in range(m)])


def rows_ref(x, w, s_w, b, rr=True):
    """The per-sample dynamic Linear: quantized::linear_dynamic of every row alone."""
    return np.concatenate([qref.linear_dynamic(x[i:i + 1], w, s_w, b, reduce_range=rr)
                           for i in range(x.shape[0])])


def rows_qparams(x, rr=True):
    """(scale [m] fp32, zero_point [m] int32) of the rows."""
    sz = [qref.choose_qparams_dynamic(r.min(), r.max(), reduce_range=rr) for r in x]
    return np.array([s for s, _ in sz], F32), np.array([z for _, z in sz], np.int32)


@functools.lru_cache(maxsize=None)
def case(m, k, n, seed=11):
    """(x, w, s_pt, s_pc, b) of one shape; shared, so treat as read-only."""
    return (mixed_rows(m, k, seed),) + E.dyn_weights(k, n, k + n)
