"""Numpy restatement of the evaluator's scoring rule (include/qconvnet.h,
qcn_eval_topk_f32) and the input families its tests use.

Order: NaN above everything and all NaNs equal, -0.0 == +0.0, otherwise the
usual order with +-inf as values.  For a row x[0..C) with label l:
  rank = #{ j : x[j] > x[l]  or  (x[j] == x[l] and j < l) }
  top-k hit iff rank < k; top-1 hit iff rank == 0;
  pred = the lowest j whose value is maximal.
A label outside [0, C) makes the row a miss, counted in rows and bad_labels
and in no class bin or confusion cell.

Written with float comparisons and isnan, not with the kernel's integer keys,
so the two do not share a mistake."""
import numpy as np

F32 = np.float32
BAD_LABELS = (-1, None, 2 ** 40 + 3)     # None stands for `cols`


def gt(a, b):
    """a strictly above b in the order."""
    an, bn = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        return (an & ~bn) | (~an & ~bn & (a > b))


def eq(a, b):
    an, bn = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        return (an & bn) | (~an & ~bn & (a == b))   # -0.0 == +0.0 in IEEE


def in_range(labels, cols):
    labels = np.asarray(labels, np.int64)
    return (labels >= 0) & (labels < cols)


def rank(x, labels):
    """int64 [rows]: columns that beat the label's (-1 for a bad label)."""
    x = np.asarray(x, F32)
    rows, cols = x.shape
    labels = np.asarray(labels, np.int64)
    ok = in_range(labels, cols)
    l = np.where(ok, labels, 0)
    t = x[np.arange(rows), l][:, None]
    j = np.arange(cols)[None, :]
    beats = gt(x, t) | (eq(x, t) & (j < l[:, None]))
    return np.where(ok, beats.sum(1), -1).astype(np.int64)


def pred(x):
    """int64 [rows]: the lowest index of a maximal value (the first NaN if any)."""
    x = np.asarray(x, F32)
    nan = np.isnan(x)
    has = nan.any(1)
    clean = np.where(nan, -np.inf, x)
    top = clean.max(1, keepdims=True)
    first_max = (clean == top).argmax(1)          # argmax of bools: the first True
    return np.where(has, nan.argmax(1), first_max).astype(np.int64)


def score(x, labels, k, rank_pred=None):
    """(counters int64 [4 + 2C], confusion int64 [C, C], pred int64 [rows]).
    ``rank_pred``: (rank(x, labels), pred(x)) when the caller already has them
    (they do not depend on k)."""
    x = np.asarray(x, F32)
    rows, cols = x.shape
    labels = np.asarray(labels, np.int64)
    ok = in_range(labels, cols)
    r, p = rank_pred if rank_pred is not None else (rank(x, labels), pred(x))
    top1, topk = ok & (r == 0), ok & (r < k)
    counters = np.zeros(4 + 2 * cols, np.int64)
    counters[0], counters[1], counters[2], counters[3] = rows, top1.sum(), topk.sum(), (~ok).sum()
    counters[4:4 + cols] = np.bincount(labels[ok], minlength=cols)
    counters[4 + cols:] = np.bincount(labels[top1], minlength=cols)
    confusion = np.zeros((cols, cols), np.int64)
    np.add.at(confusion, (labels[ok], p[ok]), 1)
    return counters, confusion, p


def result(x, labels, k, confusion=False):
    """score() as the dict EvalCounts.result() returns."""
    c, conf, _ = score(x, labels, k)
    cols = np.asarray(x).shape[1]
    return {"rows": int(c[0]), "top1": int(c[1]), "topk": int(c[2]), "bad_labels": int(c[3]),
            "class_total": c[4:4 + cols], "class_correct": c[4 + cols:],
            "confusion": conf if confusion else None}


def same_result(a, b):
    for key in ("rows", "top1", "topk", "bad_labels"):
        if a[key] != b[key]:
            return False
    for key in ("class_total", "class_correct", "confusion"):
        if (a[key] is None) != (b[key] is None):
            return False
        if a[key] is not None and not np.array_equal(a[key], b[key]):
            return False
    return True


# ------------------------------------------------------------ input families
def quantised(rng, rows, cols, levels):
    """0.25 * (q - levels // 2), q uniform in 0..levels: what static int8
    logits s * (q - zp) look like — ties are the normal case."""
    q = rng.integers(0, levels, (rows, cols))
    return (0.25 * (q - levels // 2)).astype(F32)


def special(rng, rows, cols, levels):
    """quantised() with NaN, +inf, -inf and -0.0 written in: about 2 % of the
    elements each up to 25 columns; above that 0.5 / cols each, so that a wide
    row holds a NaN about four times in ten, not always (a row whose maximum
    is always NaN would leave +inf and the finite levels nothing to decide)."""
    x = quantised(rng, rows, cols, levels)
    p = min(0.02, 0.5 / cols)
    u = rng.random((rows, cols))
    for i, v in enumerate((np.nan, np.inf, -np.inf, -0.0)):
        x[(u >= p * i) & (u < p * (i + 1))] = v
    return x


def tiefree(rng, rows, cols):
    """A per-row permutation of 0..cols, with a NaN in 30 % of the rows."""
    x = rng.permuted(np.tile(np.arange(cols, dtype=F32), (rows, 1)), axis=1)
    hit = rng.random(rows) < 0.3
    x[hit, rng.integers(0, cols, rows)[hit]] = np.nan
    return x


NEAR_TOP = 8   # labels(): how many leading columns a near-top label is drawn from


def labels(rng, rows, cols, bad=0.03, x=None):
    """Uniform in range; about `bad` of them replaced by -1, cols and
    2**40 + 3.

    A uniform label has rank r with probability exactly 1 / cols for every r
    (each row has one column of each rank), so above 16 columns uniform labels
    cannot give 2 % of top-1 hits whatever the values are.  With ``x`` given
    and cols > 16, half the rows therefore take their label from the row's
    NEAR_TOP leading columns (descending, stable; NaN first) instead: ranks
    0 .. 7, on both sides of k = 1 and k = 5.  The other half stays uniform."""
    lab = rng.integers(0, cols, rows).astype(np.int64)
    if x is not None and cols > 16:
        lead = np.argsort(-np.where(np.isnan(x), np.inf, x), axis=1, kind="stable")
        near = rng.random(rows) < 0.5
        pick = lead[np.arange(rows), rng.integers(0, min(NEAR_TOP, cols), rows)]
        lab[near] = pick[near]
    if bad:
        u = rng.random(rows)
        kinds = np.array([cols if b is None else b for b in BAD_LABELS], np.int64)
        sel = u < bad
        lab[sel] = kinds[rng.integers(0, len(kinds), rows)[sel]]
    return lab


def levels_for(cols):
    """Level count for quantised() at ``cols`` columns.  With L levels a level
    holds cols / L columns on average.  The label's value is tied across the
    k = 1 or k = 5 boundary only if its level's run of columns straddles rank
    k, and a hit is decided by value, not by index, only if levels change
    within the first few ranks: both want a few columns per level among the
    leading ones.  8 levels up to 16 columns (1.25 per level at 10 columns);
    above that cols // 4 levels, four columns per level, so the level count
    grows with cols and the NEAR_TOP leading columns span two or three levels
    (with two per level, `special` rows — whose maximum is often a lone NaN or
    +inf — tie across k = 1 in only about 5 % of rows).
    The tests assert the resulting coverage; nothing here is assumed."""
    return 8 if cols <= 16 else max(8, cols // 4)


def tied_across(x, labels, k):
    """bool [rows]: the label's value is tied across the k boundary — the row
    would flip between hit and miss under another tie order: strictly fewer
    than k columns are above it, and at least k are above or equal to it
    (itself excluded)."""
    x = np.asarray(x, F32)
    rows, cols = x.shape
    labels = np.asarray(labels, np.int64)
    ok = in_range(labels, cols)
    l = np.where(ok, labels, 0)
    t = x[np.arange(rows), l][:, None]
    above = gt(x, t).sum(1)
    same = eq(x, t).sum(1) - 1
    return ok & (above < k) & (above + same >= k)
