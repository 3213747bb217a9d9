"""Bounds and checks of the validation scores (XL_EPI_ROWSCORE, xl_rowscore_combine, xl_score_rows) against float64, on top of
tests/bounds.py.  Each check returns [(output name, worst |err| / bound)] and raises on the first output beyond its bound.

Where the bounds come from:
  record slots 0-2   XL_EPI_ROWMAX's, unchanged: bounds.rowmax_record_bounds, the admissible segment argmax
  record slot 3      x_label is ONE accumulator value of the launch: within the element bound e of bounds.rowmax_logit_error (the
                     bound of the fp32 accumulator against the float64 logit: no further arithmetic touches it) in the label's
                     segment; exactly -inf in every other segment and for every label outside [0, N)
  row_nll            lse - x_label: bounds.rowmax_composed_bounds' lse bound plus e at the label, plus the subtraction's rounding
                     U32 |nll|; exactly 0 for an ignored label
  row_max            the maximum of perturbed values lies within the largest perturbation of the true maximum: max_n e
  row_pred           bounds.check_admissible over the whole row, and never a pad column
  totals             [1] and [2] are counts below 2^24: exact in fp32 -- [2] against the row_pred RETURNED (the kernel's hits are
                     hits of its own prediction); [0] is an fp32 sum of the M returned row_nll in some fixed order:
                     bounds.sum_bound(sum |nll|, M), on top of the previous value's rounding
  xl_score_rows      logits in memory are exact inputs: argmax and maximum exact (lowest index), lse within bounds.ce_bounds, nll =
                     lse - x_label adds one rounding
"""
import torch

import bounds as Bd
from bounds import SLACK, TINY, U32, check, check_admissible, check_exact


def valid_labels(labels, n_cols):
    return (labels >= 0) & (labels < n_cols)


def check_rowscore_records(aux, pre, e, labels, what="gemm ROWSCORE"):
    """every record of the epilogue against the float64 logits pre [M, N] (pad columns included), labels [M] int64"""
    M, N = pre.shape
    n_seg = N // 64
    mx, se, idx, slot = Bd.rowmax_records(aux, n_seg, M)
    ref_mx, ref_se, E, b_mx, b_se = Bd.rowmax_record_bounds(pre, e)
    res = [("max", check(mx.t(), ref_mx, b_mx, f"{what} segment max")),
           ("sum exp", check(se.t(), ref_se, b_se, f"{what} segment sum exp"))]
    local = idx.t() - torch.arange(n_seg, device=idx.device)[None, :] * 64
    check_admissible(pre.reshape(M * n_seg, 64), local.reshape(-1), E.reshape(-1), f"{what} segment argmax")
    res.append(("argmax admissible", 0.0))
    inside = valid_labels(labels, N)
    ref = torch.full((M, n_seg), -float("inf"), dtype=torch.float64, device=pre.device)
    bnd = torch.zeros(M, n_seg, dtype=torch.float64, device=pre.device)
    rows = inside.nonzero()[:, 0]
    lab = labels[rows]
    ref[rows, lab // 64] = pre[rows, lab]
    bnd[rows, lab // 64] = e[rows, lab] + TINY
    res.append(("x_label", check(slot.t().double(), ref, bnd, f"{what} label slot")))
    return res


def rowscore_row_bounds(pre, e, n_seg, labels, n_cols):
    """float64 reference and bounds of row_nll and row_max; pre [M, N] with the pad columns, labels [M]"""
    lse, _, E, b_lse, _ = Bd.rowmax_composed_bounds(pre, e, n_seg)
    valid = valid_labels(labels, n_cols)
    col = labels.clamp(0, n_cols - 1)
    xl, el = pre.gather(1, col[:, None])[:, 0], e.gather(1, col[:, None])[:, 0]
    nll = torch.where(valid, lse - xl, torch.zeros_like(lse))
    b_nll = torch.where(valid, b_lse + el + U32 * nll.abs(), torch.zeros_like(lse))
    return nll, b_nll, pre.amax(-1), E + TINY, E, valid


def check_rowscore_rows(pre, e, n_seg, labels, n_cols, got_nll, got_pred, got_max, what="ROWSCORE + combine"):
    nll, b_nll, mx, b_mx, E, valid = rowscore_row_bounds(pre, e, n_seg, labels, n_cols)
    res = []
    if got_pred is not None:
        check_admissible(pre, got_pred, E, f"{what} row_pred")
        assert int(got_pred.max()) < n_cols, f"{what}: a pad column was predicted ({int(got_pred.max())} >= {n_cols})"
        res.append(("row_pred admissible", 0.0))
    if got_nll is not None:
        res.append(("row_nll", check(got_nll, nll, b_nll, f"{what} row_nll")))
    if got_max is not None:
        res.append(("row_max", check(got_max, mx, b_mx, f"{what} row_max")))
    return res


def check_totals(before, after, labels, n_cols, got_nll, got_pred, what="totals"):
    """totals[0:3] after a launch that started from `before`: counts exact, the nll sum within the fp32 sum bound of the row_nll
    the launch returned.  totals[3] is not touched."""
    valid = valid_labels(labels, n_cols)
    M = labels.numel()
    d = (after.double() - before.double())
    assert float(after[1]) == float(before[1]) + int(valid.sum()), (what, "count", float(after[1]), float(before[1]), int(valid.sum()))
    hits = int((valid & (got_pred.long() == labels)).sum())
    assert float(after[2]) == float(before[2]) + hits, (what, "correct", float(after[2]), float(before[2]), hits)
    ref = got_nll.double().sum()
    b = Bd.sum_bound(got_nll.double().abs().sum(), M, ref) + U32 * (before[0].double().abs() + after[0].double().abs())
    r = check(d[0:1], ref.reshape(1), b.reshape(1), f"{what} nll sum")
    check_exact(after[3:4], before[3:4], f"{what} fourth float")
    return [("totals nll sum", r), ("totals count", 0.0), ("totals correct", 0.0)]


def rowscore_combine_bounds(ws, n_seg, M, labels, n_cols):
    """xl_rowscore_combine on the records `ws` it read (fp32, the kernel's own: exact inputs), as bounds.check_rowmax_combine checks
    xl_rowmax_combine.  The merge of (max, sum exp, argmax) is rowmax_combine_kernel's: row_pred is exact (the lowest column among
    the segments that hold the global maximum), row_max is exact (a maximum of inputs), lse within bounds.rowmax_combine_bounds;
    x_label = the maximum over the label slots (one is not -inf) is exact, and row_nll = lse - x_label rounds once more (SLACK U32
    |nll|, as score_rows_bounds has it); exactly 0 for a label outside [0, n_cols).
    Returns (nll, its bound, row_pred, row_max, valid)."""
    mx, se, idx, slot = Bd.rowmax_records(ws, n_seg, M)
    lse, _, b_lse, _, _ = Bd.rowmax_combine_bounds(mx, se, n_seg)
    gmx = mx.amax(0)
    pred = torch.where(mx == gmx[None, :], idx, torch.full_like(idx, 2 ** 31 - 1)).amin(0)
    valid = valid_labels(labels, n_cols) if labels is not None else torch.zeros(M, dtype=torch.bool, device=ws.device)
    nll = torch.where(valid, lse - slot.double().amax(0), torch.zeros_like(lse))
    b_nll = torch.where(valid, b_lse + SLACK * U32 * nll.abs() + TINY, torch.zeros_like(lse))
    return nll, b_nll, pred, gmx, valid


def check_rowscore_combine(ws, n_seg, M, labels, n_cols, got_nll, got_pred, got_max, what="rowscore_combine"):
    nll, b_nll, pred, gmx, _ = rowscore_combine_bounds(ws, n_seg, M, labels, n_cols)
    res = []
    if got_pred is not None:
        res.append(("row_pred", check_exact(got_pred[:M].long(), pred, f"{what} row_pred")))
    if got_max is not None:
        res.append(("row_max", check_exact(got_max[:M].double(), gmx, f"{what} row_max")))
    if got_nll is not None:
        res.append(("row_nll", check(got_nll[:M], nll, b_nll, f"{what} row_nll")))
    return res


def check_totals_ref(before, after, valid, hits, nll, b_nll, what="totals"):
    """check_totals for a launch that returned no row_nll or no row_pred: the counts against `valid` and the float64 hits (exact
    wherever row_pred is: on the kernel's own records, on logits in memory), the nll sum against the float64 row_nll -- the fp32
    sum bound of check_totals plus the rows' own bounds sum_m b_nll."""
    M = valid.numel()
    assert float(after[1]) == float(before[1]) + int(valid.sum()), (what, "count", float(after[1]), float(before[1]), int(valid.sum()))
    assert float(after[2]) == float(before[2]) + int(hits.sum()), (what, "correct", float(after[2]), float(before[2]), int(hits.sum()))
    ref = nll.sum()
    b = Bd.sum_bound(nll.abs().sum() + b_nll.sum(), M, ref) + b_nll.sum() + U32 * (before[0].double().abs() + after[0].double().abs())
    r = check((after.double() - before.double())[0:1], ref.reshape(1), b.reshape(1), f"{what} nll sum")
    check_exact(after[3:4], before[3:4], f"{what} fourth float")
    return [("totals nll sum", r), ("totals count", 0.0), ("totals correct", 0.0)]


def score_rows_bounds(x, labels):
    """xl_score_rows over float64 copies x [M, K] of the fp32 logits it read"""
    M, K = x.shape
    lse = torch.logsumexp(x, 1)
    valid = valid_labels(labels, K) if labels is not None else torch.zeros(M, dtype=torch.bool, device=x.device)
    b_lse, _ = Bd.ce_bounds(x, valid.double(), 0.0, lse, torch.zeros_like(x), torch.float32)
    xl = x.gather(1, (labels if labels is not None else torch.zeros(M, dtype=torch.int64, device=x.device)).clamp(0, K - 1)[:, None])[:, 0]
    nll = torch.where(valid, lse - xl, torch.zeros_like(lse))
    b_nll = torch.where(valid, b_lse + SLACK * U32 * nll.abs() + TINY, torch.zeros_like(lse))
    first = (x == x.amax(-1, keepdim=True)).double().argmax(-1)
    return nll, b_nll, first, x.amax(-1), valid


def check_score_rows(x, labels, got_nll, got_pred, got_max, what="score_rows"):
    nll, b_nll, first, mx, _ = score_rows_bounds(x, labels)
    res = []
    if got_pred is not None:
        res.append(("row_pred", check_exact(got_pred.long(), first, f"{what} row_pred")))
    if got_max is not None:
        res.append(("row_max", check_exact(got_max.double(), mx, f"{what} row_max")))
    if got_nll is not None:
        res.append(("row_nll", check(got_nll, nll, b_nll, f"{what} row_nll")))
    return res
