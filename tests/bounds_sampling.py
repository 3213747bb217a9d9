"""Per-element bounds of the temperature samplers' kernels against float64 (tests/fake_ops_sampling.py in float64), in the style of
tests/bounds.py, whose constants and admissible-argmax rule they use.

G_ABS (derived, as ERF_ABS is; csrc/common.h states the same derivation).  g = -log(-log u) with u = (2k + 1) 2^-24.  The kernel
forms w = 1 - u exactly (a 24-bit odd integer times 2^-24), t = -log1pf(-w) and g = -logf(t), with the ocml functions:
    log1pf <= 2 ulp          t^ = t (1 + d), |d| <= 2 * 2^-23 = 2^-22; t in [2^-24, 16.64] is never denormal
    -log t^ = -log t - log(1 + d)    an ABSOLUTE error <= 2^-22 (1 + 2^-22) in g, however small t is: this is why the small side is
                                     generated directly -- log(u) itself near u = 1 has an absolute error of 2^-24 or so, which is
                                     RELATIVE error 1 in t = 2^-24 and an absolute error of log 2 in g
    logf <= 3 ulp of g       |g| <= log 2^24 = 16.64 < 32, ulp <= 2^-19: <= 3 * 2^-19
    G_ABS = 3 * 2^-19 + 2^-22 (1 + 2^-22) = 5.96e-6
The check of xl_gumbel_from_bits is U32 |g| + SLACK G_ABS (the final rounding unscaled, as everywhere in bounds.py).

The drawn index.  z = y + g in fp32: the logit error e of rowmax_logit_error (computed on the TEMPERED operands: pre = y = alpha acc +
bias / T, absdot = |alpha| |A| |B|^T, bias_abs = |bias / T|, so it is "T-scaled" by construction), G_ABS, and the rounding of the sum
U32 |z|:  E_n = e_n + G_ABS + U32 |z_n|.  A pad column (y = -1e30) carries no allowance: 0 alpha - 1e30 is exact, and -1e30 + g = -1e30
exactly in fp32 and in float64 (|g| < 17 is far below half an ulp of 1e30 in both).  With E the largest E_n of the row (or segment),
bounds.argmax_admissible on z64 = y64 + g64 is the rule: z64[got] >= max z64 - 2 SLACK E, no position exempted.
Exact rows: where y has no error at all AND all y of the row are equal (an all-zero A row without bias), z = g + const and the tests
demand the float64 argmax of g itself (test_sampling_gpu.py, the exact-tie case) instead of widening anything here.

y_s (fourth float of a record; what row_prob is computed from): the kernel's value of the logit at ITS OWN index s: SLACK e_s + TINY.

row_lse: bounds.rowmax_composed_bounds unchanged -- XL_EPI_ROWSAMPLE keeps ROWMAX's (max, sum exp) arithmetic and xl_rowsample_combine
merges them with rowmax_combine_kernel's expressions, so (b_lse) holds as derived there.  xl_sample_rows: a term passes through at
most ceil(K / 64) serial additions in its lane and 6 butterfly levels, one __expf: the same formula with n_seg = ceil(K / 64) + 6.

row_prob = expf(y_s - lse) at the kernel's own index:  p = exp(y64_s - lse64);  the exponent moves by the error of y_s (SLACK e_s)
and of lse (b_lse), its subtraction rounds once (U32 |y_s - lse|), the ocml expf is within 3 ulp and scales its argument (U32 |arg|):
    U32 p + SLACK p (SLACK e_s + b_lse + 2 U32 |y_s - lse| + 3 U32)
"""
import math

import torch

import bounds as Bd
from bounds import SLACK, TINY, U32

G_ABS = 3 * 2.0 ** -19 + 2.0 ** -22 * (1 + 2.0 ** -22)
PAD_BIAS = -1e30
T_MIN, T_MAX = 1e-3, 1e3          # the accepted temperatures (Engine.TEMPERATURE_MIN / MAX; the pad-column guarantee's range)


def gumbel_bound(g_ref):
    """xl_gumbel_from_bits against float64"""
    return U32 * g_ref.abs() + SLACK * G_ABS


def draw_error(y, g, e):
    """E_n of the module docstring for every element of y [M, N] (float64), e from bounds.rowmax_logit_error (or any per-logit error);
    pad columns (y <= -1e29): 0"""
    z = y + g
    return torch.where(y > -1e29, e + G_ABS + U32 * z.abs(), torch.zeros_like(z)), z


def check_draw(y, g, e, got, what, n_seg=1):
    """admissible draw per row (n_seg = 1) or per 64-column segment (got [M, n_seg] of GLOBAL columns): returns the number of
    admissible columns per row / segment"""
    M, N = y.shape
    En, z = draw_error(y, g, e)
    w = N // n_seg
    zz, EE = z.view(M * n_seg, w), En.view(M * n_seg, w).amax(-1)
    loc = got.reshape(M, n_seg).long() - torch.arange(n_seg, device=y.device)[None, :] * w
    real = (y.view(M * n_seg, w) > -1e29).any(-1)
    # (a segment of pad columns only has E = 0: the exact rule of argmax_admissible, the lowest column)
    n_adm = Bd.check_admissible(zz, loc.reshape(-1), EE, what)
    return n_adm.view(M, n_seg), real.view(M, n_seg)


def lse_prob_bounds(y, e, got_idx, n_seg):
    """reference and bound of row_lse and of row_prob at the kernel's own index got_idx [M]; y [M, N] float64 tempered logits"""
    lse, _, _, b_lse, _ = Bd.rowmax_composed_bounds(y, e, n_seg)
    ys = y.gather(1, got_idx.long()[:, None])[:, 0]
    es = e.gather(1, got_idx.long()[:, None])[:, 0]
    p = torch.exp(ys - lse)
    b_p = U32 * p + SLACK * p * (SLACK * es + b_lse + 2 * U32 * (ys - lse).abs() + 3 * U32) + TINY
    return lse, p, b_lse, b_p, ys, SLACK * es + TINY


def check_rows(y, g, e, n_seg, got_p, got_idx, got_lse, what):
    """the three outputs of rowsample_combine / sample_rows against float64; never a pad column.  Returns (table rows, n_adm [M])"""
    M, N = y.shape
    assert bool(((got_idx >= 0) & (got_idx < N)).all()), f"{what}: index out of range"
    assert bool((y.gather(1, got_idx.long()[:, None])[:, 0] > -1e29).all()), f"{what}: a pad column was drawn"
    n_adm, _ = check_draw(y, g, e, got_idx, f"{what} row draw")
    lse, p, b_lse, b_p, _, _ = lse_prob_bounds(y, e, got_idx, n_seg)
    res = [("row draw admissible", 0.0)]
    if got_lse is not None:                                                          # (an output the call was not given: no row)
        res.append(("row_lse", Bd.check(got_lse, lse, b_lse, f"{what} row_lse")))
    if got_p is not None:
        res.append(("row_prob", Bd.check(got_p, p, b_p, f"{what} row_prob")))
    return res, n_adm[:, 0]


def check_combine(ws, n_seg, M, seed, got_p, got_idx, got_lse, what="rowsample_combine"):
    """xl_rowsample_combine on the records `ws` it read (fp32, the kernel's own: exact inputs), as bounds.check_rowmax_combine checks
    xl_rowmax_combine.  Nothing new is derived:
      row_lse    the merge of (max, sum exp) is rowmax_combine_kernel's: bounds.rowmax_combine_bounds
      row_id     the candidates are the segments' (s, y_s); z_s = y_s + g(seed, m, s) is draw_error with e = 0 (y_s is an input): E = G_ABS
                 + U32 |z|, none for the candidate of an all-pad segment; bounds.check_admissible over the n_seg candidates of a row, the
                 lowest column where a row is exact
      row_prob   exp(y_s - lse) at the kernel's own index: lse_prob_bounds' expression with e_s = 0 and the combine's lse bound
    Without a row_id the index is the float64 draw's, and a row that admits more than one candidate is left out of row_prob."""
    import fake_ops_sampling as FS
    dev = ws.device
    mx, se, idx, ys = Bd.rowmax_records(ws, n_seg, M)                                # [n_seg, M]
    lse, _, b_lse, _, _ = Bd.rowmax_combine_bounds(mx, se, n_seg)
    ys = ys.double()
    g = FS.gumbel_noise(seed, torch.arange(M, device=dev)[None, :], idx)
    En, z = draw_error(ys, g, torch.zeros_like(ys))
    zt, E = z.t().contiguous(), En.amax(0)
    first = (zt == zt.amax(-1, keepdim=True)).double().argmax(-1)
    res = []
    if got_idx is not None:
        hit = idx == got_idx[:M].long()[None, :]
        assert bool(hit.any(0).all()), f"{what}: a row_id that is no segment's candidate"
        seg = hit.double().argmax(0)
        Bd.check_admissible(zt, seg, E, f"{what} row_id")
        res.append(("row_id admissible", 0.0))
        keep = torch.ones(M, dtype=torch.bool, device=dev)
    else:
        seg = first
        keep = Bd.argmax_admissible(zt, first, E)[1] == 1
    if got_lse is not None:
        res.append(("row_lse", Bd.check(got_lse[:M], lse, b_lse, f"{what} row_lse")))
    if got_p is not None:
        d = ys.gather(0, seg[None, :])[0] - lse
        p = torch.exp(d)
        b_p = U32 * p + SLACK * p * (b_lse + 2 * U32 * d.abs() + 3 * U32) + TINY
        res.append(("row_prob", Bd.check(got_p[:M][keep], p[keep], b_p[keep], f"{what} row_prob")))
    return res


def check_records(aux, y, g, e, what):
    """every record {max, sum exp, s, y_s} of the XL_EPI_ROWSAMPLE epilogue against float64"""
    M, N = y.shape
    n_seg = N // 64
    mx, se, idx, ys = Bd.rowmax_records(aux, n_seg, M)
    ref_mx, ref_se, _, b_mx, b_se = Bd.rowmax_record_bounds(y, e)
    res = [("max", Bd.check(mx.t(), ref_mx, b_mx, f"{what} segment max")),
           ("sum exp", Bd.check(se.t(), ref_se, b_se, f"{what} segment sum exp"))]
    got = idx.t()
    lo = torch.arange(n_seg, device=y.device)[None, :] * 64
    assert bool(((got >= lo) & (got < lo + 64)).all()), f"{what}: segment index outside its segment"
    n_adm, real = check_draw(y, g, e, got, f"{what} segment draw", n_seg)
    y_at = y.gather(1, got)
    e_at = e.gather(1, got)
    assert bool((y_at[real] > -1e29).all()), f"{what}: a pad column was drawn beside a real one"
    res.append(("draw admissible", 0.0))
    res.append(("y_s", Bd.check(ys.t().double(), y_at, SLACK * e_at + TINY, f"{what} y_s")))
    return res, n_adm


def tempered_reference(A, Bm, bias_T, alpha, seed):
    """float64 view of one XL_EPI_ROWSAMPLE launch on ITS OWN operands (A [M, K], Bm [N, K] bf16, bias_T [N] fp32 with PAD_BIAS in
    the pad columns, alpha as the kernel receives it: fp32): y = alpha A Bm^T + bias_T, the noise g, the logit error e."""
    import fake_ops_sampling as FS
    M, K = A.shape
    N = Bm.shape[0]
    dev = A.device
    a32 = float(torch.tensor(alpha, dtype=torch.float32))
    y = a32 * (A.double() @ Bm.double().t()) + bias_T.double()[None, :]
    absdot = abs(a32) * (A.double().abs() @ Bm.double().abs().t())
    bias_abs = torch.where(bias_T < -1e29, torch.zeros_like(bias_T), bias_T.abs()).double()[None, :]
    e = Bd.rowmax_logit_error(y, absdot, bias_abs, K)
    g = FS.gumbel_noise(seed, torch.arange(M, device=dev)[:, None], torch.arange(N, device=dev)[None, :])
    return y, g, e


def logits_reference(logits, K, inv_T, seed):
    """the same for xl_sample_rows on fp32 logits [M, >= K]: y = logits * fp32(inv_T), e = U32 |y| (the one multiply)"""
    import fake_ops_sampling as FS
    M = logits.shape[0]
    dev = logits.device
    y = logits[:, :K].double() * float(torch.tensor(inv_T, dtype=torch.float32))
    g = FS.gumbel_noise(seed, torch.arange(M, device=dev)[:, None], torch.arange(K, device=dev)[None, :])
    return y, g, U32 * y.abs()


# ------------------------------------------------------------------------------------------------------------------ statistics
def normal_quantile_upper(p):
    """z with P(N(0,1) > z) = p, by bisection on erfc"""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(mid / math.sqrt(2.0)) > p:
            lo = mid
        else:
            hi = mid
    return hi


def chi2_threshold(dof, p=1e-9):
    """upper p-quantile of chi-square(dof): Wilson-Hilferty, dof (1 - 2/(9 dof) + z sqrt(2/(9 dof)))^3"""
    z = normal_quantile_upper(p)
    a = 2.0 / (9.0 * dof)
    return dof * (1.0 - a + z * math.sqrt(a)) ** 3


def chi2_stat(ids, expected):
    """Pearson statistic of the counts of ids (int tensor) against `expected` counts [n]"""
    cnt = torch.bincount(ids.reshape(-1).long(), minlength=expected.numel()).double()
    assert cnt.numel() == expected.numel()
    return float(((cnt - expected) ** 2 / expected).sum())


def agreement_interval(p, n, tail=1e-9):
    """[lo, hi] for the number of agreements among n independent pairs that agree with probability p (normal approximation of the
    binomial at the two-sided `tail`, plus one count for the discreteness)"""
    z = normal_quantile_upper(tail / 2)
    s = z * math.sqrt(n * p * (1 - p)) + 1
    return n * p - s, n * p + s
