"""Bounds of xl_sample_rows_trunc against float64, in the form of tests/bounds_sampling.py (whose draw / lse / prob bounds they use)
with the constants of tests/bounds.py.  The reference is tests/fake_ops_truncation.restate in float64 ON THE KERNEL'S OWN fp32 y.

EXACT.  y = logits * fp32(1 / T) is one IEEE multiply (the kernel uses an uncontracted multiply), the rank is a comparison of those
values and of columns, the candidate set a count, the min-p cut `y >= mx + log_min_p` one fp32 add and a comparison: none of it
has an error, so k_c and k_m (the number of candidates that pass min-p) of the fp32 restatement are demanded EXACTLY: with top-p
off, row_kept == min(k_c, k_m); the drawn column must be one of the first row_kept columns of the restated rank order.

TOP-P.  The kernel tests  c^_r < fl(top_p Z^)  with  c^_r = the fp32 sum, in rank order, of e^_j = __expf(fl(y_j - mx)), j < r.
  e^_j = e_j (1 + d_j):    the subtraction rounds (U32 t_j in the exponent, t_j = mx - y_j), __expf scales its argument (U32 t_j),
                           v_exp_f32 EXP_ULP ulp:                  |d_j| <= (2 t_j + EXP_ULP) U32
  the sequential sum:      a term passes through at most r - 1 additions:     (r - 1) U32 relative
      |c^_r - c_r| <= dc_r = U32 sum_{j<r} e_j (2 t_j + EXP_ULP + r - 1)
  Z^ = Z (1 + rho):        |rho| <= r_Z, the arithmetic term of bounds.rowmax_composed_bounds with the segment count of this
                           kernel's reduction tree (N_SEG below) and no logit error:
                           r_Z = (n_seg (EXP_ULP + 3) + 4 EXP_ULP + 14) U32 + 4 U32 sum_n t_n w_n / sum_n w_n
  the product top_p Z^:    one rounding, U32
So the kernel compares q^_r = c^_r / (Z (1 + rho)(1 + u)) with top_p, and with q_r = c_r / Z in float64
      |q^_r - q_r| <= b_r = SLACK (dc_r / Z + q_r (r_Z + U32))
Rank r is surely kept if q_r < top_p - b_r and surely cut if q_r >= top_p + b_r (top_p: the fp32 value the kernel receives); rank 0
is always kept.  The kept set is a prefix: k_lo = the first rank that is not surely kept, k_hi = the first rank that is surely cut
(k_c if none), both clamped by the exact k_m; row_kept must lie in [k_lo, k_hi].  Nothing here is tuned: for the shapes of the
tests b_r stays below 1e-4 (K = 10 000, r = 256: about 6e-5), and `undecided` reports the rows with k_lo != k_hi.

N_SEG(K): a term of Z passes through ceil(K / 256) serial additions in its thread, 6 butterfly levels and 3 additions of the four wave
sums: ceil(K / 256) + 9, the count bounds_sampling.lse_prob_bounds takes for row_lse and row_prob (y is exact: e = 0).

DRAW.  Against the kernel's own k_s = row_kept: the column must have rank < k_s, and with z64 = y + g64 over the first k_s ranks
z64[s] >= max z64 - 2 SLACK E, E = max over those ranks of G_ABS + U32 |z| (bounds_sampling.draw_error with e = 0): this is
bounds.argmax_admissible, no row exempted.
"""
import math

import torch

import bounds as Bd
import bounds_sampling as BS
import fake_ops_sampling as FS
import fake_ops_truncation as FT
from bounds import EXP_ULP, SLACK, U32


def n_seg(K):
    return (K + 255) // 256 + 9


def top_p_interval(ref, top_p):
    """ref: FT.restate(..., compute=float64).  Returns (k_lo, k_hi, b [M, k_c]) before the clamp by k_m."""
    y = ref.y32.double()
    M, K = y.shape
    k_c = ref.k_c
    if FT.f32(top_p) >= 1.0:
        full = torch.full((M,), k_c, dtype=torch.int64, device=y.device)
        return full, full.clone(), torch.zeros(M, k_c, dtype=torch.float64, device=y.device)
    mx = y.amax(1, keepdim=True)
    t_all = mx - y
    w_all = torch.exp(-t_all)
    Z = w_all.sum(1)
    r_Z = (n_seg(K) * (EXP_ULP + 3) + 4 * EXP_ULP + 14) * U32 + 4 * U32 * (t_all * w_all).sum(1) / Z
    yc = y.gather(1, ref.order[:, :k_c])
    t = mx - yc
    e = torch.exp(-t)
    zero = torch.zeros(M, 1, dtype=torch.float64, device=y.device)
    c = torch.cat([zero, torch.cumsum(e, 1)[:, :-1]], 1)                                  # c_r = sum_{j<r} e_j
    a = torch.cat([zero, torch.cumsum(e * (2 * t + EXP_ULP), 1)[:, :-1]], 1)
    r = torch.arange(k_c, device=y.device, dtype=torch.float64)[None, :]
    dc = U32 * (a + (r - 1).clamp(min=0) * c)
    q = c / Z[:, None]
    b = SLACK * (dc / Z[:, None] + q * (r_Z[:, None] + U32))
    p32 = FT.f32(top_p)
    sure_keep = q < p32 - b
    sure_cut = q >= p32 + b
    sure_keep[:, 0] = True
    sure_cut[:, 0] = False
    k_lo = sure_keep.to(torch.int64).cumprod(1).sum(1)                                     # ranks before the first not surely kept
    k_hi = (~sure_cut).to(torch.int64).cumprod(1).sum(1)                                   # ranks before the first surely cut
    return k_lo, k_hi, b


def check_trunc(logits, K, inv_T, seed, top_k, top_p, log_min_p, got_p, got_idx, got_lse, got_kept, what, row0=0):
    """all four outputs of one launch on logits [M, >= K].  Returns a dict: worst ratios, the undecided share, the kept sizes."""
    ref = FT.restate(logits, K, inv_T, seed, top_k, top_p, log_min_p, torch.float64, row0=row0)
    y = ref.y32.double()
    M = y.shape[0]
    dev = y.device
    got_idx, got_kept = got_idx.long(), got_kept.long()
    assert bool(((got_idx >= 0) & (got_idx < K)).all()), f"{what}: index out of range"
    # kept count: exact parts and the top-p interval
    k_lo, k_hi, b = top_p_interval(ref, top_p)
    k_lo, k_hi = torch.minimum(k_lo, ref.k_m), torch.minimum(k_hi, ref.k_m)
    bad = (got_kept < k_lo) | (got_kept > k_hi)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {M} kept counts outside their interval; first at row {i}: got "
                             f"{int(got_kept[i])}, admissible [{int(k_lo[i])}, {int(k_hi[i])}] (k_c {ref.k_c}, min-p count {int(ref.k_m[i])})")
    # the draw, against the kernel's own kept count
    k_c = ref.k_c
    cand = ref.order[:, :k_c]
    hit = cand == got_idx[:, None]
    rank = torch.where(hit.any(1), hit.to(torch.uint8).argmax(1), torch.full((M,), k_c, dtype=torch.int64, device=dev))
    out = rank >= got_kept
    if bool(out.any()):
        i = int(out.nonzero()[0])
        raise AssertionError(f"{what}: {int(out.sum())} of {M} draws not admissible: outside the kept set; first at row {i}: column "
                             f"{int(got_idx[i])} has rank {int(rank[i]) if int(rank[i]) < k_c else '>= k_c'}, row_kept {int(got_kept[i])}")
    yc = y.gather(1, cand)
    g = FS.gumbel_noise(seed, (torch.arange(M, device=dev) + row0)[:, None], cand)
    inside = torch.arange(k_c, device=dev)[None, :] < got_kept[:, None]
    En, z = BS.draw_error(yc, g, torch.zeros_like(yc))
    E = torch.where(inside, En, torch.zeros_like(En)).amax(1)
    z = torch.where(inside, z, torch.full_like(z, -math.inf))
    n_adm = Bd.check_admissible(z, rank, E, f"{what} draw")
    # lse and the probability of the drawn column under the full softmax
    lse, p, b_lse, b_p, _, _ = BS.lse_prob_bounds(y, torch.zeros_like(y), got_idx, n_seg(K))
    return {"row_lse": Bd.check(got_lse, lse, b_lse, f"{what} row_lse"), "row_prob": Bd.check(got_p, p, b_p, f"{what} row_prob"),
            "undecided": float((k_lo != k_hi).double().mean()), "b_max": float(b.max()) if b.numel() else 0.0,
            "kept": (int(got_kept.min()), int(got_kept.median()), int(got_kept.max())), "n_adm": n_adm, "ref": ref,
            "k_lo": k_lo, "k_hi": k_hi}
