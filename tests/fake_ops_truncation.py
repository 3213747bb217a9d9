"""TEST INFRASTRUCTURE: the host restatement of truncated sampling (include/xlxmert_hip.h xl_sample_rows_trunc) on top of
tests/fake_ops_sampling.SamplingFakeOps: the same noise helpers, the rules of the header restated one by one.

  y        logits * fp32(inv_T) as ONE fp32 multiply, -0 -> +0 (the kernel's own y: exact in both, so the rank, the candidate set and
           the min-p cut are exact statements), then converted to the compute dtype
  rank     stable descending sort: ties keep the ascending column order
  min-p    y >= mx + fp32(log_min_p), one fp32 add
  top-p    c_r added sequentially in rank order in the compute dtype (an explicit loop: torch.cumsum accumulates float32 in double
           on the CPU), rank r kept iff c_r < top_p Z; rank 0 always
  draw     argmax over the kept ranks of y + g, the lower column on a tie
  outputs  row_prob under the FULL softmax

TruncationFakeOps(dtype, compute, fault=...) selects ONE deliberately wrong rule for the injected-fault tests:
  "ties"    ties in the rank go to the HIGHER column (so ties across the candidate boundary keep the wrong columns)
  "renorm"  top-p mass relative to the candidates' mass instead of Z
  "all"     argmax taken over all columns, kept set ignored
  "prob"    row_prob renormalised over the kept set
"""
import math
from types import SimpleNamespace

import torch

from fake_ops import v2
from fake_ops_sampling import SamplingFakeOps, first_argmax, gumbel_noise

TRUNC_MAX_CAND = 256
FAULTS = ("ties", "renorm", "all", "prob")


def f32(v):
    """the fp32 value of a host scalar, as a python float (what the kernel receives)"""
    return float(torch.tensor(v, dtype=torch.float32))


def tempered_y32(logits, K, inv_T):
    """the kernel's own y [M, K]: one fp32 multiply, -0 canonicalised to +0"""
    y = logits[:, :K].float() * torch.tensor(inv_T, dtype=torch.float32, device=logits.device)
    return torch.where(y == 0, torch.zeros_like(y), y)


def rank_order(y32, higher_column_first=False):
    """columns in rank order [M, K]: (y descending, column ascending); higher_column_first: the "ties" fault"""
    if higher_column_first:
        K = y32.shape[1]
        return K - 1 - torch.sort(y32.flip(1), dim=1, descending=True, stable=True).indices
    return torch.sort(y32, dim=1, descending=True, stable=True).indices


def sequential_prefix(e):
    """c[:, r] = sum_{j<r} e[:, j], added one after the other in e's dtype"""
    c = torch.zeros_like(e)
    acc = torch.zeros_like(e[:, 0])
    for r in range(e.shape[1]):
        c[:, r] = acc
        acc = acc + e[:, r]
    return c


def restate(logits, K, inv_T, seed, top_k, top_p, log_min_p, compute=torch.float32, noise="ok", fault=None, row0=0):
    """every intermediate of one xl_sample_rows_trunc launch on logits [M, >= K]"""
    assert fault is None or fault in FAULTS, fault
    M, dev = logits.shape[0], logits.device
    y32 = tempered_y32(logits, K, inv_T)
    order = rank_order(y32, fault == "ties")
    k_c = min(K, int(top_k))
    cand = order[:, :k_c]                                            # candidate columns in rank order
    y = y32.to(compute)
    yc32 = y32.gather(1, cand)
    yc = yc32.to(compute)
    mx32 = y32.amax(1)
    mx = mx32.to(compute)
    thr32 = mx32 + torch.tensor(log_min_p, dtype=torch.float32, device=dev)          # one fp32 add (-inf: off)
    k_m = (yc32 >= thr32[:, None]).sum(1)
    Z = torch.exp(y - mx[:, None]).sum(1)
    e = torch.exp(yc - mx[:, None])
    rows = torch.arange(M, device=dev) + row0
    if f32(top_p) < 1.0:
        c = sequential_prefix(e)
        total = e.sum(1) if fault == "renorm" else Z
        lim = torch.tensor(top_p, dtype=torch.float32, device=dev).to(compute) * total
        keep = c < lim[:, None]
        keep[:, 0] = True
        k_p = keep.to(torch.int64).cumprod(1).sum(1)                 # the prefix: up to the first rank that fails
    else:
        k_p = torch.full((M,), k_c, dtype=torch.int64, device=dev)
    k_s = torch.minimum(k_m, k_p)
    g = gumbel_noise(seed, rows[:, None], cand, compute, noise)
    z = yc + g
    z = torch.where(torch.arange(k_c, device=dev)[None, :] < k_s[:, None], z, torch.full_like(z, -math.inf))
    best = torch.where(z == z.amax(1, keepdim=True), cand, torch.full_like(cand, 2 ** 31 - 1))
    s = best.min(1).values                                           # the lowest column among equal z
    if fault == "all":
        cols = torch.arange(K, device=dev)
        s = first_argmax(y + gumbel_noise(seed, rows[:, None], cols[None, :], compute, noise))
    lse = mx + torch.log(Z)
    y_s = y.gather(1, s[:, None])[:, 0]
    prob = torch.exp(y_s - lse)
    if fault == "prob":
        kept_mass = torch.where(torch.arange(k_c, device=dev)[None, :] < k_s[:, None], e, torch.zeros_like(e)).sum(1)
        prob = torch.exp(y_s - mx) / kept_mass
    return SimpleNamespace(y32=y32, order=order, k_c=k_c, k_m=k_m, k_p=k_p, k_s=k_s, s=s, lse=lse, prob=prob, Z=Z)


class TruncationFakeOps(SamplingFakeOps):
    def __init__(self, dtype, compute=torch.float32, noise="ok", fault=None):
        super().__init__(dtype, compute, noise)
        self.fault = fault

    def sample_rows_trunc(self, logits, M, K, ldl, inv_T, seed, top_k, top_p, log_min_p, row_prob, row_id, row_lse=None, row_kept=None):
        assert 1 <= top_k <= TRUNC_MAX_CAND and top_p > 0 and log_min_p <= 0 and ldl >= K, (top_k, top_p, log_min_p, ldl, K)
        self.calls.append(("sample_rows_trunc", M, K, top_k, top_p, log_min_p))
        r = restate(v2(logits, M, K, ldl), K, inv_T, seed, top_k, top_p, log_min_p, self.compute, self.noise, self.fault)
        if row_id is not None:
            row_id[:M].copy_(r.s)
        if row_prob is not None:
            row_prob[:M].copy_(r.prob)
        if row_lse is not None:
            row_lse[:M].copy_(r.lse)
        if row_kept is not None:
            row_kept[:M].copy_(r.k_s)
