"""TEST INFRASTRUCTURE: the host restatement of the validation scores (include/xlxmert_hip.h XL_EPI_ROWSCORE, xl_rowscore_combine,
xl_score_rows) on top of tests/fake_ops.FakeOps.

EvalFakeOps(dtype, compute) adds the ROWSCORE branch of gemm (`residual` = int64 labels [M]; record {max, sum exp, argmax bits,
x_label or -inf} per row and 64-column segment), rowscore_combine and score_rows; the arithmetic runs in the FakeOps compute dtype
(float64: the reference of tests/bounds_eval.py).  `fault` selects ONE deliberately wrong behaviour for the injected-fault tests:
  "label_neighbour"  the label's logit is taken from the neighbouring 64-column segment (same offset inside the segment)
  "tie_high"         ties go to the HIGHER column (segment argmax, merge of the segments, xl_score_rows)
  "ignored_counted"  a row with an ignored label is counted in totals[1]
  "pad_wins"         the epilogue forgets the bias for the maximum: a pad column (zero row of B, logit 0 without its -1e30) can win
  "correct_ignored"  totals[2] counts the ignored rows too
  "totals_overwrite" totals = this launch's sums instead of totals += them
"""
import torch

from fake_ops import EPI_NONE, FakeOps, v2

EPI_ROWSCORE = 10
FAULTS = ("label_neighbour", "tie_high", "ignored_counted", "pad_wins", "correct_ignored", "totals_overwrite")
NEG_INF = -float("inf")


def first_argmax(z):
    """lowest index of the maximum along the last dimension (the documented tie rule)"""
    return (z == z.amax(-1, keepdim=True)).to(torch.uint8).argmax(-1)


def last_argmax(z):
    n = z.shape[-1]
    return n - 1 - (z.flip(-1) == z.amax(-1, keepdim=True)).to(torch.uint8).argmax(-1)


class EvalFakeOps(FakeOps):
    def __init__(self, dtype, compute=torch.float32, fault=None):
        super().__init__(dtype, compute)
        assert fault is None or fault in FAULTS, fault
        self.fault = fault

    def _argmax(self, z):
        return last_argmax(z) if self.fault == "tie_high" else first_argmax(z)

    def gemm(self, A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr=0, ldx=0, a_kmajor=1, b_kmajor=1,
             out_f32=False, epilogue=EPI_NONE, alpha=1.0, accumulate=0, p_drop=0.0, seed=0, colsum=None, ws=None):
        if epilogue != EPI_ROWSCORE:
            return super().gemm(A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr, ldx, a_kmajor, b_kmajor, out_f32, epilogue,
                                alpha, accumulate, p_drop, seed, colsum, ws)
        self.calls.append(("gemm", M, N, K, a_kmajor, b_kmajor, epilogue))
        assert a_kmajor and b_kmajor and M % 256 == 0 and N % 256 == 0 and aux.dtype == torch.float32 and C is None and p_drop == 0
        assert residual.dtype == torch.int64 and residual.numel() >= M
        acc = alpha * (v2(A, M, K, lda).to(self.compute) @ v2(B, N, K, ldb).to(self.compute).t())
        x = acc if bias is None else acc + torch.as_strided(bias, (N,), (1,)).to(self.compute)[None, :]
        n_seg = N // 64
        xs = x.view(M, n_seg, 64)
        xm = acc.view(M, n_seg, 64) if self.fault == "pad_wins" else xs          # (the fault: maximum / argmax without the bias)
        loc = self._argmax(xm)
        mx = xm.gather(-1, loc[..., None])[..., 0]
        se = torch.exp(xs - mx[..., None]).sum(-1)
        idx = (loc + torch.arange(n_seg, device=x.device)[None, :] * 64).to(torch.int32)
        lab = residual.view(-1)[:M]
        inside = (lab >= 0) & (lab < N)
        seg_of = torch.where(inside, lab // 64, torch.full_like(lab, -1))
        col = lab.clamp(0, N - 1)
        if self.fault == "label_neighbour":
            nb = torch.where(seg_of + 1 < n_seg, seg_of + 1, seg_of - 1)
            col = torch.where(inside, nb * 64 + lab % 64, col)
            seg_of = torch.where(inside, nb, seg_of)
        x_lab = x.gather(1, col[:, None])[:, 0]
        slot = torch.full((M, n_seg), NEG_INF, dtype=self.compute, device=x.device)
        rows = inside.nonzero()[:, 0]
        slot[rows, seg_of[rows]] = x_lab[rows]
        rec = aux.view(-1)[:n_seg * M * 4].view(n_seg, M, 4)
        rec[..., 0].copy_(mx.t())
        rec[..., 1].copy_(se.t())
        rec.view(torch.int32)[..., 2].copy_(idx.t())
        rec[..., 3].copy_(slot.t())

    def _finish(self, lse, x_lab, pred, mx, labels, n_cols, M, row_nll, row_pred, row_max, totals):
        lab = labels.view(-1)[:M] if labels is not None else torch.full((M,), -100, dtype=torch.int64, device=lse.device)
        valid = (lab >= 0) & (lab < n_cols)
        nll = torch.where(valid, lse - x_lab, torch.zeros_like(lse))
        if row_nll is not None:
            row_nll[:M].copy_(nll)
        if row_pred is not None:
            row_pred[:M].copy_(pred)
        if row_max is not None:
            row_max[:M].copy_(mx)
        if totals is None:
            return
        hit = valid & (pred == lab)
        cnt = valid
        if self.fault == "ignored_counted":
            cnt = torch.ones_like(valid)
        if self.fault == "correct_ignored":
            hit = hit | ~valid
        t = torch.stack([nll.sum(), cnt.to(self.compute).sum(), hit.to(self.compute).sum()]).to(totals.dtype)
        if self.fault == "totals_overwrite":
            totals[:3].copy_(t)
        else:
            totals[:3] += t

    def rowscore_combine(self, ws, n_seg, M, labels, n_cols, row_nll=None, row_pred=None, row_max=None, totals=None):
        self.calls.append(("rowscore_combine", n_seg, M, n_cols))
        rec = ws.view(-1)[:n_seg * M * 4].view(n_seg, M, 4)
        mx, se, xl = (rec[..., i].to(self.compute) for i in (0, 1, 3))
        idx = rec.view(torch.int32)[..., 2].long()
        gmx = mx.amax(0)
        tot = (se * torch.exp(mx - gmx[None, :])).sum(0)
        lse = gmx + torch.log(tot)
        if self.fault == "tie_high":
            pred = torch.where(mx == gmx[None, :], idx, torch.full_like(idx, -1)).amax(0)
        else:
            pred = torch.where(mx == gmx[None, :], idx, torch.full_like(idx, 2 ** 31 - 1)).amin(0)
        self._finish(lse, xl.amax(0), pred, gmx, labels, n_cols, M, row_nll, row_pred, row_max, totals)

    def score_rows(self, logits, M, K, ldl, labels, row_nll=None, row_pred=None, row_max=None, totals=None):
        self.calls.append(("score_rows", M, K, ldl))
        x = v2(logits, M, K, ldl).to(self.compute)
        lse = torch.logsumexp(x, 1)
        pred = self._argmax(x)
        lab = labels.view(-1)[:M] if labels is not None else torch.full((M,), -100, dtype=torch.int64, device=x.device)
        x_lab = x.gather(1, lab.clamp(0, K - 1)[:, None])[:, 0]
        self._finish(lse, x_lab, pred, x.amax(1), labels, K, M, row_nll, row_pred, row_max, totals)
