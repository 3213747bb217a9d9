"""TEST INFRASTRUCTURE: the host restatement of temperature sampling (include/xlxmert_hip.h XL_EPI_ROWSAMPLE, xl_rowsample_combine,
xl_sample_rows, xl_gumbel_from_bits) on top of tests/fake_ops.FakeOps.

The noise function of csrc/common.h in two parts:
  integers  gumbel_bits(seed, m, n): the 32-bit hash, restated bit for bit (torch int64 arithmetic masked to 32 bits)
  floats    gumbel_from_bits(h, dtype): w = (2 (k ^ 0x7FFFFF) + 1) 2^-24 = 1 - u with k = h >> 9, t = -log1p(-w), g = -log t, evaluated
            in `dtype`: float32 restates the kernel's arithmetic, float64 is the reference of tests/bounds_sampling.py (w is exact
            in both).
SamplingFakeOps(dtype, compute) adds the ROWSAMPLE branch of gemm, rowsample_combine and sample_rows; the float part runs in the
FakeOps compute dtype.  `noise` selects a deliberately WRONG noise function for the injected-fault tests:
  "row"    the row is ignored (every row of a launch draws the same noise)
  "seed"   the launch seed is ignored (every step / every user seed draws the same noise)
  "u16"    the 16-bit uniform of the dropout hash (csrc/common.h dropout_draw16: one hash per column PAIR, at most 65 536 distinct
           values, the largest about 11.8)
"""
import torch

from fake_ops import EPI_NONE, FakeOps, v2

EPI_ROWSAMPLE = 9
M32 = 0xFFFFFFFF
LAUNCH_MUL = 0x9E3779B97F4A7C15


def launch_seed(seed, step):
    """Engine.sample_launch_seed restated: seed * 0x9E3779B97F4A7C15 + step (mod 2^64)"""
    return (int(seed) * LAUNCH_MUL + int(step)) & 0xFFFFFFFFFFFFFFFF


def seed_mix(seed):
    return (seed & M32) ^ ((((seed >> 32) & M32) * 0xC2B2AE3D) & M32)


def gumbel_bits(seed, m, n):
    """the hash word of element (row m, column n) under the launch seed: int64 tensor holding the uint32 value"""
    m, n = torch.broadcast_tensors(torch.as_tensor(m), torch.as_tensor(n))
    r, c = m.to(torch.int64) & M32, n.to(torch.int64) & M32
    h = ((r * 0x9E3779B1) & M32) ^ ((c * 0x85EBCA77) & M32) ^ seed_mix(int(seed))
    h = h ^ (h >> 16); h = (h * 0x7FEB352D) & M32
    h = h ^ (h >> 15); h = (h * 0x846CA68B) & M32
    return h ^ (h >> 16)


def uniform_from_bits(h, dtype=torch.float64):
    """u = (2 k + 1) 2^-24, k = h >> 9 (exact in float32 and float64)"""
    return (2 * (h >> 9) + 1).to(dtype) * 2.0 ** -24


def gumbel_from_bits(h, dtype=torch.float64):
    k = h >> 9
    w = (2 * (k ^ 0x7FFFFF) + 1).to(dtype) * 2.0 ** -24
    return -torch.log(-torch.log1p(-w))


def gumbel_noise(seed, m, n, dtype=torch.float64, noise="ok"):
    """g(seed, m, n) in `dtype`; noise != "ok": the injected faults of the module docstring"""
    if noise == "row":
        m = torch.zeros_like(torch.as_tensor(m))
    if noise == "seed":
        seed = 0
    if noise == "u16":
        m, n = torch.broadcast_tensors(torch.as_tensor(m), torch.as_tensor(n))
        r, c = m.to(torch.int64) & M32, n.to(torch.int64) & M32
        h = ((r * 0x9E3779B1) & M32) ^ (((c >> 1) * 0x85EBCA77) & M32) ^ seed_mix(int(seed))
        h = h ^ (h >> 16); h = (h * 0x7FEB352D) & M32
        h = h ^ (h >> 15); h = (h * 0x846CA68B) & M32
        h = h ^ (h >> 16)
        draw = torch.where((c & 1) != 0, h >> 16, h & 0xFFFF)
        u = (2 * draw + 1).to(dtype) * 2.0 ** -17
        return -torch.log(-torch.log(u))
    return gumbel_from_bits(gumbel_bits(seed, m, n), dtype)


def first_argmax(z):
    """lowest index of the maximum along the last dimension (the documented tie rule)"""
    return (z == z.amax(-1, keepdim=True)).to(torch.uint8).argmax(-1)


class SamplingFakeOps(FakeOps):
    def __init__(self, dtype, compute=torch.float32, noise="ok"):
        super().__init__(dtype, compute)
        self.noise = noise

    def _g(self, seed, M, cols, device):
        return gumbel_noise(seed, torch.arange(M, device=device)[:, None], cols[None, :], self.compute, self.noise)

    def gemm(self, A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr=0, ldx=0, a_kmajor=1, b_kmajor=1,
             out_f32=False, epilogue=EPI_NONE, alpha=1.0, accumulate=0, p_drop=0.0, seed=0, colsum=None, ws=None):
        if epilogue != EPI_ROWSAMPLE:
            return super().gemm(A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr, ldx, a_kmajor, b_kmajor, out_f32, epilogue,
                                alpha, accumulate, p_drop, seed, colsum, ws)
        # no C: per row and 64-column segment {max y, sum exp(y - max), s = argmax (y + g) bits, y_s} -> aux (fp32 records)
        self.calls.append(("gemm", M, N, K, a_kmajor, b_kmajor, epilogue))
        assert a_kmajor and b_kmajor and N % 64 == 0 and aux.dtype == torch.float32
        y = alpha * (v2(A, M, K, lda).to(self.compute) @ v2(B, N, K, ldb).to(self.compute).t())
        if bias is not None:
            y = y + torch.as_strided(bias, (N,), (1,)).to(self.compute)[None, :]
        z = y + self._g(seed, M, torch.arange(N, device=y.device), y.device)
        n_seg = N // 64
        ys, zs = y.view(M, n_seg, 64), z.view(M, n_seg, 64)
        mx = ys.amax(-1)
        se = torch.exp(ys - mx[..., None]).sum(-1)
        loc = first_argmax(zs)
        y_s = ys.gather(-1, loc[..., None])[..., 0]
        idx = (loc + torch.arange(n_seg, device=y.device)[None, :] * 64).to(torch.int32)
        rec = aux.view(-1)[:n_seg * M * 4].view(n_seg, M, 4)
        rec[..., 0].copy_(mx.t())
        rec[..., 1].copy_(se.t())
        rec.view(torch.int32)[..., 2].copy_(idx.t())
        rec[..., 3].copy_(y_s.t())

    def rowsample_combine(self, ws, n_seg, M, seed, row_prob, row_id, row_lse=None):
        rec = ws.view(-1)[:n_seg * M * 4].view(n_seg, M, 4)
        mx, se, ys = (rec[..., i].to(self.compute) for i in (0, 1, 3))
        idx = rec.view(torch.int32)[..., 2].long()
        gmx = mx.amax(0)
        tot = (se * torch.exp(mx - gmx[None, :])).sum(0)
        lse = gmx + torch.log(tot)
        z = ys + gumbel_noise(seed, torch.arange(M, device=ws.device)[None, :], idx, self.compute, self.noise)
        cand = torch.where(z == z.amax(0, keepdim=True), idx, torch.full_like(idx, 2 ** 31 - 1))
        s = cand.min(0).values                                   # the lowest column among equal z
        y_s = torch.where(idx == s[None, :], ys, torch.full_like(ys, -float("inf"))).amax(0)
        if row_id is not None:
            row_id[:M].copy_(s)
        if row_prob is not None:
            row_prob[:M].copy_(torch.exp(y_s - lse))
        if row_lse is not None:
            row_lse[:M].copy_(lse)

    def sample_rows(self, logits, M, K, ldl, inv_T, seed, row_prob, row_id, row_lse=None):
        inv = float(torch.tensor(inv_T, dtype=torch.float32))    # the kernel receives the fp32 value
        y = v2(logits, M, K, ldl).to(self.compute) * inv
        z = y + self._g(seed, M, torch.arange(K, device=y.device), y.device)
        s = first_argmax(z)
        lse = torch.logsumexp(y, 1)
        if row_id is not None:
            row_id[:M].copy_(s)
        if row_prob is not None:
            row_prob[:M].copy_(torch.exp(y.gather(1, s[:, None])[:, 0] - lse))
        if row_lse is not None:
            row_lse[:M].copy_(lse)

    def gumbel_from_bits(self, h, g, n):
        g[:n].copy_(gumbel_from_bits(h[:n].to(torch.int64) & M32, self.compute))
