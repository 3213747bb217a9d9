"""tests/fake_ops.FakeOps plus the entry points of the fp32 residual stream (xl_layernorm_fwd_res / xl_layernorm_bwd_res) and a
record of what the fp32-stream wiring tests ask about: every LayerNorm call, and the residual / output element types of every
XL_EPI_RESIDUAL contraction.  FakeOps.gemm already computes XL_EPI_RESIDUAL_F32 as it stands (the residual is converted with
.to(compute), the result is stored into whatever type C has)."""
import torch

from fake_ops import EPI_RESIDUAL, FakeOps, _rc, keep_scale, v2


class FakeOpsRes(FakeOps):
    NEW_METHODS = ("layernorm_fwd_res", "layernorm_bwd_res")

    def gemm(self, A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr=0, ldx=0, a_kmajor=1, b_kmajor=1, out_f32=False,
             epilogue=0, **kw):
        if epilogue == EPI_RESIDUAL:
            self.calls.append(("gemm_residual", residual.dtype, C.dtype, bool(out_f32), N))
        super().gemm(A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr=ldr, ldx=ldx, a_kmajor=a_kmajor, b_kmajor=b_kmajor,
                     out_f32=out_f32, epilogue=epilogue, **kw)

    def layernorm_fwd(self, x, gamma, beta, y, mean, rstd, M, N, eps):
        self.calls.append(("layernorm_fwd", M, N))
        super().layernorm_fwd(x, gamma, beta, y, mean, rstd, M, N, eps)

    def layernorm_bwd(self, dy, x, *a, **kw):
        self.calls.append(("layernorm_bwd", dy.dtype, x.dtype))
        super().layernorm_bwd(dy, x, *a, **kw)

    def layernorm_fwd_res(self, x, gamma, beta, y32, y16, mean, rstd, M, N, eps):
        """y32 = LN(x); y16 = the rounding of the value STORED in y32"""
        self.calls.append(("layernorm_fwd_res", M, N))
        if self.compute != torch.float64:           # (the float64 reference runs on float64 snapshots)
            assert x.dtype == y32.dtype == torch.float32 and y16.dtype == torch.bfloat16, (x.dtype, y32.dtype, y16.dtype)
        o, m, r = self._ln(v2(x, M, N, N).to(self.compute), gamma.to(self.compute), beta.to(self.compute), eps)
        v2(y32, M, N, N).copy_(o)
        v2(y16, M, N, N).copy_(v2(y32, M, N, N))
        mean[:M].copy_(m)
        rstd[:M].copy_(r)

    def layernorm_bwd_res(self, dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dbias_prev, M, N, ws=None, dx_dropped=None,
                          p_drop=0.0, seed=0):
        """dx_dropped (the gradient entering the dense layer) is written on every call: dx * mask, i.e. dx for p_drop = 0"""
        self.calls.append(("layernorm_bwd_res", M, N))
        if self.compute != torch.float64:
            assert dy.dtype == x.dtype == dx.dtype == torch.float32 and dx_dropped.dtype == torch.bfloat16, (dy.dtype, x.dtype, dx.dtype)
        d, dg, db = self._ln_bwd(v2(dy, M, N, N).to(self.compute), v2(x, M, N, N).to(self.compute), gamma.to(self.compute),
                                 mean[:M].to(self.compute), rstd[:M].to(self.compute))
        v2(dx, M, N, N).copy_(d)
        dgamma.add_(dg)
        dbeta.add_(db)
        if p_drop > 0:
            d = d * keep_scale(self._seed(seed), *_rc(M, N, d.device), p_drop)                # the kernel masks the fp32 value, then rounds
        v2(dx_dropped, M, N, N).copy_(d)
        if dbias_prev is not None:
            dbias_prev.add_(d.sum(0))
