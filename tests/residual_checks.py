"""The recording proxy of tests/test_kernel_bounds_gpu.py extended by checkers for the entry points of the fp32 residual stream
(xl_layernorm_fwd_res / xl_layernorm_bwd_res).  xl_gemm's XL_EPI_RESIDUAL_F32 needs none of its own: HipOps.gemm keeps its
signature, the float64 restatement converts the residual with .to(compute) and bounds.gemm_bounds(..., EPI_RESIDUAL, out_dtype
fp32) already assumes an exactly represented residual and one fp32 add.  Bounds: bounds.ln_fwd_bounds / ln_bwd_bounds with
out_dtype fp32 for the fp32 outputs; the bf16 outputs are checked EXACTLY against the rounding of the fp32 value the kernel stored
where the contract says so (y16 = bf16(y32); dx_dropped = bf16(dx) without dropout) and within one bf16 rounding of the float64
value otherwise; the kept / dropped pattern of dx_dropped is compared with the restated hash exactly."""
import torch

import bounds as BD
import test_kernel_bounds_gpu as KB
from fake_ops import keep_scale
from fake_ops_res import FakeOpsRes

KB.REDUCE_OUTS.setdefault("layernorm_bwd_res", ("dgamma", "dbeta", "dbias_prev"))
# the views the two entry points may write (the recorder holds the rest of every output's storage bit-identical: "outside view")
KB.ROW_OUTS.setdefault("layernorm_fwd_res", lambda a: [KB._t(a["y32"], a["M"], a["N"]), KB._t(a["y16"], a["M"], a["N"]),
                                                       KB._t(a["mean"], a["M"]), KB._t(a["rstd"], a["M"])])
KB.ROW_OUTS.setdefault("layernorm_bwd_res", lambda a: [KB._t(a["dx"], a["M"], a["N"]), KB._t(a["dx_dropped"], a["M"], a["N"]),
                                                       KB._t(a["dgamma"], a["N"]), KB._t(a["dbeta"], a["N"]),
                                                       KB._t(a["dbias_prev"], a["N"]), KB._whole(a["ws"])])
_v2 = KB._v2


def bits(t):
    """bit patterns of a bf16 tensor"""
    return t.contiguous().view(torch.int16)


class RecorderRes(KB.Recorder):
    def __init__(self, ops):
        super().__init__(ops)
        object.__setattr__(self, "_ref", FakeOpsRes(ops.dtype, compute=torch.float64))

    def chk_layernorm_fwd_res(self, a, s, run):
        M, N = a["M"], a["N"]
        run()
        self._ref.layernorm_fwd_res(**s)
        x, y = _v2(s["x"], M, N, N).clone(), _v2(s["y32"], M, N, N)
        by, bm, br = BD.ln_fwd_bounds(x, s["gamma"].double(), y, s["mean"][:M], s["rstd"][:M], torch.float32)
        kern = self._kern
        got32, got16 = _v2(a["y32"], M, N, N), _v2(a["y16"], M, N, N)
        assert a["y32"].dtype == torch.float32 and a["y16"].dtype == torch.bfloat16
        return [("y32", BD.check(got32, y, by, "layernorm_fwd_res y32"), kern),
                ("y16 == bf16(y32)", BD.check_exact(bits(got16), bits(got32.to(torch.bfloat16)), "layernorm_fwd_res y16"), kern),
                ("mean", BD.check(a["mean"][:M], s["mean"][:M], bm, "layernorm_fwd_res mean"), kern),
                ("rstd", BD.check(a["rstd"][:M], s["rstd"][:M], br, "layernorm_fwd_res rstd"), kern)]

    def chk_layernorm_bwd_res(self, a, s, run):
        M, N = a["M"], a["N"]
        assert a["dy"].dtype == a["x"].dtype == a["dx"].dtype == torch.float32 and a["dx_dropped"].dtype == torch.bfloat16
        dy, x = _v2(s["dy"], M, N, N).clone(), _v2(s["x"], M, N, N).clone()
        mean, rstd = s["mean"][:M].clone(), s["rstd"][:M].clone()
        prev = {k: s[k].clone() for k in ("dgamma", "dbeta", "dbias_prev") if s[k] is not None}
        keep = torch.ones(M, N, dtype=torch.float64, device=dy.device)
        if a["p_drop"] > 0:
            keep = keep_scale(self._ref._seed(a["seed"]), torch.arange(M, device=dy.device)[:, None],
                              torch.arange(N, device=dy.device)[None, :], a["p_drop"]).double()
        run()
        self._ref.layernorm_bwd_res(**s)
        dx = _v2(s["dx"], M, N, N)
        bdx, t, bdg, bdb = BD.ln_bwd_bounds(dy, x, s["gamma"].double(), mean, rstd, dx, torch.float32)
        kern = self._kern
        got_dx, got_dd = _v2(a["dx"], M, N, N), _v2(a["dx_dropped"], M, N, N)
        res = [("dx", BD.check(got_dx, dx, bdx, "layernorm_bwd_res dx"), kern)]
        self._sum_out(res, "dgamma", a["dgamma"], s["dgamma"], prev["dgamma"], bdg + BD.U32 * (s["dgamma"].abs() + prev["dgamma"].abs()), kern)
        self._sum_out(res, "dbeta", a["dbeta"], s["dbeta"], prev["dbeta"], bdb + BD.U32 * (s["dbeta"].abs() + prev["dbeta"].abs()), kern)
        dd = _v2(s["dx_dropped"], M, N, N)
        bdd = BD.U16 * dd.abs() + BD.SLACK * keep * t + BD.TINY
        res.append(("dx_dropped", BD.check(got_dd, dd, bdd, "layernorm_bwd_res dx_dropped"), kern))
        if a["p_drop"] > 0:             # the dropped positions are exactly those of the restated hash (dx itself is never exactly 0 here)
            res.append(("dx_dropped zeros", BD.check_exact((got_dd == 0) | (got_dx == 0), (keep == 0) | (got_dx == 0),
                                                           "layernorm_bwd_res dropped positions"), kern))
        else:                           # the rounding of the very fp32 value that was stored
            res.append(("dx_dropped == bf16(dx)", BD.check_exact(bits(got_dd), bits(got_dx.to(torch.bfloat16)),
                                                                  "layernorm_bwd_res dx_dropped bits"), kern))
        if a["dbias_prev"] is not None:
            ref = s["dbias_prev"]
            # (the sum takes the fp32 value before the bf16 store of dx_dropped: bounds.ln_bwd_bias_bound)
            bb = BD.ln_bwd_bias_bound(keep * t + BD.U32 * dd.abs(), dd, prev["dbias_prev"], ref)
            self._sum_out(res, "dbias_prev", a["dbias_prev"], ref, prev["dbias_prev"], bb, kern)
        return res
