"""The per-element bounds of tests/bounds.py, on the host: an honest bf16 result (the float64 value rounded to nearest even, or an
fp32-accumulated computation rounded once) passes, and each plausible kernel fault below, applied to the honest result, is
rejected.  Shapes: the benchmarked step's (d = 768, dff 3072, 12 heads of 64, 64 visual / <= 20 packed language tokens), fewer rows."""
import math

import pytest
import torch

import bounds as BD
from fake_ops import EPI_DGELU, EPI_GELU, EPI_GELU_DG, EPI_NONE, EPI_RESIDUAL, EPI_TANH, FakeOps, gelu_grad, keep_scale

R64 = FakeOps(torch.bfloat16, compute=torch.float64)
R32 = FakeOps(torch.bfloat16)
D, DFF, H, DH = 768, 3072, 12, 64


def bf(x):
    return x.to(torch.bfloat16)


def rtz(x):
    """round toward zero to bf16 (drop the low 16 bits of the fp32 pattern)"""
    i = x.float().contiguous().view(torch.int32) & -65536
    return i.view(torch.float32).to(torch.bfloat16)


def must_reject(got, ref, bound, what):
    try:
        r = BD.check(got, ref, bound, what)
    except AssertionError:
        return
    pytest.fail(f"{what}: the bound is too loose -- the faulty result passes (worst |err|/bound {r:.3g})")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ GEMM
def gemm_case(epi, M=512, N=D, K=D, p_drop=0.0, seed=3):
    g = _gen(seed)
    A = bf(torch.randn(M, K, generator=g))
    W = bf(torch.randn(N, K, generator=g) / math.sqrt(K))
    bias = torch.randn(N, generator=g) * 0.1
    res = bf(torch.randn(M, N, generator=g))
    aux = bf(torch.randn(M, N, generator=g) * 2)
    return dict(A=A, W=W, bias=bias, res=res, aux=aux, M=M, N=N, K=K, epi=epi, p_drop=p_drop, seed=seed)


def gemm_run(ops, c, dtype, W=None, bias="keep"):
    M, N, K = c["M"], c["N"], c["K"]
    C = torch.zeros(M, N, dtype=dtype)
    aux = c["aux"].to(dtype).clone()
    b = c["bias"] if bias == "keep" else bias
    ops.gemm(c["A"], c["W"] if W is None else W, C, b, c["res"], aux, M, N, K, K, K, N, ldr=N, ldx=N, epilogue=c["epi"],
             p_drop=c["p_drop"], seed=c["seed"])
    return C, aux


def gemm_ref_and_bounds(c):
    C, aux = gemm_run(R64, c, torch.float64)
    A, W = c["A"].double(), c["W"].double()
    pre = A @ W.t() + c["bias"].double()
    absprod = A.abs() @ W.abs().t() + c["bias"].double().abs()
    keep = None
    if c["epi"] == EPI_RESIDUAL and c["p_drop"] > 0:
        keep = keep_scale(c["seed"], torch.arange(c["M"])[:, None], torch.arange(c["N"])[None, :], c["p_drop"]).double()
    bc, ba = BD.gemm_bounds(pre, absprod, c["K"], c["epi"], torch.bfloat16, C, aux_in=c["aux"].double(), ref_aux=aux, keep=keep)
    return C, aux, bc, ba


EPIS = [(EPI_NONE, 0.0), (EPI_GELU, 0.0), (EPI_RESIDUAL, 0.1), (EPI_DGELU, 0.0), (EPI_GELU_DG, 0.0), (EPI_TANH, 0.0)]


@pytest.mark.parametrize("epi,p_drop", EPIS, ids=["none", "gelu", "residual_dropout", "dgelu", "gelu_dg", "tanh"])
@pytest.mark.parametrize("honest", ["f64_rounded", "f32_accumulated"])
def test_gemm_honest_results_pass(epi, p_drop, honest):
    c = gemm_case(epi, p_drop=p_drop)
    C, aux, bc, ba = gemm_ref_and_bounds(c)
    ops = R64 if honest == "f64_rounded" else R32
    Cg, auxg = gemm_run(ops, c, torch.float64 if honest == "f64_rounded" else torch.float32)
    BD.check(bf(Cg), C, bc, f"gemm epi {epi} C")
    if ba is not None:
        BD.check(bf(auxg), aux, ba, f"gemm epi {epi} aux")
    cs = BD.colsum_bound(bc, C)
    BD.check(bf(Cg).double().sum(0).float(), C.sum(0), cs, "column sums")


# ------------------------------------------------------------------------------------------------------------------ attention
def attn_case(packed, p_drop, seed=5, B=6):
    g = _gen(seed)
    if packed:
        lens = torch.tensor([20, 6, 13, 1, 20, 9][:B])
        off = torch.zeros(B + 1, dtype=torch.int32)
        off[1:] = torch.cumsum(lens, 0)
        n, rows = 20, int(off[-1])
        key_mask = None
    else:
        off, n, rows = None, 64, B * 64
        key_mask = (torch.rand(B, n, generator=g) > 0.2).to(torch.uint8)
        key_mask[:, 0] = 1
    q, k, v, do = (bf(torch.randn(rows, H * DH, generator=g)) for _ in range(4))
    return dict(q=q, k=k, v=v, do=do, B=B, n=n, rows=rows, off=off, key_mask=key_mask, p_drop=p_drop, seed=seed)


def attn_fwd(ops, c, dtype):
    B, n, rows = c["B"], c["n"], c["rows"]
    o = torch.zeros(rows, H * DH, dtype=dtype)
    lse = torch.zeros(B * H * n, dtype=torch.float64 if dtype == torch.float64 else torch.float32)
    ops.sdpa_fwd(c["q"], c["k"], c["v"], c["key_mask"], o, lse, B, H, n, n, DH, H * DH, H * DH, H * DH, H * DH, 0.125,
                 p_drop=c["p_drop"], seed=c["seed"], q_off=c["off"], k_off=c["off"])
    return o, lse


def attn_fwd_bounds(c, o, lse):
    B, n, off = c["B"], c["n"], c["off"]
    Q, K, V, valid, keep = BD.attention_inputs(R64, c["q"], c["k"], c["v"], c["key_mask"], B, H, n, n, DH, H * DH, H * DH, H * DH,
                                               c["p_drop"], c["seed"], off, off)
    O, _ = R64._load(o, B, n, H, DH, H * DH, off)
    bO, bl = BD.sdpa_fwd_bounds(Q, K, V, valid, keep, 0.125, O, lse.view(B, H, n))
    return BD.attention_scatter(R64, bO, B, n, H, DH, H * DH, off, 0)[:c["rows"]], bl.reshape(-1), (Q, K, V, valid, keep)


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("honest", ["f64_rounded", "f32_accumulated"])
def test_attention_honest_results_pass(packed, honest):
    c = attn_case(packed, 0.1)
    o, lse = attn_fwd(R64, c, torch.float64)
    bo, bl, (Q, K, V, valid, keep) = attn_fwd_bounds(c, o, lse)
    ops = R64 if honest == "f64_rounded" else R32
    og, lg = attn_fwd(ops, c, torch.float64 if honest == "f64_rounded" else torch.float32)
    BD.check(bf(og), o, bo, "sdpa_fwd O")
    exist = valid.any(-1).expand(c["B"], H, c["n"]).reshape(-1)
    BD.check(lg.float()[exist], lse[exist], bl[exist], "sdpa_fwd lse")
    # backward from the reference lse
    B, n, off = c["B"], c["n"], c["off"]
    outs = {}
    for name, ops_, dt in (("ref", R64, torch.float64), ("got", ops, torch.float64 if honest == "f64_rounded" else torch.float32)):
        dq, dk, dv = (torch.zeros(c["rows"], H * DH, dtype=dt) for _ in range(3))
        ops_.sdpa_bwd(c["q"], c["k"], c["v"], c["key_mask"], c["do"], lse.to(torch.float32 if dt == torch.float32 else dt),
                      dq, dk, dv, B, H, n, n, DH, *([H * DH] * 7), 0.125, p_drop=c["p_drop"], seed=c["seed"], q_off=off, k_off=off)
        outs[name] = (dq, dk, dv)
    dO, _ = R64._load(c["do"], B, n, H, DH, H * DH, off)
    dense = [R64._load(t, B, n, H, DH, H * DH, off)[0] for t in outs["ref"]]
    bounds, _ = BD.sdpa_bwd_bounds(Q, K, V, dO, valid, keep, 0.125, lse.view(B, H, n), *dense)
    for nm, got, ref, b in zip("QKV", outs["got"], outs["ref"], bounds):
        BD.check(bf(got), ref, BD.attention_scatter(R64, b, B, n, H, DH, H * DH, off, 0)[:c["rows"]], f"sdpa_bwd d{nm}")


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def ln_case(M=256, seed=7, shift=0.0):
    g = _gen(seed)
    x = bf(torch.randn(M, D, generator=g) + shift)
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    dy = bf(torch.randn(M, D, generator=g))
    return x, gamma, beta, dy


def ln_ref(x, gamma, beta, dy):
    M = x.shape[0]
    y, mean, rstd = torch.zeros(M, D, dtype=torch.float64), torch.zeros(M, dtype=torch.float64), torch.zeros(M, dtype=torch.float64)
    R64.layernorm_fwd(x, gamma, beta, y, mean, rstd, M, D, 1e-12)
    mean32, rstd32 = mean.float(), rstd.float()            # what the forward kernel hands the backward
    dx, dg, db = torch.zeros(M, D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
    R64.layernorm_bwd(dy, x, gamma, mean32, rstd32, dx, dg, db, None, M, D)
    return y, mean, rstd, mean32, rstd32, dx, dg, db


@pytest.mark.parametrize("shift", [0.0, 100.0], ids=["centred", "mean_100x_std"])
def test_layernorm_honest_results_pass(shift):
    x, gamma, beta, dy = ln_case(shift=shift)
    M = x.shape[0]
    y, mean, rstd, mean32, rstd32, dx, dg, db = ln_ref(x, gamma, beta, dy)
    by, bm, br = BD.ln_fwd_bounds(x.double(), gamma.double(), y, mean, rstd, torch.bfloat16)
    y32, m32, r32 = torch.zeros(M, D), torch.zeros(M), torch.zeros(M)
    R32.layernorm_fwd(x, gamma, beta, y32, m32, r32, M, D, 1e-12)
    BD.check(bf(y32), y, by, "layernorm_fwd y")
    BD.check(m32, mean, bm, "layernorm_fwd mean")
    BD.check(r32, rstd, br, "layernorm_fwd rstd")
    bdx, _, bdg, bdb = BD.ln_bwd_bounds(dy.double(), x.double(), gamma.double(), mean32.double(), rstd32.double(), dx, torch.bfloat16)
    dx32, dg32, db32 = torch.zeros(M, D), torch.zeros(D), torch.zeros(D)
    R32.layernorm_bwd(dy, x, gamma, mean32, rstd32, dx32, dg32, db32, None, M, D)
    BD.check(bf(dx32), dx, bdx, "layernorm_bwd dx")
    BD.check(dg32, dg, bdg, "layernorm_bwd dgamma")
    BD.check(db32, db, bdb, "layernorm_bwd dbeta")


def test_layernorm_one_pass_statistics_are_rejected_at_mean_100x_std():
    """E[x^2] - E[x]^2 in fp32 on rows whose mean is 100x their standard deviation: what the two-pass statistics avoid"""
    x, gamma, beta, _ = ln_case(shift=100.0)
    y, mean, rstd, *_ = ln_ref(x, gamma, beta, torch.zeros_like(x))
    xf = x.float()
    m = xf.mean(1)
    var = ((xf * xf).mean(1) - m * m).clamp(min=0)
    r1 = 1 / torch.sqrt(var + 1e-12)
    _, _, br = BD.ln_fwd_bounds(x.double(), gamma.double(), y, mean, rstd, torch.bfloat16)
    must_reject(r1, rstd, br, "layernorm rstd from one-pass statistics")


# ------------------------------------------------------------------------------------------------------------------ CE / AdamW
def test_cross_entropy_honest_result_passes():
    g = _gen(9)
    M, K = 64, 10000
    logits = bf(torch.randn(M, K, generator=g) * 20).clamp(-80, 80)
    labels = torch.randint(0, K, (M,), generator=g)
    labels[::5] = -100
    counts = torch.tensor([float((labels != -100).sum())])
    out = {}
    for nm, ops, dt in (("ref", R64, torch.float64), ("got", R32, torch.float32)):
        dl, loss, lse = torch.zeros(M, K, dtype=dt), torch.zeros(1, dtype=dt), torch.zeros(M, dtype=dt)
        ops.ce_fwd_bwd(logits.to(dt), labels, counts, dl, loss, lse, None, None, M, K, K, K)
        out[nm] = (dl, loss, lse)
    dl, loss, lse = out["ref"]
    valid = (labels != -100).double()
    blse, bdl = BD.ce_bounds(logits.double(), valid, 1.0 / counts.item(), lse, dl, torch.bfloat16)
    BD.check(out["got"][2], lse, blse, "ce lse")
    BD.check(bf(out["got"][0]), dl, bdl, "ce dlogits")
    BD.check(out["got"][1], loss, BD.ce_loss_bound(logits.double(), labels, valid, counts.item(), blse, loss.item()), "ce loss")


def adamw_case(n=4096, t=3, seed=11):
    g = _gen(seed)
    p = torch.randn(n, generator=g) * 0.02
    gr = torch.randn(n, generator=g) * 1e-3
    m = torch.randn(n, generator=g) * 1e-3
    v = torch.rand(n, generator=g) * 1e-6
    return p, gr, m, v, t


def adamw_run(ops, dt, p, gr, m, v, t, lr=1e-4, t_used=None):
    tt = t if t_used is None else t_used
    lrs = torch.tensor([lr, 1 - 0.9 ** tt, 1 - 0.999 ** tt, float(tt)], dtype=torch.float32)
    P, G, Mm, Vv = (x.to(dt).clone() for x in (p, gr, m, v))
    sumsq = torch.tensor([float((gr.double() ** 2).sum())], dtype=torch.float32)
    ops.adamw(P, G, Mm, Vv, None, None, sumsq, lrs, p.numel(), 0.9, 0.999, 1e-6, 0.01, 1.0)
    return P, Mm, Vv


def adamw_bounds(p, gr, m, v, t, P, Mm, Vv, lr=1e-4):
    step = lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
    return BD.adamw_bounds(P, Mm, Vv, gr.double(), m.double(), v.double(), step, 1.0, 0.9, 0.999, 1e-6, lr, 0.0)


def test_adamw_honest_result_passes():
    p, gr, m, v, t = adamw_case()
    P, Mm, Vv = adamw_run(R64, torch.float64, p, gr, m, v, t)
    bp, bm, bv = adamw_bounds(p, gr, m, v, t, P, Mm, Vv)
    P32, M32, V32 = adamw_run(R32, torch.float32, p, gr, m, v, t)
    BD.check(P32, P, bp, "adamw p")
    BD.check(M32, Mm, bm, "adamw m")
    BD.check(V32, Vv, bv, "adamw v")


# ------------------------------------------------------------------------------------------------------------------ faults
def _extra_key_row(c, o, b, h, qi, extra_key_row):
    """o with query row (b, h, qi) recomputed as if key row `extra_key_row` of k / v also attended (float64, rounded)"""
    B, n, off = c["B"], c["n"], c["off"]
    Q, K, V, valid, keep = BD.attention_inputs(R64, c["q"], c["k"], c["v"], c["key_mask"], B, H, n, n, DH, *([H * DH] * 3),
                                               0.0, 0, off, off)
    q = Q[b, h, qi]
    ks = torch.cat([K[b, h][valid[b, 0, qi]], c["k"][extra_key_row, h * DH:(h + 1) * DH].double()[None]])
    vs = torch.cat([V[b, h][valid[b, 0, qi]], c["v"][extra_key_row, h * DH:(h + 1) * DH].double()[None]])
    row = torch.softmax(ks @ q * 0.125, 0) @ vs
    r = b * n + qi if off is None else int(off[b]) + qi
    o = o.clone()
    o[r, h * DH:(h + 1) * DH] = row
    return o


FAULTS = ["round_toward_zero", "k_block_missing_in_one_tile", "bias_missing_in_one_column", "dropout_mask_shifted_one_column",
          "masked_key_left_in_one_row", "packed_row_sees_next_example_key", "gelu_derivative_saved_from_output",
          "adamw_bias_correction_one_step_off", "ln_bwd_c2_missing_on_one_row"]


@pytest.mark.parametrize("fault", FAULTS)
def test_bounds_reject_plausible_kernel_faults(fault):
    if fault in ("round_toward_zero", "k_block_missing_in_one_tile", "bias_missing_in_one_column"):
        c = gemm_case(EPI_NONE, M=512)
        C, _, bc, _ = gemm_ref_and_bounds(c)
        C32, _ = gemm_run(R32, c, torch.float32)
        if fault == "round_toward_zero":
            must_reject(rtz(C32), C, bc, fault)
        elif fault == "k_block_missing_in_one_tile":
            bad = C32.clone()
            bad[:256, :256] -= c["A"][:256, 64:128].float() @ c["W"][:256, 64:128].float().t()
            must_reject(bf(bad), C, bc, fault)
        else:
            bad = C32.clone()
            bad[:, 77] -= c["bias"][77]
            must_reject(bf(bad), C, bc, fault)
    elif fault == "dropout_mask_shifted_one_column":
        c = gemm_case(EPI_RESIDUAL, p_drop=0.1)
        C, _, bc, _ = gemm_ref_and_bounds(c)
        A, W = c["A"].float(), c["W"].float()
        keep = keep_scale(c["seed"], torch.arange(c["M"])[:, None], torch.arange(c["N"])[None, :], 0.1)
        keep = torch.roll(keep, 1, 1)
        must_reject(bf((A @ W.t() + c["bias"]) * keep + c["res"].float()), C, bc, fault)
    elif fault == "gelu_derivative_saved_from_output":
        c = gemm_case(EPI_GELU_DG)
        C, aux, bc, ba = gemm_ref_and_bounds(c)
        pre = c["A"].float() @ c["W"].float().t() + c["bias"]
        must_reject(bf(gelu_grad(torch.nn.functional.gelu(pre))), aux, ba, fault)
    elif fault in ("masked_key_left_in_one_row", "packed_row_sees_next_example_key"):
        packed = fault == "packed_row_sees_next_example_key"
        c = attn_case(packed, 0.0)
        o, lse = attn_fwd(R64, c, torch.float64)
        bo, _, _ = attn_fwd_bounds(c, o, lse)
        o32, _ = attn_fwd(R32, c, torch.float32)
        if packed:                                    # example 2's last query also attends to example 3's (only) key
            bad = _extra_key_row(c, o32.double(), 2, 4, 12, int(c["off"][3]))
        else:                                         # one masked key of example 1 left in query 5's row
            masked = (c["key_mask"][1] == 0).nonzero()[0, 0].item()
            bad = _extra_key_row(c, o32.double(), 1, 4, 5, 1 * c["n"] + masked)
        must_reject(bf(bad), o, bo, fault)
    elif fault == "adamw_bias_correction_one_step_off":
        p, gr, m, v, t = adamw_case()
        P, Mm, Vv = adamw_run(R64, torch.float64, p, gr, m, v, t)
        bp, _, _ = adamw_bounds(p, gr, m, v, t, P, Mm, Vv)
        P32, _, _ = adamw_run(R32, torch.float32, p, gr, m, v, t, t_used=t + 1)
        must_reject(P32, P, bp, fault)
    elif fault == "ln_bwd_c2_missing_on_one_row":
        x, gamma, beta, dy = ln_case()
        M = x.shape[0]
        y, mean, rstd, mean32, rstd32, dx, dg, db = ln_ref(x, gamma, beta, dy)
        bdx, _, _, _ = BD.ln_bwd_bounds(dy.double(), x.double(), gamma.double(), mean32.double(), rstd32.double(), dx, torch.bfloat16)
        dx32, dg32, db32 = torch.zeros(M, D), torch.zeros(D), torch.zeros(D)
        R32.layernorm_bwd(dy, x, gamma, mean32, rstd32, dx32, dg32, db32, None, M, D)
        xh = (x[17].float() - mean32[17]) * rstd32[17]
        c2 = (gamma * dy[17].float() * xh).mean()
        dx32[17] += rstd32[17] * xh * c2               # the row's "- xh c2" term left out
        must_reject(bf(dx32), dx, bdx, fault)
    else:
        raise AssertionError(fault)
