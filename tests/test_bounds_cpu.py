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


# ------------------------------------------------------------------------------------------------------------------ sampler head
# The fused sampler head (XL_EPI_ROWMAX records + xl_rowmax_combine), BCE, attn_probs and the sampler's index kernels: an fp32
# emulation of each kernel's arithmetic passes; every fault of SAMPLER_FAULTS, built into that emulation, is rejected.
N_REAL, N_PAD, K_HEAD = 300, 512, 256


def rowmax_case(seed=13, M=64):
    """300 real codes padded to 512 (segment 4: 44 real + 20 padded columns, segments 5..7 all padded: zero operand rows, bias
    -1e30).  Row 0 of A is all zero: its logits are the biases, exactly, and bias 10 == bias 12 == bias 200 is the largest -- an
    exact tie inside segment 0 and between segments 0 and 3.  Row 1's maximum is forced into the last real column."""
    g = _gen(seed)
    A = bf(torch.randn(M, K_HEAD, generator=g))
    W = torch.zeros(N_PAD, K_HEAD, dtype=torch.bfloat16)
    W[:N_REAL] = bf(torch.randn(N_REAL, K_HEAD, generator=g) * (2.0 / math.sqrt(K_HEAD)))
    bias = torch.full((N_PAD,), -1e30)
    bias[:N_REAL] = torch.randn(N_REAL, generator=g)
    bias[[10, 12, 200]] = 4.0
    A[0] = 0
    W[N_REAL - 1] = A[1] * 0.5
    return dict(A=A, W=W, bias=bias, M=M)


def rowmax_reference(c):
    A, W, b = c["A"].double(), c["W"].double(), c["bias"].double()
    pre = A @ W.t() + b
    e = BD.rowmax_logit_error(pre, A.abs() @ W.abs().t(), b.abs()[None, :], K_HEAD)
    return pre, e


def rowmax_emulate(c, fault=None):
    """fp32 emulation of the epilogue and the combine: records [n_seg, M, 4] and (maxprob, argmax, lse)"""
    M, n_seg = c["M"], N_PAD // 64
    bias = c["bias"].clone()
    if fault == "padded_column_wins":
        bias[N_REAL:] = 1e30                       # the sign of the padding bias lost
    if fault == "padded_column_adds_to_sum":
        bias[N_REAL:] = 0.0                        # the padding bias not applied: 212 logits of 0 join the sums
    acc = c["A"].float() @ c["W"].float().t()
    x = acc + bias
    seg = x.view(M, n_seg, 64)
    if fault == "bias_added_after_maximum":
        am = acc.view(M, n_seg, 64).argmax(-1)
        mx = seg.gather(-1, am[..., None])[..., 0]
    else:
        mx = seg.amax(-1)
        tie = seg == mx[..., None]
        am = (tie.float().argmax(-1) if fault != "argmax_highest_index_on_tie" else 63 - tie.flip(-1).float().argmax(-1))
    se = torch.exp(seg - mx[..., None]).sum(-1)
    idx = (am + torch.arange(n_seg)[None, :] * 64).to(torch.int32)
    rec = torch.stack([mx, se, idx.view(torch.float32), torch.zeros_like(mx)], -1).permute(1, 0, 2).contiguous()   # [n_seg, M, 4]
    mxs, ses, ids = rec[..., 0], rec[..., 1], idx.t()
    if fault == "segment_left_out_of_combine":
        mxs, ses, ids = mxs[1:], ses[1:], ids[1:]
    gmx = mxs.amax(0)
    if fault == "segment_sums_combined_as_if_against_the_row_maximum":
        tot = ses.sum(0)
    else:
        tot = (ses * torch.exp(mxs - gmx[None, :])).sum(0)
    hold = mxs == gmx[None, :]
    if fault == "argmax_highest_index_on_tie":
        arg = torch.where(hold, ids, torch.full_like(ids, -1)).amax(0)
    else:
        arg = torch.where(hold, ids, torch.full_like(ids, 2 ** 31 - 1)).amin(0)
    return rec, 1.0 / tot, arg.to(torch.int32), gmx + torch.log(tot)


def rowmax_check_all(c, rec, p, arg, lse):
    pre, e = rowmax_reference(c)
    n_seg = N_PAD // 64
    BD.check_rowmax_records(rec, pre, e)
    BD.check_rowmax_combine(R64, rec, n_seg, c["M"], p, arg, lse)
    _, n_adm = BD.check_rowmax_rows(pre, e, n_seg, p, arg, lse)
    return n_adm


def test_rowmax_honest_result_passes_with_exact_ties_and_padding():
    c = rowmax_case()
    rec, p, arg, lse = rowmax_emulate(c)
    n_adm = rowmax_check_all(c, rec, p, arg, lse)
    assert int(arg[0]) == 10 and int(arg[1]) == N_REAL - 1          # the tie goes to the lowest index; the last real column can win
    assert int(n_adm.max()) < 8
    # the float64 restatement of the combine rounded to fp32 passes as well
    pr, lr, ir = torch.zeros(c["M"], dtype=torch.float64), torch.zeros(c["M"], dtype=torch.float64), torch.zeros(c["M"], dtype=torch.int32)
    R64.rowmax_combine(rec, N_PAD // 64, c["M"], pr, ir, lr)
    rowmax_check_all(c, rec, pr.float(), ir, lr.float())


# ------------------------------------------------------------------------------------------------------------------ BCE
def bce_case(seed=17, M=6, N=3129, ld=3136):
    g = _gen(seed)
    x = torch.randn(M, N, generator=g) * 4
    t = (torch.rand(M, N, generator=g) < 0.3).float() * torch.rand(M, N, generator=g).round()      # sparse soft targets, many 1.0
    return x, t, M, N, ld


def bce_emulate(x, t, M, N, ld, dtype, fault=None):
    xs = x.to(torch.bfloat16).float() if fault == "sigmoid_of_bf16_rounded_logit" else x
    e = torch.exp(-xs.abs())
    sg = torch.where(xs >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    scale = 1.0 / M if fault == "bce_gradient_divided_by_M" else 1.0 / (M * N)
    d = torch.full((M, ld), float("nan"))                          # (the checked buffer starts as NaN: unwritten elements show)
    d[:, :N] = (sg - t) * torch.tensor(scale, dtype=torch.float32)
    if fault != "padded_dlogits_columns_unwritten":
        d[:, N:] = 0
    loss = ((x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).sum() * torch.tensor(1.0 / (M * N))).float()
    return d.to(dtype), loss


def bce_reference(x, t, M, N, ld, dtype):
    dl = torch.zeros(M, ld, dtype=torch.float64)
    loss = torch.zeros(1, dtype=torch.float64)
    R64.bce_logits_fwd_bwd(x, t, dl, loss, M, N, N, N, ld)
    b_dl, b_loss = BD.bce_bounds(x.double(), t.double(), M, N, dl[:, :N], float(loss), 0.0, dtype)
    bound = torch.full((M, ld), BD.TINY, dtype=torch.float64)
    bound[:, :N] = b_dl
    return dl, loss, bound, b_loss


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_bce_honest_result_passes(dtype):
    c = bce_case()
    dl, loss, bound, b_loss = bce_reference(*c, dtype)
    d, l = bce_emulate(*c, dtype)
    BD.check(d, dl, bound, "bce dlogits")
    BD.check(l.reshape(1), loss, b_loss, "bce loss")


# ------------------------------------------------------------------------------------------------------------------ attn_probs
def attn_probs_run(ops, c, lse, dtype, seed=None):
    B, n = c["B"], c["n"]
    probs = torch.zeros(B, H, n, n, dtype=dtype)
    ops.attn_probs(c["q"], c["k"], c["key_mask"], lse, probs, B, H, n, n, DH, H * DH, H * DH, 0.125, p_drop=c["p_drop"],
                   seed=c["seed"] if seed is None else seed, q_off=c["off"], k_off=c["off"])
    return probs


def attn_probs_ref(c):
    B, n, off = c["B"], c["n"], c["off"]
    _, lse = attn_fwd(R32, c, torch.float32)                        # the lse a forward kernel saved (fp32)
    P = attn_probs_run(R64, c, lse.double(), torch.float64)
    Q, K, V, valid, keep = BD.attention_inputs(R64, c["q"], c["k"], c["v"], c["key_mask"], B, H, n, n, DH, H * DH, H * DH, H * DH,
                                               c["p_drop"], c["seed"], off, off)
    lse3 = lse.double().view(B, H, n)
    return lse, P, BD.attn_probs_bound(Q, K, V, valid, keep, 0.125, lse3, P), keep


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("p_drop", [0.0, 0.1], ids=["no_dropout", "dropout"])
def test_attn_probs_honest_result_passes(packed, p_drop):
    c = attn_case(packed, p_drop)
    lse, P, bound, _ = attn_probs_ref(c)
    BD.check(attn_probs_run(R32, c, lse, torch.float32), P, bound, "attn_probs")


# ------------------------------------------------------------------------------------------------------------------ index kernels
def sampler_state(seed=19, B=16, V=64):
    g = _gen(seed)
    prob = torch.rand(B, V, generator=g)
    prob[3] = 0.25                                                  # a row of all-equal confidences
    prob[4, 7] = prob[4, 50] = prob[4].min() / 2                    # a tie at the bottom
    pred = torch.randint(0, 10000, (B, V), generator=g, dtype=torch.int32)
    ids = torch.randint(0, 10000, (B, V), generator=g)
    return prob, pred, ids, B, V


def test_sampler_index_kernels_reference_rules():
    """what check_exact compares the kernels with: stable ascending order, exactly n_mask per row, first index of the maximum"""
    prob, pred, ids, B, V = sampler_state()
    for n_mask in (0, 1, 16, 48, V):
        m = torch.zeros(B, V, dtype=torch.uint8)
        R64.remask_lowest(prob.double(), m, B, V, n_mask)
        assert bool((m.sum(1) == n_mask).all())
        if 0 < n_mask < V:
            assert m[3, :n_mask].all() and not m[3, n_mask:].any()
        if n_mask == 1:
            assert m[4, 7] == 1 and m[4, 50] == 0
    visited, vm = torch.zeros(B, V, dtype=torch.uint8), torch.ones(B, V, dtype=torch.uint8)
    p2 = prob.clone()
    p2[5, 9] = p2[5, 33] = 2.0
    R64.sampler_ar_update(p2.double(), pred, visited, vm, ids.clone(), B, V, -1)
    assert visited[5, 9] == 1 and visited[5, 33] == 0 and visited[3, 0] == 1 and int(visited.sum()) == B


SAMPLER_FAULTS = ["argmax_highest_index_on_tie", "segment_left_out_of_combine", "padded_column_wins", "padded_column_adds_to_sum",
                  "bias_added_after_maximum", "segment_sums_combined_as_if_against_the_row_maximum",
                  "sigmoid_of_bf16_rounded_logit", "bce_gradient_divided_by_M", "padded_dlogits_columns_unwritten",
                  "remask_highest_instead_of_lowest", "remask_one_too_many", "remask_one_too_few",
                  "sampler_update_writes_unmasked_positions", "sampler_ar_update_chooses_a_visited_position",
                  "attn_probs_dropout_mask_of_the_neighbouring_head", "take_f32_keeps_values_outside_the_owned_range"]


def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    pytest.fail(f"{what}: the checks are too loose -- the faulty result passes")


@pytest.mark.parametrize("fault", SAMPLER_FAULTS)
def test_sampler_and_task_bounds_reject_plausible_kernel_faults(fault):
    if fault in SAMPLER_FAULTS[:6]:
        c = rowmax_case()
        out = rowmax_emulate(c, fault)
        _rejected(lambda: rowmax_check_all(c, *out), fault)
    elif fault in SAMPLER_FAULTS[6:9]:
        dtype = torch.float32 if fault == "sigmoid_of_bf16_rounded_logit" else torch.bfloat16
        c = bce_case()
        dl, _, bound, _ = bce_reference(*c, dtype)
        d, _ = bce_emulate(*c, dtype, fault)
        must_reject(d, dl, bound, fault)
    elif fault.startswith("remask"):
        prob, _, _, B, V = sampler_state()
        ref = torch.zeros(B, V, dtype=torch.uint8)
        R64.remask_lowest(prob.double(), ref, B, V, 16)
        bad = torch.zeros(B, V, dtype=torch.uint8)
        if fault == "remask_highest_instead_of_lowest":
            R64.remask_lowest(-prob.double(), bad, B, V, 16)
        else:
            R64.remask_lowest(prob.double(), bad, B, V, 17 if fault == "remask_one_too_many" else 15)
        _rejected(lambda: BD.check_exact(bad, ref, fault), fault)
        if fault != "remask_highest_instead_of_lowest":            # (that one masks the right number of wrong positions)
            _rejected(lambda: BD.check_exact(bad.sum(1), torch.full((B,), 16), fault + " (per-row count)"), fault)
    elif fault == "sampler_update_writes_unmasked_positions":
        prob, pred, ids, B, V = sampler_state()
        vm = (prob < 0.5).to(torch.uint8)
        ref = ids.clone()
        R64.sampler_update(pred, vm, ref, B * V)
        _rejected(lambda: BD.check_exact(pred.long(), ref, fault), fault)
    elif fault == "sampler_ar_update_chooses_a_visited_position":
        prob, pred, ids, B, V = sampler_state()
        visited = torch.zeros(B, V, dtype=torch.uint8)
        visited[torch.arange(B), prob.argmax(1)] = 1                # every row's most confident position is taken already
        ref_v, ref_m, ref_i = visited.clone(), torch.ones(B, V, dtype=torch.uint8), ids.clone()
        R64.sampler_ar_update(prob.double(), pred, ref_v, ref_m, ref_i, B, V, -1)
        bad_v, bad_m, bad_i = torch.zeros(B, V, dtype=torch.uint8), torch.ones(B, V, dtype=torch.uint8), ids.clone()
        R64.sampler_ar_update(prob.double(), pred, bad_v, bad_m, bad_i, B, V, -1)       # (as if nothing had been visited)
        _rejected(lambda: BD.check_exact(bad_m, ref_m, fault), fault)
        _rejected(lambda: BD.check_exact(bad_i, ref_i, fault), fault)
    elif fault == "attn_probs_dropout_mask_of_the_neighbouring_head":
        c = attn_case(False, 0.1)
        lse, P, bound, keep = attn_probs_ref(c)
        clean = attn_probs_run(R32, dict(c, p_drop=0.0), lse, torch.float32)
        must_reject(clean * torch.roll(keep, 1, 1).float(), P, bound, fault)
    elif fault == "take_f32_keeps_values_outside_the_owned_range":
        src = torch.arange(1.0, 101.0)
        idx = torch.tensor([0, 5, 40, 41, 99, 60], dtype=torch.int32)
        ref = torch.zeros(6, dtype=torch.float64)
        R64.take_f32(src.double(), idx, 5, 60, ref)
        assert ref.tolist() == [0.0, 6.0, 41.0, 42.0, 0.0, 0.0]
        _rejected(lambda: BD.check_exact(src[idx.long()].double(), ref, fault), fault)
    else:
        raise AssertionError(fault)


# ------------------------------------------------------------------------------------------------------------------ sharpness
def test_admissible_argmax_rule_is_sharp_on_the_oracle_sampler_step():
    """The admissible-argmax rule accepts every column within 2 SLACK E of the float64 maximum; it says nothing if many columns
    are.  On the float64 oracle (full-size model, make_state_dict(oc, 19), make_inputs(oc, 23, 8), all 64 grid positions masked =
    sampler step 1, head operands rounded to bf16 as the kernel reads them) 5.1 % of the 512 rows have two admissible columns and
    none has more (logit std 14.7, worst E 0.10).  Caps, 3x / 2x over that for other seeds and steps: at most 15 % of the rows with
    more than one admissible column, never more than 4 in a row -- the same caps the GPU sampler test applies at every step."""
    import lxmert_oracle as O
    oc = O.OracleConfig()
    sd = O.make_state_dict(oc, 19, dtype=torch.float64)
    inp = O.make_inputs(oc, 23, 8)
    B, V = 8, 64
    code = sd["mask_feat"].view(1, 1, -1).expand(B, V, -1)
    with torch.no_grad():
        _, vis, _ = O.lxmert_model(sd, oc, inp["input_ids"], code, inp["visual_pos"].double(), inp["input_ids"] > 0)
        feat, _ = O.visual_obj_head(sd, oc, vis)
    A = feat.reshape(B * V, -1).to(torch.bfloat16).double()
    W = sd["vis_emb.weight"].to(torch.bfloat16).double()
    b = sd["obj_predict_head.out_cluster.bias"].double()
    pre = A @ W.t() + b
    e = BD.rowmax_logit_error(pre, A.abs() @ W.abs().t(), b.abs()[None, :], A.shape[1])
    E = e.amax(-1)
    _, n_adm = BD.argmax_admissible(pre, pre.argmax(-1), E)
    share, most = BD.sharpness(n_adm)
    top2 = pre.topk(2, -1).values
    print(f"\nsharpness: {int((n_adm > 1).sum())} of {n_adm.numel()} rows ({100 * share:.1f} %) with more than one admissible column, "
          f"at most {most} in a row; logit std {float(pre.std()):.1f}, worst E {float(E.max()):.2f}, median top-1/top-2 gap "
          f"{float(((top2[:, 0] - top2[:, 1]) / (2 * BD.SLACK * E)).median()):.1f} x the acceptance width")
    assert share <= BD.MAX_SHARE_AMBIGUOUS and most <= BD.MAX_ADMISSIBLE, (share, most)


# ------------------------------------------------------------------------------------------------------------------ recorder
TINY = dict(vocab_size=200, hidden_size=128, num_attention_heads=2, intermediate_size=256, max_position_embeddings=32,
            visual_feat_dim=64, num_clusters=96, l_layers=2, x_layers=2, r_layers=2)


@pytest.mark.parametrize("workload", ["nar_sampler", "ar_sampler", "vqa", "nlvr2", "word_mask", "matched", "output_attentions",
                                      "temperature_sampler", "evaluate_fused", "evaluate_logits"])
def test_recorded_workloads_pass_over_the_host_restatement(workload, monkeypatch):
    """the recording proxy, every checker and the "must have called" sets of tests/test_workload_bounds_gpu.py, driven here by the
    fp32 host restatement on bf16 storage at a tiny geometry: an honest implementation of every op is inside every bound, and the
    GPU tests' own code runs wherever the suite runs"""
    import lxmert_oracle as O
    import test_workload_bounds_gpu as W
    cfg, oc = W._cfgs(**TINY)
    ops = FakeOps(torch.bfloat16)
    if workload == "nar_sampler":
        rec = W.nar_sampler(cfg, oc, O.make_state_dict(oc, 19), 4, 4, "cpu", ops)
        assert len(rec.sharp) == 4
    elif workload == "ar_sampler":
        for mode in ("confidence", "tlbr"):
            W.ar_sampler(cfg, oc, O.make_state_dict(oc, 19), 4, mode, 3, "cpu", FakeOps(torch.bfloat16))
    elif workload == "vqa":
        W.vqa_step(cfg, O.make_vqa_state_dict(oc, 29, 41), 4, 29, "cpu", ops)
    elif workload == "nlvr2":
        W.nlvr2_step(cfg, O.make_nlvr2_state_dict(oc, 41), 4, "cpu", ops)
    elif workload in ("word_mask", "matched"):
        W.lang_step(cfg, O.make_cls_state_dict(oc, 41), workload, 4, "cpu", ops)
    elif workload == "temperature_sampler":
        rec = W.temperature_sampler(cfg, oc, O.make_state_dict(oc, 19), 4, dev="cpu", ops=_predict_ops_cls()(torch.bfloat16))
        assert len(rec.sharp) == 2
    elif workload in ("evaluate_fused", "evaluate_logits"):
        if workload == "evaluate_logits":
            monkeypatch.setenv("XL_FUSED_PREDICT", "0")
        cfg, oc = W._cfgs(**dict(TINY, max_position_embeddings=64))          # (64 tokens a row: 256 language rows at bs 4)
        W.evaluate_tasks(cfg, oc, (O.make_state_dict(oc, 19), O.make_cls_state_dict(oc, 41)), 4, workload == "evaluate_fused", "cpu",
                         _predict_ops_cls()(torch.bfloat16))
    else:
        W.attentions_forward(cfg, oc, O.make_state_dict(oc, 19), 4, "cpu", ops)


def test_dropout_mask_restatement_in_torch_integers_equals_the_numpy_statement():
    """fake_ops.keep_scale hashes index tensors that live on an accelerator with keep_scale_torch: the same mask, bit for bit"""
    from fake_ops import keep_scale_torch
    g = _gen(29)
    for seed in (0, 3, 5 + 7 * 1000003, (1 << 40) + 12345, (1 << 63) - 1):
        row = torch.randint(0, 1 << 31, (257, 1), generator=g)
        col = torch.randint(0, 70000, (1, 130), generator=g)
        for p_drop in (0.1, 0.5, 0.013):
            assert torch.equal(keep_scale(seed, row, col, p_drop), keep_scale_torch(seed, *torch.broadcast_tensors(row, col), p_drop))
    assert torch.equal(keep_scale(9, torch.arange(300)[:, None], torch.arange(64)[None, :], 0.1),
                       keep_scale_torch(9, torch.arange(300)[:, None], torch.arange(64)[None, :], 0.1))


# ------------------------------------------------------------------------------------------------------------------ long attention
# Attention with 65..512 tokens per side (csrc/sdpa.hip sdpa_fwd_flash, sdpa_bwd_flash_q, sdpa_bwd_flash_k): a host emulation of
# the blocked algorithm in plain torch -- fp32 arithmetic, 64-key / 64-query blocks, the un-normalised P~ rounded to bf16 before
# the PV product, dS rounded to bf16 -- passes the block-aware bounds, and every fault of LONG_FAULTS built into it is rejected.
# Inputs: 12 heads of 64, q scaled by 1.5 (score standard deviation 1.5: the running maximum rises in later blocks on most rows).
LONG_SHAPES = [(128, 128), (200, 70), (70, 200)]
LONG_SCALE = 0.125


def long_case(nq, nk, p_drop, kind, seed=17):
    """kind "masked": B = 3 dense, random key mask with key 0 valid, example 1 with its first 64 keys ALL masked (later keys valid).
    kind "packed": B = 4, both sides packed, lengths 1 / 64 / 65 / 128 (clipped to the side's capacity), no key mask."""
    g = _gen(seed)
    if kind == "packed":
        B = 4
        lens = torch.tensor([1, 64, 65, 128])
        len_q, len_k = lens.clamp(max=nq), lens.clamp(max=nk)
        q_off, k_off = (torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(l, 0)]).to(torch.int32) for l in (len_q, len_k))
        rows_q, rows_k, key_mask = int(q_off[-1]), int(k_off[-1]), None
    else:
        B = 3
        len_q, len_k, q_off, k_off = torch.full((B,), nq), torch.full((B,), nk), None, None
        rows_q, rows_k = B * nq, B * nk
        key_mask = (torch.rand(B, nk, generator=g) > 0.2).to(torch.uint8)
        key_mask[:, 0] = 1
        key_mask[1, :64] = 0
        key_mask[1, 64:] = 1
    q = bf(torch.randn(rows_q, H * DH, generator=g) * 1.5)
    k, v = (bf(torch.randn(rows_k, H * DH, generator=g)) for _ in range(2))
    do = bf(torch.randn(rows_q, H * DH, generator=g))
    return dict(q=q, k=k, v=v, do=do, B=B, nq=nq, nk=nk, rows_q=rows_q, rows_k=rows_k, q_off=q_off, k_off=k_off, len_q=len_q,
                len_k=len_k, key_mask=key_mask, p_drop=p_drop, seed=seed)


def long_reference(c):
    """float64 restatement (FakeOps) and the block-aware bounds, everything in the dense [B, H, n, dh] layout"""
    B, nq, nk, HD = c["B"], c["nq"], c["nk"], H * DH
    kw = dict(p_drop=c["p_drop"], seed=c["seed"], q_off=c["q_off"], k_off=c["k_off"])
    o = torch.zeros(c["rows_q"], HD, dtype=torch.float64)
    lse = torch.zeros(B * H * nq, dtype=torch.float64)
    R64.sdpa_fwd(c["q"], c["k"], c["v"], c["key_mask"], o, lse, B, H, nq, nk, DH, HD, HD, HD, HD, LONG_SCALE, **kw)
    Q, K, V, valid, keep = BD.attention_inputs(R64, c["q"], c["k"], c["v"], c["key_mask"], B, H, nq, nk, DH, HD, HD, HD, c["p_drop"],
                                               c["seed"], c["q_off"], c["k_off"])
    lse = lse.view(B, H, nq)
    lse32 = lse.float()                                   # what the forward kernel hands the backward
    O_ = R64._load(o, B, nq, H, DH, HD, c["q_off"])[0]
    n_kblk, n_qblk = (nk + 63) // 64, (nq + 63) // 64
    bO, bl = BD.sdpa_fwd_bounds(Q, K, V, valid, keep, LONG_SCALE, O_, lse, n_kblk=n_kblk)
    dq, dk, dv = (torch.zeros(r, HD, dtype=torch.float64) for r in (c["rows_q"], c["rows_k"], c["rows_k"]))
    R64.sdpa_bwd(c["q"], c["k"], c["v"], c["key_mask"], c["do"], lse32.double().reshape(-1), dq, dk, dv, B, H, nq, nk, DH,
                 *([HD] * 7), LONG_SCALE, **kw)
    dO = R64._load(c["do"], B, nq, H, DH, HD, c["q_off"])[0]
    dense = [R64._load(t, B, n, H, DH, HD, off)[0] for t, n, off in ((dq, nq, c["q_off"]), (dk, nk, c["k_off"]), (dv, nk, c["k_off"]))]
    bb, _ = BD.sdpa_bwd_bounds(Q, K, V, dO, valid, keep, LONG_SCALE, lse32.double(), *dense, n_kblk=n_kblk, n_qblk=n_qblk)
    exist = valid.any(-1).expand(B, H, nq)
    return dict(Q=Q, K=K, V=V, dO=dO, O=O_, lse=lse, lse32=lse32, exist=exist, bO=bO, bl=bl, grads=dense, bgrads=bb)


def _pad_rows(t, n):
    return torch.nn.functional.pad(t, (0, 0, 0, n - t.shape[-2]))


def _long_masks(c, nkp, fault):
    """per example: the keys a block treats as attending (mask bit and key < length) over the padded key range, and the dropout
    keep scale over the padded range"""
    B, nq, nk = c["B"], c["nq"], c["nk"]
    ar = torch.arange(nkp)
    in_len = ar[None, :] < c["len_k"][:, None]
    bits = torch.ones(B, nkp, dtype=torch.bool)
    if c["key_mask"] is not None:                         # (key_bits: lanes beyond the capacity read no byte: bit off)
        bits = torch.nn.functional.pad(c["key_mask"] != 0, (0, nkp - nk))
    if fault == "mask_bit_read_from_the_neighbouring_block":
        bits = bits.view(B, nkp // 64, 64).roll(-1, 1).reshape(B, nkp)
    ok = bits if fault == "key_beyond_nk_in_the_last_partial_block_counted_valid" else bits & in_len
    keepm = torch.ones(B, H, nq, nkp)
    if c["p_drop"] > 0:
        col = ar % 64 if fault == "dropout_column_counter_without_the_block_offset" else ar
        keepm = keep_scale(c["seed"], torch.arange(B * H * nq).view(B, H, nq, 1), col.view(1, 1, 1, nkp), c["p_drop"])
    return ok, keepm


def flash_fwd_emulate(c, r, fault=None):
    """sdpa_fwd_flash in fp32: per 64-key block the scores, the running maximum and sum, the accumulators rescaled by
    exp(m_old - m_new), P~ rounded to bf16 for the PV product; division by the sum and lse = m + log(sum) at the end"""
    B, nq, nk = c["B"], c["nq"], c["nk"]
    nb = (nk + 63) // 64
    Q, K, V = r["Q"].float(), _pad_rows(r["K"].float(), nb * 64), _pad_rows(r["V"].float(), nb * 64)
    ok, keepm = _long_masks(c, nb * 64, fault)
    ninf = torch.tensor(-math.inf)
    mx, sm, acc = torch.full((B, H, nq), -math.inf), torch.zeros(B, H, nq), torch.zeros(B, H, nq, DH)
    bm = mx
    for i in range(nb):
        ks = slice(i * 64, (i + 1) * 64)
        s = torch.where(ok[:, None, None, ks], (Q @ K[:, :, ks].transpose(-1, -2)) * LONG_SCALE, ninf)
        bm = s.amax(-1)
        nm = torch.maximum(mx, bm)
        corr = torch.where(mx == -math.inf, torch.zeros(()), torch.exp(mx - nm))
        e = torch.where(s == -math.inf, torch.zeros(()), torch.exp(s - nm[..., None]))
        pv = bf(e * keepm[..., ks]).float()
        sm = sm * (1.0 if fault == "running_sum_not_rescaled" else corr) + e.sum(-1)
        acc = acc * (1.0 if fault == "accumulators_not_rescaled" else corr[..., None]) + pv @ V[:, :, ks]
        mx = nm
    inv = torch.where(sm > 0, 1.0 / sm, torch.zeros(()))
    m_lse = bm if fault == "lse_from_the_last_block_maximum" else mx
    lse = torch.where(m_lse == -math.inf, torch.zeros(()), m_lse) + torch.log(sm)
    qv = (torch.arange(nq)[None, :] < c["len_q"][:, None]).view(B, 1, nq, 1)
    return acc * inv[..., None] * qv, lse


def flash_bwd_emulate(c, r, fault=None):
    """sdpa_bwd_flash_q (two passes over the key blocks: delta, then dQ) and sdpa_bwd_flash_k (one pass over the query blocks with
    the saved lse and delta) in fp32, dS and P~ rounded to bf16 before their products"""
    B, nq, nk = c["B"], c["nq"], c["nk"]
    nkb, nqb = (nk + 63) // 64, (nq + 63) // 64
    nkp, nqp = nkb * 64, nqb * 64
    Q, dO = _pad_rows(r["Q"].float(), nqp), _pad_rows(r["dO"].float(), nqp)
    K, V = _pad_rows(r["K"].float(), nkp), _pad_rows(r["V"].float(), nkp)
    lse = torch.nn.functional.pad(r["lse32"], (0, nqp - nq))
    ok_k, keepm = _long_masks(c, nkp, None)
    keepm = torch.nn.functional.pad(keepm, (0, 0, 0, nqp - nq), value=1.0)
    ok_q = torch.arange(nqp)[None, :] < c["len_q"][:, None]
    ok = ok_k[:, None, None, :] & ok_q[:, None, :, None]
    zero = torch.zeros(())
    # query side
    S = Q @ K.transpose(-1, -2)
    P = torch.where(ok, torch.exp(S * LONG_SCALE - lse[..., None]), zero)
    dP = (dO @ V.transpose(-1, -2)) * keepm
    delta = torch.zeros(B, H, nqp)
    for i in range(nkb):
        prod = (P * dP)[..., i * 64:(i + 1) * 64]
        if fault == "delta_not_combined_across_the_half_waves":
            prod = prod[..., (torch.arange(64) & 4) == 0]            # the keys of the low half-wave's accumulator rows
        if fault == "delta_covers_the_first_key_block_only" and i > 0:
            continue
        delta = delta + prod.sum(-1)
    dQ = torch.zeros(B, H, nqp, DH)
    for i in range(nkb):
        ks = slice(i * 64, (i + 1) * 64)
        dS = bf(P[..., ks] * (dP[..., ks] - delta[..., None]) * LONG_SCALE).float()
        dQ = dQ + dS @ K[:, :, ks]
    # key side
    dK, dV = torch.zeros(B, H, nkp, DH), torch.zeros(B, H, nkp, DH)
    for j in range(nqb):
        qs = slice(j * 64, (j + 1) * 64)
        okb = ok[:, :, qs]
        if fault == "dk_dv_miss_the_last_partial_query_block":
            partial = ((j + 1) * 64 > c["len_q"]) & (c["len_q"] % 64 != 0)
            okb = okb & ~partial.view(B, 1, 1, 1)
        arg = S[:, :, qs] * (1.0 if fault == "key_side_p_from_unscaled_scores" else LONG_SCALE) - lse[:, :, qs, None]
        Pb = torch.where(okb, torch.exp(arg), zero)
        dPb = dP[:, :, qs]
        dS = bf(Pb * (dPb - delta[:, :, qs, None]) * LONG_SCALE).float()
        Pt = bf(Pb * keepm[:, :, qs]).float()
        dV = dV + Pt.transpose(-1, -2) @ dO[:, :, qs]
        dK = dK + dS.transpose(-1, -2) @ Q[:, :, qs]
    return dQ[:, :, :nq], dK[:, :, :nk], dV[:, :, :nk]


@pytest.mark.parametrize("kind", ["masked", "packed"])
@pytest.mark.parametrize("p_drop", [0.1, 0.0], ids=["dropout", "no_dropout"])
@pytest.mark.parametrize("nq,nk", LONG_SHAPES)
def test_long_attention_honest_blocked_emulation_passes(nq, nk, p_drop, kind):
    c = long_case(nq, nk, p_drop, kind)
    r = long_reference(c)
    o, lse = flash_fwd_emulate(c, r)
    BD.check(bf(o), r["O"], r["bO"], "flash fwd O")
    BD.check(lse[r["exist"]], r["lse"][r["exist"]], r["bl"][r["exist"]], "flash fwd lse")
    for nm, got, ref, b in zip(("dQ", "dK", "dV"), flash_bwd_emulate(c, r), r["grads"], r["bgrads"]):
        BD.check(bf(got), ref, b, f"flash bwd {nm}")


# fault -> (nq, nk, p_drop, kind, the outputs that must be rejected)
LONG_FAULTS = {
    "accumulators_not_rescaled": (128, 128, 0.0, "masked", ("O",)),
    "running_sum_not_rescaled": (128, 128, 0.0, "masked", ("O", "lse")),
    "lse_from_the_last_block_maximum": (128, 128, 0.0, "masked", ("lse",)),
    "dropout_column_counter_without_the_block_offset": (128, 128, 0.1, "masked", ("O",)),
    "key_beyond_nk_in_the_last_partial_block_counted_valid": (200, 70, 0.0, "packed", ("O", "lse")),
    "mask_bit_read_from_the_neighbouring_block": (128, 128, 0.0, "masked", ("O", "lse")),
    "delta_covers_the_first_key_block_only": (128, 128, 0.1, "masked", ("dQ", "dK")),
    "delta_not_combined_across_the_half_waves": (128, 128, 0.1, "masked", ("dQ", "dK")),
    "dk_dv_miss_the_last_partial_query_block": (70, 200, 0.1, "masked", ("dK", "dV")),
    "key_side_p_from_unscaled_scores": (128, 128, 0.1, "masked", ("dK", "dV")),
}


@pytest.mark.parametrize("fault", sorted(LONG_FAULTS))
def test_long_attention_bounds_reject_blocked_kernel_faults(fault):
    nq, nk, p_drop, kind, outs = LONG_FAULTS[fault]
    c = long_case(nq, nk, p_drop, kind)
    r = long_reference(c)
    o, lse = flash_fwd_emulate(c, r, fault)
    dq, dk, dv = flash_bwd_emulate(c, r, fault)
    ex = r["exist"]
    got = {"O": (bf(o), r["O"], r["bO"]), "lse": (lse[ex], r["lse"][ex], r["bl"][ex]), "dQ": (bf(dq), r["grads"][0], r["bgrads"][0]),
           "dK": (bf(dk), r["grads"][1], r["bgrads"][1]), "dV": (bf(dv), r["grads"][2], r["bgrads"][2])}
    for nm in outs:
        must_reject(*got[nm], f"{fault}: {nm}")
    for nm in set(got) - set(outs):          # a fault moves nothing but what it is built into (the emulation stays honest elsewhere)
        if (nm in ("O", "lse")) != (outs[0] in ("O", "lse")):
            BD.check(*got[nm], f"{fault}: untouched {nm}")


def test_attention_bounds_without_block_counts_are_the_on_chip_bounds_bit_for_bit():
    """the three bound functions called as before (no block count) and with a count of 1 return what the unchanged formulas,
    written out here, give -- torch.equal, not a tolerance"""
    c = attn_case(False, 0.1)
    o, lse = attn_fwd(R64, c, torch.float64)
    B, n = c["B"], c["n"]
    Q, K, V, valid, keep = BD.attention_inputs(R64, c["q"], c["k"], c["v"], c["key_mask"], B, H, n, n, DH, H * DH, H * DH, H * DH,
                                               c["p_drop"], c["seed"], None, None)
    O_ = R64._load(o, B, n, H, DH, H * DH, None)[0]
    L = lse.view(B, H, n)
    U16, U32, SL, TINY = 2.0 ** -8, 2.0 ** -24, 2.0, 2.0 ** -126
    s, P, Pk, eS = BD.attention_parts(Q, K, V, valid, keep, 0.125)
    pv = Pk.abs() @ V.abs()
    want_O = U16 * O_.abs() + SL * (U16 + 2 * eS + (n + 4) * U32) * pv + TINY
    want_l = SL * (eS[..., 0] + (n + 4) * U32 + 2 * U32 * L.abs() + 2.0 ** -21)
    dflt = {"out_dtype": torch.bfloat16, "arith": "mfma"}            # the defaults of the output-type / arithmetic arguments
    for kw in ({}, {"n_kblk": 1}, dflt):
        bO, bl = BD.sdpa_fwd_bounds(Q, K, V, valid, keep, 0.125, O_, L, **kw)
        assert torch.equal(bO, want_O) and torch.equal(bl, want_l)
    # the fp32 arithmetic of the generic kernels: no designed bf16 term -- strictly tighter for a bf16 store, 2^-16 of it for an fp32 one
    g16, gl = BD.sdpa_fwd_bounds(Q, K, V, valid, keep, 0.125, O_, L, arith="fp32")
    g32, _ = BD.sdpa_fwd_bounds(Q, K, V, valid, keep, 0.125, O_, L, out_dtype=torch.float32, arith="fp32")
    assert torch.equal(gl, want_l) and bool((g16 <= want_O).all()) and bool((g32 <= g16).all())
    assert torch.equal(g32, U32 * O_.abs() + SL * (n * U32 + 2 * eS + (n + 4) * U32) * pv + TINY)
    # attn_probs
    ref = torch.exp(s - L[..., None]).masked_fill(~valid.expand_as(s), 0.0) * keep
    arg = (s - L[..., None]).abs().masked_fill(~valid.expand_as(s), 0.0).nan_to_num(0.0, posinf=0.0)
    want_p = U32 * ref.abs() + SL * ref.abs() * (eS + 2 * U32 * arg + (2.0 + 2) * U32) + TINY
    for kw in ({}, {"n_kblk": 1}):
        assert torch.equal(BD.attn_probs_bound(Q, K, None, valid.expand_as(s), keep, 0.125, L, ref, **kw), want_p)
    # backward
    dO = R64._load(c["do"], B, n, H, DH, H * DH, None)[0]
    dq, dk, dv = (torch.zeros(c["rows"], H * DH, dtype=torch.float64) for _ in range(3))
    R64.sdpa_bwd(c["q"], c["k"], c["v"], c["key_mask"], c["do"], lse, dq, dk, dv, B, H, n, n, DH, *([H * DH] * 7), 0.125,
                 p_drop=c["p_drop"], seed=c["seed"])
    dense = [R64._load(t, B, n, H, DH, H * DH, None)[0] for t in (dq, dk, dv)]
    sc = 0.125
    s0 = (Q @ K.transpose(-1, -2)) * sc
    Pb = torch.exp(s0 - L[..., None]).masked_fill(~valid, 0.0).nan_to_num(0.0, posinf=0.0)
    sabs = (Q.abs() @ K.abs().transpose(-1, -2)) * sc
    eP = DH * U32 * sabs + 2 * U32 + U32 * (s0 - L[..., None]).abs().masked_fill(~valid, 0.0).nan_to_num(0.0, posinf=0.0)
    dP = (dO @ V.transpose(-1, -2)) * keep
    edP = DH * U32 * (dO.abs() @ V.abs().transpose(-1, -2)) * keep
    delta = (Pb * dP).sum(-1, keepdim=True)
    edelta = (eP * Pb * dP.abs() + Pb * edP).sum(-1, keepdim=True) + n * U32 * (Pb * dP.abs()).sum(-1, keepdim=True)
    dS = Pb * (dP - delta) * sc
    edS = sc * (eP * Pb * (dP - delta).abs() + Pb * (edP + edelta)) + 3 * U32 * dS.abs() + U16 * dS.abs()
    Pk2 = (Pb * keep).abs()
    tV = (U16 + eP.amax(-2, keepdim=True).transpose(-1, -2) + (n + 2) * U32) * (Pk2.transpose(-1, -2) @ dO.abs())
    tQ = edS @ K.abs() + n * U32 * (dS.abs() @ K.abs())
    tK = edS.transpose(-1, -2) @ Q.abs() + n * U32 * (dS.abs().transpose(-1, -2) @ Q.abs())
    want = [U16 * g.abs() + SL * t + TINY for g, t in zip(dense, (tQ, tK, tV))]
    for kw in ({}, {"n_kblk": 1, "n_qblk": 1}, dflt):
        bounds, terms = BD.sdpa_bwd_bounds(Q, K, V, dO, valid, keep, 0.125, L, *dense, **kw)
        assert all(torch.equal(b, w) for b, w in zip(bounds, want))
        assert all(torch.equal(t, w) for t, w in zip(terms, (tQ, tK, tV)))
    b32, t32 = BD.sdpa_bwd_bounds(Q, K, V, dO, valid, keep, 0.125, L, *dense, out_dtype=torch.float32, arith="fp32")
    assert all(bool((t <= w).all()) for t, w in zip(t32, (tQ, tK, tV)))
    assert all(torch.equal(b, U32 * g.abs() + SL * t + TINY) for b, g, t in zip(b32, dense, t32))


# ------------------------------------------------------------------------------------------------------------------ GEMM dispatch edges
# tests/test_gemm_edges_bounds_gpu.py over the host restatement: the same calls (tests/gemm_edge_cases.py), the same recorder, the
# same label assertions.  The tail-split shape is the GPU test's own (4300, 4090, 1096), no stand-in: a few seconds of host float64.
GEMM_EDGE_RUNS = {
    **{f"shapes-{sw}": ("run_shapes", (sw,)) for sw in ("default", "pingpong_forced", "mfma_128_only", "transpose_read_off")},
    **{f"epilogues-{sw}": ("run_epilogues", (sw,)) for sw in ("default", "pingpong_forced", "mfma_128_only", "transpose_read_off")},
    **{f"colsums-{sw}": ("run_colsums", (sw,)) for sw in ("default", "pingpong_forced")},
    **{f"ksplits-{sw}-{'slabs' if sl else 'atomics'}": ("run_ksplits", (sw, sl)) for sw in ("default", "pingpong_forced")
       for sl in (False, True)},
    "tail_split": ("run_tail_split", ()), "duo": ("run_duo", ()),
    "wgrad_groups-atomics": ("run_wgrad_groups", (False,)), "wgrad_groups-slabs": ("run_wgrad_groups", (True,))}


@pytest.mark.parametrize("run", list(GEMM_EDGE_RUNS))
def test_gemm_edge_cases_pass_over_the_host_restatement(run):
    """an honest implementation (fp32 arithmetic on bf16 storage that reads the logical extents only and stores into the logical
    views only) is inside every bound at the inputs of the edge cases, guard rows included, and the sweep reaches the kernel labels
    the GPU tests expect"""
    import test_gemm_edges_bounds_gpu as G
    fn, args = GEMM_EDGE_RUNS[run]
    getattr(G, fn)(*args, ops=FakeOps(torch.bfloat16), dev="cpu")


class FaultyOps(FakeOps):
    """the host restatement with ONE kernel fault, applied at every call it can apply to:
      m_major_lost_term   the last row of an M-major A (last column of an N-major B) loses its final K term
      pad_as_k_term       the pad element behind the last row of a K-major A enters as one more K term
      short_slice_dropped the last, short K slice of a K split is dropped (K no multiple of 64: the K % 64 tail and what the
                          rounded slice leaves)
      stale_edge_tile     accumulate = 0 leaves the old C in the edge tile (the clearing pass stops at the last whole 128 x 128 tile)
      store_in_pad_column one store lands in C[0, N]
      store_in_row_m      one store lands in row M of a taller allocation
      overwrite_ignored   the overwrite bit of grouped problem 0 is ignored"""

    def __init__(self, fault):
        super().__init__(torch.bfloat16)
        self.fault, self.applied = fault, 0

    def gemm(self, A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr=0, ldx=0, a_kmajor=1, b_kmajor=1, out_f32=False,
             epilogue=EPI_NONE, alpha=1.0, accumulate=0, p_drop=0.0, seed=0, colsum=None, ws=None):
        f = self.fault
        kw = dict(ldr=ldr, ldx=ldx, a_kmajor=a_kmajor, b_kmajor=b_kmajor, out_f32=out_f32, epilogue=epilogue, alpha=alpha,
                  accumulate=accumulate, p_drop=p_drop, seed=seed, colsum=colsum, ws=ws)
        old = torch.as_strided(C, (M, N), (ldc, 1)).clone()
        if f == "m_major_lost_term" and not (a_kmajor and b_kmajor) and K > 1:
            if not a_kmajor:
                A = A.clone()
                A[(K - 1) * lda + M - 1] = 0
            else:
                B = B.clone()
                B[(K - 1) * ldb + N - 1] = 0
            self.applied += 1
        if f == "short_slice_dropped" and out_f32 and epilogue == EPI_NONE and K >= 1024 and K % 512:
            K -= K % 512 if K % 512 < 256 else K % 64
            self.applied += 1
        super().gemm(A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, **kw)
        c = torch.as_strided(C, (M, N), (ldc, 1))
        if f == "pad_as_k_term" and a_kmajor and lda > K and epilogue == EPI_NONE and not accumulate:
            b_last = (torch.as_strided(B, (N,), (ldb,), B.storage_offset() + K - 1) if b_kmajor
                      else torch.as_strided(B, (N,), (1,), B.storage_offset() + (K - 1) * ldb))
            c[M - 1] = (c[M - 1].double() + alpha * float(A[(M - 1) * lda + K]) * b_last.double()).to(c.dtype)
            self.applied += 1
        if f == "stale_edge_tile" and out_f32 and not accumulate and (M % 128 or N % 128):
            c[M - M % 128:, N - N % 128:] += old[M - M % 128:, N - N % 128:]
            self.applied += 1
        if f == "store_in_pad_column" and ldc > N:
            C[N] = 0
            self.applied += 1
        if f == "store_in_row_m" and C.numel() > M * ldc:
            C[M * ldc] = 0
            self.applied += 1

    def gemm_wgrad_group(self, problems, overwrite_mask=0):
        if self.fault == "overwrite_ignored" and overwrite_mask & 1:
            overwrite_mask &= ~1
            self.applied += 1
        super().gemm_wgrad_group(problems, overwrite_mask)


@pytest.mark.parametrize("fault,family", [("m_major_lost_term", "shapes"), ("pad_as_k_term", "shapes"), ("short_slice_dropped", "ksplits"),
                                          ("stale_edge_tile", "ksplits"), ("store_in_pad_column", "shapes"), ("store_in_row_m", "shapes"),
                                          ("overwrite_ignored", "wgrad_groups")])
def test_gemm_edge_cases_reject_plausible_kernel_faults(fault, family):
    """the same recorder run as the honest pass, over an implementation with one fault: it must fail, at EVERY call the fault
    applied to (each such call shows the fault on its own: none hides behind another's failure)"""
    import gemm_edge_cases as GE
    from test_kernel_bounds_gpu import Recorder
    ops = FaultyOps(fault)
    rec = Recorder(ops)
    g = torch.Generator().manual_seed(101)
    if family == "shapes":
        n = GE.shapes(rec, "cpu", g, shapes_=GE.SHAPES[3:9], f32_shapes=GE.F32_SHAPES[1:3])
    elif family == "ksplits":
        n = GE.ksplits(rec, "cpu", g, mn=GE.KSPLIT_MN[:1])
    else:
        n = GE.wgrad_groups(rec, "cpu", g, Ks=(72, 4104))
    assert len(rec.checked) + len(rec.failures) == n and ops.applied > 0
    print(f"{fault}: applied at {ops.applied} of {n} calls, {len(rec.failures)} failed")
    assert len(rec.failures) == ops.applied, (fault, ops.applied, len(rec.failures), rec.failures[:3])
    word = {"store_in_pad_column": "outside", "store_in_row_m": "outside"}.get(fault, "beyond their bound")
    assert all(word in f for f in rec.failures), rec.failures[:3]


# ------------------------------------------------------------------------------------------------------------------ row-kernel dispatch edges
# tests/test_rowop_edges_bounds_gpu.py over the host restatement: the same calls (tests/rowop_edge_cases.py), the same recorder, the
# same label assertions (the labels depend on the arguments only).
ROWOP_EDGE_RUNS = {
    **{f"{fam}-{dt}": (f"run_{fam}", (dt,)) for fam in ("layernorm", "visn_ln", "embeddings", "colsums", "deferred", "cross_entropy",
                                                         "elementwise", "optimizer") for dt in ("bf16", "fp32")},
    "layernorm_res": ("run_layernorm_res", ())}


class HonestRowOps(FakeOps):
    """FakeOps as a KERNEL stand-in: the restatement poisons the gradient of an AdamW chunk flagged keep (bit 2) with NaN so that a
    reader of it shows up in the engine tests; the kernel leaves it as it is, and so does this"""

    def adamw(self, p, g, m, v, p_compute, decay_flags, sumsq, lr_and_steps, n, beta1, beta2, eps, weight_decay, max_norm,
              grad_scale=1.0, chunk_steps=None, zero_grad=False):
        g0 = g[:n].clone()
        super().adamw(p, g, m, v, p_compute, decay_flags, sumsq, lr_and_steps, n, beta1, beta2, eps, weight_decay, max_norm,
                      grad_scale=grad_scale, chunk_steps=chunk_steps, zero_grad=zero_grad)
        g[:n].copy_(torch.where(torch.isnan(g[:n]), g0, g[:n]))


def _rowop_fake(fn, dt):
    from fake_ops_res import FakeOpsRes
    return FakeOpsRes(torch.bfloat16) if fn == "run_layernorm_res" else HonestRowOps({"bf16": torch.bfloat16, "fp32": torch.float32}[dt])


@pytest.mark.parametrize("run", list(ROWOP_EDGE_RUNS))
def test_rowop_edge_cases_pass_over_the_host_restatement(run):
    """an honest implementation (fp32 arithmetic on bf16 / fp32 storage that reads the logical extents only and stores into the
    logical views only) is inside every bound at the inputs of the edge cases, guard rows included, and every sweep reaches the
    kernel labels the GPU tests expect; in the cross-entropy family every row but the planted ties admits ONE argmax column on
    the float64 logits alone (asserted inside run_cross_entropy)"""
    import test_rowop_edges_bounds_gpu as R
    fn, args = ROWOP_EDGE_RUNS[run]
    dt = args[0] if args else "bf16"
    getattr(R, fn)(*(R.DTYPES[a] for a in args), ops=_rowop_fake(fn, dt), dev="cpu")


class FaultyRowOps(HonestRowOps):
    """the host restatement with ONE row-kernel / optimizer fault, applied at every call it can apply to (`applied` counts the calls
    whose result it changed):
      ln_stats_padded_width           LayerNorm statistics divided by the row length rounded up to whole 64-lane passes
      ln_last_vector_out_of_variance  the last live vector of a ragged row is left out of the variance
      second_stage_drops_last_slab    the second stage of a column sum leaves slab G - 1 out
      second_stage_stores             the second stage stores its sum instead of adding it to the destination
      ce_pad_slots_in_sum             the slots K .. K8 of a row enter the log-sum-exp of the register kernels
      ce_tie_highest_index            ties of the row maximum are resolved to the highest index
      ce_rows_past_cap_stale          the register kernels leave the rows past their grid cap unwritten
      embed_33rd_dropped              the sorted embedding backward drops the 33rd occurrence of a token (a chunk boundary)
      embed_9th_type_match_dropped    the token-type kernel drops the 9th match of a 64-row chunk
      adamw_flags_wrong_chunk         AdamW indexes its flags by chunks of 128 elements
      adamw_second_pass_missing       AdamW stops after one pass of its grid (256 blocks x 1024 threads x 4 elements)
      adamw_clip_ignores_grad_scale   the clip compares max_norm with the norm of the UNSCALED gradient
      sumsq_drops_tail                the n & 3 elements behind the last whole float4 are left out
      sumsq_overwrites                *out = sum instead of *out += sum
      schedule_off_by_one             the schedule is evaluated at the 1-based index of the update instead of the completed updates
      store_in_pad_column             one store lands in the first pad column of dlogits
      store_in_row_m                  one store lands in row M of y"""

    def __init__(self, fault, dtype=torch.bfloat16):
        super().__init__(dtype)
        self.fault, self.applied = fault, 0

    def layernorm_fwd(self, x, gamma, beta, y, mean, rstd, M, N, eps):
        f = self.fault
        V = 8 if x.dtype == torch.bfloat16 else 4
        Np = -(-N // (64 * V)) * 64 * V
        xx = torch.as_strided(x, (M, N), (N, 1)).float()
        if f == "ln_stats_padded_width" and Np != N:
            mu = xx.sum(1, keepdim=True) / Np
            var = ((xx - mu) ** 2).sum(1, keepdim=True) / Np
        elif f == "ln_last_vector_out_of_variance" and Np != N and N > V:
            mu = xx.mean(1, keepdim=True)
            var = ((xx - mu)[:, :N - V] ** 2).sum(1, keepdim=True) / N
        else:
            super().layernorm_fwd(x, gamma, beta, y, mean, rstd, M, N, eps)
            if f == "store_in_row_m":
                torch.as_strided(y, (1,), (1,), y.storage_offset() + M * N).zero_()
                self.applied += 1
            return
        r = 1.0 / torch.sqrt(var + eps)
        torch.as_strided(y, (M, N), (N, 1)).copy_((xx - mu) * r * gamma.float() + beta.float())
        mean[:M].copy_(mu[:, 0])
        rstd[:M].copy_(r[:, 0])
        self.applied += 1

    def _colsum(self, x, mask, out, M, N, ldx, ws):
        rpb = 128
        if ws is not None:
            while -(-M // rpb) > 128:
                rpb *= 2
        G = -(-M // rpb)
        xx = torch.as_strided(x, (M, N), (ldx, 1)).float()
        if mask is not None:
            xx = xx * (mask.view(-1, 1) != 0)
        if self.fault == "second_stage_drops_last_slab" and ws is not None and G > 1 and bool((xx[(G - 1) * rpb:] != 0).any()):
            xx = xx[:(G - 1) * rpb]
            self.applied += 1
        o = torch.as_strided(out, (N,), (1,))
        if self.fault == "second_stage_stores" and ws is not None:
            o.copy_(xx.sum(0))
            self.applied += 1
        else:
            o.add_(xx.sum(0))

    def colsum(self, x, out, M, N, ldx, ws=None):
        self._colsum(x, None, out, M, N, ldx, ws)

    def masked_colsum(self, x, mask, out, M, N, ldx, ws=None):
        self._colsum(x, mask, out, M, N, ldx, ws)

    def ce_fwd_bwd(self, logits, labels, counts, dlogits, loss_out, row_lse, row_argmax, row_maxprob, M, K, ldl, lddl, grad_scale=1.0):
        from fake_ops import ce_in_regs
        f = self.fault
        K8 = (K + 7) // 8 * 8
        regs = ce_in_regs(logits, dlogits, K, ldl, lddl)
        cap = None if not regs else 1024 if K8 > 10240 else 2048
        vecs = [t for t in (row_lse, row_argmax, row_maxprob) if t is not None]
        stale = f == "ce_rows_past_cap_stale" and cap is not None and M > cap and (dlogits is not None or vecs)
        if stale:
            old = [t[cap:M].clone() for t in vecs]
            old_dl = torch.as_strided(dlogits, (M, K8), (lddl, 1))[cap:].clone() if dlogits is not None else None
        if f == "ce_pad_slots_in_sum" and regs and K % 8 and bool((torch.as_strided(logits, (M, K8), (ldl, 1))[:, K:] > 0).any()):
            super().ce_fwd_bwd(logits, labels, counts, dlogits, loss_out, row_lse, row_argmax, row_maxprob, M, K8, ldl, lddl, grad_scale)
            if dlogits is not None:
                torch.as_strided(dlogits, (M, K8), (lddl, 1))[:, K:].zero_()
            self.applied += 1
            return
        super().ce_fwd_bwd(logits, labels, counts, dlogits, loss_out, row_lse, row_argmax, row_maxprob, M, K, ldl, lddl, grad_scale)
        if f == "ce_tie_highest_index" and row_argmax is not None:
            lg = torch.as_strided(logits, (M, K), (ldl, 1))
            last = (K - 1 - (lg == lg.amax(1, keepdim=True)).flip(1).float().argmax(1)).int()
            if bool((last != row_argmax).any()):
                row_argmax.copy_(last)
                self.applied += 1
        if stale:
            for t, o in zip(vecs, old):
                t[cap:M].copy_(o)
            if dlogits is not None:
                torch.as_strided(dlogits, (M, K8), (lddl, 1))[cap:].copy_(old_dl)
            self.applied += 1
        if f == "store_in_pad_column" and dlogits is not None and lddl > (K8 if regs else K):
            dlogits.view(-1)[K8 if regs else K] = 0
            self.applied += 1

    def embed_bwd(self, dpre, ids, tt, dword, dpos, dtype_tab, B, L, N, order=None, n_types=2):
        super().embed_bwd(dpre, ids, tt, dword, dpos, dtype_tab, B, L, N, order=order, n_types=n_types)
        M = B * L
        d, idf = torch.as_strided(dpre, (M, N), (N, 1)).float(), ids.view(-1)
        hit = False
        if self.fault == "embed_33rd_dropped" and order is not None:
            for tok in idf.unique().tolist():
                rows = (idf == tok).nonzero()[:, 0]              # ascending rows: the order inside the token's run
                if tok != 0 and len(rows) >= 33:
                    dword[tok] -= d[rows[32]]
                    hit = True
        if self.fault == "embed_9th_type_match_dropped" and tt is not None and n_types > 1:
            per = ((M + 3) // 4 + 63) // 64 * 64                 # a wave's quarter of the rows, in 64-row chunks
            ttf = tt.view(-1)
            for t in range(1, n_types):
                for w in range(4):
                    for c0 in range(w * per, min(M, (w + 1) * per), 64):
                        rows = c0 + (ttf[c0:min(c0 + 64, M, (w + 1) * per)] == t).nonzero()[:, 0]
                        if len(rows) >= 9:
                            dtype_tab[t] -= d[rows[8]]
                            hit = True
        self.applied += int(hit)

    def adamw(self, p, g, m, v, p_compute, decay_flags, sumsq, lr_and_steps, n, beta1, beta2, eps, weight_decay, max_norm,
              grad_scale=1.0, chunk_steps=None, zero_grad=False):
        f = self.fault
        kw = dict(grad_scale=grad_scale, chunk_steps=chunk_steps, zero_grad=zero_grad)
        rest = (lr_and_steps, n, beta1, beta2, eps, weight_decay, max_norm)
        state = [t for t in (p, g, m, v, p_compute) if t is not None]
        chunks = n // 256
        if f == "adamw_flags_wrong_chunk" and decay_flags is not None and chunks > 1:
            halves = []
            for h in (0, 1):                  # the flags the first / second 128 elements of every chunk would read
                fl = decay_flags[(2 * torch.arange(chunks) + h) % chunks]
                c = [t.clone() for t in state]
                super().adamw(c[0], c[1], c[2], c[3], c[4] if p_compute is not None else None, fl, sumsq, *rest, **kw)
                halves.append(c)
            first = (torch.arange(n) % 256) < 128
            for i, t in enumerate(state):
                t[:n].copy_(torch.where(first, halves[0][i][:n], halves[1][i][:n]))
            self.applied += 1
            return
        one_pass = 256 * 1024 * 4
        before = [t[one_pass:n].clone() for t in state] if (f == "adamw_second_pass_missing" and n > one_pass) else None
        if f == "adamw_clip_ignores_grad_scale" and max_norm > 0 and sumsq is not None and grad_scale != 1.0:
            honest = min(1.0, max_norm / (math.sqrt(float(sumsq[0])) * grad_scale + 1e-6))
            sumsq = sumsq / grad_scale ** 2
            self.applied += int(min(1.0, max_norm / (math.sqrt(float(sumsq[0])) * grad_scale + 1e-6)) != honest)
        super().adamw(p, g, m, v, p_compute, decay_flags, sumsq, *rest, **kw)
        if before is not None:
            changed = any(not torch.equal(t[one_pass:n], b) for t, b in zip(state, before))
            for t, b in zip(state, before):
                t[one_pass:n].copy_(b)
            self.applied += int(changed)

    def sumsq(self, g, out, n, scratch=None):
        if self.fault == "sumsq_drops_tail" and n & 3:
            n -= n & 3
            self.applied += 1
        prev = out[0].clone()
        super().sumsq(g, out, n, scratch)
        if self.fault == "sumsq_overwrites":
            out[0] -= prev
            self.applied += 1

    def schedule_step(self, step, base_lr, warmup_steps, total_steps, beta1, beta2, lr_and_steps):
        super().schedule_step(step, base_lr, warmup_steps, total_steps, beta1, beta2, lr_and_steps)
        if self.fault == "schedule_off_by_one":
            t = int(step[0])
            f = t / max(1, warmup_steps) if t < warmup_steps else max(0.0, (total_steps - t) / max(1, total_steps - warmup_steps))
            if torch.tensor(base_lr * f, dtype=lr_and_steps.dtype) != lr_and_steps[0]:
                lr_and_steps[0] = base_lr * f
                self.applied += 1


ROW_FAULTS = {
    "ln_stats_padded_width": "layernorm", "ln_last_vector_out_of_variance": "layernorm", "store_in_row_m": "layernorm",
    "second_stage_drops_last_slab": "colsums", "second_stage_stores": "colsums",
    "ce_pad_slots_in_sum": "cross_entropy", "ce_tie_highest_index": "cross_entropy", "ce_rows_past_cap_stale": "cross_entropy",
    "store_in_pad_column": "cross_entropy",
    "embed_33rd_dropped": "embeddings", "embed_9th_type_match_dropped": "embeddings",
    "adamw_flags_wrong_chunk": "optimizer", "adamw_second_pass_missing": "optimizer", "adamw_clip_ignores_grad_scale": "optimizer",
    "sumsq_drops_tail": "optimizer", "sumsq_overwrites": "optimizer", "schedule_off_by_one": "optimizer"}
# reduced sweeps (the faults do not depend on the large shapes, except where a family says so)
ROW_FAULT_SWEEPS = {"layernorm": dict(Ns=(8, 504, 512, 520, 2056), bwd_M=(7,), cap_N=(), dma=()),
                    "colsums": dict(Ms=(1, 127, 129, 16385)),
                    "cross_entropy": dict(Ks=(50, 1003, 4096), big=((2049, 50),)),
                    "embeddings": dict(Ns=(8, 520)),
                    "optimizer": dict(sumsq_n=(1, 3, 4, 1027, 524291))}


@pytest.mark.parametrize("fault", list(ROW_FAULTS))
def test_rowop_edge_cases_reject_plausible_kernel_faults(fault):
    """the same recorder run as the honest pass, over an implementation with one fault: it must fail at EVERY call the fault
    changed (each such call shows the fault on its own), and only there"""
    import test_rowop_edges_bounds_gpu as R
    family = ROW_FAULTS[fault]
    ops = FaultyRowOps(fault)
    rec, n = getattr(R, "run_" + family)(torch.bfloat16, ops=ops, dev="cpu", **ROW_FAULT_SWEEPS[family])
    assert len(rec.checked) + len(rec.failures) == n and ops.applied > 0, (len(rec.checked), len(rec.failures), n, ops.applied)
    print(f"{fault}: applied at {ops.applied} of {n} calls, {len(rec.failures)} failed")
    assert len(rec.failures) == ops.applied, (fault, ops.applied, len(rec.failures), rec.failures[:3])
    word = "outside" if fault.startswith("store_in") else "beyond their bound|differ|not admissible"
    import re
    assert all(re.search(word, f) for f in rec.failures), rec.failures[:3]


class Refused(RuntimeError):
    pass


class RejectingRowOps(HonestRowOps):
    """the argument checks the launchers make before any launch (csrc/rowops.hip CHECK_ROW / DISPATCH_NIT, csrc/optim.hip), restated:
    (-1) XL_ERR_BAD_SHAPE, (-3) XL_ERR_UNALIGNED"""

    def _row(self, what, N, limit=8):
        V = 8 if self.dtype == torch.bfloat16 else 4
        if N <= 0 or N % V:
            raise Refused(f"{what} failed (-1): row length {N} must be a multiple of {V}")
        if -(-N // (64 * V)) > limit:
            raise Refused(f"{what} failed (-1): row length {N} too large")

    def layernorm_fwd(self, x, gamma, beta, y, mean, rstd, M, N, eps):
        self._row("xl_layernorm_fwd", N)
        super().layernorm_fwd(x, gamma, beta, y, mean, rstd, M, N, eps)

    def layernorm_fwd_res(self, x, gamma, beta, y32, y16, mean, rstd, M, N, eps):
        if N <= 0 or N % 4:
            raise Refused(f"xl_layernorm_fwd_res failed (-1): row length {N}")
        if x.data_ptr() % 16 or y32.data_ptr() % 16 or y16.data_ptr() % 8:
            raise Refused("xl_layernorm_fwd_res failed (-3): unaligned rows")
        raise AssertionError("not reached by the rejected family")

    def visn_ln_fwd(self, xv, pos, wbox, bbox, gv, bv, gb, bb, y, mean_v, rstd_v, mean_b, rstd_b, M, N, P, eps):
        self._row("xl_visn_ln_fwd", N)
        if not 1 <= P <= 8:
            raise Refused(f"xl_visn_ln_fwd failed (-1): pos dim {P} not in 1..8")
        super().visn_ln_fwd(xv, pos, wbox, bbox, gv, bv, gb, bb, y, mean_v, rstd_v, mean_b, rstd_b, M, N, P, eps)

    def embed_bwd(self, dpre, ids, tt, dword, dpos, dtype_tab, B, L, N, order=None, n_types=2):
        self._row("xl_embed_bwd", N)
        if N > 1024:
            raise Refused(f"xl_embed_bwd failed (-1): hidden size {N} > 1024")
        super().embed_bwd(dpre, ids, tt, dword, dpos, dtype_tab, B, L, N, order=order, n_types=n_types)

    def adamw(self, p, g, m, v, p_compute, decay_flags, sumsq, lr_and_steps, n, *a, **kw):
        if n <= 0 or n % 256:
            raise Refused(f"xl_adamw failed (-1): n={n} must be a positive multiple of 256")
        if any(t.data_ptr() % 16 for t in (p, g, m, v)):
            raise Refused("xl_adamw failed (-3): unaligned buffer")
        super().adamw(p, g, m, v, p_compute, decay_flags, sumsq, lr_and_steps, n, *a, **kw)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_rowop_rejected_calls_raise_and_write_nothing_over_the_restated_argument_checks(dt):
    import test_rowop_edges_bounds_gpu as R
    R.run_rejected(R.DTYPES[dt], ops=RejectingRowOps(R.DTYPES[dt]), dev="cpu", error=Refused)


# ------------------------------------------------------------------------------------------------------------------ on-chip attention edges
# tests/test_sdpa_edges_bounds_gpu.py over the host restatement of the attention entry points as a kernel stand-in
# (tests/fake_ops_sdpa.SdpaOps): the same calls (tests/sdpa_edge_cases.py), the same recorder, the same label, count, keep_bits and
# outside-view assertions.
BF16, FP32 = torch.bfloat16, torch.float32
SDPA_EDGE_RUNS = {
    **{f"fragments-dh{dh}-{'tr' if tr else 'plain'}": ("run_fragments", (dh, tr), BF16) for dh in (16, 32, 64) for tr in (1, 0)},
    "eligibility-bf16": ("run_eligibility", (BF16,), BF16), "eligibility-fp32": ("run_eligibility", (FP32,), FP32),
    "packed-mfma": ("run_packed", (BF16, "mfma"), BF16), "packed-generic": ("run_packed", (BF16, "generic"), BF16),
    "packed-fp32": ("run_packed", (FP32, "mfma"), FP32),
    "bias_gradients": ("run_bias_gradients", (), BF16), "dropout": ("run_dropout", (), BF16), "extremes": ("run_extremes", (), BF16),
    "attn_probs-bf16": ("run_attn_probs", (BF16,), BF16), "attn_probs-fp32": ("run_attn_probs", (FP32,), FP32)}


@pytest.mark.parametrize("run", list(SDPA_EDGE_RUNS))
def test_sdpa_edge_cases_pass_over_the_host_restatement(run):
    """an honest implementation (fp32 arithmetic on bf16 / fp32 storage; keep_bits in the documented layout; lse of missing queries,
    rows beyond the capacity and everything outside the logical views left alone) is inside every bound at the inputs of the edge
    cases -- the scores of +-60 included -- and every sweep reaches the kernel labels the GPU tests expect"""
    import test_sdpa_edges_bounds_gpu as S
    from fake_ops_sdpa import SdpaOps
    fn, args, dt = SDPA_EDGE_RUNS[run]
    getattr(S, fn)(*args, ops=SdpaOps(dt), dev="cpu")


SHAPES_33 = dict(shapes=((32, 32), (33, 33), (31, 64), (64, 1)))
SDPA_FAULT_RUNS = {
    "key32_dropped": ("run_fragments", (32, 1), BF16, SHAPES_33), "mask_by_length": ("run_packed", (BF16, "mfma"), BF16, {}),
    "mask_255_off": ("run_fragments", (16, 1), BF16, dict(shapes=((32, 32), (33, 33), (31, 64)))), "pad_not_zeroed": ("run_packed", (BF16, "mfma"), BF16, {}),
    "pad_one_row_too_far": ("run_packed", (BF16, "generic"), BF16, {}), "store_next_head": ("run_fragments", (64, 0), BF16, SHAPES_33),
    "lse_missing_query": ("run_packed", (BF16, "mfma"), BF16, {}), "dropout_row_by_length": ("run_packed", (BF16, "mfma"), BF16, {}),
    "step_seed_ignored_bwd": ("run_dropout", (), BF16, {}), "keep_bit_halves_swapped": ("run_dropout", (), BF16, {}),
    "bias_overwritten": ("run_bias_gradients", (), BF16, {}), "bias_stale_pad_row": ("run_bias_gradients", (), BF16, {}),
    "dv_without_dropout_scale": ("run_fragments", (64, 1), BF16, SHAPES_33),
    "delta_second_fragment_lost": ("run_fragments", (32, 0), BF16, SHAPES_33),
    "generic_tail_features_dropped": ("run_eligibility", (BF16,), BF16, {}), "fp32_through_bf16": ("run_eligibility", (FP32,), FP32, {}),
    "round_toward_zero": ("run_eligibility", (BF16,), BF16, {})}


@pytest.mark.parametrize("fault", list(SDPA_FAULT_RUNS))
def test_sdpa_edge_cases_reject_plausible_kernel_faults(fault):
    """the same recorder run as the honest pass, over an implementation with one fault: it must fail at EVERY call the fault
    changed (each such call shows the fault on its own), and only there"""
    import test_sdpa_edges_bounds_gpu as S
    from fake_ops_sdpa import FAULTS, SdpaOps
    assert set(SDPA_FAULT_RUNS) == set(FAULTS)
    fn, args, dt, subset = SDPA_FAULT_RUNS[fault]
    ops = SdpaOps(dt, fault=fault)
    rec, n = getattr(S, fn)(*args, ops=ops, dev="cpu", **subset)
    assert len(rec.checked) + len(rec.failures) == n and ops.applied > 0, (len(rec.checked), len(rec.failures), n, ops.applied)
    print(f"{fault}: applied at {ops.applied} of {n} calls, {len(rec.failures)} failed")
    assert len(rec.failures) == ops.applied, (fault, ops.applied, len(rec.failures), rec.failures[:3])
    import re
    word = "outside" if fault in ("pad_one_row_too_far", "store_next_head", "lse_missing_query") else "beyond their bound|differ|outside"
    assert all(re.search(word, f) for f in rec.failures), rec.failures[:3]


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_sdpa_rejected_calls_raise_and_write_nothing_over_the_restated_argument_checks(dt):
    import test_sdpa_edges_bounds_gpu as S
    from fake_ops_sdpa import Refused, SdpaOps
    S.run_rejected(S.DTYPES[dt], ops=SdpaOps(S.DTYPES[dt], checks=True), dev="cpu", error=Refused)


# ------------------------------------------------------------------------------------------------------------------ predict-tail edges
# tests/test_predict_edges_bounds_gpu.py over the host restatement: the same calls (tests/predict_edge_cases.py), the same recorder,
# the same label, count and outside-view assertions.  The 272-tile shape runs for the XL_EPI_ROWMAX arm only.
def _predict_ops_cls():
    from fake_ops_eval import EvalFakeOps
    from fake_ops_sampling import SamplingFakeOps, first_argmax

    class PredictOps(SamplingFakeOps, EvalFakeOps):
        """FakeOps with the XL_EPI_ROWSAMPLE and the XL_EPI_ROWSCORE branches of gemm and the combines / logits kernels of both (each
        gemm passes an epilogue it does not know on to the next class); XL_EPI_ROWMAX with the documented tie rule spelled out.  alpha
        and a NULL bias are FakeOps.gemm's own: x = alpha acc (+ bias)."""

        def gemm(self, A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr=0, ldx=0, a_kmajor=1, b_kmajor=1, out_f32=False,
                 epilogue=EPI_NONE, alpha=1.0, accumulate=0, p_drop=0.0, seed=0, colsum=None, ws=None):
            if epilogue != BD.EPI_ROWMAX:
                return super().gemm(A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr, ldx, a_kmajor, b_kmajor, out_f32,
                                    epilogue, alpha, accumulate, p_drop, seed, colsum, ws)
            self.calls.append(("gemm", M, N, K, a_kmajor, b_kmajor, epilogue))
            x = alpha * (torch.as_strided(A, (M, K), (lda, 1)).to(self.compute) @ torch.as_strided(B, (N, K), (ldb, 1)).to(self.compute).t())
            if bias is not None:
                x = x + torch.as_strided(bias, (N,), (1,)).to(self.compute)[None, :]
            n_seg = N // 64
            xs = x.view(M, n_seg, 64)
            loc = first_argmax(xs)
            mx = xs.amax(-1)
            rec = aux.view(-1)[:n_seg * M * 4].view(n_seg, M, 4)
            rec[..., 0].copy_(mx.t())
            rec[..., 1].copy_(torch.exp(xs - mx[..., None]).sum(-1).t())
            rec.view(torch.int32)[..., 2].copy_((loc + torch.arange(n_seg)[None, :] * 64).to(torch.int32).t())
            rec[..., 3].zero_()
    return PredictOps


PREDICT_EDGE_RUNS = {"fused": ("run_fused", {}), "rounds-two_rounds": ("run_rounds", dict(tail=False, epis=(BD.EPI_ROWMAX,))),
                     "rounds-tail_split": ("run_rounds", dict(tail=True, epis=(BD.EPI_ROWMAX,))),
                     **{f"switches-{sw}": ("run_switches", dict(sw=sw)) for sw in ("mfma_128_only", "duo_everywhere", "wgrad_slabs")},
                     "combines": ("run_combines", {}), "logits": ("run_logits", {})}


@pytest.mark.parametrize("run", list(PREDICT_EDGE_RUNS))
def test_predict_edge_cases_pass_over_the_host_restatement(run):
    """an honest implementation (fp32 arithmetic on bf16 storage that reads the logical extents only and stores into the logical
    views only) is inside every bound at the inputs of the edge cases, the ambiguity cap holds at every launch (asserted inside the
    case module), and every sweep reaches the kernel labels the GPU tests expect"""
    import test_predict_edges_bounds_gpu as P
    fn, kw = PREDICT_EDGE_RUNS[run]
    ops = _predict_ops_cls()(torch.bfloat16)
    if fn == "run_switches":
        kw = dict(kw, ops_default=_predict_ops_cls()(torch.bfloat16))
    getattr(P, fn)(ops=ops, dev="cpu", **kw)


def _last_argmax(z):
    n = z.shape[-1]
    return n - 1 - (z.flip(-1) == z.amax(-1, keepdim=True)).to(torch.uint8).argmax(-1)


def _faulty_predict_ops(fault):
    """the host restatement of the predict tail with ONE kernel fault, applied at every call it can apply to (`applied` counts the
    calls it changed):
      pad_as_k_term                         the leading-dimension pad element behind the last row of A enters as one more K term
      ragged_k_tile_dropped                 the last, ragged K tile (K % 64 of a K above 64) is dropped
      alpha_ignored_by_rowmax               XL_EPI_ROWMAX computes acc + bias
      bias_of_first_column_tile_everywhere  every column tile adds the bias of columns 0 .. 255
      tie_to_higher_column                  an exact tie inside a segment (a row of logits in memory) goes to the higher column
      tie_to_later_segment_in_combine       equal maxima of two segments: the combine keeps the later segment's column
      label_truncated_to_32_bits            the epilogue cuts a label to its low 32 bits (2^32 + 5 becomes column 5)
      labels_of_row_m_plus_64_swapped       the two quads of a wave's 128 rows take each other's labels
      second_row_tile_reads_first_tiles_labels   labels[m % 256]
      pad_column_label_counted_valid        the combine accepts a label below 64 n_seg instead of below n_cols
      noise_row_local_to_tile               the noise function is given the row inside the tile
      noise_column_local_to_segment         the noise function is given the column inside the segment
      rows_past_grid_cap_skipped            the scores kernels stop at 1024 blocks: later rows are neither written nor counted
      totals_ticket_not_reset               a ticket set is left at its last count: its second launch never finds a last block
      record_stored_past_aux                one record lands behind the (N / 64) M records of aux"""
    Base = _predict_ops_cls()
    from fake_ops_sampling import EPI_ROWSAMPLE, gumbel_noise
    from fake_ops_eval import EPI_ROWSCORE
    ROW = (BD.EPI_ROWMAX, EPI_ROWSAMPLE, EPI_ROWSCORE)

    class FaultyPredictOps(Base):
        def __init__(self):
            super().__init__(torch.bfloat16)
            self.fault, self.applied, self.totals_launches, self._in_gemm = fault, 0, 0, False

        def _g(self, seed, M, cols, device):
            rows = torch.arange(M, device=device)
            if self._in_gemm and self.fault == "noise_row_local_to_tile":
                rows = rows % 256
            if self._in_gemm and self.fault == "noise_column_local_to_segment":
                cols = cols % 64
            return gumbel_noise(seed, rows[:, None], cols[None, :], self.compute, self.noise)

        def gemm(self, A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr=0, ldx=0, a_kmajor=1, b_kmajor=1, out_f32=False,
                 epilogue=EPI_NONE, alpha=1.0, accumulate=0, p_drop=0.0, seed=0, colsum=None, ws=None):
            f = self.fault
            assert epilogue in ROW
            n_seg = N // 64
            if f == "pad_as_k_term" and lda > K:
                A2 = torch.zeros(M, K + 1, dtype=A.dtype)
                A2[:, :K] = torch.as_strided(A, (M, K), (lda, 1))
                A2[M - 1, K] = A[(M - 1) * lda + K]
                B2 = torch.zeros(N, K + 1, dtype=B.dtype)
                B2[:, :K] = torch.as_strided(B, (N, K), (ldb, 1))
                B2[:, K] = B2[:, K - 1]
                A, B, K, lda, ldb = A2.reshape(-1), B2.reshape(-1), K + 1, K + 1, K + 1
                self.applied += 1
            if f == "ragged_k_tile_dropped" and K > 64 and K % 64:
                K -= K % 64
                self.applied += 1
            if f == "alpha_ignored_by_rowmax" and epilogue == BD.EPI_ROWMAX and alpha != 1.0:
                alpha = 1.0
                self.applied += 1
            if f == "bias_of_first_column_tile_everywhere" and bias is not None and N > 256:
                bias = torch.as_strided(bias, (256,), (1,)).repeat(N // 256)
                self.applied += 1
            if epilogue == EPI_ROWSCORE:
                lab = residual.reshape(-1)[:M].clone()
                if f == "label_truncated_to_32_bits":
                    lab = ((lab & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000
                if f == "labels_of_row_m_plus_64_swapped":
                    lab = lab.view(M // 128, 2, 64).flip(1).reshape(-1)
                if f == "second_row_tile_reads_first_tiles_labels":
                    lab = lab[torch.arange(M) % 256]
                self.applied += int(not torch.equal(lab, residual.reshape(-1)[:M]))
                residual = lab
            self._in_gemm = True
            self.applied += int(epilogue == EPI_ROWSAMPLE and ((f == "noise_row_local_to_tile" and M > 256)
                                                               or (f == "noise_column_local_to_segment" and N > 64)))
            super().gemm(A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr, ldx, a_kmajor, b_kmajor, out_f32, epilogue, alpha,
                         accumulate, p_drop, seed, colsum, ws)
            self._in_gemm = False
            if f == "tie_to_higher_column" and epilogue != EPI_ROWSAMPLE:
                x = alpha * (torch.as_strided(A, (M, K), (lda, 1)).float() @ torch.as_strided(B, (N, K), (ldb, 1)).float().t())
                if bias is not None:
                    x = x + torch.as_strided(bias, (N,), (1,))[None, :]
                idx = (_last_argmax(x.view(M, n_seg, 64)) + torch.arange(n_seg)[None, :] * 64).to(torch.int32).t()
                slot = aux.view(-1)[:n_seg * M * 4].view(n_seg, M, 4).view(torch.int32)[..., 2]
                self.applied += int(not torch.equal(slot, idx))
                slot.copy_(idx)
            if f == "record_stored_past_aux":
                torch.as_strided(aux, (4,), (1,), aux.storage_offset() + n_seg * M * 4).fill_(1.0)
                self.applied += 1

        def _later_segment(self, ws, n_seg, M, out):
            if self.fault != "tie_to_later_segment_in_combine" or out is None:
                return
            rec = ws.view(-1)[:n_seg * M * 4].view(n_seg, M, 4)
            mx, idx = rec[..., 0], rec.view(torch.int32)[..., 2]
            last = torch.where(mx == mx.amax(0)[None, :], idx, torch.full_like(idx, -1)).amax(0)
            self.applied += int(not torch.equal(out[:M], last))
            out[:M].copy_(last)

        def rowmax_combine(self, ws, n_seg, M, row_maxprob, row_argmax, row_lse=None):
            super().rowmax_combine(ws, n_seg, M, row_maxprob, row_argmax, row_lse)
            self._later_segment(ws, n_seg, M, row_argmax)

        def _totals(self, totals):
            """the ticket fault: the launch whose ticket set was used before never sees a last block -- totals stay as they are"""
            if totals is None:
                return None
            self.totals_launches += 1
            if self.fault == "totals_ticket_not_reset" and self.totals_launches > 8:
                self.applied += 1
                return None
            return totals

        def rowscore_combine(self, ws, n_seg, M, labels, n_cols, row_nll=None, row_pred=None, row_max=None, totals=None):
            f = self.fault
            totals = self._totals(totals)
            if f == "pad_column_label_counted_valid" and labels is not None:
                lab = labels.reshape(-1)[:M]
                if bool(((lab >= n_cols) & (lab < 64 * n_seg)).any()):
                    n_cols = 64 * n_seg
                    self.applied += 1
            if f == "rows_past_grid_cap_skipped" and M > 64 * 1024:
                assert n_seg == 1
                M = 64 * 1024
                self.applied += 1
            super().rowscore_combine(ws, n_seg, M, labels, n_cols, row_nll, row_pred, row_max, totals)
            self._later_segment(ws, n_seg, M, row_pred)

        def score_rows(self, logits, M, K, ldl, labels, row_nll=None, row_pred=None, row_max=None, totals=None):
            totals = self._totals(totals)
            if self.fault == "rows_past_grid_cap_skipped" and M > 4 * 1024:
                M = 4 * 1024
                self.applied += 1
            super().score_rows(logits, M, K, ldl, labels, row_nll, row_pred, row_max, totals)
            if self.fault == "tie_to_higher_column" and row_pred is not None:
                last = _last_argmax(torch.as_strided(logits, (M, K), (ldl, 1)))
                self.applied += int(not torch.equal(row_pred[:M].long(), last))
                row_pred[:M].copy_(last)
    return FaultyPredictOps()


PREDICT_FAULTS = {
    "pad_as_k_term": ("fused",), "ragged_k_tile_dropped": ("fused",), "alpha_ignored_by_rowmax": ("fused",),
    "bias_of_first_column_tile_everywhere": ("fused",), "tie_to_higher_column": ("fused", "logits"),
    "tie_to_later_segment_in_combine": ("fused", "combines"), "label_truncated_to_32_bits": ("fused",),
    "labels_of_row_m_plus_64_swapped": ("fused",), "second_row_tile_reads_first_tiles_labels": ("fused",),
    "pad_column_label_counted_valid": ("fused", "combines"), "noise_row_local_to_tile": ("fused",),
    "noise_column_local_to_segment": ("fused",), "rows_past_grid_cap_skipped": ("combines", "logits"),
    "totals_ticket_not_reset": ("combines",), "record_stored_past_aux": ("fused",)}
PREDICT_FAULT_SWEEPS = {"fused": dict(shapes=None), "combines": dict(strict=False), "logits": dict(Ks=(2, 65))}


@pytest.mark.parametrize("fault", list(PREDICT_FAULTS))
def test_predict_edge_cases_reject_plausible_kernel_faults(fault):
    """the same recorder runs as the honest pass, over an implementation with one fault: it must fail at EVERY call the fault
    changed (each such call shows the fault on its own), and only there"""
    import re
    import predict_edge_cases as PE
    import test_predict_edges_bounds_gpu as P
    for family in PREDICT_FAULTS[fault]:
        ops = _faulty_predict_ops(fault)
        kw = dict(PREDICT_FAULT_SWEEPS[family])
        if family == "fused":
            kw["shapes"] = PE.FUSED_SHAPES
        rec, n = getattr(P, "run_" + family)(ops=ops, dev="cpu", **kw)
        assert len(rec.checked) + len(rec.failures) == n and ops.applied > 0, (family, len(rec.checked), len(rec.failures), n, ops.applied)
        print(f"{fault} / {family}: applied at {ops.applied} of {n} calls, {len(rec.failures)} failed")
        assert len(rec.failures) == ops.applied, (fault, family, ops.applied, len(rec.failures), rec.failures[:3])
        word = "outside" if fault == "record_stored_past_aux" else "beyond their bound|differ|not admissible|count|correct|candidate"
        assert all(re.search(word, f) for f in rec.failures), rec.failures[:3]


class RejectingPredictOps:
    """the argument checks xl_gemm makes for the three row-reducing epilogues, and those of the combines and logits kernels, restated
    (csrc/gemm.hip, csrc/rowops.hip): (-1) XL_ERR_BAD_SHAPE, (-5) XL_ERR_BAD_ARG.  Nothing is computed: every call of the rejected
    family must be refused."""

    def __init__(self, dtype):
        self.dtype, self.tr_read = dtype, True

    def set_lds_transpose_read(self, enable):
        self.tr_read = bool(enable)

    def workspace_floats(self, N):
        return 256 * 10 * N

    @staticmethod
    def _al(t, k=16):
        return t is not None and t.data_ptr() % k == 0

    def gemm(self, A, B, C, bias, residual, aux, M, N, K, lda, ldb, ldc, ldr=0, ldx=0, a_kmajor=1, b_kmajor=1, out_f32=False,
             epilogue=EPI_NONE, alpha=1.0, accumulate=0, p_drop=0.0, seed=0, colsum=None, ws=None):
        assert epilogue in (5, 9, 10) and M > 0 and N > 0 and K > 0
        ok = (self.dtype == torch.bfloat16 and A.dtype == torch.bfloat16 and a_kmajor and b_kmajor and M % 256 == 0 and N % 256 == 0
              and K % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0 and self._al(aux) and self._al(A) and self._al(B)
              and (bias is None or self._al(bias)) and not accumulate and colsum is None and self.tr_read)
        if epilogue in (9, 10):
            ok = ok and p_drop == 0
        if epilogue == 10:
            ok = ok and self._al(residual, 8)
        if not ok:
            raise Refused(f"xl_gemm failed (-1): the row-reducing epilogue {epilogue} takes bf16 K-major operands with M, N multiples of 256")
        raise AssertionError("not reached by the rejected family")

    def _combine(self, what, ws, n_seg, M, n_cols=1):
        if not (ws is not None and n_seg > 0 and M > 0 and self._al(ws) and 0 < n_cols <= 64 * n_seg):
            raise Refused(f"{what} failed (-5): bad args")
        raise AssertionError("not reached by the rejected family")

    def rowmax_combine(self, ws, n_seg, M, row_maxprob, row_argmax, row_lse=None):
        self._combine("xl_rowmax_combine", ws, n_seg, M)

    def rowsample_combine(self, ws, n_seg, M, seed, row_prob, row_id, row_lse=None):
        self._combine("xl_rowsample_combine", ws, n_seg, M)

    def rowscore_combine(self, ws, n_seg, M, labels, n_cols, row_nll=None, row_pred=None, row_max=None, totals=None):
        self._combine("xl_rowscore_combine", ws, n_seg, M, n_cols)

    def score_rows(self, logits, M, K, ldl, labels, row_nll=None, row_pred=None, row_max=None, totals=None):
        if not (logits is not None and M > 0 and K > 0 and ldl >= K):
            raise Refused(f"xl_score_rows failed (-5): M={M} K={K} ldl={ldl}")
        raise AssertionError("not reached by the rejected family")

    def sample_rows(self, logits, M, K, ldl, inv_T, seed, row_prob, row_id, row_lse=None):
        if not (logits is not None and M > 0 and K > 0 and ldl >= K and 0 < inv_T < math.inf):
            raise Refused(f"xl_sample_rows failed (-5): M={M} K={K} ldl={ldl} inv_T={inv_T}")
        raise AssertionError("not reached by the rejected family")


def test_predict_rejected_calls_raise_and_write_nothing_over_the_restated_argument_checks():
    import test_predict_edges_bounds_gpu as P
    P.run_rejected(ops=RejectingPredictOps(torch.bfloat16), ops_f32=RejectingPredictOps(torch.float32), dev="cpu", error=Refused)
