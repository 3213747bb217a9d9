"""Per-element error bounds of the bf16 kernels against a float64 restatement (tests/fake_ops.FakeOps(dtype, torch.float64)).

Every function returns a tensor `bound` of the output's shape such that a correct kernel satisfies |got - ref| <= bound element by
element, `ref` being the float64 value of the same operation on the same (bf16 / fp32) inputs.  The terms and where they come from:

  u_out       unit roundoff of the output format: bf16 2^-8, fp32 2^-24 (round to nearest even: |fl(x) - x| <= u |x|)
  K U32 |A||B| fp32 accumulation of a K-deep contraction in ANY summation order (MFMA chains, split-K slices, slabs, tree
              reductions: every product is exact in fp32 -- 8 x 8 mantissa bits -- and every term passes through at most K-1
              fp32 additions, Higham's gamma_{K-1} <= K u).  K_eff = K unless a function says otherwise.
  U16 |X||Y|  one term per intermediate operand that a kernel rounds to bf16 BY DESIGN (attention P and dS between MFMAs)
  ERF_ABS     the Abramowitz-Stegun 7.1.26 erf of csrc/common.h (<= 1.5e-7 absolute) plus its fp32 evaluation: one v_rcp_f32 (1 ulp)
              raised to the 5th power in the polynomial, one v_exp_f32 (2 ulp), eight fma/mul roundings: <= 16 U32 absolute
  Lipschitz   max |gelu'| = 1.1289 (at x = sqrt 2), max |gelu''| = 2 phi(0) = 0.798, |tanh'| <= 1
  TINY        2^-126: flush of fp32 denormals to zero

SLACK = 2 multiplies every term that is NOT the final rounding of the output (first-order derivations, MFMA internals); the final
rounding term u_out |ref| is never scaled, so that a wrong rounding mode (round toward zero: up to 2 u_out) stays visible.
"""
import math

import torch

U16 = 2.0 ** -8
U32 = 2.0 ** -24
TINY = 2.0 ** -126
SLACK = 2.0
ERF_ABS = 1.5e-7 + 16 * U32
GELU_L1 = 1.13
GELU_L2 = 0.80

EPI_NONE, EPI_GELU, EPI_RESIDUAL, EPI_DGELU, EPI_TANH, EPI_ROWMAX, EPI_GELU_DG, EPI_MULAUX = 0, 1, 2, 3, 4, 5, 6, 7


def unit(dtype):
    """unit roundoff of a storage type"""
    return {torch.bfloat16: U16, torch.float32: U32, torch.float64: 0.0}[dtype]


def check(got, ref, bound, what):
    """assert |got - ref| <= bound element by element; returns the worst ratio |err| / bound (the headroom is 1 / ratio).
    Equal values (also equal infinities) are an error of 0.  On failure: how many elements failed, the worst one (index, got,
    ref, bound) and the worst ratio."""
    got, ref = got.double(), ref.double()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=ref.device).expand_as(ref)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = torch.where(got == ref, torch.zeros_like(ref), (got - ref).abs())
    err = torch.nan_to_num(err, nan=math.inf)
    ratio = err / bound.clamp(min=1e-300)
    if ratio.numel() == 0:
        return 0.0
    worst = int(ratio.reshape(-1).argmax())
    r = float(ratio.reshape(-1)[worst])
    bad = int((err > bound).sum())
    if bad:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ref.shape))
        raise AssertionError(f"{what}: {bad} of {ref.numel()} elements beyond their bound; worst at {idx}: got "
                             f"{float(got.reshape(-1)[worst]):.9g}, ref {float(ref.reshape(-1)[worst]):.9g}, bound "
                             f"{float(bound.reshape(-1)[worst]):.3g}, |err|/bound {r:.3g}")
    return r


def check_exact(got, ref, what):
    """integer, index and mask outputs"""
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bad = got != ref
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements differ; first at flat {i}: got "
                             f"{got.reshape(-1)[i].item()}, ref {ref.reshape(-1)[i].item()}")
    return 0.0


# ------------------------------------------------------------------------------------------------------------------ contractions
def gemm_bounds(pre, absprod, K, epilogue, out_dtype, ref_c, aux_in=None, ref_aux=None, keep=None, aux_dtype=torch.bfloat16):
    """xl_gemm.  pre = alpha A B^T + bias in float64 (the argument of the epilogue), absprod = |alpha| |A| |B|^T + |bias|.

    Contraction: the fp32 accumulator differs from pre by e = K U32 absprod (K_eff = K: the MFMA chain, the tail split's K
    slices and the slab / split-K partial tiles only re-associate the same K products) + 2 U32 |pre| (alpha, bias).
    Epilogue, first order in e:
      NONE / accumulate   C = pre (+ C_prev)                 e
      GELU                aux = pre (rounded);  C = gelu(pre) 1.13 e + 0.5 |pre| ERF_ABS + 4 U32 |pre|   (A-S erf; the scalar
                          path of ragged tiles uses erff, more accurate: the same bound holds)
      RESIDUAL            C = keep * pre + res               keep e + U32 (|keep pre| + |C|)  (keep = 0 or the fp32 1/(1-p))
      DGELU               C = pre gelu'(aux)                  1.13 e + |pre| (ERF_ABS + 4 U32)  (gelu' = Phi + x phi: Phi carries
                          half the erf error, x phi(x) <= 0.25 times 4 U32 of exp / rounding)
      GELU_DG             aux = gelu'(pre) (rounded);  C = gelu(pre)   aux: 0.80 e + ERF_ABS + 4 U32
      TANH                C = tanh(pre)                       e + 4 U32 |C|   (tanhf: 2 ulp, one multiply)
      MULAUX              C = pre aux                         |aux| e + U32 |C|
    Each output: u_out |ref| + SLACK * (the term above) + TINY.  Returns (bound of C, bound of aux or None)."""
    e = K * U32 * absprod + 2 * U32 * pre.abs()
    ap = pre.abs()
    b_aux = None
    if epilogue == EPI_GELU:
        t = GELU_L1 * e + 0.5 * ap * ERF_ABS + 4 * U32 * ap
        b_aux = unit(aux_dtype) * ref_aux.abs() + SLACK * e + TINY
    elif epilogue == EPI_RESIDUAL:
        k = keep if keep is not None else 1.0
        t = k * e + U32 * (k * ap + ref_c.abs())
    elif epilogue == EPI_DGELU:
        t = GELU_L1 * e + ap * (ERF_ABS + 4 * U32)
    elif epilogue == EPI_GELU_DG:
        t = GELU_L1 * e + 0.5 * ap * ERF_ABS + 4 * U32 * ap
        b_aux = unit(aux_dtype) * ref_aux.abs() + SLACK * (GELU_L2 * e + ERF_ABS + 4 * U32) + TINY
    elif epilogue == EPI_TANH:
        t = e + 4 * U32 * ref_c.abs()
    elif epilogue == EPI_MULAUX:
        t = aux_in.abs() * e + U32 * ref_c.abs()
    else:
        t = e
    return unit(out_dtype) * ref_c.abs() + SLACK * t + TINY, b_aux


def colsum_bound(elem_bound, stored_ref, prev_ref=None):
    """fused / separate column sums of C over M rows into fp32: the sum of the stored values differs from the sum of the
    references by at most sum_m bound[m, n]; the fp32 sum adds (M + 1) U32 sum_m |C[m, n]| (K_eff = M + 1: partial slabs per
    64 rows, their combine and the += into the target only re-associate).  SLACK on the accumulation term."""
    M = stored_ref.shape[0]
    acc = (M + 1) * U32 * stored_ref.abs().sum(0)
    if prev_ref is not None:
        acc = acc + U32 * prev_ref.abs()
    return elem_bound.sum(0) + SLACK * acc + TINY


def sum_bound(terms_abs_sum, n_terms, ref, out_dtype=torch.float32):
    """any fp32 sum of n_terms exact terms (embedding-table gradients, masked column sums, the step's sum of squares): K_eff =
    n_terms; u_out |ref| for the final store."""
    return unit(out_dtype) * ref.abs() + SLACK * n_terms * U32 * terms_abs_sum + TINY


# ------------------------------------------------------------------------------------------------------------------ attention
def attention_parts(Q, K, V, valid, keep, scale):
    """float64 pieces of one attention core in the dense [B, H, n, dh] layout: scores s, probabilities P (0 on invalid keys),
    P' = P keep (dropout), |P'| |V|, and the per-row score error e_S = dh U32 scale max_k |q||k| + U32 max_k |s_k - max s|
    (the fp32 QK^T chain plus the rounding of exp's argument)."""
    s = (Q @ K.transpose(-1, -2)) * scale
    s = s.masked_fill(~valid, -math.inf)
    P = torch.softmax(s, -1).nan_to_num(0.0)
    Pk = P * keep
    sabs = (Q.abs() @ K.abs().transpose(-1, -2)) * abs(scale)
    sv = s.masked_fill(~valid, 0.0)
    mx = s.amax(-1, keepdim=True).nan_to_num(0.0, neginf=0.0)
    rng = ((sv - mx).abs() * valid).amax(-1, keepdim=True)
    eS = Q.shape[-1] * U32 * (sabs * valid).amax(-1, keepdim=True) + U32 * rng
    return s, P, Pk, eS


def sdpa_fwd_bounds(Q, K, V, valid, keep, scale, O_ref, lse_ref):
    """xl_sdpa_fwd (sdpa_fwd_mfma).  P' = softmax(s) keep is rounded to bf16 before the PV MFMA (design: U16 |P'||V|).  A score
    error e_S moves every p_j by at most p_j (|ds_j| + sum_k p_k |ds_k|) <= 2 e_S p_j; exp (v_exp_f32, 2 ulp), 1/sum (1 ulp) and
    the nk-deep fp32 sum add (nk + 4) U32 relative to the row.  So
        |dO| <= U16 |O| + SLACK (U16 + 2 e_S + (nk + 4) U32) |P'| |V|.
    lse = max + log(sum): e_S + (nk + 4) U32 + 2 U32 |lse| + 2^-21 (__logf on a sum in [1, nk])."""
    nk = K.shape[-2]
    _, P, Pk, eS = attention_parts(Q, K, V, valid, keep, scale)
    pv = Pk.abs() @ V.abs()
    bO = U16 * O_ref.abs() + SLACK * (U16 + 2 * eS + (nk + 4) * U32) * pv + TINY
    lse_f = lse_ref.nan_to_num(0.0, neginf=0.0)
    bl = SLACK * (eS[..., 0] + (nk + 4) * U32 + 2 * U32 * lse_f.abs() + 2.0 ** -21)
    return bO, bl


def sdpa_bwd_bounds(Q, K, V, dO, valid, keep, scale, lse, dQ_ref, dK_ref, dV_ref):
    """xl_sdpa_bwd (sdpa_bwd_mfma).  P = exp(s - lse) from the saved lse (the reference uses the same lse): e_P = e_S + 2 U32 +
    U32 |s - lse| relative.  dP = dO V^T (dh-deep: dh U32 |dO||V|^T), times keep.  delta = sum_k P dP': nk-deep.
    dS = P (dP' - delta) scale, |err| <= scale (e_P P |dP' - delta| + P (|ddP| + |ddelta|)) + 3 U32 |dS|, then rounded to bf16
    (design: U16 |dS|).  With |dS_err| the sum of both:
        dV = P'^T dO   U16 |dV| + SLACK (U16 + e_P + (nq + 2) U32) |P'|^T |dO|            (P' rounded to bf16 by design)
        dQ = dS K      U16 |dQ| + SLACK (|dS_err| |K| + nk U32 |dS| |K|)
        dK = dS^T Q    U16 |dK| + SLACK (|dS_err|^T |Q| + nq U32 |dS|^T |Q|)
    Returns the three bounds and the per-element fp32 error terms (without the final rounding) for the fused bias sums."""
    nq, nk, dh = Q.shape[-2], K.shape[-2], Q.shape[-1]
    s = (Q @ K.transpose(-1, -2)) * scale
    P = torch.exp(s - lse[..., None]).masked_fill(~valid, 0.0).nan_to_num(0.0, posinf=0.0)
    sabs = (Q.abs() @ K.abs().transpose(-1, -2)) * abs(scale)
    eP = dh * U32 * sabs + 2 * U32 + U32 * (s - lse[..., None]).abs().masked_fill(~valid, 0.0).nan_to_num(0.0, posinf=0.0)
    dP = (dO @ V.transpose(-1, -2)) * keep
    edP = dh * U32 * (dO.abs() @ V.abs().transpose(-1, -2)) * keep
    delta = (P * dP).sum(-1, keepdim=True)
    edelta = (eP * P * dP.abs() + P * edP).sum(-1, keepdim=True) + nk * U32 * (P * dP.abs()).sum(-1, keepdim=True)
    dS = P * (dP - delta) * scale
    edS = abs(scale) * (eP * P * (dP - delta).abs() + P * (edP + edelta)) + 3 * U32 * dS.abs() + U16 * dS.abs()
    Pk = (P * keep).abs()
    tV = (U16 + eP.amax(-2, keepdim=True).transpose(-1, -2) + (nq + 2) * U32) * (Pk.transpose(-1, -2) @ dO.abs())
    tQ = edS @ K.abs() + nk * U32 * (dS.abs() @ K.abs())
    tK = edS.transpose(-1, -2) @ Q.abs() + nq * U32 * (dS.abs().transpose(-1, -2) @ Q.abs())
    return ((U16 * dQ_ref.abs() + SLACK * tQ + TINY, U16 * dK_ref.abs() + SLACK * tK + TINY, U16 * dV_ref.abs() + SLACK * tV + TINY),
            (tQ, tK, tV))


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd_bounds(x, gamma, y_ref, mean_ref, rstd_ref, out_dtype, x_err=None):
    """xl_layernorm_fwd and the LayerNorm halves of xl_visn_ln_fwd / xl_embed_ln_fwd: two-pass statistics in fp32 over N columns.
    mean: N U32 mean|x| + U32 |mean|.  var = mean((x - mean)^2): (N + 3) U32 relative (a mean error d adds d^2 only);
    rstd = 1 / sqrt(var + eps): half of that + 3 U32 (sqrt, rcp: 1 ulp each).
    y = (x - mean) rstd g + b:  |g| rstd (e_mean + |x - mean| (e_rstd + 3 U32)) + U32 |y|, and, when the input itself carries an
    error x_err (a box projection computed in fp32), |g| rstd 2 max|x_err|.  Returns bounds of y, mean, rstd."""
    N = x.shape[-1]
    e_mean = N * U32 * x.abs().mean(-1, keepdim=True) + U32 * mean_ref.abs()[:, None]
    e_rstd = 0.5 * (N + 3) * U32 + 3 * U32
    xc = (x - mean_ref[:, None]).abs()
    t = gamma.abs() * rstd_ref[:, None] * (e_mean + xc * (e_rstd + 3 * U32)) + U32 * y_ref.abs()
    if x_err is not None:
        t = t + gamma.abs() * rstd_ref[:, None] * 2 * x_err.amax(-1, keepdim=True)
    by = unit(out_dtype) * y_ref.abs() + SLACK * t + TINY
    return by, SLACK * e_mean[:, 0] + TINY, SLACK * e_rstd * rstd_ref.abs() + TINY


def ln_bwd_bounds(dy, x, gamma, mean, rstd, dx_ref, out_dtype, x_err=None):
    """xl_layernorm_bwd (plain / DMA kernels; the DMA variant's weight-gradient slabs re-associate the same column sums).
    xh = (x - mean) rstd (2 U32 relative), gd = g dy, c1 = mean(gd), c2 = mean(gd xh): N-deep fp32 sums.
    dx = rstd (gd - c1 - xh c2):  rstd (N U32 mean|gd| + |xh| (N U32 mean|gd xh| + 2 U32 mean|gd xh|) + 2 U32 |xh| |c2|) + 4 U32 |dx|.
    dgamma += sum_m dy xh, dbeta += sum_m dy: M-deep fp32 (K_eff = M + 1, slabs included) + 2 U32 |dy xh| from xh.
    An input that carries an error x_err (the fp32 box projection of xl_visn_ln_bwd) moves xh by dxh = 2 rstd max|x_err|:
    rstd (dxh |c2| + |xh| mean|gd| dxh) more in dx, sum_m |dy| dxh more in dgamma.
    Returns bounds of dx (and its per-element fp32 term, for the dropped copy and the bias sum), dgamma, dbeta."""
    N, M = x.shape[-1], x.shape[0]
    xh = (x - mean[:, None]) * rstd[:, None]
    gd = gamma * dy
    c2 = (gd * xh).mean(-1, keepdim=True)
    t = rstd.abs()[:, None] * (N * U32 * gd.abs().mean(-1, keepdim=True)
                               + xh.abs() * ((N + 2) * U32 * (gd * xh).abs().mean(-1, keepdim=True) + 2 * U32 * c2.abs())) \
        + 4 * U32 * dx_ref.abs()
    tg = (M + 3) * U32 * (dy * xh).abs().sum(0)
    if x_err is not None:
        dxh = 2 * rstd.abs()[:, None] * x_err.amax(-1, keepdim=True)
        t = t + rstd.abs()[:, None] * (dxh * c2.abs() + xh.abs() * gd.abs().mean(-1, keepdim=True) * dxh)
        tg = tg + (dy.abs() * dxh).sum(0)
    bdx = unit(out_dtype) * dx_ref.abs() + SLACK * t + TINY
    bdg = SLACK * tg + TINY
    bdb = SLACK * ((M + 1) * U32 * dy.abs().sum(0)) + TINY
    return bdx, t, bdg, bdb


# ------------------------------------------------------------------------------------------------------------------ elementwise
def scaled_copy_bound(ref, out_dtype):
    """dropout / cast: one fp32 multiply by an fp32 scale, then the store: u_out |ref| + SLACK U32 |ref|"""
    return unit(out_dtype) * ref.abs() + SLACK * U32 * ref.abs() + TINY


def gelu_bwd_bound(dy, pre, ref, out_dtype):
    """xl_gelu_bwd: dy gelu'(pre) with the A-S erf: |dy| (ERF_ABS + 4 U32) + U32 |ref|, then the store"""
    return unit(out_dtype) * ref.abs() + SLACK * (dy.abs() * (ERF_ABS + 4 * U32) + U32 * ref.abs()) + TINY


def tanh_bwd_bound(dy, y, ref, out_dtype):
    """xl_tanh_bwd: dy (1 - y^2): 3 fp32 roundings"""
    return unit(out_dtype) * ref.abs() + SLACK * 3 * U32 * (dy.abs() * (1 + y * y)) + TINY


# ------------------------------------------------------------------------------------------------------------------ losses
def ce_bounds(logits, valid, grad_scale_over_cnt, lse_ref, dl_ref, out_dtype):
    """xl_ce_fwd_bwd over K classes.  lse = max + log(sum_k exp(x_k - max)): U32 |max| + (K + 4) U32 + 2 U32 |lse| + 2^-21 (the
    argument x - max of each exp is rounded: U32 |x - max| relative in that p_k, <= U32 * range).  p_k = exp(x_k - lse):
    p_k (e_lse + U32 |x_k - lse| + 2 U32).  dlogits = (p - onehot) grad_scale / count: |scale| (that) + U32 |ref|, then the store.
    Returns bounds of the row lse and of dlogits."""
    K = logits.shape[-1]
    mx = logits.amax(-1, keepdim=True)
    e_lse = U32 * mx.abs() + (K + 4) * U32 + 2 * U32 * lse_ref.abs()[:, None] + U32 * (logits - mx).abs().amax(-1, keepdim=True) \
        + 2.0 ** -21
    p = torch.exp(logits - lse_ref[:, None])
    ep = p * (e_lse + U32 * (logits - lse_ref[:, None]).abs() + 2 * U32)
    bdl = unit(out_dtype) * dl_ref.abs() + SLACK * (abs(grad_scale_over_cnt) * valid[:, None] * ep + U32 * dl_ref.abs()) + TINY
    return SLACK * e_lse[:, 0] + TINY, bdl


def ce_loss_bound(logits, labels, valid, cnt, lse_bound_rows, loss_ref):
    """loss += sum_rows valid (lse - x_label) / count: the rows' lse bounds plus an M-deep fp32 sum of the terms"""
    M = logits.shape[0]
    nll = (lse_bound_rows + U32 * logits.abs().amax(-1)) * valid
    terms = (logits.logsumexp(-1) - logits.gather(1, labels.clamp(min=0)[:, None])[:, 0]).abs() * valid
    return SLACK * ((nll.sum() + (M + 2) * U32 * terms.sum()) / cnt) + U32 * abs(loss_ref) + TINY


def featloss_bounds(pred, target, w, F, dref, loss_ref, out_dtype):
    """xl_featloss_fwd_bwd: d = pred - target (exact in fp32 for bf16 inputs up to one rounding: U32 |d|), SmoothL1 per element
    (3 U32), row mean over F (F-deep) times the weight w, sum over rows (M-deep).  dpred = grad_scale w / F clamp(d, -1, 1): three
    multiplies (3 U32), then the store."""
    M = pred.shape[0]
    d = (pred - target).abs()
    sl1 = torch.where(d < 1, 0.5 * d * d, d - 0.5)
    loss_b = SLACK * ((F + M + 6) * U32 * (w.abs()[:, None] * sl1).sum() / F) + U32 * abs(loss_ref) + TINY
    return loss_b, unit(out_dtype) * dref.abs() + SLACK * 4 * U32 * dref.abs() + TINY


# ------------------------------------------------------------------------------------------------------------------ optimizer
def sumsq_bound(g, ref, threads=512 * 256):
    """xl_sumsq: every thread accumulates ~n / (16 threads) squares serially into four registers (4 squares per 16-byte load), then
    the 256-thread block tree (8 levels) and the <= 512 block partials (9 levels) and the += into out: K_eff = n / (4 threads) + 24.
    Squares: one rounding (U32 g^2)."""
    n = g.numel()
    k_eff = n // (4 * threads) + 24
    return U32 * abs(ref) + SLACK * (k_eff + 1) * U32 * float((g.double() ** 2).sum()) + TINY


def adamw_bounds(p_ref, m_ref, v_ref, g, m0, v0, step, clip, beta1, beta2, eps, lr, wd):
    """xl_adamw in fp32 (everything below is relative to the float64 values on the same inputs):
      gg = g clip            clip = min(1, max_norm / (sqrt(sumsq) grad_scale + 1e-6)): 4 U32 (sqrt, add, div, mul)
      m = b1 m0 + (1-b1) gg   U32 (b1 |m0| + (1-b1) |gg| (5 + 1) + b1 |gg|) + U32 |m|
      v = b2 v0 + (1-b2) gg^2  U32 (b2 |v0| + (1-b2) gg^2 (2 * 5 + 2) + b2 gg^2) + U32 |v|
          (the betas reach the kernel as fp32: 1 - fl(b) is off by up to U32 b absolute, i.e. U32 b / (1 - b) relative -- 6e-5
          for b2 = 0.999, measured 1.3e-5 -- hence the b |gg| and b gg^2 terms)
      upd = step m / (sqrt(v) + eps): step (lr sqrt(1 - b2^t) / (1 - b1^t) in fp32: 4 U32), m, sqrt (1/2 of v's + 1 U32), add, div
            (v_rcp + mul: 2 U32) -> |upd| (4 + e_m + e_v / 2 + 5) U32-relative
      p = p0 - upd - lr wd p': |upd| and |lr wd p| errors plus 3 U32 |p|.
    Returns bounds of p, m, v."""
    gg = (g * clip).abs()
    em = U32 * (beta1 * m0.abs() + (1 - beta1) * gg * 6 + beta1 * gg) + U32 * m_ref.abs()
    ev = U32 * (beta2 * v0.abs() + (1 - beta2) * gg * gg * 12 + beta2 * gg * gg) + U32 * v_ref.abs()
    sv = v_ref.sqrt()
    den = sv + eps
    upd = (step * m_ref / den).abs()
    rel_v = ev / v_ref.abs().clamp(min=1e-300)
    rel_den = (0.5 * rel_v * sv + 2 * U32 * sv) / den
    e_upd = upd * (9 * U32 + rel_den) + (step / den).abs() * em
    ep = e_upd + 3 * U32 * p_ref.abs() + abs(lr * wd) * 2 * U32 * p_ref.abs()
    return U32 * p_ref.abs() + SLACK * ep + TINY, U32 * m_ref.abs() + SLACK * em + TINY, U32 * v_ref.abs() + SLACK * ev + TINY


# ------------------------------------------------------------------------------------------------------------------ layouts
def attention_inputs(ref, q, k, v, key_mask, B, H, nq, nk, dh, ldq, ldk, ldv, p_drop, seed, q_off=None, k_off=None):
    """the dense [B, H, n, dh] operands of one attention core as the restatement reads them (packed sides unpacked), the
    valid (query, key) pairs and the dropout keep scale (1.0 without dropout).  `ref` is the float64 FakeOps."""
    (Q, qv), (K, kv), (V, _) = (ref._load(t, B, n, H, dh, ld, off)
                                for t, n, ld, off in ((q, nq, ldq, q_off), (k, nk, ldk, k_off), (v, nk, ldv, k_off)))
    valid = torch.ones(B, 1, nq, nk, dtype=torch.bool, device=Q.device)
    if key_mask is not None:
        valid &= key_mask.reshape(-1)[:B * nk].view(B, 1, 1, nk) != 0
    if kv is not None:
        valid &= kv.view(B, 1, 1, nk)
    if qv is not None:
        valid &= qv.view(B, 1, nq, 1)
    keep = ref._pmask(B, H, nq, nk, p_drop, ref._seed(seed), Q.device) if p_drop > 0 else 1.0
    return Q, K, V, valid, keep


def attention_rows(ref, t, B, n, H, dh, ld, off, pad):
    """[rows, H*dh] view of a q- or k-side output buffer: B*n dense rows, or max(pad, off[B]) packed rows"""
    rows = B * n if off is None else max(int(pad), int(off.reshape(-1)[B]))
    return torch.as_strided(t, (rows, H * dh), (ld, 1))


def attention_scatter(ref, dense, B, n, H, dh, ld, off, pad):
    """a dense [B, H, n, dh] tensor (a bound) laid out as the output buffer is: rows beyond an example's length get 0"""
    rows = B * n if off is None else max(int(pad), int(off.reshape(-1)[B]))
    dst = torch.zeros(rows * ld + H * dh, dtype=torch.float64, device=dense.device)
    ref._store(dst, dense, B, n, H, dh, ld, off, pad)
    return attention_rows(ref, dst, B, n, H, dh, ld, off, pad)
