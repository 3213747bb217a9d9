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


def score_range(s, valid):
    """max_k |s_k - max s| over the valid keys of every query row (0 for a row without one): attention_parts' `rng`"""
    mx = s.amax(-1, keepdim=True).nan_to_num(0.0, neginf=0.0)
    return ((s.masked_fill(~valid, 0.0) - mx).abs() * valid).amax(-1, keepdim=True)


def blocked_rescale_error(n_blk, rng):
    """relative error that the online softmax of sdpa_fwd_flash / sdpa_fwd_long adds to every term of the running sum and of the
    output accumulators.  Key block i multiplies both by corr_i = __expf(m_{i-1} - m_i) (m the running maximum; corr = 0 exactly
    while no key has been seen, 1 exactly while the maximum stays): the subtraction and the log2 e scaling of the argument round
    once each (2 U32 |m_{i-1} - m_i| relative to corr_i), v_exp_f32 EXP_ULP, the multiply 1.  The running maximum only rises and
    ends at max s, starting from a valid score, so sum_i |m_{i-1} - m_i| <= rng = max_k |s_k - max s|.  A term passes at most
    n_blk - 1 rescales:   (n_blk - 1) (EXP_ULP + 1) U32 + 2 U32 rng."""
    return (n_blk - 1) * (EXP_ULP + 1) * U32 + 2 * U32 * rng


def sdpa_fwd_bounds(Q, K, V, valid, keep, scale, O_ref, lse_ref, n_kblk=1, out_dtype=torch.bfloat16, arith="mfma"):
    """xl_sdpa_fwd (sdpa_fwd_mfma).  P' = softmax(s) keep is rounded to bf16 before the PV MFMA (design: U16 |P'||V|).  A score
    error e_S moves every p_j by at most p_j (|ds_j| + sum_k p_k |ds_k|) <= 2 e_S p_j; exp (v_exp_f32, 2 ulp), 1/sum (1 ulp) and
    the nk-deep fp32 sum add (nk + 4) U32 relative to the row.  So
        |dO| <= U16 |O| + SLACK (U16 + 2 e_S + (nk + 4) U32) |P'| |V|.
    lse = max + log(sum): e_S + (nk + 4) U32 + 2 U32 |lse| + 2^-21 (__logf on a sum in [1, nk]).

    n_kblk > 1: the kernels that walk the keys in n_kblk = ceil(nk / 64) blocks (sdpa_fwd_flash; the plain sdpa_fwd_long is the
    same algorithm with one key per step, fp32 throughout and P not rounded to bf16: it stays inside this bound).  What changes:
      * the un-normalised P~ = exp(s - m_running) keep is what is rounded to bf16, relative to the RUNNING maximum: the same
        relative U16 per term, and the later rescales are common factors of the term -- U16 |P'||V| as before;
      * the rounding of exp's argument s - m_running is U32 |s - m_running| <= U32 rng: e_S has it;
      * every term of the sum and of the accumulators carries r = blocked_rescale_error(n_kblk, rng); numerator and denominator of
        O = acc / sum each move by r relative to |P'||V|:  2 r |P'||V|;
      * O^T += V^T P^T is an fp32 MFMA chain over all nk keys carried across the blocks, and the division by the sum is one
        multiply of the accumulator at the end:  (nk + 1) U32 |P'||V|;
      * lse = m + __logf(sum) with the sum accumulated (and rescaled) across the blocks:  + r.
    With n_kblk = 1 none of these terms exists and the result is the on-chip bound, bit for bit.

    out_dtype, arith: the storage type of O and the arithmetic of the kernel.  The defaults (bf16, "mfma") are the bound above, bit
    for bit.  arith = "fp32" is sdpa_fwd_generic<T> (one lane per query, T = bf16 or fp32): a score is a serial dh-deep fmaf chain
    (one rounding per step: the dh U32 |q||k| of e_S, also for fp32 operands, whose products an fma does not round), expf (2 ulp
    like v_exp_f32 or better), a serial nk-deep sum and ONE division -- the (nk + 4) U32 of the row; P is NOT rounded to bf16: the
    designed U16 |P'||V| is replaced by the serial nk-deep fmaf chain of O = P' V, nk U32 |P'||V| (the multiply by 1 / sum and by
    the keep scale are inside the + 4); the store rounds once to the output format, u_out |O| (fp32: 2^-24).  lse has no bf16
    term: unchanged (logf instead of __logf is the more accurate one)."""
    nk = K.shape[-2]
    assert arith in ("mfma", "fp32"), arith
    u_out, u_p = unit(out_dtype), (U16 if arith == "mfma" else nk * U32)
    s, P, Pk, eS = attention_parts(Q, K, V, valid, keep, scale)
    pv = Pk.abs() @ V.abs()
    bO = u_out * O_ref.abs() + SLACK * (u_p + 2 * eS + (nk + 4) * U32) * pv + TINY
    lse_f = lse_ref.nan_to_num(0.0, neginf=0.0)
    bl = SLACK * (eS[..., 0] + (nk + 4) * U32 + 2 * U32 * lse_f.abs() + 2.0 ** -21)
    if n_kblk > 1:
        assert n_kblk == (nk + 63) // 64, (n_kblk, nk)
        r = blocked_rescale_error(n_kblk, score_range(s, valid))
        bO = bO + SLACK * (2 * r + (nk + 1) * U32) * pv
        bl = bl + SLACK * r[..., 0]
    return bO, bl


def sdpa_bwd_bounds(Q, K, V, dO, valid, keep, scale, lse, dQ_ref, dK_ref, dV_ref, n_kblk=1, n_qblk=1, out_dtype=torch.bfloat16,
                    arith="mfma"):
    """xl_sdpa_bwd (sdpa_bwd_mfma).  P = exp(s - lse) from the saved lse (the reference uses the same lse): e_P = e_S + 2 U32 +
    U32 |s - lse| relative.  dP = dO V^T (dh-deep: dh U32 |dO||V|^T), times keep.  delta = sum_k P dP': nk-deep.
    dS = P (dP' - delta) scale, |err| <= scale (e_P P |dP' - delta| + P (|ddP| + |ddelta|)) + 3 U32 |dS|, then rounded to bf16
    (design: U16 |dS|).  With |dS_err| the sum of both:
        dV = P'^T dO   U16 |dV| + SLACK (U16 + e_P + (nq + 2) U32) |P'|^T |dO|            (P' rounded to bf16 by design)
        dQ = dS K      U16 |dQ| + SLACK (|dS_err| |K| + nk U32 |dS| |K|)
        dK = dS^T Q    U16 |dK| + SLACK (|dS_err|^T |Q| + nq U32 |dS|^T |Q|)
    Returns the three bounds and the per-element fp32 error terms (without the final rounding) for the fused bias sums.

    n_kblk, n_qblk > 1: the two-launch backward of the long path (sdpa_bwd_flash_q over n_kblk = ceil(nk / 64) key blocks,
    sdpa_bwd_flash_k over n_qblk = ceil(nq / 64) query blocks; sdpa_bwd_long_q / _k are the same sums one key / query per step,
    fp32 throughout: inside this bound).  Term by term:
      * P = __expf(s scale - lse) is recomputed per block, in both launches, from the same saved lse by the same expression: e_P
        as above, nothing accumulates across blocks;
      * delta: a lane sums its 32 products of a block serially, adds the block's partial to its running delta (n_kblk additions)
        and the two half-waves combine once.  Every product still passes fewer than nk additions (32 + n_kblk + 1 <= nk for
        nk > 64), but the partials are additions outside any one chain, so the bound counts them:  K_eff = nk + n_kblk + 1.
        delta reaches the key-side launch through an fp32 workspace: exact;
      * dQ^T += K^T dS^T over the key blocks, dK^T += Q^T dS and dV^T += dO^T P~ over the query blocks: MFMA accumulators carried
        in fp32 across the blocks, depth nk resp. nq -- the terms above already have these depths (rows of a partial block
        beyond the length are exact zeros); n_qblk adds nothing and is accepted so that a caller states the geometry;
      * dS and P~ are rounded to bf16 per block exactly as on chip: U16 |dS|, U16 |P'|.
    With both counts 1 the result is the on-chip bound, bit for bit.

    out_dtype, arith: as in sdpa_fwd_bounds; the defaults give the bound above, bit for bit.  arith = "fp32" is sdpa_bwd_generic<T>:
    s and dP are serial dh-deep fmaf chains (dh U32, as above), P = expf(s scale - lse) (e_P as above), delta a serial nk-deep sum
    (K_eff = nk), dS = P (dP' - delta) scale in fp32 (the 3 U32 |dS|) and NOT rounded to bf16, P' = P keep likewise: both designed
    U16 terms drop out.  dQ is a serial nk-deep fmaf chain (nk U32 |dS||K|); dK and dV are sums of nq products each, gathered by
    atomic adds in LDS in whatever order the lanes arrive -- any order is inside nq U32 |dS|^T|Q| resp. (nq + 2) U32 |P'|^T|dO|,
    a product rounds once before it is added (inside the + 2 and SLACK).  The store rounds once: u_out |ref|."""
    nq, nk, dh = Q.shape[-2], K.shape[-2], Q.shape[-1]
    assert n_kblk >= 1 and n_qblk >= 1
    assert arith in ("mfma", "fp32"), arith
    u_out, u_mid = unit(out_dtype), (U16 if arith == "mfma" else 0.0)
    if n_kblk > 1 or n_qblk > 1:
        assert n_kblk == (nk + 63) // 64 and n_qblk == (nq + 63) // 64, (n_kblk, nk, n_qblk, nq)
    k_delta = nk if n_kblk == 1 else nk + n_kblk + 1
    s = (Q @ K.transpose(-1, -2)) * scale
    P = torch.exp(s - lse[..., None]).masked_fill(~valid, 0.0).nan_to_num(0.0, posinf=0.0)
    sabs = (Q.abs() @ K.abs().transpose(-1, -2)) * abs(scale)
    eP = dh * U32 * sabs + 2 * U32 + U32 * (s - lse[..., None]).abs().masked_fill(~valid, 0.0).nan_to_num(0.0, posinf=0.0)
    dP = (dO @ V.transpose(-1, -2)) * keep
    edP = dh * U32 * (dO.abs() @ V.abs().transpose(-1, -2)) * keep
    delta = (P * dP).sum(-1, keepdim=True)
    edelta = (eP * P * dP.abs() + P * edP).sum(-1, keepdim=True) + k_delta * U32 * (P * dP.abs()).sum(-1, keepdim=True)
    dS = P * (dP - delta) * scale
    edS = abs(scale) * (eP * P * (dP - delta).abs() + P * (edP + edelta)) + 3 * U32 * dS.abs() + u_mid * dS.abs()
    Pk = (P * keep).abs()
    tV = (u_mid + eP.amax(-2, keepdim=True).transpose(-1, -2) + (nq + 2) * U32) * (Pk.transpose(-1, -2) @ dO.abs())
    tQ = edS @ K.abs() + nk * U32 * (dS.abs() @ K.abs())
    tK = edS.transpose(-1, -2) @ Q.abs() + nq * U32 * (dS.abs().transpose(-1, -2) @ Q.abs())
    return ((u_out * dQ_ref.abs() + SLACK * tQ + TINY, u_out * dK_ref.abs() + SLACK * tK + TINY, u_out * dV_ref.abs() + SLACK * tV + TINY),
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


def adamw_chunk_step(lr, beta1, beta2, t):
    """xl_adamw with chunk_steps: the step size of a chunk at its own update count t >= 1,
        step = lr sqrt(1 - b2^t) / (1 - b1^t),    b^t = exp2f(t log2f(b)) in fp32  (csrc/optim.hip adamw_kernel).
    Error of b^t, relative: t U32 (b reaches the kernel as fp32: (b (1 + d))^t), ln 2 |t log2 b| 3 U32 (log2f 2 ulp and the
    multiply by t move the exponent of exp2f absolutely), EXP_ULP U32 (exp2f).  THE CANCELLATION TERM: 1 - b^t divides that absolute
    error by 1 - b^t -- 1000 x at b2 = 0.999, t = 1 -- and adds its own rounding U32.  step: half of b2's, all of b1's, and 4 U32
    (sqrt, two multiplies / divides, lr).  Returns (float64 step per element, its relative error per element)."""
    t = t.double()
    rel = torch.zeros_like(t)
    for b, w in ((beta1, 1.0), (beta2, 0.5)):
        bt = b ** t
        e_pow = bt * (t * U32 + math.log(2.0) * (t * abs(math.log2(b))) * 3 * U32 + EXP_ULP * U32)
        rel = rel + w * (e_pow / (1.0 - bt) + U32)
    step = lr * torch.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    return step, rel + 4 * U32


def ln_bwd_bias_bound(t, dx_ref, prev, ref):
    """dbias_prev += column sums of dx (of the dropped dx with dropout): the kernel adds the fp32 value BEFORE its store, so a
    summand carries its fp32 term t only (ln_bwd_bounds' t; with dropout keep t + U32 |dx_dropped| for the multiply by the keep
    scale), no output rounding; M-deep fp32 sum through slabs or atomics (K_eff = M + 1) and the += ."""
    M = dx_ref.shape[0]
    return SLACK * t.sum(0) + SLACK * (M + 1) * U32 * (dx_ref.abs().sum(0) + prev.abs()) + U32 * ref.abs() + TINY


def adamw_bounds(p_ref, m_ref, v_ref, g, m0, v0, step, clip, beta1, beta2, eps, lr, wd, step_rel=0.0):
    """xl_adamw in fp32 (everything below is relative to the float64 values on the same inputs):
      gg = g clip            clip = min(1, max_norm / (sqrt(sumsq) grad_scale + 1e-6)): 4 U32 (sqrt, add, div, mul)
      m = b1 m0 + (1-b1) gg   U32 (b1 |m0| + (1-b1) |gg| (5 + 1) + b1 |gg|) + U32 |m|
      v = b2 v0 + (1-b2) gg^2  U32 (b2 |v0| + (1-b2) gg^2 (2 * 5 + 2) + b2 gg^2) + U32 |v|
          (the betas reach the kernel as fp32: 1 - fl(b) is off by up to U32 b absolute, i.e. U32 b / (1 - b) relative -- 6e-5
          for b2 = 0.999, measured 1.3e-5 -- hence the b |gg| and b gg^2 terms)
      upd = step m / (sqrt(v) + eps): step (lr sqrt(1 - b2^t) / (1 - b1^t) in fp32: 4 U32), m, sqrt (1/2 of v's + 1 U32), add, div
            (v_rcp + mul: 2 U32) -> |upd| (4 + e_m + e_v / 2 + 5) U32-relative
      p = p0 - upd - lr wd p': |upd| and |lr wd p| errors plus 3 U32 |p|.
    step may be a tensor (one step size per element: chunk_steps) with the relative error step_rel of adamw_chunk_step.
    Returns bounds of p, m, v."""
    gg = (g * clip).abs()
    em = U32 * (beta1 * m0.abs() + (1 - beta1) * gg * 6 + beta1 * gg) + U32 * m_ref.abs()
    ev = U32 * (beta2 * v0.abs() + (1 - beta2) * gg * gg * 12 + beta2 * gg * gg) + U32 * v_ref.abs()
    sv = v_ref.sqrt()
    den = sv + eps
    upd = (step * m_ref / den).abs()
    rel_v = ev / v_ref.abs().clamp(min=1e-300)
    rel_den = (0.5 * rel_v * sv + 2 * U32 * sv) / den
    e_upd = upd * (9 * U32 + rel_den + step_rel) + (step / den).abs() * em
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


# ------------------------------------------------------------------------------------------------------------------ sampler head
# Transcendental constants (not derivable; the places this file already takes them from): v_exp_f32 2 ulp (ERF_ABS above, as in
# sdpa_fwd_bounds), v_rcp_f32 / an IEEE division 1 ulp (csrc/common.h, the comment at the A-S erf's __builtin_amdgcn_rcpf),
# logf / __logf on a sum >= 1: 2 U32 |log| + 2^-21 (ce_bounds).  __expf(x) is v_exp_f32(x log2 e): the scaling of the argument
# rounds once more, U32 |x| relative to the result.
EXP_ULP = 2.0
RCP_ULP = 1.0
LOG_ABS = 2.0 ** -21


def rowmax_logit_error(pre, absdot, bias_abs, K):
    """per-logit error e of the XL_EPI_ROWMAX accumulator, as gemm_bounds has it: K U32 (|alpha||A||B|^T + |bias|) + 2 U32 |pre| --
    except where the contraction has no non-zero product (absdot == 0: an all-zero operand row, the zero rows that pad the
    codebook): 0 alpha + bias is exact there, e = 0.  So a padded column (bias -1e30) carries no error allowance at all."""
    e = K * U32 * (absdot + bias_abs) + 2 * U32 * pre.abs()
    return torch.where(absdot == 0, torch.zeros_like(e), e)


def rowmax_record_bounds(pre, e):
    """records of the XL_EPI_ROWMAX epilogue, aux[(n/64) M + m] = {max, sum exp(x - max), argmax bits, 0} per row and 64-column
    segment; pre [M, N] float64 logits (bias added), e from rowmax_logit_error.  With E = max of e over the segment:
      max       the maximum of perturbed values is within the largest perturbation of the true maximum: SLACK E + U32 |max|
      sum exp   every exponent x_n - max moves by at most 2 E (first order: 2 E relative in that term); its rounding and the
                __expf scaling add 2 U32 t_n, t_n = max - x_n, relative in the term (the partial maxima of the 8-column lanes and
                of the three butterfly levels telescope to the same t_n); four exp (4 EXP_ULP U32), three multiplies and <= 11
                additions on a term's way to the segment sum: (4 EXP_ULP + 14) U32.  Sum over the terms w_n = exp(-t_n):
                U32 sum + SLACK ((2 E + (4 EXP_ULP + 14) U32) sum + 2 U32 sum_n t_n w_n)
    A padded column has t_n = 1e30 next to any real column: w_n = 0 exactly, in the reference and -- exp underflows -- in fp32.
    Returns (ref max, ref sum, E, bound of max, bound of sum), each [M, N / 64]."""
    M, N = pre.shape
    x, ee = pre.view(M, N // 64, 64), e.view(M, N // 64, 64)
    mx, E = x.amax(-1), ee.amax(-1)
    t = mx[..., None] - x
    w = torch.exp(-t)
    sm = w.sum(-1)
    b_max = SLACK * E + U32 * mx.abs() + TINY
    b_sum = U32 * sm + SLACK * ((2 * E + (4 * EXP_ULP + 14) * U32) * sm + 2 * U32 * (t * w).sum(-1)) + TINY
    return mx, sm, E, b_max, b_sum


def argmax_admissible(x, got, E):
    """the admissible-argmax rule, no position exempted.  x [R, n] float64 logits of R rows (a 64-column segment or a whole row),
    got [R] indices into the n columns, E [R] the largest logit error of the row.  An index is admissible iff
        0 <= got < n  and  x[got] >= max x - 2 SLACK E
    (the kernel's value of the true maximum and of its own choice are each within SLACK E of the float64 ones), and, where the
    row is exact (E == 0: ties of exact values, the documented rule), iff it is the LOWEST index of the maximum.
    A padded column (-1e30, e = 0) is 1e30 below any real one: never admissible beside a real column.
    Returns the bool [R] of admissible rows and the number of admissible columns per row (the rule's sharpness)."""
    R, n = x.shape
    g = got.long()
    inside = (g >= 0) & (g < n)
    mx = x.amax(-1)
    thr = mx - 2 * SLACK * E
    val = x.gather(1, g.clamp(0, n - 1)[:, None])[:, 0]
    ok = inside & (val >= thr)
    first = (x == mx[:, None]).double().argmax(-1)
    ok = torch.where(E == 0, inside & (g == first), ok)
    return ok, (x >= thr[:, None]).sum(-1)


def check_admissible(x, got, E, what):
    ok, n_adm = argmax_admissible(x, got, E)
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        g = int(got[i])
        v = float(x[i, g]) if 0 <= g < x.shape[1] else float("nan")
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} argmax indices not admissible; first at row {i}: got "
                             f"index {g} (logit {v:.9g}), row maximum {float(x[i].max()):.9g} at {int(x[i].argmax())}, "
                             f"acceptance width {float(2 * SLACK * E[i]):.3g}")
    return n_adm


def rowmax_combine_bounds(mx, se, n_seg):
    """xl_rowmax_combine on the kernel's OWN records mx, se [n_seg, M] (float64 copies of the fp32 values): gmx = max_s mx (exact),
    tot = sum_s se_s exp(mx_s - gmx).  A segment's term passes through at most n_seg merges (each: one exp of its running factor,
    one multiply, one addition: (EXP_ULP + 2) U32) and its exponents telescope to d_s = gmx - mx_s (2 U32 d_s: subtraction and
    __expf scaling):  |dtot| <= n_seg (EXP_ULP + 3) U32 tot + 2 U32 sum_s d_s se_s exp(-d_s).
      row_lse = gmx + log(tot)   U32 |lse| + SLACK (dtot / tot + 2 U32 |log tot| + LOG_ABS)
      row_maxprob = 1 / tot      U32 |p| + SLACK p (dtot / tot + RCP_ULP U32)
    Returns (ref lse, ref maxprob, bound of lse, bound of maxprob, dtot / tot)."""
    gmx = mx.amax(0)
    d = gmx[None, :] - mx
    term = se * torch.exp(-d)
    tot = term.sum(0)
    rel = n_seg * (EXP_ULP + 3) * U32 + 2 * U32 * (d * term).sum(0) / tot
    lse, p = gmx + torch.log(tot), 1.0 / tot
    b_lse = U32 * lse.abs() + SLACK * (rel + 2 * U32 * torch.log(tot).abs() + LOG_ABS) + TINY
    b_p = U32 * p + SLACK * p * (rel + RCP_ULP * U32) + TINY
    return lse, p, b_lse, b_p, rel


def rowmax_composed_bounds(pre, e, n_seg):
    """GEMM epilogue + combine against the float64 logits of the whole row: a perturbation of every logit by at most E_row = max_n
    e moves the log-sum-exp by at most E_row and the largest probability exp(max - lse) by at most 2 E_row relative; the fp32
    arithmetic of both kernels adds r = (n_seg (EXP_ULP + 3) + 4 EXP_ULP + 14) U32 + 4 U32 sum_n t_n w_n / sum_n w_n  (t_n = max -
    x_n, w_n = exp(-t_n): the terms' exponent roundings of rowmax_record_bounds and rowmax_combine_bounds together):
      row_lse      U32 |lse| + SLACK (E_row + r + 2 U32 |lse - max| + LOG_ABS) + U32 |max|
      row_maxprob  U32 p + SLACK p (2 E_row + r + RCP_ULP U32)
    Returns (ref lse, ref maxprob, E_row, bound of lse, bound of maxprob)."""
    mx = pre.amax(-1)
    E = e.amax(-1)
    t = mx[:, None] - pre
    w = torch.exp(-t)
    tot = w.sum(-1)
    r = (n_seg * (EXP_ULP + 3) + 4 * EXP_ULP + 14) * U32 + 4 * U32 * (t * w).sum(-1) / tot
    lse, p = mx + torch.log(tot), 1.0 / tot
    b_lse = U32 * lse.abs() + SLACK * (E + r + 2 * U32 * torch.log(tot).abs() + LOG_ABS) + U32 * mx.abs() + TINY
    b_p = U32 * p + SLACK * p * (2 * E + r + RCP_ULP * U32) + TINY
    return lse, p, E, b_lse, b_p


# ------------------------------------------------------------------------------------------------------------------ BCE
def bce_bounds(x, t, M, N, dl_ref, loss_ref, loss_prev, out_dtype):
    """xl_bce_logits_fwd_bwd on fp32 logits x and soft targets t [M, N], scale = 1 / (M N) (fp32: 2 U32 relative).
    e = __expf(-|x|): (EXP_ULP + |x|) U32 relative; sigma = 1 / (1 + e) (x >= 0) or e / (1 + e): d sigma / sigma = (1 - sigma) de / e
    in both branches, plus the addition and the division (2 + RCP_ULP) U32:
      dlogits = (sigma - t) scale    u_out |ref| + SLACK scale (sigma (1 - sigma) (EXP_ULP + |x|) U32 + 3 U32 sigma) + SLACK 4 U32 |ref|
                (the subtraction, the scale and its own rounding: 4 U32); columns N .. ld_dlogits are exactly 0 (bound TINY)
      loss += scale sum_mn l,  l = max(x, 0) - x t + log1p(e) >= 0: every term carries U32 (2 max(x, 0) + 2 |x t| + 4 log1p(e)) +
                (EXP_ULP + |x|) U32 e of its own (the pieces may cancel: absolute, not relative to l), and the sum of the M N
                terms in any order is sum_bound(sum l, M N): wave and block trees, one fp32 atomic per row.
    Returns the bounds of dlogits [M, N] and of the loss."""
    sg = torch.sigmoid(x)
    e = torch.exp(-x.abs())
    scale = 1.0 / (M * N)
    b_dl = unit(out_dtype) * dl_ref.abs() + SLACK * scale * (sg * (1 - sg) * (EXP_ULP + x.abs()) * U32 + 3 * U32 * sg) \
        + SLACK * 4 * U32 * dl_ref.abs() + TINY
    l = x.clamp(min=0) - x * t + torch.log1p(e)
    l_err = U32 * (2 * x.clamp(min=0) + 2 * (x * t).abs() + 4 * torch.log1p(e)) + (EXP_ULP + x.abs()) * U32 * e
    b_loss = sum_bound(float(l.abs().sum()) * scale, M * N, torch.as_tensor(float(loss_ref), dtype=torch.float64)) \
        + SLACK * scale * float(l_err.sum()) + SLACK * 2 * U32 * abs(float(loss_ref)) + U32 * abs(float(loss_prev))
    return b_dl, float(b_loss)


# ------------------------------------------------------------------------------------------------------------------ attn_probs
def attn_probs_bound(Q, K, V_unused, valid, keep, scale, lse, ref, n_kblk=1):
    """xl_attn_probs: probs = exp(s - lse) keep from the forward's saved lse (the reference reads the same lse), fp32 out, a serial
    dh-deep fma chain per score.  With attention_parts' per-row score error e_S (the dh-deep contraction and the rounding of the
    exponent) every probability moves by p (e_S + U32 |s - lse| (subtraction + expf scaling: 2) + EXP_ULP U32), the dropout scale
    is one more multiply:  U32 |ref| + SLACK |ref| (e_S + 2 U32 |s - lse| + (EXP_ULP + 2) U32).
    No bf16 rounding of P here: the designed U16 |P'| of sdpa_fwd_bounds belongs to the PV MFMA, which this kernel does not have.
    Invalid pairs (masked keys, rows / keys beyond a packed example's length) are exactly 0.
    n_kblk = ceil(nk / 64) > 1 (long sequences): attn_probs_kernel is one lane per query with the keys in a serial loop -- no
    running maximum, no rescale, no state carried from one key to the next -- and the lse it reads is the one the reference
    reads, whichever forward kernel wrote it.  No term depends on the block count; it is accepted (and checked against nk) so that
    the caller states the geometry it ran."""
    assert n_kblk == 1 or n_kblk == (K.shape[-2] + 63) // 64, (n_kblk, K.shape[-2])
    s, _, _, eS = attention_parts(Q, K, Q[..., :1, :], valid, keep, scale)
    arg = (s - lse[..., None]).abs().masked_fill(~valid, 0.0).nan_to_num(0.0, posinf=0.0)
    return U32 * ref.abs() + SLACK * ref.abs() * (eS + 2 * U32 * arg + (EXP_ULP + 2) * U32) + TINY


# ------------------------------------------------------------------------------------------------------------------ sampler checks
# The comparisons themselves, shared by the host proofs (tests/test_bounds_cpu.py) and the recorder of the GPU tests: each returns
# [(output name, worst |err| / bound)] and raises on the first output beyond its bound.
def rowmax_records(aux, n_seg, M):
    """the fp32 record buffer as (max, sum exp) in float64 and the argmax (an int32 bit pattern in the third float) as int64"""
    rec = aux.reshape(-1)[:n_seg * M * 4].view(n_seg, M, 4)
    assert rec.dtype == torch.float32
    return rec[..., 0].double(), rec[..., 1].double(), rec[..., 2].contiguous().view(torch.int32).long(), rec[..., 3]


def check_rowmax_records(aux, pre, e, what="gemm ROWMAX"):
    """every record of the epilogue against the float64 logits pre [M, N]: max, sum exp, an admissible segment argmax (global
    column index), the fourth float 0.  Returns the rows of the headroom table and the admissible-column counts [M, n_seg]."""
    M, N = pre.shape
    n_seg = N // 64
    mx, se, idx, zero = rowmax_records(aux, n_seg, M)
    ref_mx, ref_se, E, b_mx, b_se = rowmax_record_bounds(pre, e)
    res = [("max", check(mx.t(), ref_mx, b_mx, f"{what} segment max")),
           ("sum exp", check(se.t(), ref_se, b_se, f"{what} segment sum exp"))]
    local = idx.t() - torch.arange(n_seg, device=idx.device)[None, :] * 64
    n_adm = check_admissible(pre.reshape(M * n_seg, 64), local.reshape(-1), E.reshape(-1), f"{what} segment argmax")
    res.append(("argmax admissible", 0.0))
    res.append(("pad float", check_exact(zero, torch.zeros_like(zero), f"{what} fourth float")))
    return res, n_adm.view(M, n_seg)


def check_rowmax_rows(pre, e, n_seg, got_p, got_idx, got_lse, what="ROWMAX + combine"):
    """the composed result of epilogue and combine against the float64 logits: admissible row argmax, row_lse, row_maxprob.
    Returns the table rows and the admissible-column count per row."""
    lse, p, E, b_lse, b_p = rowmax_composed_bounds(pre, e, n_seg)
    n_adm = check_admissible(pre, got_idx, E, f"{what} row argmax")
    res = [("row argmax admissible", 0.0)]
    if got_p is not None:
        res.append(("row_maxprob", check(got_p, p, b_p, f"{what} row_maxprob")))
    if got_lse is not None:
        res.append(("row_lse", check(got_lse, lse, b_lse, f"{what} row_lse")))
    return res, n_adm


def check_rowmax_combine(ref_ops, ws, n_seg, M, got_p, got_idx, got_lse, what="rowmax_combine"):
    """xl_rowmax_combine on the records `ws` it read (fp32, the kernel's own) against ref_ops.rowmax_combine in float64: the argmax
    exact (lowest index among the segments that hold the global maximum), row_lse and row_maxprob within rowmax_combine_bounds"""
    dev = ws.device
    rp, rl = (torch.zeros(M, dtype=torch.float64, device=dev) for _ in range(2))
    ri = torch.zeros(M, dtype=torch.int32, device=dev)
    ref_ops.rowmax_combine(ws, n_seg, M, rp, ri, rl)
    mx, se, _, _ = rowmax_records(ws, n_seg, M)
    lse, p, b_lse, b_p, _ = rowmax_combine_bounds(mx, se, n_seg)
    res = []
    if got_idx is not None:
        res.append(("row_argmax", check_exact(got_idx[:M].long(), ri.long(), f"{what} row_argmax")))
    if got_p is not None:
        res.append(("row_maxprob", check(got_p[:M], rp, b_p, f"{what} row_maxprob")))
    if got_lse is not None:
        res.append(("row_lse", check(got_lse[:M], rl, b_lse, f"{what} row_lse")))
    return res


def sharpness(n_adm):
    """the two figures of the admissible-argmax rule's sharpness: share of rows with more than one admissible column, and the
    largest number of admissible columns in a row"""
    return float((n_adm > 1).double().mean()), int(n_adm.max())


MAX_SHARE_AMBIGUOUS, MAX_ADMISSIBLE = 0.15, 4     # caps of the sharpness condition (tests/test_bounds_cpu.py pins them on the oracle)
