"""The calls of tests/test_predict_edges_bounds_gpu.py and of its host twin in tests/test_bounds_cpu.py: the predict tail -- xl_gemm with
XL_EPI_ROWMAX / XL_EPI_ROWSAMPLE / XL_EPI_ROWSCORE, their combines xl_rowmax_combine / xl_rowsample_combine / xl_rowscore_combine and
the fp32 logits twins xl_sample_rows / xl_score_rows -- at the edges of their dispatch (csrc/gemm.hip, csrc/rowops.hip;
tests/test_kernel_bounds_gpu.gemm_kernel / rowop_kernel restate it).  Plain functions, no tests: each family takes a recorder-like
`ops` (Recorder(..., every_call=True) over HipOps or over the host restatement: alpha, the seed and the temperature are no part of a
signature, so every call is checked), a device and a seeded CPU generator -- the data is drawn on the host and moved, so both sides run
the same numbers --, issues its calls and returns how many it issued.

Storage, as in gemm_edge_cases.py / rowop_edge_cases.py.  A of order 1, B of order K^-1/2, bias of order 0.5.  EVERY OPERAND lies in a
poisoned allocation: +-2^12 in the leading-dimension pads, in one whole row past the extent, in guards in front and behind, and around
the bias.  aux, every per-row output, totals and the labels lie between guards of a non-zero sentinel; the recorder holds everything
outside the logical views to its earlier bits.  Pad columns are zero rows of B with bias -1e30, NOT divided by T for XL_EPI_ROWSAMPLE.

Planted rows.  Row TIE_ROW of every row tile of A is zero: its logits are the bias, exact (error allowance 0), and the two largest
biases are made equal -- inside one 8-column group, across two segments, across two column tiles, in turn -- so the lowest column must
win in the record and in the combine (the exact rule of bounds.argmax_admissible).

Ambiguity cap.  The admissible-argmax / admissible-draw rules accept any column within the error width; so that the width cannot hide
a wrong kernel, every GEMM call of the families `fused` and `rounds` asserts HERE, from the float64 reference alone, that at most 5 % of
its rows admit more than one column (the planted rows do not count).  A seed that exceeds the cap is changed, never the cap."""
import torch

import bounds as BD
import bounds_sampling as BS
import rowop_edge_cases as RE
from fake_ops_eval import EPI_ROWSCORE
from fake_ops_sampling import EPI_ROWSAMPLE, first_argmax, gumbel_noise

BF, F32 = torch.bfloat16, torch.float32
EPI_ROWMAX = BD.EPI_ROWMAX
EPIS = (EPI_ROWMAX, EPI_ROWSAMPLE, EPI_ROWSCORE)
GUARD = RE.GUARD
PAD_BIAS = -1e30
TIE_ROW = 3
MAX_AMBIGUOUS = 0.05
# ((M, N, K), real columns): one short K tile; a whole and a second, ragged K tile; a half-pad and an all-pad segment with three K
# tiles (the steady-state loop runs once); two row tiles; duo-eligible M and N, which must stay on 256x256 tiles
FUSED_SHAPES = (((256, 256, 8), 256), ((256, 256, 64), 256), ((256, 256, 72), 256), ((256, 512, 136), 412), ((512, 256, 200), 256),
                ((512, 768, 200), 700))
SWITCH_SHAPE = FUSED_SHAPES[-1]
ROUNDS_SHAPE = ((4352, 4096, 1096), 4000)                # 17 x 16 = 272 tiles: one round and a remainder of 16
SEEDS = (0, 3, 2 ** 40 + 11, 2 ** 64 - 1)
TEMPS = (0.5, 1.0, 4.0)
COMBINE_M = (1, 63, 64, 65, 257)
COMBINE_SEG = (1, 4, 7, 160, 480)
SCORE_CAP_COMBINE = 65537                                  # 1025 blocks of 64 rows: one row past the grid cap of rowscore_combine_kernel
SCORE_CAP_ROWS = (4097, 50, 56)                            # 1025 blocks of 4 rows: one row past the cap of score_rows_kernel
LOGITS_K = (1, 2, 63, 64, 65, 1000)


def up8(n):
    return (n + 7) // 8 * 8


def operand(g, dev, data, ld):
    """[rows, cols] data with row stride ld inside POISON: a guard in front, the pad columns, one whole row past the extent and a
    guard behind; the flat tensor at the operand's base (16-byte aligned)"""
    rows, cols = data.shape
    buf = RE._poison(g, GUARD + (rows + 1) * ld + GUARD, data.dtype)
    torch.as_strided(buf, (rows, cols), (ld, 1), GUARD).copy_(data)
    return buf.to(dev)[GUARD:GUARD + (rows + 1) * ld]


def edge_labels(n_cols, N):
    """the labels at the edges of a segment, a tile, the real columns and the launch, and the ones outside: the first pad column,
    N - 1, N, -1, the ignore label, and two that would alias column 5 if a kernel cut them to 32 bits"""
    return [0, 63, 64, 255, 256, n_cols - 1, n_cols, N - 1, N, -1, -100, 2 ** 32 + 5, -2 ** 32 + 5]


def labels_of(g, M, n_cols, N):
    """random valid labels, a tenth ignored; the edge labels in rows 8 .. 20 of every 256-row tile, and in the rows 64 further down the
    same labels in reverse order (the two quads of a wave's 128 rows carry different labels); every tile in an order of its own"""
    lab = torch.randint(0, n_cols, (M,), generator=g)
    lab[torch.randperm(M, generator=g)[:M // 10]] = -100
    edges = torch.tensor(edge_labels(n_cols, N))
    for t in range(0, M, 256):
        if t + 72 + len(edges) <= M:
            e = edges.roll(t // 256)
            lab[t + 8:t + 8 + len(e)] = e
            lab[t + 72:t + 72 + len(e)] = e.flip(0)
        else:
            k = min(len(edges), M - t)
            lab[t:t + k] = edges[:k]
    return lab


def draw_case(g, M, N, K, n_real, scale=1.0, bias=True, tie=0, T=1.0):
    """host operands of one launch -> (A [M, K] bf16, B [N, K] bf16 with zero pad rows, bias [N] fp32 or None, the planted rows)"""
    A = (torch.randn(M, K, generator=g) * scale).to(BF)
    B = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF)
    B[n_real:] = 0
    planted = list(range(TIE_ROW, M, 256))
    A[planted] = 0
    if not bias:
        assert n_real == N, "pad columns need a bias"
        return A, B, None, planted
    b = torch.randn(N, generator=g) * 0.5
    c0 = 10
    c1 = c0 + (1, 64, 256)[tie]
    if c1 >= n_real:
        c1 = c0 + (64 if c0 + 64 < n_real else 1)
    b[c0] = b[c1] = float(b[:n_real].max()) + 1.0
    b = b / T
    b[n_real:] = PAD_BIAS
    return A, B, b, planted


def ambiguity(A, B, b, alpha, epi, seed, planted):
    """share of the rows (the planted ones left out) that admit more than one column: the admissible-argmax rule of bounds.py, for
    XL_EPI_ROWSAMPLE the admissible-draw rule of bounds_sampling.py -- from the float64 reference alone"""
    M, K = A.shape
    N = B.shape[0]
    Ad, Bd = A.double(), B.double()
    al = float(torch.tensor(alpha, dtype=F32))
    pre, absdot = al * (Ad @ Bd.t()), abs(al) * (Ad.abs() @ Bd.abs().t())
    b_abs = torch.zeros(1, N, dtype=torch.float64, device=A.device)
    if b is not None:
        pre, b_abs = pre + b.double()[None, :], b.double().abs()[None, :]
    e = BD.rowmax_logit_error(pre, absdot, b_abs, K)
    x, E = pre, e.amax(-1)
    if epi == EPI_ROWSAMPLE:
        gn = gumbel_noise(seed, torch.arange(M, device=A.device)[:, None], torch.arange(N, device=A.device)[None, :])
        En, x = BS.draw_error(pre, gn, e)
        E = En.amax(-1)
    _, n_adm = BD.argmax_admissible(x, x.argmax(-1), E)
    keep = torch.ones(M, dtype=torch.bool, device=A.device)
    keep[planted] = False
    return float((n_adm[keep] > 1).double().mean()), int((n_adm[keep] > 1).sum())


def row_outputs(dev, M):
    return RE.out(dev, M), RE.out(dev, M, torch.int32), RE.out(dev, M)


def fused_call(ops, dev, g, epi, shape, pad, alpha=1.0, scale=1.0, bias=True, tie=0, seed=0, T=1.0, case=None, keep=None):
    """one launch of `epi` and its combine behind it -> calls issued (2).  case: operands drawn before (shared by the arms of one
    shape); keep: a list that receives every output tensor of the two calls"""
    (M, N, K), n_real = shape
    if epi == EPI_ROWSAMPLE:
        alpha = 1.0 / T
    else:
        T, seed = 1.0, 0
    A, B, b, planted = case if case is not None else draw_case(g, M, N, K, n_real, scale, bias, tie, T)
    ld = K + pad
    Ad, Bd = operand(g, dev, A, ld), operand(g, dev, B, ld)
    bd = RE.inp(g, dev, b) if b is not None else None
    share, rows = ambiguity(torch.as_strided(Ad, (M, K), (ld, 1)), torch.as_strided(Bd, (N, K), (ld, 1)), bd, alpha, epi, seed, planted)
    print(f"ambiguity epilogue={epi} M={M} N={N} K={K} alpha={alpha:g}: {rows} of {M - len(planted)} rows ({100 * share:.2f} %)", flush=True)
    assert share <= MAX_AMBIGUOUS, (epi, shape, share)
    n_seg = N // 64
    aux = RE.out(dev, n_seg * M * 4)
    labels = RE.out(dev, M, torch.int64, fill=labels_of(g, M, n_real, N)) if epi == EPI_ROWSCORE else None
    ops.gemm(Ad, Bd, None, bd, labels, aux, M, N, K, ld, ld, N, epilogue=epi, alpha=alpha, seed=seed)
    o = row_outputs(dev, M)
    outs = [aux, *o]
    if epi == EPI_ROWMAX:
        ops.rowmax_combine(aux, n_seg, M, o[0], o[1], o[2])
    elif epi == EPI_ROWSAMPLE:
        ops.rowsample_combine(aux, n_seg, M, seed, o[0], o[1], o[2])
    else:
        totals = RE.out(dev, 4, fill=torch.tensor([2.0, 3.0, 1.0, -7.0]))
        ops.rowscore_combine(aux, n_seg, M, labels, n_real, o[0], o[1], o[2], totals)
        outs.append(totals)
    if keep is not None:
        keep.extend(outs)
    return 2


# ------------------------------------------------------------------------------------------------------------------ families
def fused(ops, dev, g, shapes=FUSED_SHAPES, epis=EPIS):
    """every shape x tight / padded leading dimensions x epilogue, alpha 1 and 0.5 (XL_EPI_ROWSAMPLE: 1 / T, T in 0.5, 1, 4, the four
    seeds), the three kinds of planted ties in turn; per epilogue one launch without a bias (all columns real) and one with the logits
    spread to about +-60 (A of scale 20: exp(x - max) underflows inside segments)"""
    n = c = 0
    for shape in shapes:
        for pad in (0, 8):
            for epi in epis:
                n += fused_call(ops, dev, g, epi, shape, pad, alpha=(1.0, 0.5)[(c + c // 2) % 2], tie=c % 3, seed=SEEDS[c % 4],
                                T=TEMPS[c % 3])
            c += 1
    for epi in epis:
        n += fused_call(ops, dev, g, epi, ((256, 256, 64), 256), 8, bias=False, seed=SEEDS[2], T=TEMPS[0])
        n += fused_call(ops, dev, g, epi, ((512, 256, 200), 256), 8, scale=20.0, tie=1, seed=SEEDS[3], T=TEMPS[1])
    return n


def rounds(ops, dev, g, epis=EPIS, shape=ROUNDS_SHAPE, keep=None):
    """272 tiles: two rounds; with a slab workspace and set_gemm_tail_split(64, 1024) (the caller's) XL_EPI_ROWMAX runs its last 16
    tiles as two K slices each.  One set of operands for the arms (T = 1, alpha = 1)."""
    (M, N, K), n_real = shape
    case = draw_case(g, M, N, K, n_real, tie=2)
    n = 0
    for epi in epis:
        n += fused_call(ops, dev, g, epi, shape, 8, seed=SEEDS[1], case=case, keep=keep)
    return n


def switch_calls(ops, dev, g, epis=EPIS):
    """the (512, 768, 200) launches of `fused` -> (calls issued, every output tensor): run once under the default switches and once
    under a switch set, from the same seed, the outputs are bit-identical"""
    keep, n = [], 0
    for pad in (0, 8):
        for epi in epis:
            n += fused_call(ops, dev, g, epi, SWITCH_SHAPE, pad, alpha=(1.0, 0.5)[pad // 8], tie=2, seed=SEEDS[2], T=TEMPS[2], keep=keep)
    return n, keep


def records_of(g, M, n_seg, kind, seed=0, labels=None):
    """synthetic segment records [n_seg][M] of four floats as a launch of `kind` leaves them, from fp32 logits of scale 3 whose last
    100 columns (n_seg = 1: 14) are pad columns -- an all-pad segment from n_seg = 4 on --; row 0 has equal maxima in segments 0 and 1,
    row 1 a first segment whose sum of exponentials is exactly 1 -> (flat fp32 records, real columns)"""
    N = n_seg * 64
    n_real = N - 100 if n_seg >= 4 else 50
    y = torch.randn(M, N, generator=g) * 3
    if n_seg >= 4:
        y[0, 5] = y[0, 69] = float(y[0].max()) + 1.0
    if M > 1:
        y[1, :64] = -200.0
        y[1, 3] = 0.0
    y[:, n_real:] = PAD_BIAS
    ys = y.view(M, n_seg, 64)
    base = torch.arange(n_seg)[None, :] * 64
    mx = ys.amax(-1)
    se = torch.exp(ys - mx[..., None]).sum(-1)
    if M > 1:
        assert float(se[1, 0]) == 1.0
    fourth = torch.zeros(M, n_seg)
    if kind == EPI_ROWSAMPLE:
        z = y + gumbel_noise(seed, torch.arange(M)[:, None], torch.arange(N)[None, :], F32)
        loc = first_argmax(z.view(M, n_seg, 64))
        fourth = ys.gather(-1, loc[..., None])[..., 0]
    else:
        loc = first_argmax(ys)
        if kind == EPI_ROWSCORE:
            fourth = torch.full((M, n_seg), -float("inf"))
            rows = ((labels >= 0) & (labels < N)).nonzero()[:, 0]
            fourth[rows, labels[rows] // 64] = y[rows, labels[rows]]
    rec = torch.stack([mx, se, (loc + base).to(torch.int32).view(F32), fourth], -1)          # [M, n_seg, 4]
    return rec.permute(1, 0, 2).reshape(-1).contiguous(), n_real


def _nulled(outs, k):
    return [None if i == k else o for i, o in enumerate(outs)]


def combines(ops, dev, g, Ms=COMBINE_M, segs=COMBINE_SEG, cap_M=SCORE_CAP_COMBINE, strict=True):
    """the three combines over synthetic records, no GEMM in front: M on both sides of a block of 64 rows, n_seg on both sides of the
    four threads of a row up to the 30k vocabulary's 480; each optional output NULL in turn; xl_rowscore_combine one row past its
    grid cap; nine launches into one `totals` (the eight ticket sets wrap), each increment of the count slots equal to the first,
    and two runs of those nine into fresh accumulators, bit-identical (strict=False: the host twin's injected faults leave these
    two assertions to the recorder's check of every launch)"""
    n = c = 0
    for M in Ms:
        for n_seg in segs:
            N = n_seg * 64
            rec, n_real = records_of(g, M, n_seg, EPI_ROWMAX)
            o = _nulled(row_outputs(dev, M), c % 4)
            ops.rowmax_combine(RE.out(dev, rec.numel(), fill=rec), n_seg, M, o[0], o[1], o[2])
            seed = SEEDS[c % 4]
            rec, _ = records_of(g, M, n_seg, EPI_ROWSAMPLE, seed)
            o = _nulled(row_outputs(dev, M), (c + 1) % 4)
            ops.rowsample_combine(RE.out(dev, rec.numel(), fill=rec), n_seg, M, seed, o[0], o[1], o[2])
            lab = labels_of(g, M, n_real, N)
            rec, _ = records_of(g, M, n_seg, EPI_ROWSCORE, labels=lab)
            o = _nulled([*row_outputs(dev, M), RE.out(dev, 4, fill=torch.tensor([2.0, 3.0, 1.0, -7.0]))], c % 5)
            ops.rowscore_combine(RE.out(dev, rec.numel(), fill=rec), n_seg, M, RE.out(dev, M, torch.int64, fill=lab), n_real, *o)
            n += 3
            c += 1
    if cap_M:
        M, n_seg = cap_M, 1
        lab = labels_of(g, M, 50, 64)
        rec, n_real = records_of(g, M, n_seg, EPI_ROWSCORE, labels=lab)
        ops.rowscore_combine(RE.out(dev, rec.numel(), fill=rec), n_seg, M, RE.out(dev, M, torch.int64, fill=lab), n_real,
                             *row_outputs(dev, M), RE.out(dev, 4, fill=torch.tensor([2.0, 3.0, 1.0, -7.0])))
        n += 1
    M, n_seg = 257, 4
    lab = labels_of(g, M, 156, 256)
    rec, n_real = records_of(g, M, n_seg, EPI_ROWSCORE, labels=lab)
    ws, labels = RE.out(dev, rec.numel(), fill=rec), RE.out(dev, M, torch.int64, fill=lab)
    finals = []
    for start in ([2.0, 3.0, 1.0, -7.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]):
        totals = RE.out(dev, 4, fill=torch.tensor(start))
        prev, first = totals.cpu().double(), None
        for _ in range(9):
            ops.rowscore_combine(ws, n_seg, M, labels, n_real, *row_outputs(dev, M), totals)
            n += 1
            now = totals.cpu().double()
            inc = now - prev
            first = inc if first is None else first
            assert not strict or (torch.equal(inc[1:3], first[1:3]) and float(inc[1]) > 0), ("count slots of a repeated launch", inc, first)
            prev = now
        finals.append(totals.cpu().clone())
    assert not strict or torch.equal(finals[1].view(torch.int32), finals[2].view(torch.int32)), ("totals of two runs of nine launches", finals[1:])
    return n


def logits_case(g, M, K):
    """fp32 logits of scale 3; row 3 (if there is one) an exact tie of all columns"""
    x = RE.rn(g, M, K, scale=3.0)
    if M > 3:
        x[3] = x[3, 0]
    return x


def logits(ops, dev, g, Ks=LOGITS_K, cap=SCORE_CAP_ROWS):
    """xl_score_rows one row past its grid cap; both logits kernels at M = 5 with K below, at and past the 64 lanes of a row's wave,
    the leading dimension padded and poisoned; the edge labels and labels = NULL; inv_T at both ends of the accepted range"""
    n = 0
    if cap:
        M, K, ldl = cap
        ops.score_rows(RE.inp(g, dev, logits_case(g, M, K), ld=ldl), M, K, ldl, RE.out(dev, M, torch.int64, fill=labels_of(g, M, K, K)),
                       *row_outputs(dev, M), RE.out(dev, 4, fill=torch.tensor([2.0, 3.0, 1.0, -7.0])))
        n += 1
    for i, K in enumerate(Ks):
        M, ldl = 5, up8(K) + 8
        x = RE.inp(g, dev, logits_case(g, M, K), ld=ldl)
        lab = torch.tensor(edge_labels(K, K)).roll(-2 * i)[:M]
        ops.score_rows(x, M, K, ldl, RE.out(dev, M, torch.int64, fill=lab), *row_outputs(dev, M),
                       RE.out(dev, 4, fill=torch.tensor([2.0, 3.0, 1.0, -7.0])))
        ops.score_rows(x, M, K, ldl, None, *row_outputs(dev, M), RE.out(dev, 4, fill=torch.tensor([2.0, 3.0, 1.0, -7.0])))
        n += 2
        for j, inv_T in enumerate((1e-3, 1.0, 1e3)):
            ops.sample_rows(x, M, K, ldl, inv_T, SEEDS[(i + j) % 4], *row_outputs(dev, M))
            n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------ rejected
def rejected(ops, dev, g, error, ops_f32=None):
    """calls the launchers refuse before any launch, each precondition violated alone: each raises `error` with the documented code,
    every output storage keeps its bits -> cases run"""
    import pytest
    n = 0

    def refuse(outs, fn, code):
        nonlocal n
        raw = [(o, o.untyped_storage()) for o in outs if o is not None]
        before = [torch.tensor([], dtype=torch.uint8, device=o.device).set_(st, 0, (st.nbytes(),), (1,)).clone() for o, st in raw]
        with pytest.raises(error, match=code):
            fn()
        for (o, st), was in zip(raw, before):
            now = torch.tensor([], dtype=torch.uint8, device=o.device).set_(st, 0, (st.nbytes(),), (1,))
            assert torch.equal(now, was), "a refused call wrote to an output"
        n += 1
    SHAPE, ARG = r"\(-1\)", r"\(-5\)"
    M, N, K, ld = 256, 256, 64, 72
    A, B, b, _ = draw_case(g, M, N, K, N)
    Ad, Bd, bd = operand(g, dev, A, ld), operand(g, dev, B, ld), RE.inp(g, dev, b)
    A32, B32 = operand(g, dev, A.float(), ld), operand(g, dev, B.float(), ld)
    At, Bt = operand(g, dev, A.t().contiguous(), M + 8), operand(g, dev, B.t().contiguous(), N + 8)
    aux = RE.out(dev, (N // 64 + 2) * (M + 256) * 4)                       # (room for the records of every shape tried below)
    C = RE.out(dev, M * N, BF)
    colsum, ws = RE.out(dev, N), torch.zeros(ops.workspace_floats(N), device=dev)
    lab = RE.out(dev, M + 256, torch.int64, fill=labels_of(g, M + 256, N, N))
    lab4 = lab.view(torch.int32)[1:]                                           # the same storage, 4 bytes further on
    for epi in EPIS:
        res = lab if epi == EPI_ROWSCORE else None
        outs = [aux, C, colsum]

        def call(A_=Ad, B_=Bd, bias=bd, aux_=aux, M_=M, N_=N, K_=K, lda=ld, ldb=ld, ak=1, bk=1, acc=0, p=0.0, cs=None, res_=res, o=ops):
            return lambda: o.gemm(A_, B_, None, bias, res_, aux_, M_, N_, K_, lda, ldb, N_, a_kmajor=ak, b_kmajor=bk, epilogue=epi,
                                  accumulate=acc, p_drop=p, colsum=cs, ws=ws if cs is not None else None)
        if ops_f32 is not None:
            refuse(outs, call(A_=A32, B_=B32, o=ops_f32), SHAPE)              # fp32 operands
        refuse(outs, call(A_=At, lda=M + 8, ak=0), SHAPE)                     # A M-major
        refuse(outs, call(B_=Bt, ldb=N + 8, bk=0), SHAPE)                     # B N-major
        refuse(outs, call(M_=257), SHAPE)
        refuse(outs, call(N_=320), SHAPE)
        refuse(outs, call(K_=12), SHAPE)
        refuse(outs, call(lda=ld + 4), SHAPE)                                 # (one row past the extent is allocated: ld + 4 stays inside)
        refuse(outs, call(ldb=ld + 4), SHAPE)
        refuse(outs, call(aux_=None), SHAPE)
        refuse(outs, call(aux_=aux[1:]), SHAPE)                               # aux, A, B, bias off 16 bytes, each alone
        refuse(outs, call(A_=Ad[1:]), SHAPE)
        refuse(outs, call(B_=Bd[1:]), SHAPE)
        refuse(outs, call(bias=bd[1:]), SHAPE)
        refuse(outs, call(acc=1), SHAPE)
        refuse(outs, call(cs=colsum), SHAPE)
        ops.set_lds_transpose_read(0)
        try:
            refuse(outs, call(), SHAPE)                                       # the transpose read off
        finally:
            ops.set_lds_transpose_read(1)
        if epi != EPI_ROWMAX:
            refuse(outs, call(p=0.1), SHAPE)
        if epi == EPI_ROWSCORE:
            refuse(outs, call(res_=None), SHAPE)                              # labels NULL, labels off 8 bytes
            refuse(outs, call(res_=lab4), SHAPE)
    # combines and logits kernels
    M, n_seg = 65, 4
    rec, n_real = records_of(g, M, n_seg, EPI_ROWMAX)
    wsr = RE.out(dev, rec.numel() + 4, fill=torch.cat([rec, torch.zeros(4)]))
    o = row_outputs(dev, M)
    totals = RE.out(dev, 4, fill=torch.tensor([2.0, 3.0, 1.0, -7.0]))
    labc = RE.out(dev, M, torch.int64, fill=labels_of(g, M, n_real, n_seg * 64))
    refuse([*o, totals], lambda: ops.rowscore_combine(wsr, n_seg, M, labc, 64 * n_seg + 1, *o, totals), ARG)     # n_cols > 64 n_seg
    refuse([*o, totals], lambda: ops.rowscore_combine(wsr[1:], n_seg, M, labc, n_real, *o, totals), ARG)          # ws off 16 bytes
    refuse(list(o), lambda: ops.rowmax_combine(wsr[1:], n_seg, M, *o), ARG)
    refuse(list(o), lambda: ops.rowsample_combine(wsr[1:], n_seg, M, 3, *o), ARG)
    K, ldl = 50, 56
    x = RE.inp(g, dev, logits_case(g, M, K), ld=ldl)
    refuse([*o, totals], lambda: ops.score_rows(x, M, K, K - 1, labc, *o, totals), ARG)                           # ldl < K
    refuse(list(o), lambda: ops.sample_rows(x, M, K, K - 1, 1.0, 3, *o), ARG)
    refuse(list(o), lambda: ops.sample_rows(x, M, K, ldl, 0.0, 3, *o), ARG)                                       # inv_T 0, inf
    refuse(list(o), lambda: ops.sample_rows(x, M, K, ldl, float("inf"), 3, *o), ARG)
    return n
