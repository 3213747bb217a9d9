"""The calls of tests/test_rowop_edges_bounds_gpu.py and of its host twin in tests/test_bounds_cpu.py: the entry points of
csrc/rowops.hip and csrc/optim.hip at the edges of their dispatch (tests/test_kernel_bounds_gpu.rowop_kernel restates it).  Plain
functions, no tests: each family takes a recorder-like `ops` (Recorder / RecorderRes over HipOps or over the host restatement), a
device and a seeded CPU generator -- the data is drawn on the host and moved, so both sides run the same numbers --, issues its
calls and returns how many it issued.  Every call has a signature of its own (shape, which optional tensors are present, dropout on
or off, alignment, kernel label), so the recorder checks every one.

Storage.  EVERY OUTPUT is a view inside a larger allocation with GUARD elements in front of it and behind it; the guards -- and
the pad columns of an output that has a leading dimension -- hold SENTINEL (never zero: several kernels write zeros), and the
recorder holds everything outside the logical views to its earlier bits (the row "outside view").  EVERY FLOATING OPERAND sits
between guards of +-2^12 (POISON), and so do its pad columns: one element read past a row, a row past M or in front of the base
enters a sum orders of magnitude beyond any bound.  Column-sum destinations, losses and tables start non-zero: every reduction of
the library is a +=.  The guards are whole 16-byte pieces, so every base stays aligned; a base is shifted only where the launcher
itself branches on alignment (cross entropy) or rejects it.

LayerNorm rows have a mean of three standard deviations: a statistic taken over the padded width instead of N fails its bound."""
import torch

BF, F32 = torch.bfloat16, torch.float32
GUARD = 64
POISON = 4096.0
SENTINEL = 12345.0
EPS = 1e-12

LN_N = {BF: (8, 504, 512, 520, 1024, 1032, 2048, 2056, 4096), F32: (4, 252, 256, 260, 512, 516, 1024, 1028, 2048)}
LN_FWD_M = (1, 3, 5)
LN_BWD_M = (1, 7, 9)
LN_CAP_M = 4099                                           # 513 blocks of 8 rows: the 512-block cap, a second, ragged pass
LN_CAP_N = {BF: (8, 520, 1032, 2056), F32: (4, 260, 516, 1028)}                  # one row length per NIT
LN_DMA = ((8191, 512), (8192, 512), (8192, 520), (8192, 1024), (8192, 1032), (8200, 264))
# (workspace, dbias_prev, a dropped copy is passed, p_drop)
LN_VARIANTS = ((True, True, True, 0.1), (False, False, False, 0.0), (True, True, True, 0.0), (False, True, True, 0.1),
               (True, False, True, 0.1))
RES_N = (4, 256, 260, 512, 516, 768, 772, 1024, 1028, 2048)
RES_CAP_N = (4, 260, 516, 772, 1028)                      # one row length per NIT of DISPATCH_NIT_RES
RES_VARIANTS = ((True, True, 0.1), (False, False, 0.0), (True, True, 0.0), (False, True, 0.1))
VISN_N = {BF: (8, 512, 520, 768, 1024, 1032), F32: (4, 256, 260, 512, 516, 768)}
VISN_P = (1, 4, 5, 8)
# M -> the backward variants (workspace, dbias_visn) run at it; 2049 is past the 256-block cap of either block shape
VISN_M = {1: ((True, True),), 9: ((False, False), (True, False)), 2049: ((True, True), (False, True))}
EMBED_N = {BF: (8, 512, 520, 1024), F32: (4, 256, 260, 512, 516, 1024)}
EMBED_RUNS = (1, 2, 32, 33, 34, 256, 257, 258)            # occurrences of single tokens: the sorted kernel walks 32 candidates per chunk
COLSUM_M = (1, 127, 129, 16384, 16385)
CE_K = (2, 50, 1003, 4096, 4097, 10240, 10241, 30522, 32768, 32769)
CE_BIG = ((2049, 50), (2049, 4097), (1025, 10241))        # past the grid cap of ce_row_kernel<2,256>, <5,256>, <4,1024>
# (labels, dlogits, loss, row_lse, row_argmax, row_maxprob): which tensors a call is given
# (valid labels without a gradient store: the loss path alone; no labels with a loss_out: it must stay untouched)
CE_PATTERNS = (("mixed", 1, 1, 1, 1, 1), (None, 1, 0, 1, 1, 1), ("none_valid", 0, 1, 0, 1, 0), ("mixed", 1, 1, 0, 0, 0),
               ("none_valid", 1, 1, 1, 0, 1), ("mixed", 0, 1, 1, 0, 0), (None, 1, 1, 0, 1, 0))
SUMSQ_N = (1, 3, 4, 1027, 524291, 2359299)
ADAMW_BIG = 1048832                                       # 262208 float4: 256 blocks x 1024 threads and 64 more -- a second pass


def vec(dtype):
    return 8 if dtype == BF else 4


def _sentinel(dtype):
    return SENTINEL if dtype.is_floating_point else (0xA5 if dtype == torch.uint8 else -12345)


def out(dev, n, dtype=F32, fill=None):
    """an n-element output between guards of SENTINEL; `fill`: its content before the call"""
    buf = torch.full((GUARD + n + GUARD,), _sentinel(dtype), dtype=dtype)
    if fill is not None:
        buf[GUARD:GUARD + n] = fill.reshape(-1).to(dtype)
    return buf.to(dev)[GUARD:GUARD + n]


def out2(dev, M, N, ld, dtype, fill=None):
    """an [M, N] output with row stride ld (pad columns and guards: SENTINEL), as the flat tensor at its base"""
    buf = torch.full((GUARD + M * ld + GUARD,), _sentinel(dtype), dtype=dtype)
    if fill is not None:
        torch.as_strided(buf, (M, N), (ld, 1), GUARD).copy_(fill.to(dtype))
    return buf.to(dev)[GUARD:GUARD + M * ld]


def _poison(g, n, dtype):
    return ((torch.randint(0, 2, (n,), generator=g) * 2 - 1).float() * POISON).to(dtype)


def inp(g, dev, data, ld=None, shift=0):
    """the [M, N] (or [n]) floating operand `data` with row stride ld inside POISON: guards, pad columns, and `shift` elements in
    front of a base advanced by that many"""
    data = data if data.dim() == 2 else data.reshape(1, -1)
    M, N = data.shape
    ld = N if ld is None else ld
    buf = _poison(g, GUARD + shift + M * ld + GUARD, data.dtype)
    torch.as_strided(buf, (M, N), (ld, 1), GUARD + shift).copy_(data)
    return buf.to(dev)[GUARD + shift:GUARD + shift + M * ld]


def rn(g, *shape, scale=1.0, shift=0.0, dtype=F32):
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype)


def workspace(ops, dev, N):
    return torch.zeros(ops.workspace_floats(N), device=dev)


def _affine(g, dev, N):
    return inp(g, dev, rn(g, N, scale=0.1, shift=1.0)), inp(g, dev, rn(g, N, scale=0.1))


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_pair(ops, dev, g, dtype, M, N, variants):
    """forward at (M, N), then one backward per variant on the forward's statistics -> calls issued"""
    x = inp(g, dev, rn(g, M, N, shift=3.0, dtype=dtype))
    gamma, beta = _affine(g, dev, N)
    mean, rstd = out(dev, M), out(dev, M)
    ops.layernorm_fwd(x, gamma, beta, out2(dev, M, N, N, dtype), mean, rstd, M, N, EPS)
    dy = inp(g, dev, rn(g, M, N, dtype=dtype))
    ws = workspace(ops, dev, N)
    for use_ws, with_bias, with_copy, p in variants:
        dg, db = out(dev, N, fill=rn(g, N)), out(dev, N, fill=rn(g, N))
        dbp = out(dev, N, fill=rn(g, N)) if with_bias else None
        dxd = out2(dev, M, N, N, dtype) if with_copy else None
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, out2(dev, M, N, N, dtype), dg, db, dbp, M, N, ws=ws if use_ws else None,
                          dx_dropped=dxd, p_drop=p, seed=5)
    return 1 + len(variants)


def layernorm(ops, dev, g, dtype, Ns=None, fwd_M=LN_FWD_M, bwd_M=LN_BWD_M, cap_N=None, dma=None):
    """xl_layernorm_fwd / _bwd: every NIT of DISPATCH_NIT with whole and ragged last vectors; fewer rows than waves and a ragged
    last block; the backward with a workspace and with atomics, with and without dbias_prev, with a dropped copy, and with
    p_drop = 0 (the dropped copy handed over stays untouched, dbias_prev is still written); 4099 rows (the grid cap, a second,
    ragged pass of the blocks); for bf16 the boundary of the DMA variant"""
    Ns = LN_N[dtype] if Ns is None else Ns
    cap_N = LN_CAP_N[dtype] if cap_N is None else cap_N
    dma = (LN_DMA if dtype == BF else ()) if dma is None else dma
    n = 0
    for N in Ns:
        for M in sorted(set(fwd_M) | set(bwd_M)):
            n += _ln_pair(ops, dev, g, dtype, M, N, LN_VARIANTS if M in bwd_M else ())
    for N in cap_N:
        n += _ln_pair(ops, dev, g, dtype, LN_CAP_M, N, (LN_VARIANTS[0], LN_VARIANTS[3]))
    for M, N in dma:
        n += _ln_pair(ops, dev, g, dtype, M, N, (LN_VARIANTS[0], LN_VARIANTS[1]))
    return n


def layernorm_res(ops, dev, g, Ns=RES_N, bwd_M=LN_BWD_M, cap_N=RES_CAP_N):
    """xl_layernorm_fwd_res / _bwd_res (fp32 rows, bf16 copies): every NIT of DISPATCH_NIT_RES, the same rows and variants"""
    n = 0
    for N in Ns:
        ws = workspace(ops, dev, N)
        for M in sorted(set(LN_FWD_M) | set(bwd_M)) + ([LN_CAP_M] if N in cap_N else []):
            x = inp(g, dev, rn(g, M, N, shift=3.0))
            gamma, beta = _affine(g, dev, N)
            mean, rstd = out(dev, M), out(dev, M)
            ops.layernorm_fwd_res(x, gamma, beta, out2(dev, M, N, N, F32), out2(dev, M, N, N, BF), mean, rstd, M, N, EPS)
            n += 1
            if M not in bwd_M and M != LN_CAP_M:
                continue
            dy = inp(g, dev, rn(g, M, N))
            for use_ws, with_bias, p in (RES_VARIANTS if M != LN_CAP_M else (RES_VARIANTS[0], RES_VARIANTS[3])):
                dg, db = out(dev, N, fill=rn(g, N)), out(dev, N, fill=rn(g, N))
                dbp = out(dev, N, fill=rn(g, N)) if with_bias else None
                ops.layernorm_bwd_res(dy, x, gamma, mean, rstd, out2(dev, M, N, N, F32), dg, db, dbp, M, N,
                                      ws=ws if use_ws else None, dx_dropped=out2(dev, M, N, N, BF), p_drop=p, seed=5)
                n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------ feature encoder
def visn_ln(ops, dev, g, dtype, Ns=None, Ps=VISN_P, Ms=None):
    """xl_visn_ln_fwd / _bwd across N <= 128 VEC (the LDS kernels, P <= 4) and the NIT2 split, P on both sides of 4, rows below a
    block, and past the backward's 256-block cap; workspace or atomics, dbias_visn present or not"""
    Ns = VISN_N[dtype] if Ns is None else Ns
    Ms = VISN_M if Ms is None else Ms
    n = 0
    for N in Ns:
        ws = workspace(ops, dev, N)               # (xl_workspace_floats(N) holds the 256 slabs of 10 vectors)
        for P in Ps:
            wbox, bbox = inp(g, dev, rn(g, N, P, scale=0.5)), inp(g, dev, rn(g, N, scale=0.5))
            (gv, bv), (gb, bb) = _affine(g, dev, N), _affine(g, dev, N)
            for M, variants in Ms.items():
                xv = inp(g, dev, rn(g, M, N, shift=3.0, dtype=dtype))
                pos = inp(g, dev, torch.rand(M, P, generator=g))
                st = [out(dev, M) for _ in range(4)]
                ops.visn_ln_fwd(xv, pos, wbox, bbox, gv, bv, gb, bb, out2(dev, M, N, N, dtype), *st, M, N, P, EPS)
                dy = inp(g, dev, rn(g, M, N, dtype=dtype))
                for use_ws, with_bias in variants:
                    sums = [out(dev, N, fill=rn(g, N)) for _ in range(4)]
                    dwbox, dbbox = out(dev, N * P, fill=rn(g, N * P)).view(N, P), out(dev, N, fill=rn(g, N))
                    dbias = out(dev, N, fill=rn(g, N)) if with_bias else None
                    ops.visn_ln_bwd(dy, xv, pos, wbox, bbox, gv, gb, *st, out2(dev, M, N, N, dtype), *sums, dwbox, dbbox, dbias,
                                    M, N, P, ws=ws if use_ws else None)
                n += 1 + len(variants)
    return n


# ------------------------------------------------------------------------------------------------------------------ embeddings
def embed_ids(g, B, L, vocab=40, runs=EMBED_RUNS):
    """[B, L] ids in which single tokens occur runs[i] times each -- the LARGEST id of all carries the LONGEST run, which so ends
    exactly at position M of the sorted order (the sorted kernel's last chunk of candidates is cut by jj < M) --, some rows carry
    the padding id 0, the rest are drawn from the remaining ids; in random order"""
    M = B * L
    ids = []
    for i, r in enumerate(sorted(runs, reverse=True)):
        ids += [vocab - 1 - i] * r
    assert len(ids) + 16 <= M, (len(ids), M)
    ids += [0] * 16
    ids += torch.randint(1, vocab - len(runs), (M - len(ids),), generator=g).tolist()
    ids = torch.tensor(ids)[torch.randperm(M, generator=g)]
    return ids.view(B, L)


def embed_types(g, M, n_types):
    """token types with 8, 9 and 64 rows of type 1 in the first three 64-row chunks (the type kernel takes 8 matches per round)"""
    tt = torch.randint(0, n_types, (M,), generator=g)
    if n_types > 1 and M >= 192:
        for c, k in enumerate((8, 9, 64)):
            tt[64 * c:64 * c + 64] = 0
            tt[64 * c + torch.randperm(64, generator=g)[:k]] = 1
    return tt


def _embed_bwd(ops, dev, g, dtype, ids, N, order, tt, n_types):
    from xlxmert_amd.trainer import word_order_of
    B, L = ids.shape
    vocab = int(ids.max()) + 1
    dpre = inp(g, dev, rn(g, B * L, N, dtype=dtype))
    dword, dpos = out(dev, vocab * N, fill=rn(g, vocab * N)).view(vocab, N), out(dev, L * N, fill=rn(g, L * N)).view(L, N)
    nt = max(n_types, 2)
    dtype_tab = out(dev, nt * N, fill=rn(g, nt * N)).view(nt, N)
    ops.embed_bwd(dpre, ids.to(dev), tt.view(B, L).to(dev) if tt is not None else None, dword, dpos, dtype_tab, B, L, N,
                  order=word_order_of(ids).to(dev) if order else None, n_types=n_types)


def embeddings(ops, dev, g, dtype, Ns=None, big=(137, 7), small=((1, 65), (7, 10), (9, 8))):
    """xl_embed_ln_fwd at every NIT boundary (token types all zero and mixed, padding rows); xl_embed_bwd over passes 1 / 2 / 4,
    sorted and scanning word kernels (runs of 1 .. 258 occurrences, the last run at the end of the order), the type kernel with 1, 2
    and 3 types (8, 9 and 64 matches in a chunk; 65 rows: two waves without rows), the position kernel with B = 1, 7, 9, 137 and
    N = 72 (a partly live last block of 64 columns).  The tables start non-zero; their rows 0 are frozen."""
    Ns = EMBED_N[dtype] if Ns is None else Ns
    n = 0
    for i, N in enumerate(LN_N[dtype]):
        B, L, vocab = 3, 5, 11
        ids = torch.randint(0, vocab, (B, L), generator=g)
        ids[0, 1] = ids[2, 4] = 0
        tt = torch.zeros(B, L, dtype=torch.long) if i % 2 == 0 else torch.randint(0, 2, (B, L), generator=g)
        word, pos, typ = (inp(g, dev, rn(g, r, N, dtype=dtype)).view(r, N) for r in (vocab, L, 2))
        gamma, beta = _affine(g, dev, N)
        M = B * L
        ops.embed_ln_fwd(ids.to(dev), tt.to(dev), word, pos, typ, gamma, beta, out2(dev, M, N, N, dtype), out2(dev, M, N, N, dtype),
                         out(dev, M), out(dev, M), B, L, N, EPS)
        n += 1
    B, L = big
    ids = embed_ids(g, B, L)
    for N in Ns:
        _embed_bwd(ops, dev, g, dtype, ids, N, True, embed_types(g, B * L, 3), 3)
        _embed_bwd(ops, dev, g, dtype, ids, N, False, None, 2)
        n += 2
    N = 72
    _embed_bwd(ops, dev, g, dtype, ids, N, True, embed_types(g, B * L, 2), 2)
    _embed_bwd(ops, dev, g, dtype, ids, N, False, torch.zeros(B * L, dtype=torch.long), 1)
    _embed_bwd(ops, dev, g, dtype, ids, N, True, None, 2)                      # sorted word kernel, no type kernel
    _embed_bwd(ops, dev, g, dtype, ids, N, False, embed_types(g, B * L, 3), 3)   # scanning word kernel with the type kernel
    n += 4
    for B, L in small:
        ids = torch.randint(0, 6, (B, L), generator=g)
        ids[0, L - 1] = 7                                         # the largest id once, at the end of the order
        _embed_bwd(ops, dev, g, dtype, ids, N, True, embed_types(g, B * L, 2), 2)
        n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------ column sums
def colsums(ops, dev, g, dtype, Ms=COLSUM_M):
    """xl_colsum / xl_masked_colsum: one row, a slab short of and past 128 rows, 16384 / 16385 rows (rows_per_block doubles; a
    ragged last slab), N on and off 64 VEC, ldx = N + VEC, workspace or atomics, masks of zeros, of ones and random; destinations
    of order 64, so that a sum stored instead of added is beyond the M-deep bound at every M"""
    V = vec(dtype)
    Ns = (V, 64 * V, 65 * V)
    ws = workspace(ops, dev, max(Ns))
    n = 0
    for M in Ms:
        for N in Ns:
            data = rn(g, M, N, dtype=dtype)
            if M > 128:         # the last slab of 128 rows (a single row at 129 and 16385) weighs in: left out, it is beyond the M-deep bound
                data[(M - 1) // 128 * 128:] *= 256
            x = inp(g, dev, data, ld=N + V)
            for use_ws in (True, False):
                ops.colsum(x, out(dev, N, fill=rn(g, N, scale=64.0)), M, N, N + V, ws=ws if use_ws else None)
                kind = n % 3
                mask = (torch.zeros(M) if kind == 0 else torch.ones(M) if kind == 1 else torch.rand(M, generator=g) < 0.5).to(torch.uint8)
                ops.masked_colsum(x, mask.to(dev), out(dev, N, fill=rn(g, N, scale=64.0)), M, N, N + V, ws=ws if use_ws else None)
                n += 2
    return n


def deferred(ops, dev, g, dtype):
    """eight producers of deferred second stages on one stream -- LayerNorm backward, column sums, feature-encoder backward, with
    different N and numbers of slabs; the first and the second add into ONE dgamma / dbeta, so the flush cuts its first batch
    after one entry (the alias), fills the second to kBatch = 6 entries (producers 1 .. 6) and launches the last producer alone:
    batches of 1, 6 and 1 --, then one flush.  Returns (calls issued, the destinations, the workspaces: a pending second stage reads its
    producer's workspace at the flush, so the caller keeps them alive until then, the destinations per producer)."""
    V = vec(dtype)
    dests, keep, groups = [], [], []

    def dest(n):
        dests.append(out(dev, n, fill=rn(g, n)))
        groups[-1].append(dests[-1])
        return dests[-1]
    shared = None
    n = 0
    for i, (kind, M, N) in enumerate((("ln", 300, 8 * V), ("ln", 4099, 8 * V), ("ln", 9, 64 * V), ("colsum", 129, 65 * V),
                                      ("visn", 9, 8 * V), ("colsum", 16385, V), ("visn", 2049, 65 * V), ("colsum", 1, 64 * V))):
        ws = workspace(ops, dev, N)               # a deferred producer needs a workspace region of its own
        keep.append(ws)
        groups.append([])
        if kind == "ln":
            x, dy = inp(g, dev, rn(g, M, N, shift=3.0, dtype=dtype)), inp(g, dev, rn(g, M, N, dtype=dtype))
            gamma, _ = _affine(g, dev, N)
            xf = torch.as_strided(x, (M, N), (N, 1)).float()
            mean, rstd = inp(g, dev, xf.mean(1)), inp(g, dev, 1.0 / torch.sqrt(xf.var(1, unbiased=False) + EPS))
            if i in (0, 1):
                if shared is None:
                    shared = (dest(N), dest(N))
                else:
                    groups[-1].extend(shared)
                dg, db = shared
            else:
                dg, db = dest(N), dest(N)
            ops.layernorm_bwd(dy, x, gamma, mean, rstd, out2(dev, M, N, N, dtype), dg, db, dest(N), M, N, ws=ws)
        elif kind == "colsum":
            ops.colsum(inp(g, dev, rn(g, M, N, dtype=dtype), ld=N + V), dest(N), M, N, N + V, ws=ws)
        else:
            P = 4
            wbox, bbox = inp(g, dev, rn(g, N, P, scale=0.5)), inp(g, dev, rn(g, N, scale=0.5))
            (gv, _), (gb, _) = _affine(g, dev, N), _affine(g, dev, N)
            xv, dy = inp(g, dev, rn(g, M, N, shift=3.0, dtype=dtype)), inp(g, dev, rn(g, M, N, dtype=dtype))
            pos = inp(g, dev, torch.rand(M, P, generator=g))
            xf = torch.as_strided(xv, (M, N), (N, 1)).float()
            box = torch.as_strided(pos, (M, P), (P, 1)) @ torch.as_strided(wbox, (N, P), (P, 1)).t() + bbox
            st = [inp(g, dev, t) for t in (xf.mean(1), 1.0 / torch.sqrt(xf.var(1, unbiased=False) + EPS), box.mean(1),
                                           1.0 / torch.sqrt(box.var(1, unbiased=False) + EPS))]
            ops.visn_ln_bwd(dy, xv, pos, wbox, bbox, gv, gb, *st, out2(dev, M, N, N, dtype), dest(N), dest(N), dest(N), dest(N),
                            dest(N * P).view(N, P), dest(N), dest(N), M, N, P, ws=ws)
        n += 1
    return n, dests, keep, groups


def flush_batches(groups, k_batch=6):
    """xl_flush_reductions_on restated: the pending entries (each a producer's destinations) in registration order, up to kBatch per
    launch, a launch cut in front of an entry that adds into a destination some entry of the launch already adds into -> sizes"""
    sizes, cur = [], []
    for outs in groups:
        rng = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in outs]
        alias = any(a0 < b1 and b0 < a1 for a0, a1 in rng for e in cur for b0, b1 in e)
        if cur and (alias or len(cur) == k_batch):
            sizes.append(len(cur))
            cur = []
        cur.append(rng)
    return sizes + [len(cur)]


# ------------------------------------------------------------------------------------------------------------------ cross entropy
def ce_logits(g, M, K):
    """random logits of scale 3; row 0: an exact tie of the maximum between the first and the last column (the lowest index
    wins); row 1: the maximum in column K - 1; row 2: spread over +-80 -> (logits, number of tied rows)"""
    x = rn(g, M, K, scale=3.0)
    x[0, 0] = x[0, K - 1] = x[0].max() + 1.0
    if M > 1:
        x[1, K - 1] = x[1].max() + 1.0
    if M > 2:
        x[2] = torch.rand(K, generator=g) * 160 - 80
    return x, 1


def ce_call(ops, dev, g, dtype, M, K, ldl, lddl, pattern, shift=0):
    labels_kind, with_dl, with_loss, with_lse, with_am, with_mp = pattern
    x, _ = ce_logits(g, M, K)
    logits = inp(g, dev, x, ld=ldl, shift=shift)
    labels = counts = None
    if labels_kind is not None:
        labels = torch.randint(0, K, (M,), generator=g)
        labels[0] = K - 1
        labels[1::7] = -100
        if labels_kind == "none_valid":
            labels[:] = -100
        counts = inp(g, dev, torch.tensor([float((labels != -100).sum())]))
        labels = labels.to(dev)
    ops.ce_fwd_bwd(logits, labels, counts, out2(dev, M, (K + 7) // 8 * 8 if lddl >= (K + 7) // 8 * 8 else K, lddl, dtype) if with_dl else None,
                   out(dev, 1, fill=torch.tensor([0.5])) if with_loss else None, out(dev, M) if with_lse else None,
                   out(dev, M, torch.int32) if with_am else None, out(dev, M) if with_mp else None, M, K, ldl, lddl, grad_scale=0.5)


def cross_entropy(ops, dev, g, dtype, Ks=CE_K, big=CE_BIG, fallbacks=True):
    """xl_ce_fwd_bwd: the three register kernels on both sides of their K thresholds, the scalar kernel for each reason it is
    chosen, rows past the grid cap, labels absent / all ignored / mixed (one equal to K - 1), each optional output present and
    absent, ties of the maximum, the maximum in the last column, logits spread to +-80"""
    n = 0
    for K in Ks:
        K8 = (K + 7) // 8 * 8
        for pattern in CE_PATTERNS:
            ce_call(ops, dev, g, dtype, 3, K, K8 + 8, K8 + 8, pattern)
            n += 1
    for M, K in big:
        K8 = (K + 7) // 8 * 8
        ce_call(ops, dev, g, dtype, M, K, K8 + 8, K8 + 8, CE_PATTERNS[0])
        n += 1
    if fallbacks:
        K, K8 = 1003, 1008
        for ldl, lddl, shift in ((K, K8 + 8, 0), (K8 + 2, K8 + 8, 0), (K8 + 8, K8 + 4, 0), (K8 + 8, K8 + 8, 1)):
            ce_call(ops, dev, g, dtype, 3, K, ldl, lddl, CE_PATTERNS[0], shift=shift)
            n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------ elementwise
def elementwise(ops, dev, g, dtype):
    """the copy / mask / loss kernels at a size off their block, with padded leading dimensions"""
    V = vec(dtype)
    n = 0
    M, N = 37, 9 * V
    for ldx, ldy in ((N + V, N + 2 * V), (N, N)):
        ops.dropout(inp(g, dev, rn(g, M, N, dtype=dtype), ld=ldx), out2(dev, M, N, ldy, dtype), M, N, ldx, ldy, 0.1, 7)
        n += 1
    nn = 1001 * V                                             # whole vectors, no whole block
    ops.gelu_bwd(inp(g, dev, rn(g, nn, dtype=dtype)), inp(g, dev, (torch.linspace(-10, 10, nn) + rn(g, nn, scale=0.1)).to(dtype)),
                 out(dev, nn, dtype), nn)
    ops.tanh_bwd(inp(g, dev, rn(g, nn, dtype=dtype)), inp(g, dev, torch.tanh(rn(g, nn, scale=2.0)).to(dtype)), out(dev, nn, dtype), nn)
    n += 2
    M, N = 5, 37
    for with_dl in (True, False):
        ops.bce_logits_fwd_bwd(inp(g, dev, rn(g, M, N, scale=4.0), ld=40), inp(g, dev, torch.rand(M, N, generator=g), ld=41),
                               out2(dev, M, N, 48, dtype) if with_dl else None, out(dev, 1, fill=torch.tensor([0.5])), M, N, 40, 41, 48)
        n += 1
    N = 5 * V
    src = inp(g, dev, rn(g, 8, N, dtype=dtype), ld=N + V)
    rows = torch.tensor([3, 3, 0, -1, 7, 2, 2, 5, 1], dtype=torch.int32)               # repeated, out of order, a padding entry
    ops.gather_rows(src, rows.to(dev), out2(dev, 9, N, N + 2 * V, dtype), 9, N, N + V, N + 2 * V)
    rows = torch.tensor([4, -1, 0, 6, 2], dtype=torch.int32)
    ops.scatter_rows(src, rows.to(dev), out2(dev, 7, N, N + 2 * V, dtype, fill=rn(g, 7, N, dtype=dtype)), 5, N, N + V, N + 2 * V)
    labels = torch.randint(-100, 50, (50,), generator=g)
    rows = torch.randint(-1, 50, (300,), generator=g).to(torch.int32)
    ops.gather_labels(labels.to(dev), rows.to(dev), out(dev, 300, torch.int64), 300)
    n += 3
    for F in (8, 2056):
        for masked in (False, True):
            M, K = 9, 11
            cent = inp(g, dev, rn(g, K, F, dtype=dtype)).view(K, F)
            cid = torch.randint(0, K, (M,), generator=g).to(dev)
            vm = (torch.rand(M, generator=g) < 0.4).to(torch.uint8).to(dev) if masked else None
            ops.codebook_gather(cid, vm, cent, inp(g, dev, rn(g, F)) if masked else None, out2(dev, M, F, F, dtype), M, F)
            n += 1
    for B, Vv in ((25, 41), (17, 65)):                        # 1025 elements: one past the block; more rows than waves, than lanes
        labels = torch.where(torch.rand(B * Vv, generator=g) < 0.3, torch.full((B * Vv,), -100), torch.randint(0, 9, (B * Vv,), generator=g))
        vm = (torch.rand(B, Vv, generator=g) < 0.4).to(torch.uint8)
        ops.mask_counts(labels.to(dev), vm.to(dev), out(dev, 1), out(dev, B), B, Vv)
        n += 1
    B, Vv, F, K = 3, 5, 70 * V, 11
    cent = inp(g, dev, rn(g, K, F, dtype=dtype)).view(K, F)
    cid = torch.randint(0, K, (B, Vv), generator=g).to(dev)
    vm = (torch.rand(B, Vv, generator=g) < 0.6).to(torch.uint8)
    nm = inp(g, dev, vm.sum(1).float())
    rows = torch.tensor([14, 3, -1, 0, 7, 7, 9], dtype=torch.int32)
    ops.featloss_fwd_bwd(inp(g, dev, rn(g, 7, F, dtype=dtype)), cent, cid, vm.to(dev), nm, out2(dev, 7, F, F, dtype),
                         out(dev, 1, fill=torch.tensor([0.5])), B, Vv, F, grad_scale=0.5, rows=rows.to(dev), n_rows=7)
    ops.featloss_fwd_bwd(inp(g, dev, rn(g, B * Vv, F, dtype=dtype)), None, None, vm.to(dev), nm, out2(dev, B * Vv, F, F, dtype),
                         out(dev, 1, fill=torch.tensor([0.5])), B, Vv, F, targets=inp(g, dev, rn(g, B * Vv, F, dtype=dtype)))
    return n + 2


# ------------------------------------------------------------------------------------------------------------------ optimizer
def adamw_state(g, dev, n):
    return (out(dev, n, fill=rn(g, n)), out(dev, n, fill=rn(g, n, scale=0.01)), out(dev, n, fill=rn(g, n, scale=0.01)),
            out(dev, n, fill=torch.rand(n, generator=g) * 1e-4))


def adamw_call(ops, dev, g, dtype, n, flags, steps, clip, grad_scale, zero_grad, copy):
    """clip: None (no sumsq), "binding" or "loose" (max_norm below / above the gradient norm)"""
    p, gr, m, v = adamw_state(g, dev, n)
    chunks = n // 256
    fl = None
    if flags:
        fl = torch.randint(0, 8, (chunks,), generator=g).to(torch.uint8) if chunks > 1 else torch.tensor([1], dtype=torch.uint8)
        fl = fl.to(dev)
    cs = torch.randint(1, 2000, (chunks,), generator=g).to(torch.int32).to(dev) if steps else None
    ss, max_norm = None, 0.0
    if clip is not None:
        sq = float((gr.double() ** 2).sum())
        ss = inp(g, dev, torch.tensor([sq]))
        norm = sq ** 0.5 * grad_scale
        max_norm = norm * (0.25 if clip == "binding" else 4.0)
    t = 3.0
    lrs = inp(g, dev, torch.tensor([1e-3, 1 - 0.9 ** t, 1 - 0.999 ** t, t]))
    pc = out(dev, n, dtype) if copy else None
    ops.adamw(p, gr, m, v, pc, fl, ss, lrs, n, 0.9, 0.999, 1e-6, 0.01, max_norm, grad_scale=grad_scale, chunk_steps=cs, zero_grad=zero_grad)


def optimizer(ops, dev, g, dtype, sumsq_n=SUMSQ_N, adamw_big=ADAMW_BIG):
    """xl_sumsq (the unrolled loop, the single loop, the n & 3 tail; a non-zero out; one scratch for all launches), xl_adamw (one
    chunk, and a second grid-stride pass: flags with all of bits 0 / 1 / 2, chunk_steps, a binding and a loose clip, grad_scale
    1 and 1/4, zero_grad, a compute copy), xl_schedule_step (warm-up 0 and 5; steps 0, warmup - 1, warmup, total - 1, total + 3),
    the casts and the sparse fp32 side car at a size off 256"""
    n = 0
    scratch = ops.sumsq_scratch(dev) if hasattr(ops, "sumsq_scratch") else torch.zeros(516, device=dev)
    total = out(dev, 1, fill=torch.tensor([0.25]))
    for k in sumsq_n:
        data = rn(g, k)
        if k & 3:                                             # a tail that weighs in: three elements of 2.4 million would not
            data[k - (k & 3):] = 32.0
        ops.sumsq(inp(g, dev, data), total, k, scratch)
        n += 1
    for nn, flags, steps, clip, gs, zg, copy in ((256, False, False, None, 1.0, False, False), (256, True, True, "binding", 0.25, True, True),
                                                 (adamw_big, True, False, "loose", 1.0, True, True),
                                                 (adamw_big, True, True, "binding", 0.25, False, False),
                                                 (adamw_big, False, False, "binding", 0.25, False, True)):
        adamw_call(ops, dev, g, dtype, nn, flags, steps, clip, gs, zg, copy)
        n += 1
    i = 0
    for warmup in (0, 5):
        for done in ("0", "warmup-1", "warmup", "total-1", "total+3"):
            tot = 20 + i                                      # (a total of its own: every call is a signature of its own)
            i += 1
            d = {"0": 0, "warmup-1": warmup - 1, "warmup": warmup, "total-1": tot - 1, "total+3": tot + 3}[done]
            if d < 0:
                continue
            ops.schedule_step(out(dev, 1, torch.int64, fill=torch.tensor([d])), 1e-3, warmup, tot, 0.9, 0.999, out(dev, 4))
            n += 1
    k = 1000
    ops.cast_from_f32(inp(g, dev, rn(g, k)), out(dev, k, dtype), k)
    ops.cast_to_f32(inp(g, dev, rn(g, k, dtype=dtype)), out(dev, k), k)
    idx = torch.randperm(k, generator=g)[:300].to(torch.int32).to(dev)
    ops.take_f32(inp(g, dev, rn(g, k)), idx, 100, 700, out(dev, 300))
    ops.put_f32(out(dev, k, fill=rn(g, k)), idx, inp(g, dev, rn(g, 300)))
    return n + 4


# ------------------------------------------------------------------------------------------------------------------ rejected
def rejected(ops, dev, g, dtype, error):
    """calls the launchers refuse before any launch: each raises `error`, every output storage keeps its bits -> cases run"""
    import pytest
    V = vec(dtype)
    n = 0

    def refuse(outs, fn, code):
        nonlocal n
        raw = [(o, o.untyped_storage()) for o in outs]
        before = [torch.tensor([], dtype=torch.uint8, device=o.device).set_(st, 0, (st.nbytes(),), (1,)).clone() for o, st in raw]
        with pytest.raises(error, match=code):
            fn()
        for (o, st), was in zip(raw, before):
            now = torch.tensor([], dtype=torch.uint8, device=o.device).set_(st, 0, (st.nbytes(),), (1,))
            assert torch.equal(now, was), "a refused call wrote to an output"
        n += 1
    N = 4104 if dtype == BF else 2052                         # whole vectors, past NIT = 8
    M = 3
    gamma, beta = _affine(g, dev, N)
    x = inp(g, dev, rn(g, M, N, shift=3.0, dtype=dtype))
    y, mean, rstd = out2(dev, M, N, N, dtype), out(dev, M), out(dev, M)
    refuse([y, mean, rstd], lambda: ops.layernorm_fwd(x, gamma, beta, y, mean, rstd, M, N, EPS), r"\(-1\)")
    for Nb in (V + 1, 3):                                     # off VEC
        x = inp(g, dev, rn(g, M, 2 * V, dtype=dtype))
        y = out2(dev, M, 2 * V, 2 * V, dtype)
        refuse([y, mean, rstd], lambda: ops.layernorm_fwd(x, gamma, beta, y, mean, rstd, M, Nb, EPS), r"\(-1\)")
    N = 1032 if dtype == BF else 1028
    ids = torch.randint(1, 5, (2, 3), generator=g).to(dev)
    dpre = inp(g, dev, rn(g, 6, N, dtype=dtype))
    tabs = [out(dev, 5 * N, fill=rn(g, 5 * N)).view(5, N), out(dev, 3 * N, fill=rn(g, 3 * N)).view(3, N), out(dev, 2 * N, fill=rn(g, 2 * N)).view(2, N)]
    refuse(tabs, lambda: ops.embed_bwd(dpre, ids, None, *tabs, 2, 3, N), r"\(-1\)")
    lrs = inp(g, dev, torch.tensor([1e-3, 0.1, 0.1, 1.0]))
    st = adamw_state(g, dev, 260)
    refuse(st, lambda: ops.adamw(*st, None, None, None, lrs, 255, 0.9, 0.999, 1e-6, 0.0, 0.0), r"\(-1\)")
    refuse(st, lambda: ops.adamw(st[0][1:], st[1], st[2], st[3], None, None, None, lrs, 256, 0.9, 0.999, 1e-6, 0.0, 0.0), r"\(-3\)")
    N = 8
    xr = inp(g, dev, rn(g, M, N, shift=3.0), shift=1)
    gamma, beta = _affine(g, dev, N)
    y32, y16 = out2(dev, M, N, N, F32), out2(dev, M, N, N, BF)
    refuse([y32, y16, mean, rstd], lambda: ops.layernorm_fwd_res(xr, gamma, beta, y32, y16, mean, rstd, M, N, EPS), r"\(-3\)")
    P = 9
    N = 8 * V
    xv, pos = inp(g, dev, rn(g, M, N, dtype=dtype)), inp(g, dev, torch.rand(M, P, generator=g))
    wbox, bbox = inp(g, dev, rn(g, N, P)), inp(g, dev, rn(g, N))
    (gv, bv), (gb, bb) = _affine(g, dev, N), _affine(g, dev, N)
    y = out2(dev, M, N, N, dtype)
    st4 = [out(dev, M) for _ in range(4)]
    refuse([y] + st4, lambda: ops.visn_ln_fwd(xv, pos, wbox, bbox, gv, bv, gb, bb, y, *st4, M, N, P, EPS), r"\(-1\)")
    return n
