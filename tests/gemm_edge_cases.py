"""The calls of tests/test_gemm_edges_bounds_gpu.py and of the host tests of tests/test_bounds_cpu.py: xl_gemm and
xl_gemm_wgrad_group at the edges of their dispatch (csrc/gemm.hip).  Plain functions, no tests: each takes a recorder-like `ops`
(tests/test_kernel_bounds_gpu.Recorder over HipOps or over the host restatement), a device and a seeded CPU generator -- the data is
drawn on the host and moved, so both sides run the same numbers -- issues its calls and returns how many it issued.  Every call has
a signature of its own (shape, leading dimensions, layout, epilogue, output type, alignment), so the recorder checks every one.

Data: bf16; A of order 1, B of order K^-1/2, bias of order 0.5; the operands of the epilogue family are spread to |x| ~ 10 (A and
aux of scale 3).  PADS CARRY POISON: every element of A and B (and of a residual / aux operand) outside the logical extents -- the
leading-dimension pad, one whole row past the extent, the element in front of a shifted base -- is +-2^12, finite, so that one pad
element entering as a K term overshoots any bound by orders of magnitude (finite, because a kernel may load pad elements into
accumulators it never stores).  Outputs are allocated one row taller than M; their pads hold SENTINEL for the recorder's
stray-store guard.

Leading dimensions of an operand whose contiguous extent is n:
  tight    n rounded up to 8            the last 16-byte piece of a row holds pad elements
  padded   tight + 8
  odd      n + 1 (n + 2 if that is a multiple of 8)        -> the generic 64x64 kernel
  shifted  padded, base pointer advanced by one element: ld % 8 == 0 but the pointer is off 16 bytes  -> the generic 64x64 kernel"""
import torch

import bounds as BD

BF = torch.bfloat16
POISON = 4096.0
SENTINEL = 12345.0
LAYOUTS = ((1, 1), (1, 0), (0, 1), (0, 0))            # (a_kmajor, b_kmajor): forward NT, dX NN, TN, dW TT
SHAPES = ((1, 8, 8), (1, 257, 72), (257, 1, 72), (33, 31, 3), (64, 64, 1), (127, 129, 65), (129, 127, 137), (255, 257, 200),
          (257, 255, 264), (393, 391, 1000), (511, 513, 1031))
F32_SHAPES = ((33, 31, 3), (127, 129, 65), (257, 255, 264), (511, 513, 1031))
# (policy of A, policy of B): both MFMA policies, then each generic-kernel policy on either operand
LD_MFMA = (("tight", "tight"), ("padded", "padded"))
LD_GENERIC = (("odd", "tight"), ("tight", "odd"), ("shifted", "padded"), ("padded", "shifted"))
EPILOGUES = ((BD.EPI_NONE, 0.0), (BD.EPI_GELU, 0.0), (BD.EPI_RESIDUAL, 0.1), (BD.EPI_DGELU, 0.0), (BD.EPI_GELU_DG, 0.0),
             (BD.EPI_TANH, 0.0), (BD.EPI_MULAUX, 0.0))
EPI_SHAPES = ((255, 257, 200), (129, 264, 72))
DUO_SHAPES = ((128, 192, 8), (256, 384, 72), (384, 192, 1000))
KSPLIT_MN = ((129, 255), (257, 300))
KSPLIT_K = (1024, 1096, 1544, 2056)
TAIL_SHAPE = (4300, 4090, 1096)                       # 17 x 16 = 272 tiles of 256x256: one round and a remainder of 16
WGRAD_PROBLEMS = ((3129, 136), (257, 255), (64, 1031))


def up8(n):
    return (n + 7) // 8 * 8


def ld_of(extent, policy):
    if policy == "tight":
        return up8(extent)
    if policy in ("padded", "shifted"):
        return up8(extent) + 8
    assert policy == "odd", policy
    return extent + 1 if (extent + 1) % 8 else extent + 2


def _poison(g, n, dtype=BF):
    return ((torch.randint(0, 2, (n,), generator=g) * 2 - 1).float() * POISON).to(dtype)


def operand(g, dev, rows, cols, policy="tight", scale=1.0, dtype=BF):
    """[rows, cols] random data of `scale` inside a poisoned allocation of rows + 1 rows of ld_of(cols, policy) -> (tensor whose
    data pointer is the operand's base, ld)"""
    ld = ld_of(cols, policy)
    off = 1 if policy == "shifted" else 0
    buf = _poison(g, (rows + 1) * ld + off, dtype)
    torch.as_strided(buf, (rows, cols), (ld, 1), off).copy_((torch.randn(rows, cols, generator=g) * scale).to(dtype))
    return buf.to(dev)[off:], ld


def a_operand(g, dev, M, K, a_kmajor, policy, scale=1.0):
    return operand(g, dev, M, K, policy, scale) if a_kmajor else operand(g, dev, K, M, policy, scale)


def b_operand(g, dev, N, K, b_kmajor, policy):
    return operand(g, dev, N, K, policy, K ** -0.5) if b_kmajor else operand(g, dev, K, N, policy, K ** -0.5)


def output(g, dev, M, N, ld, dtype, fill=None):
    """an [M, N] output inside (M + 1) rows of ld: SENTINEL everywhere, random data of scale `fill` in the view when given"""
    buf = torch.full(((M + 1) * ld,), SENTINEL, dtype=dtype)
    if fill is not None:
        torch.as_strided(buf, (M, N), (ld, 1)).copy_((torch.randn(M, N, generator=g) * fill).to(dtype))
    return buf.to(dev)


def bias_of(g, dev, N, shifted=False):
    b = torch.full((N + 9,), SENTINEL)
    off = 1 if shifted else 0
    b[off:off + N] = torch.randn(N, generator=g) * 0.5
    return b.to(dev)[off:]


# ------------------------------------------------------------------------------------------------------------------ families
def shapes(ops, dev, g, lds=LD_MFMA + LD_GENERIC, shapes_=SHAPES, f32_shapes=F32_SHAPES, layouts=LAYOUTS):
    """every shape x layout x leading-dimension policy: bf16 out, bias, EPI_NONE; a subset again with fp32 output"""
    n = 0
    for out_f32, shp in ((False, shapes_), (True, f32_shapes)):
        for M, N, K in shp:
            for ak, bk in layouts:
                for pa, pb in (lds if not out_f32 else lds[:1] + lds[2:3]):
                    A, lda = a_operand(g, dev, M, K, ak, pa)
                    B, ldb = b_operand(g, dev, N, K, bk, pb)
                    ldc = up8(N) if pa == "tight" else up8(N) + 8
                    C = output(g, dev, M, N, ldc, torch.float32 if out_f32 else BF)
                    ops.gemm(A, B, C, bias_of(g, dev, N), None, None, M, N, K, lda, ldb, ldc, a_kmajor=ak, b_kmajor=bk, out_f32=out_f32)
                    n += 1
    return n


def epilogues(ops, dev, g, shapes_=EPI_SHAPES, layouts=LAYOUTS):
    """all seven epilogues x layout at two ragged shapes, with (a) 16-byte rows of C / residual / aux, (b) rows off 8 elements --
    the scalar epilogue everywhere --, (c) 16-byte rows but the bias pointer advanced by one float -- no templated epilogue; and
    one call with alpha = 0.125 (fp32 out, so that it is a signature of its own)"""
    n = 0
    for M, N, K in shapes_:
        for ak, bk in layouts:
            A, lda = a_operand(g, dev, M, K, ak, "padded", scale=3.0)
            B, ldb = b_operand(g, dev, N, K, bk, "padded")
            for variant in "abc":
                pol = "odd" if variant == "b" else "padded"
                bias = bias_of(g, dev, N, shifted=variant == "c")
                res, ldr = operand(g, dev, M, N, pol)
                aux_in, ldx = operand(g, dev, M, N, pol, scale=3.0)
                ldc = ldr
                for epi, p in EPILOGUES:
                    C = output(g, dev, M, N, ldc, BF)
                    aux = output(g, dev, M, N, ldx, BF) if epi in (BD.EPI_GELU, BD.EPI_GELU_DG) else aux_in.clone()
                    ops.gemm(A, B, C, bias, res, aux, M, N, K, lda, ldb, ldc, ldr=ldr, ldx=ldx, a_kmajor=ak, b_kmajor=bk, epilogue=epi,
                             p_drop=p, seed=11)
                    n += 1
    M, N, K = shapes_[0]
    A, lda = a_operand(g, dev, M, K, 1, "padded")
    B, ldb = b_operand(g, dev, N, K, 1, "padded")
    ldc = up8(N) + 8
    ops.gemm(A, B, output(g, dev, M, N, ldc, torch.float32), bias_of(g, dev, N), None, None, M, N, K, lda, ldb, ldc, out_f32=True,
             alpha=0.125)
    return n + 1


def colsums(ops, dev, g, Ms=(64, 65, 256, 300), Ns=(256, 264)):
    """column sums of C added into a non-zero fp32 target: fused into the epilogue when every tile is whole, a pass of its own
    otherwise; forward and dX layouts"""
    n = 0
    for M in Ms:
        for N in Ns:
            for ak, bk in ((1, 1), (1, 0)):
                K = 136
                A, lda = a_operand(g, dev, M, K, ak, "padded")
                B, ldb = b_operand(g, dev, N, K, bk, "padded")
                ldc = N + 8
                C = output(g, dev, M, N, ldc, BF)
                cs = torch.full((N + 8,), SENTINEL)
                cs[:N] = torch.randn(N, generator=g)
                cs = cs.to(dev)
                ws = torch.zeros(ops.workspace_floats(N), device=dev)
                ops.gemm(A, B, C, bias_of(g, dev, N), None, None, M, N, K, lda, ldb, ldc, a_kmajor=ak, b_kmajor=bk, colsum=cs, ws=ws)
                n += 1
    return n


def ksplits(ops, dev, g, mn=KSPLIT_MN, Ks=KSPLIT_K):
    """fp32 out, EPI_NONE, deep K and few tiles: the K split (last slice short wherever K is no multiple of the rounded slice),
    accumulate 0 (C cleared through the strided memset, ldc > N) and 1, over a C that holds order-1 data"""
    n = 0
    for M, N in mn:
        for K in Ks:
            for ak, bk in ((0, 0), (1, 1)):
                A, lda = a_operand(g, dev, M, K, ak, "tight")
                B, ldb = b_operand(g, dev, N, K, bk, "tight")
                ldc = N + 8
                for acc in (0, 1):
                    C = output(g, dev, M, N, ldc, torch.float32, fill=1.0)
                    ops.gemm(A, B, C, None, None, None, M, N, K, lda, ldb, ldc, a_kmajor=ak, b_kmajor=bk, out_f32=True, accumulate=acc)
                    n += 1
    return n


def tail_split(ops, dev, g, shape=TAIL_SHAPE):
    """more than one round of 256x256 tiles with a short last round (caller: set_gemm_tail_split(64, 1024) and a registered
    workspace): forward layout with EPI_RESIDUAL (dropout on), dX layout with EPI_NONE"""
    M, N, K = shape
    ldc = up8(N) + 8
    for (ak, bk), epi, p in (((1, 1), BD.EPI_RESIDUAL, 0.1), ((1, 0), BD.EPI_NONE, 0.0)):
        A, lda = a_operand(g, dev, M, K, ak, "padded")
        B, ldb = b_operand(g, dev, N, K, bk, "padded")
        res, ldr = operand(g, dev, M, N, "padded")
        ops.gemm(A, B, output(g, dev, M, N, ldc, BF), bias_of(g, dev, N), res, None, M, N, K, lda, ldb, ldc, ldr=ldr, a_kmajor=ak,
                 b_kmajor=bk, epilogue=epi, p_drop=p, seed=13)
    return 2


def duo(ops, dev, g, shapes_=DUO_SHAPES):
    """M % 128 == N % 192 == 0 in the forward and dX layouts (caller: set_gemm_duo(2)): EPI_NONE and a GELU-family epilogue"""
    n = 0
    for M, N, K in shapes_:
        for (ak, bk), epi2 in (((1, 1), BD.EPI_GELU), ((1, 0), BD.EPI_DGELU)):
            A, lda = a_operand(g, dev, M, K, ak, "padded", scale=3.0)
            B, ldb = b_operand(g, dev, N, K, bk, "padded")
            ldc = N + 8
            aux_in, ldx = operand(g, dev, M, N, "padded", scale=3.0)
            for epi in (BD.EPI_NONE, epi2):
                aux = output(g, dev, M, N, ldx, BF) if epi == BD.EPI_GELU else aux_in.clone()
                ops.gemm(A, B, output(g, dev, M, N, ldc, BF), bias_of(g, dev, N), None, aux, M, N, K, lda, ldb, ldc, ldx=ldx, a_kmajor=ak,
                         b_kmajor=bk, epilogue=epi)
                n += 1
    return n


def _wgrad_problem(g, dev, M, N, K, ldc):
    A, lda = operand(g, dev, K, M, "tight")
    B, ldb = operand(g, dev, K, N, "tight", scale=K ** -0.5)
    return (A, B, output(g, dev, M, N, ldc, torch.float32, fill=1.0), M, N, K, lda, ldb, ldc)


def wgrad_groups(ops, dev, g, Ks=(72, 2056, 4104), mn=WGRAD_PROBLEMS):
    """one launch of three ragged problems dW_i (+)= dY_i^T X_i, overwrite bits 0b101 over non-zero C (the middle one accumulates,
    into rows off 16 bytes); then the same with one member's K = 1031 (K % 8 != 0: one xl_gemm per member), and a launch of one
    problem with an odd N.  With the library's thresholds (a grouped launch needs >= 96 workgroups: 20 tiles x K / 512 splits) the
    launches of K = 72 and 2056 run as one xl_gemm per member, K = 4104 as ONE grouped launch split 8 ways."""
    n = 0
    for K in Ks:
        probs = [_wgrad_problem(g, dev, M, N, K, ld_of(N, "odd") if i == 1 else up8(N) + 8) for i, (M, N) in enumerate(mn)]
        ops.gemm_wgrad_group(probs, 0b101)
        n += 1
    probs = [_wgrad_problem(g, dev, M, N, 1031 if i == 1 else 2056, up8(N) + 8) for i, (M, N) in enumerate(mn)]
    ops.gemm_wgrad_group(probs, 0b101)
    ops.gemm_wgrad_group([_wgrad_problem(g, dev, 300, 255, 1096, 256)], 0)
    return n + 2
