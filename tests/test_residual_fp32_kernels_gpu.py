"""The kernels of the fp32 residual stream against the float64 restatement, element by element within the bounds of tests/bounds.py
(the recording proxy of tests/test_kernel_bounds_gpu.py, extended in tests/residual_checks.py): xl_gemm's XL_EPI_RESIDUAL_F32 at the
training step's shapes and off the tile grid, on every kernel the dispatch can select, and xl_layernorm_fwd_res /
xl_layernorm_bwd_res, eager and with deferred column sums.  Exact checks: y16 = bf16(y32), dx_dropped = bf16(dx) without dropout,
and the kept / dropped pattern of both dropout sites equals the bf16 entry points' for the same seed."""
import time

import pytest
import torch

import bounds as BD
from residual_checks import RecorderRes, bits
from test_kernel_bounds_gpu import _done, _table

pytestmark = pytest.mark.gpu


def _rec():
    from xlxmert_amd.ops import HipOps
    return RecorderRes(HipOps(torch.bfloat16))


def _rn(g, *shape, scale=1.0, dtype=torch.bfloat16):
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)


def _res_gemm(rec, g, M, N, K, b_kmajor, p_drop, pad=0, seed=11):
    """one XL_EPI_RESIDUAL_F32 launch through the recorder (bf16 A / B, fp32 residual and output)"""
    lda, ldc = K + pad, N + pad
    ldb = (K if b_kmajor else N) + pad
    A = _rn(g, M, lda, scale=2.0)
    W = _rn(g, N if b_kmajor else K, ldb, scale=1.0 / K ** 0.5)
    bias = torch.randn(N, generator=g, device="cuda") * 0.5 if b_kmajor else None
    res = _rn(g, M, ldc, scale=3.0, dtype=torch.float32)
    C = torch.zeros(M, ldc, dtype=torch.float32, device="cuda")
    rec.gemm(A, W, C, bias, res, None, M, N, K, lda, ldb, ldc, ldr=ldc, a_kmajor=1, b_kmajor=b_kmajor, out_f32=True,
             epilogue=BD.EPI_RESIDUAL, p_drop=p_drop, seed=seed)
    return C


@pytest.mark.parametrize("pingpong", [1, 2, 0], ids=["default_dispatch", "pingpong_forced", "tile128_only"])
def test_residual_f32_epilogue_at_the_step_shapes_within_bounds(pingpong):
    """the visual side (16384 rows: ping-pong 256x256) and a packed language side (3328 rows: the 128x192 duo tiles by default, the
    128x128 MFMA kernel with the ping-pong family off), N 768, K 768 and 3072, forward and dX layouts, dropout off and on"""
    t0 = time.time()
    rec = _rec()
    rec.set_gemm_pingpong(pingpong)
    if pingpong == 0:
        rec.set_gemm_duo(0)
    g = torch.Generator(device="cuda").manual_seed(17)
    n = 0
    for M in (16384, 3328):
        for K, b_kmajor, p in ((768, 1, 0.1), (3072, 1, 0.1), (768, 1, 0.0), (2304, 0, 0.0), (3072, 0, 0.0)):
            _res_gemm(rec, g, M, 768, K, b_kmajor, p)
            n += 1
    _done(rec, t0, n)


@pytest.mark.parametrize("pingpong", [1, 2, 0], ids=["default_dispatch", "pingpong_forced", "tile128_only"])
def test_residual_f32_epilogue_ragged_tiles_padded_ld_and_generic_kernel_within_bounds(pingpong):
    """M, N off the tile grid with leading dimensions padded by 8 (interior tiles take the vector epilogue, edge tiles the scalar
    one); leading dimensions padded by 4 (fp32 rows stay 16-byte aligned, the bf16 operands do not: the generic 64x64 kernel);
    in place (C is the residual: Engine.gemm_dx_plain)"""
    t0 = time.time()
    rec = _rec()
    rec.set_gemm_pingpong(pingpong)
    g = torch.Generator(device="cuda").manual_seed(23)
    for M, N, K in ((300, 264, 200), (520, 776, 840)):
        for b_kmajor in (1, 0):
            for p in (0.0, 0.1):
                _res_gemm(rec, g, M, N, K, b_kmajor, p, pad=8)
        _res_gemm(rec, g, M, N, K, 1, 0.1, pad=4)
    M, N, K = 512, 768, 1536
    A, W = _rn(g, M, K), _rn(g, K, N, scale=1.0 / K ** 0.5)
    C = _rn(g, M, N, dtype=torch.float32)
    rec.gemm(A, W, C, None, C, None, M, N, K, K, N, N, ldr=N, a_kmajor=1, b_kmajor=0, out_f32=True, epilogue=BD.EPI_RESIDUAL)
    _done(rec, t0, 11)


def test_residual_f32_epilogue_drops_what_the_bf16_epilogue_drops():
    """same seed, same (row, column) hash: with a zero residual the dropped positions are the zeros of the output, in both epilogues,
    on the vector path (whole tiles), the scalar path (ragged edges) and with a step seed registered"""
    from xlxmert_amd.ops import HipOps
    ops = HipOps(torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(29)
    step = torch.tensor([12345], dtype=torch.int64, device="cuda")
    for M, N, K, with_step in ((16384, 768, 768, False), (3328, 768, 768, True), (300, 264, 200, False)):
        A, W = _rn(g, M, K, scale=2.0), _rn(g, N, K, scale=1.0 / K ** 0.5)
        C16 = torch.ones(M, N, dtype=torch.bfloat16, device="cuda")
        C32 = torch.ones(M, N, dtype=torch.float32, device="cuda")
        ops.set_step_seed_ptr(step if with_step else None)
        ops.gemm(A, W, C16, None, torch.zeros_like(C16), None, M, N, K, K, K, N, ldr=N, epilogue=BD.EPI_RESIDUAL, p_drop=0.1, seed=7)
        ops.gemm(A, W, C32, None, torch.zeros_like(C32), None, M, N, K, K, K, N, ldr=N, out_f32=True, epilogue=BD.EPI_RESIDUAL,
                 p_drop=0.1, seed=7)
        ops.set_step_seed_ptr(None)
        torch.cuda.synchronize()
        z32 = C32 == 0
        frac = z32.float().mean().item()
        print(f"M={M} N={N}: dropped {frac:.4f}")
        assert 0.08 < frac < 0.12
        # (a kept bf16 product can round to zero only if its fp32 value is below 2^-133: never here)
        BD.check_exact(C16 == 0, z32, "dropped positions, bf16 against fp32 residual epilogue")
        # the kept values: the bf16 epilogue stores the rounding of what the fp32 one stores (same accumulator, same scale)
        BD.check_exact(bits(C16), bits(C32.to(torch.bfloat16)), "kept values")


def _ln_inputs(g, M, N):
    x = torch.randn(M, N, generator=g, device="cuda") * 1.5 + 0.3
    dy = torch.randn(M, N, generator=g, device="cuda") * 0.01
    gamma = 1.0 + 0.1 * torch.randn(N, generator=g, device="cuda")
    beta = 0.1 * torch.randn(N, generator=g, device="cuda")
    return x, dy, gamma, beta


@pytest.mark.parametrize("M,N", [(16384, 768), (3328, 768), (261, 768), (37, 64), (16, 1536)])
def test_layernorm_fwd_res_within_bounds_and_bf16_copy_exact(M, N):
    t0 = time.time()
    rec = _rec()
    g = torch.Generator(device="cuda").manual_seed(31)
    x, _, gamma, beta = _ln_inputs(g, M, N)
    y32 = torch.zeros(M, N, device="cuda")
    y16 = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    mean, rstd = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
    rec.layernorm_fwd_res(x, gamma, beta, y32, y16, mean, rstd, M, N, 1e-12)
    _done(rec, t0, 4)


@pytest.mark.parametrize("deferred", [False, True], ids=["eager", "deferred"])
@pytest.mark.parametrize("M,N", [(16384, 768), (3328, 768), (261, 768), (37, 64)])
def test_layernorm_bwd_res_within_bounds_eager_and_deferred(M, N, deferred):
    """dx fp32, dx_dropped bf16 written with and without dropout, dgamma / dbeta / dbias_prev accumulated onto non-zero contents
    through the workspace (second stage at once, or at xl_flush_reductions) and -- no workspace -- through atomics"""
    t0 = time.time()
    rec = _rec()
    g = torch.Generator(device="cuda").manual_seed(37)
    x, dy, gamma, beta = _ln_inputs(g, M, N)
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-12)
    outs = []
    if deferred:
        rec.set_deferred_reduce(1)
    try:
        for p, with_ws, with_bias in ((0.0, True, True), (0.1, True, True), (0.1, True, False)) + (() if deferred else ((0.0, False, True),)):
            dx = torch.zeros(M, N, device="cuda")
            dd = torch.ones(M, N, dtype=torch.bfloat16, device="cuda")
            dgm, dbt, dbp = (torch.randn(N, generator=g, device="cuda") for _ in range(3))
            ws = torch.zeros(rec.workspace_floats(N), device="cuda") if with_ws else None
            rec.layernorm_bwd_res(dy, x, gamma, mean, rstd, dx, dgm, dbt, dbp if with_bias else None, M, N, ws=ws, dx_dropped=dd,
                                  p_drop=p, seed=5)
            outs.append((dx, dd, dgm, dbt, dbp, ws))
        if deferred:
            rec.flush_reductions()
    finally:
        if deferred:
            rec.set_deferred_reduce(0)
    assert not rec.leftover(), rec.leftover()
    if deferred:
        assert rec.flushes_checked == 1
    _done(rec, t0, 3 * 3 + (8 if deferred else 8 + 6))


def test_layernorm_bwd_res_drops_what_layernorm_bwd_drops():
    """the same seed gives the same kept / dropped pattern as xl_layernorm_bwd (plain and LDS-DMA kernels), step seed included"""
    from xlxmert_amd.ops import HipOps
    ops = HipOps(torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(41)
    step = torch.tensor([777], dtype=torch.int64, device="cuda")
    for M, N in ((16384, 768), (261, 768)):
        x, dy, gamma, _ = _ln_inputs(g, M, N)
        mean = x.mean(1)
        rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-12)
        dgm, dbt = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        dx32, dd32 = torch.zeros(M, N, device="cuda"), torch.ones(M, N, dtype=torch.bfloat16, device="cuda")
        dx16, dd16 = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda"), torch.ones(M, N, dtype=torch.bfloat16, device="cuda")
        ops.set_step_seed_ptr(step)
        ops.layernorm_bwd_res(dy, x, gamma, mean, rstd, dx32, dgm, dbt, None, M, N, dx_dropped=dd32, p_drop=0.1, seed=9)
        ops.layernorm_bwd(dy.bfloat16(), x.bfloat16(), gamma, mean, rstd, dx16, dgm, dbt, None, M, N, dx_dropped=dd16, p_drop=0.1, seed=9)
        ops.set_step_seed_ptr(None)
        torch.cuda.synchronize()
        live = (dx32 != 0) & (dx16 != 0)
        frac = ((dd32 == 0) & live).float().mean().item()
        print(f"M={M}: dropped {frac:.4f}")
        assert 0.08 < frac < 0.12
        BD.check_exact((dd32 == 0) & live, (dd16 == 0) & live, "dropped positions, fp32-stream against bf16 LayerNorm backward")
