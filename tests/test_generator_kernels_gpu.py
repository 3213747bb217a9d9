"""The generator's kernels alone on the device (csrc/generator.hip): every output a view between guards, every element against float64
under the bounds derived in tests/generator_cases.py; refused arguments write nothing."""
import numpy as np
import pytest
import torch

import generator_cases as GC
from fake_ops_generator import normal_bits, normal_from_bits64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0


def _ops(dtype):
    from xlxmert_amd.ops import HipOps
    return HipOps(dtype)


def _conv_case(ops, dtype, B, H, W, Cin, Cout, ks, groups, epi, with_noise, seed, ldx=None, ldy=None, ldaux=None):
    """one xl_conv2d_nhwc call against float64; returns the worst |error| / bound"""
    gen = torch.Generator().manual_seed(seed)
    Cy = Cout // 2 if epi == 3 else Cout
    ldx, ldy, ldaux = ldx or Cin, ldy or Cy, ldaux or Cy
    Cg = Cin // groups
    g = GC.Guarded()
    x = g("x", (B, H, W, ldx), dtype, torch.randn(B, H, W, ldx, generator=gen))
    w = g("w", (ks * ks, Cout, Cg), dtype, torch.randn(ks * ks, Cout, Cg, generator=gen) / (ks * ks * Cg) ** 0.5)
    bias = g("bias", (Cout,), torch.float32, torch.randn(Cout, generator=gen) * 0.3)
    y = g("y", (B, H, W, ldy), dtype, torch.full((B, H, W, ldy), SENT))
    aux = mean = rstd = noise = None
    if epi in (2, 3):
        aux = g("aux", (B, H, W, ldaux), dtype, torch.randn(B, H, W, ldaux, generator=gen) * 2 + 1)
    if epi == 3:
        mean = g("mean", (B, Cy), torch.float32, torch.randn(B, Cy, generator=gen) * 0.5 + 1)
        rstd = g("rstd", (B, Cy), torch.float32, torch.rand(B, Cy, generator=gen) + 0.5)
        if with_noise:
            noise = g("noise", (B, H * W), torch.float32, torch.randn(B, H * W, generator=gen))
    ops.conv2d_nhwc(x, w, bias, y, B, H, W, Cin, Cout, ks, groups, ldx=ldx, ldy=ldy, epilogue=epi, aux=aux, ldaux=ldaux if aux is not None else 0,
                    mean=mean, rstd=rstd, noise=noise, noise_w=0.3, slope=0.2)
    torch.cuda.synchronize()
    g.check()
    assert bool((y[..., Cy:] == SENT).all()), "channels beyond Cout of a strided output were written"
    c = lambda t: None if t is None else t.cpu()          # noqa: E731
    ref, bound = GC.conv_reference(c(x)[..., :Cin], c(w), c(bias), B, H, W, Cin, Cout, ks, groups, epi, None if aux is None else c(aux)[..., :Cy],
                                   c(mean), c(rstd), c(noise), 0.3, 0.2, dtype)
    return GC.worst_ratio(y[..., :Cy], ref, bound)


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("cin,cout", GC.MFMA_CHANNELS)
def test_conv_mfma_channels_and_epilogues(cin, cout, ks):
    """bf16, every (Cin, Cout) of the MFMA path x every epilogue at 9 x 33 pixels (one tile extent plus one both ways), B = 3"""
    ops = _ops(torch.bfloat16)
    for epi, nz in GC.EPILOGUES:
        r = _conv_case(ops, torch.bfloat16, 3, 9, 33, cin, cout, ks, 1, epi, nz, seed=cin + cout + ks + epi)
        print(f"  conv mfma {cin}->{cout} ks={ks} epi={epi} noise={nz}: worst |err| / bound {r:.3f}")
        assert r <= 1.0, (epi, nz, r)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", GC.SPATIAL)
def test_conv_mfma_spatial(H, W, B):
    """bf16 32 -> 32 (conv1 / conv2) and 128 -> 64 as a SPADE with noise at every spatial case, the tile extent -1 / 0 / +1 included"""
    ops = _ops(torch.bfloat16)
    for cin, cout, ks, epi, nz in ((32, 32, 3, 0, False), (128, 64, 3, 3, True), (32, 32, 1, 2, False)):
        r = _conv_case(ops, torch.bfloat16, B, H, W, cin, cout, ks, 1, epi, nz, seed=H * 41 + W)
        assert r <= 1.0, (cin, cout, ks, epi, r)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,groups", GC.GENERIC_CHANNELS)
def test_conv_generic(cin, cout, groups, dtype):
    """the plain-FMA kernel: grouped, Cout = 3, Cout = 16; both element types, both kernel sizes, every epilogue it admits"""
    ops = _ops(dtype)
    for ks in (1, 3):
        for epi, nz in GC.EPILOGUES:
            if epi == 3 and (cout % 2 or groups != 1):
                continue
            for B, H, W in ((3, 7, 7), (1, 17, 9)):
                r = _conv_case(ops, dtype, B, H, W, cin, cout, ks, groups, epi, nz, seed=cin + cout + ks + epi)
                assert r <= 1.0, (ks, epi, nz, B, H, W, r)


@pytest.mark.parametrize("H,W", GC.SPATIAL)
def test_conv_fp32_at_the_mfma_shapes(H, W):
    """fp32 at channel counts that bf16 would run on the MFMA kernel: the generic kernel, fp32 bound"""
    ops = _ops(torch.float32)
    for epi, nz in ((0, False), (3, True)):
        assert _conv_case(ops, torch.float32, 3, H, W, 32, 64, 3, 1, epi, nz, seed=H + W) <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_pixel_strides_wider_than_the_channels(dtype):
    ops = _ops(dtype)
    assert _conv_case(ops, dtype, 3, 9, 33, 32, 32, 3, 1, 2, False, seed=5, ldx=48, ldy=40, ldaux=56) <= 1.0
    assert _conv_case(ops, dtype, 3, 9, 33, 128, 64, 3, 1, 3, True, seed=6, ldx=136, ldy=40, ldaux=48) <= 1.0
    assert _conv_case(ops, dtype, 2, 7, 7, 32, 3, 3, 1, 0, False, seed=7, ldx=33, ldy=5) <= 1.0


def test_conv_refuses_bad_arguments_without_writing():
    from xlxmert_amd._lib import XlError
    ops = _ops(torch.float32)
    g = GC.Guarded()
    B, H, W, C = 2, 4, 4, 8
    x, w = torch.zeros(B, H, W, C, device=DEV), torch.zeros(9, C, C, device=DEV)
    bias, aux = torch.zeros(C, device=DEV), torch.zeros(B, H, W, C, device=DEV)
    st = torch.ones(B, C, device=DEV)
    y = g("y", (B, H, W, C), torch.float32, torch.full((B, H, W, C), SENT))

    def bad(**kw):
        a = dict(x=x, w=w, bias=bias, y=y, B=B, H=H, W=W, Cin=C, Cout=C, ks=3, groups=1, ldx=C, ldy=C, epilogue=0, aux=None, ldaux=0,
                 mean=None, rstd=None)
        a.update(kw)
        with pytest.raises(XlError):
            ops.conv2d_nhwc(**a)
    bad(ks=2)
    bad(ks=5)
    bad(B=0)
    bad(H=0)
    bad(Cin=0)
    bad(groups=3)
    bad(groups=0)
    bad(ldx=C - 1)
    bad(ldy=C - 1)
    bad(epilogue=4)
    bad(epilogue=-1)
    bad(epilogue=2)                                 # ADD without aux
    bad(epilogue=2, aux=aux, ldaux=C - 1)
    bad(epilogue=3, aux=aux, ldaux=C)               # SPADE without statistics
    bad(epilogue=3, aux=aux, ldaux=C, mean=st, rstd=st, Cout=7, ldy=3)
    bad(epilogue=3, aux=aux, ldaux=C, mean=st, rstd=st, groups=2)
    bad(w=None)
    bad(B=1 << 20, H=1 << 6, W=1 << 6)              # B*H*W*ld reaches 2^31
    torch.cuda.synchronize()
    g.check(unchanged=("y",))
    assert "xl_conv2d_nhwc" in ops.lib.raw("xl_last_error")().decode()


# ---------------------------------------------------------------------------------------------- statistics
def _stats_case(ops, dtype, x):
    B, HW, C = x.shape
    g = GC.Guarded()
    xd = g("x", (B, HW, C), dtype, x)
    mean, rstd = g("mean", (B, C), torch.float32), g("rstd", (B, C), torch.float32)
    ws = g("ws", (ops.instnorm_ws_floats(B, HW, C),), torch.float32)
    ops.instnorm_stats(xd, mean, rstd, ws, B, HW, C, C)
    torch.cuda.synchronize()
    g.check()
    m_ref, r_ref, m_b, r_b = GC.stats_reference(xd.cpu())
    return GC.worst_ratio(mean, m_ref, m_b), GC.worst_ratio(rstd, r_ref, r_b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("HW", [1, 49, 64, 1025, 65536])
def test_instnorm_stats(HW, dtype):
    ops = _ops(dtype)
    gen = torch.Generator().manual_seed(HW)
    for C in (3, 16, 32):
        rm, rr = _stats_case(ops, dtype, torch.randn(2, HW, C, generator=gen) * 1.5 + 0.3)
        print(f"  stats HW={HW} C={C} {dtype}: mean {rm:.3f} rstd {rr:.3f} of the bound")
        assert rm <= 1.0 and rr <= 1.0


@pytest.mark.parametrize("HW", [49, 1025, 65536])
def test_instnorm_stats_constant_and_offset_planes(HW):
    """a constant plane (variance exactly 0: rstd = eps^-1/2) and the mean-100 / std-0.1 plane, fp32"""
    ops = _ops(torch.float32)
    gen = torch.Generator().manual_seed(HW)
    rm, rr = _stats_case(ops, torch.float32, torch.full((2, HW, 16), 3.25))
    assert rm <= 1.0 and rr <= 1.0
    rm, rr = _stats_case(ops, torch.float32, torch.randn(2, HW, 16, generator=gen) * 0.1 + 100.0)
    print(f"  stats mean-100 / std-0.1 HW={HW}: mean {rm:.3f} rstd {rr:.3f} of the bound")
    assert rm <= 1.0 and rr <= 1.0


# ---------------------------------------------------------------------------------------------- resize, ToRGB tail
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("r_in,r_out", [(8, 16), (7, 14), (8, 32), (16, 16), (5, 12)])
def test_resize_bilinear(r_in, r_out, dtype):
    ops = _ops(dtype)
    gen = torch.Generator().manual_seed(r_in * 100 + r_out)
    for B, C, ldx, ldy in ((3, 16, 16, 16), (2, 5, 7, 9)):
        g = GC.Guarded()
        x = g("x", (B, r_in, r_in, ldx), dtype, torch.randn(B, r_in, r_in, ldx, generator=gen))
        y = g("y", (B, r_out, r_out, ldy), dtype, torch.full((B, r_out, r_out, ldy), SENT))
        ops.resize_bilinear_nhwc(x, y, B, r_in, r_in, r_out, r_out, C, ldx, ldy)
        torch.cuda.synchronize()
        g.check()
        assert bool((y[..., C:] == SENT).all())
        ref, bound = GC.resize_reference(x.cpu()[..., :C], r_out, r_out, dtype)
        assert GC.worst_ratio(y[..., :C], ref, bound) <= 1.0
    # a non-square case
    g = GC.Guarded()
    x = g("x", (2, 5, 8, 4), dtype, torch.randn(2, 5, 8, 4, generator=gen))
    y = g("y", (2, 12, 9, 4), dtype)
    ops.resize_bilinear_nhwc(x, y, 2, 5, 8, 12, 9, 4)
    torch.cuda.synchronize()
    g.check()
    ref, bound = GC.resize_reference(x.cpu(), 12, 9, dtype)
    assert GC.worst_ratio(y, ref, bound) <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_torgb_accumulates_and_applies_tanh_last(dtype):
    ops = _ops(dtype)
    gen = torch.Generator().manual_seed(9)
    B, T = 3, 28
    g = GC.Guarded()
    acc, out = g("acc", (B, 3, T, T), torch.float32), g("out", (B, 3, T, T), torch.float32)
    total = torch.zeros(B, 3, T, T, dtype=torch.float64)
    bound = torch.zeros_like(total)
    for i, r in enumerate((7, 14, 28)):
        rgb = g(f"rgb{r}", (B, r, r, 3), dtype, torch.randn(B, r, r, 3, generator=gen) * 0.6)
        ops.torgb_accum(rgb, acc, out if r == T else None, B, r, T, 3, first=i == 0)
        up, b = GC.resize_reference(rgb.cpu(), T, T, torch.float32)
        total += up.permute(0, 3, 1, 2)
        bound += b.permute(0, 3, 1, 2) + 2 * GC.U32 * total.abs()
    torch.cuda.synchronize()
    g.check()
    assert GC.worst_ratio(acc, total, bound) <= 1.0
    # tanhf: <= 5 ulp of a value <= 1, and 1-Lipschitz in the sum
    assert GC.worst_ratio(out, torch.tanh(total), bound + 6 * 2.0 ** -24) <= 1.0


# ---------------------------------------------------------------------------------------------- normal planes
def test_normal_planes_hash_is_exact_and_transform_within_bound():
    ops = _ops(torch.float32)
    B, P, seed, site = 3, 1000, 0x1234_5678_9ABC_DEF0, 5
    g = GC.Guarded()
    out = g("out", (B, P), torch.float32)
    ops.normal_planes(out, seed, site, B, P)
    h0, h1 = normal_bits(seed, site, B, P)
    z = g("z", (B * P,), torch.float32)
    ops.normal_from_bits(torch.from_numpy(h0.view(np.int32).reshape(-1)).to(DEV),
                         torch.from_numpy(h1.view(np.int32).reshape(-1)).to(DEV), z, B * P)
    torch.cuda.synchronize()
    g.check()
    # the device's own hash and the host's hash fed through the same float code: identical bits = the integer part agrees
    assert torch.equal(out.view(-1), z)
    ref = torch.from_numpy(normal_from_bits64(h0, h1)).view(-1)
    err = float((z.double().cpu() - ref).abs().max())
    print(f"  normal planes: worst |z - z64| = {err:.3e} (bound {GC.NORMAL_ABS:.3e})")
    assert err <= GC.NORMAL_ABS
    other = torch.empty(B, P, device=DEV)
    ops.normal_planes(other, seed, site + 1, B, P)
    assert not torch.equal(other, out)


def test_normal_planes_moments():
    """2^20 draws at a fixed seed: the mean within 5 / sqrt(n), the variance within 5 sqrt(2 / n)"""
    ops = _ops(torch.float32)
    n = 1 << 20
    out = torch.empty(4, n // 4, device=DEV)
    ops.normal_planes(out, 20240229, 0, 4, n // 4)
    z = out.double().view(-1)
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    print(f"  normal planes: mean {mean:.5f} var {var:.5f} over {n} draws")
    assert abs(mean) <= 5 / n ** 0.5 and abs(var - 1.0) <= 5 * (2 / n) ** 0.5


def test_the_other_kernels_refuse_bad_arguments_without_writing():
    from xlxmert_amd._lib import XlError
    ops = _ops(torch.float32)
    g = GC.Guarded()
    x = torch.zeros(2, 16, 4, device=DEV)
    mean, rstd, ws = g("mean", (2, 4), torch.float32), g("rstd", (2, 4), torch.float32), g("ws", (16,), torch.float32)
    y, acc, z = g("y", (2, 8, 8, 4), torch.float32), g("acc", (2, 3, 8, 8), torch.float32), g("z", (2, 16), torch.float32)
    names = ("mean", "rstd", "ws", "y", "acc", "z")
    for call in (lambda: ops.instnorm_stats(x, mean, rstd, ws, 2, 16, 4, 3),                # pixel stride below the channels
                 lambda: ops.instnorm_stats(x, mean, rstd, ws, 2, 0, 4, 4),
                 lambda: ops.instnorm_stats(x, mean, rstd, ws[:8], 2, 16, 4, 4),            # workspace too small
                 lambda: ops.instnorm_stats(x, mean, rstd, ws, 2, 16, 4, 4, eps=0.0),
                 lambda: ops.resize_bilinear_nhwc(x, y, 2, 4, 4, 8, 8, 4, 3, 4),
                 lambda: ops.resize_bilinear_nhwc(x, y, 2, 4, 4, 0, 8, 4),
                 lambda: ops.torgb_accum(x, acc, None, 2, 4, 8, 2),                         # ld below 3
                 lambda: ops.torgb_accum(x, acc, None, 0, 4, 8, 3),
                 lambda: ops.normal_planes(z, 1, -1, 2, 16),
                 lambda: ops.normal_planes(z, 1, 0, 2, 0)):
        with pytest.raises(XlError):
            call()
    torch.cuda.synchronize()
    g.check(unchanged=names)
