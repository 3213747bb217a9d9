"""TEST INFRASTRUCTURE: the host restatement of the image generator's device calls (include/xlxmert_hip.h, section "image generator") on top
of tests/fake_ops.FakeOps -- each call restated with torch.nn.functional on the CPU, from the header's rules alone:

conv2d_nhwc           w [ks*ks, Cout, Cin/groups] -> torch's [Cout, Cin/groups, kh, kw]; zero pad ks // 2; the four epilogues
instnorm_stats        mean and 1 / sqrt(biased variance + eps) over the pixels
resize_bilinear_nhwc  F.interpolate(mode="bilinear", align_corners=False)
torgb_accum           acc (+)= F.interpolate(rgb -> T x T); out = tanh(acc)
normal_planes         the integer hash restated in numpy (normal_bits), Box-Muller in float64

GeneratorFakeOps(dtype, compute, fault=...) selects ONE deliberately wrong rule for the injected-fault tests:
  "align_corners"   both resizes with align_corners=True
  "unbiased_var"    the variance divided by n - 1
  "gamma_no_one"    the modulation x * gamma + beta instead of x * (1 + gamma) + beta
  "noise_after"     the noise added after the LeakyReLU
  "halves_swapped"  the first C rows of the SPADE weight read as beta, the last C as gamma
  "taps_transposed" kernel taps read (kw, kh)
  "edge_clamp"      the border padded by clamping instead of zeros
"power_iter" is the eighth fault: it lives in the host-side fold (power_iter_fold below replaces xlxmert_amd.generator.fold_spectral_norm)."""
import numpy as np
import torch
import torch.nn.functional as F

from fake_ops import FakeOps

CONV_NONE, CONV_RELU, CONV_ADD, CONV_SPADE = 0, 1, 2, 3
FAULTS = ("align_corners", "unbiased_var", "gamma_no_one", "noise_after", "halves_swapped", "taps_transposed", "edge_clamp", "power_iter")


def power_iter_fold(weight_orig, u, v):
    """the fold with ONE power iteration applied first (what torch's spectral_norm does in train mode)"""
    wm = weight_orig.flatten(1)
    v = F.normalize(torch.mv(wm.t(), u), dim=0, eps=1e-12)
    u = F.normalize(torch.mv(wm, v), dim=0, eps=1e-12)
    return weight_orig / torch.dot(u, torch.mv(wm, v))


def nhwc(t, B, H, W, C, ld):
    return torch.as_strided(t, (B, H, W, C), (H * W * ld, W * ld, ld, 1))


def normal_bits(seed, site, B, P):
    """the integer part of xl_normal_planes: uint32 arrays h0, h1 of shape [B, P]"""
    u32, m64 = np.uint32, (1 << 64) - 1
    s = (int(seed) + int(site) * 0x9E3779B97F4A7C15) & m64
    mix = u32((s & 0xFFFFFFFF) ^ (((s >> 32) * 0xC2B2AE3D) & 0xFFFFFFFF))
    b = np.arange(B, dtype=np.uint32)[:, None]
    p = np.arange(P, dtype=np.uint32)[None, :]
    out = []
    with np.errstate(over="ignore"):
        for i in (0, 1):
            h = (b * u32(0x9E3779B1)) ^ ((u32(2) * p + u32(i)) * u32(0x85EBCA77)) ^ mix
            h ^= h >> u32(16); h = h * u32(0x7FEB352D)
            h ^= h >> u32(15); h = h * u32(0x846CA68B)
            h ^= h >> u32(16)
            out.append(h)
    return out


def normal_from_bits64(h0, h1):
    """the float part in float64: u1 = (2 (h0 >> 9) + 1) 2^-24, u2 = (h1 >> 8) 2^-24, z = sqrt(-2 ln u1) cos(2 pi u2)"""
    u1 = (2.0 * (np.asarray(h0, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (np.asarray(h1, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


class GeneratorFakeOps(FakeOps):
    def __init__(self, dtype, compute=torch.float32, fault=None):
        assert fault is None or fault in FAULTS, fault
        super().__init__(dtype, compute)
        self.gen_fault = fault

    @staticmethod
    def instnorm_ws_floats(B, HW, C):
        return 2 * B * ((HW + 1023) // 1024) * C

    def conv2d_nhwc(self, x, w, bias, y, B, H, W, Cin, Cout, ks, groups=1, ldx=None, ldy=None, epilogue=CONV_NONE, aux=None, ldaux=0,
                    mean=None, rstd=None, noise=None, noise_w=0.0, slope=0.2):
        f, cp = self.gen_fault, self.compute
        assert ks in (1, 3) and Cin % groups == 0 and Cout % groups == 0
        Cy = Cout // 2 if epilogue == CONV_SPADE else Cout
        ldx, ldy = Cin if ldx is None else ldx, Cy if ldy is None else ldy
        self.calls.append(("conv2d_nhwc", B, H, W, Cin, Cout, ks, groups, epilogue))
        xi = nhwc(x, B, H, W, Cin, ldx).to(cp).permute(0, 3, 1, 2)
        wt = w.reshape(-1)[:ks * ks * Cout * (Cin // groups)].view(ks, ks, Cout, Cin // groups).to(cp).permute(2, 3, 0, 1)
        if f == "taps_transposed":
            wt = wt.transpose(2, 3)
        if f == "edge_clamp" and ks == 3:
            acc = F.conv2d(F.pad(xi, (1, 1, 1, 1), mode="replicate"), wt, None, padding=0, groups=groups)
        else:
            acc = F.conv2d(xi, wt, None, padding=ks // 2, groups=groups)
        if bias is not None:
            acc = acc + bias.view(-1)[:Cout].to(cp).view(1, -1, 1, 1)
        if epilogue == CONV_RELU:
            acc = torch.relu(acc)
        elif epilogue == CONV_ADD:
            acc = acc + nhwc(aux, B, H, W, Cout, ldaux).to(cp).permute(0, 3, 1, 2)
        elif epilogue == CONV_SPADE:
            gamma, beta = acc[:, :Cy], acc[:, Cy:]
            if f == "halves_swapped":
                gamma, beta = beta, gamma
            xa = nhwc(aux, B, H, W, Cy, ldaux).to(cp).permute(0, 3, 1, 2)
            xn = (xa - mean.view(-1)[:B * Cy].to(cp).view(B, Cy, 1, 1)) * rstd.view(-1)[:B * Cy].to(cp).view(B, Cy, 1, 1)
            t = xn * (gamma if f == "gamma_no_one" else 1 + gamma) + beta
            nz = noise_w * noise.reshape(-1)[:B * H * W].to(cp).view(B, 1, H, W) if noise is not None else None
            if nz is not None and f != "noise_after":
                t = t + nz
            t = F.leaky_relu(t, slope)
            if nz is not None and f == "noise_after":
                t = t + nz
            acc = t
        nhwc(y, B, H, W, Cy, ldy).copy_(acc.permute(0, 2, 3, 1))

    def instnorm_stats(self, x, mean, rstd, ws, B, HW, C, ld, eps=1e-5):
        assert ws.numel() >= self.instnorm_ws_floats(B, HW, C)
        self.calls.append(("instnorm_stats", B, HW, C))
        xv = torch.as_strided(x, (B, HW, C), (HW * ld, ld, 1)).to(self.compute)
        m = xv.mean(1)
        var = ((xv - m[:, None, :]) ** 2).sum(1) / (HW - 1 if self.gen_fault == "unbiased_var" and HW > 1 else HW)
        mean.view(-1)[:B * C].copy_(m.reshape(-1))
        rstd.view(-1)[:B * C].copy_((1.0 / torch.sqrt(var + eps)).reshape(-1))

    def _resize(self, t, size):
        return F.interpolate(t, size=size, mode="bilinear", align_corners=self.gen_fault == "align_corners")

    def resize_bilinear_nhwc(self, x, y, B, Hin, Win, Hout, Wout, C, ldx=None, ldy=None):
        ldx, ldy = C if ldx is None else ldx, C if ldy is None else ldy
        self.calls.append(("resize_bilinear_nhwc", B, Hin, Win, Hout, Wout, C))
        xi = nhwc(x, B, Hin, Win, C, ldx).to(self.compute).permute(0, 3, 1, 2)
        nhwc(y, B, Hout, Wout, C, ldy).copy_(self._resize(xi, (Hout, Wout)).permute(0, 2, 3, 1))

    def torgb_accum(self, rgb, acc, out, B, r, T, ld=3, first=False):
        self.calls.append(("torgb_accum", B, r, T, bool(first)))
        up = self._resize(nhwc(rgb, B, r, r, 3, ld).to(self.compute).permute(0, 3, 1, 2), (T, T))
        a = acc.view(B, 3, T, T)
        s = up if first else a.to(self.compute) + up
        a.copy_(s)
        if out is not None:
            out.view(B, 3, T, T).copy_(torch.tanh(s))

    def normal_planes(self, out, seed, site, B, P):
        self.calls.append(("normal_planes", site, B, P))
        h0, h1 = normal_bits(seed, site, B, P)
        out.view(B, P).copy_(torch.from_numpy(normal_from_bits64(h0, h1)))
