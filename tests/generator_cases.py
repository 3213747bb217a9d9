"""TEST INFRASTRUCTURE shared by tests/test_generator_cpu.py, test_generator_kernels_gpu.py and test_generator_gpu.py: the fixture loader,
the runner harness, the shape lists and the per-element bounds of the generator kernels against float64 (in the manner of tests/bounds.py).

BOUNDS (derivations, not measurements; u32 = 2^-24, u = the unit roundoff of the stored type, fp32 2^-24, bf16 2^-8 as in
tests/bounds.py):
  convolution     K = ks*ks*Cin/groups products accumulated in fp32 in some order: |acc - exact| <= (K + 2) u32 S with
                  S = sum |x||w| + |bias| (first order; SLACK = 2 covers the (1 + u)^K tail: K <= 1152).  NONE / RELU / ADD are
                  1-Lipschitz in acc: bound = SLACK (K + 2) u32 S + 2 u32 |y| + u |y|  (the epilogue's add, the store's rounding).
  SPADE           y = lrelu(xn (1 + g) + b + n): e_g, e_b as above for the two halves; xn = (x - mean) rstd evaluated in fp32 from the
                  given fp32 mean / rstd: |xn| 3 u32; four more fp32 operations on a sum of magnitude A = |xn| |1 + g| + |b| + |n|:
                  bound = SLACK (|xn| e_g + e_b + 8 u32 A) + u |y|   (the LeakyReLU is 1-Lipschitz)
  statistics      shifted sums: d = x - K with K a pixel of the plane, |d| <= spread = max - min, each d one fp32 rounding
                  (<= u32 spread).  A chunk of <= 1024 pixels is summed in fp32, then the chunks are combined: n_c = min(n, 1024) +
                  ceil(n / 1024) additions deep.  mean_bound = SLACK ((n_c + 8) u32 spread + u32 spread) + 4 u32 |mean|;
                  var = M2 / n with the squares of d: var_bound = SLACK (2 (n_c + 8) u32 spread^2 + 4 spread (u32 spread) + 2 (u32 spread)^2);
                  rstd = (var + eps)^-1/2: rstd_bound = 0.5 rstd^3 var_bound + 4 u32 rstd.
  resize          the source coordinate is three fp32 operations on values <= `in` with a rounded scale: |d src| <= 4 u32 in per axis,
                  which moves a weight by as much and the result by <= 2 max|x| |d src| per axis; four products and three sums of
                  weights in [0, 1] add 16 u32 max|x|:  bound = 16 (1 + in) u32 max|x| + u |y|   (in = the larger input side)
  normal planes   NORMAL_ABS below."""
import math
import os

import numpy as np
import torch

U32 = 2.0 ** -24
SLACK = 2.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# z = sqrt(-2 ln u1) cos(2 pi u2) in fp32 from exact u1, u2: logf <= 3 ulp, the product by -2 exact, sqrtf correctly rounded (<= 0.5 ulp, it
# halves the relative error of its argument), cospif <= 4 ulp of a value <= 1 (ulp <= 2^-24), the product one rounding.
# r = sqrt(-2 ln u1) <= sqrt(2 * 24 ln 2) = 5.77:  |dz| <= r (1.5 * 2^-23 + 2^-24 + 2^-24) + r * 4 * 2^-24 = r * 9 * 2^-24 < 3.1e-6; with the
# house SLACK of 2:
NORMAL_ABS = SLACK * 5.77 * 9 * U32


def unit(dtype):
    return {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}[dtype]


def load_fixture(name):
    """-> (cfg dict, state_dict of torch tensors in the reference's key order, arrays dict)"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in z["config"].tolist()}
    sd, n = {}, 0
    while os.path.exists(os.path.join(GOLDEN, f"{name}_sd{n}.npz")):
        s = np.load(os.path.join(GOLDEN, f"{name}_sd{n}.npz"))
        sd.update({k: torch.from_numpy(s[k]) for k in s.files})
        n += 1
    keys = z["keys"].tolist()
    assert set(keys) == set(sd), "the state_dict shards do not hold the fixture's key list"
    return cfg, {k: sd[k] for k in keys}, {k: z[k] for k in z.files}


def make_generator(cfg, sd, ops, device, dtype, **kw):
    from xlxmert_amd.generator import Generator
    G = Generator(**cfg, device=device, dtype=dtype, ops=ops, **kw)
    G.load_state_dict(sd, strict=True)
    G.keep_blocks = True
    return G


def run_generator(G, x, planes):
    """-> {"h": [NCHW per block], "pre_tanh", "image"} on the CPU in float64"""
    img = G(x, train=planes is not None, noise=planes)
    hs = [torch.cat([c[i] for c in G.block_out], 0).permute(0, 3, 1, 2).double().cpu() for i in range(len(G.blocks))]
    return {"h": hs, "pre_tanh": G.pre_tanh.double().cpu(), "image": img.double().cpu()}


def fixture_reference(arrays, tag):
    n = int(arrays["n_blocks"])
    return {"h": [torch.from_numpy(arrays[f"{tag}_h{i}"]).double() for i in range(n)],
            "pre_tanh": torch.from_numpy(arrays[f"{tag}_pre_tanh"]).double(), "image": torch.from_numpy(arrays[f"{tag}_image"]).double()}


def fixture_planes(arrays):
    return [torch.from_numpy(arrays[f"noise{i}"]) for i in range(int(arrays["n_planes"]))]


def worst_fixture_excess(got, ref, rel):
    """max over the tensors of max|got - ref| / (rel * max(1, max|ref|)): <= 1 passes"""
    worst = 0.0
    for g, r in zip(got["h"] + [got["pre_tanh"], got["image"]], ref["h"] + [ref["pre_tanh"], ref["image"]]):
        assert g.shape == r.shape, (g.shape, r.shape)
        worst = max(worst, float((g - r).abs().max()) / (rel * max(1.0, float(r.abs().max()))))
    return worst


# ---------------------------------------------------------------------------------------------- kernel cases
MFMA_TILE = (8, 32)                     # csrc/generator.hip CT_H, CT_W
SPATIAL = [(1, 1), (2, 3), (7, 7), (8, 8), (17, 9), (33, 40)] + [(h, w) for h in (7, 8, 9) for w in (31, 32, 33)]
MFMA_CHANNELS = [(ci, co) for ci in (16, 32, 128) for co in (32, 64, 128)]
GENERIC_CHANNELS = [(4, 3, 1), (32, 3, 1), (16, 16, 1), (64, 32, 4)]       # (Cin, Cout, groups); the last: 8 outputs per group
EPILOGUES = [(0, False), (1, False), (2, False), (3, False), (3, True)]     # (epilogue, noise plane)


def conv_reference(x, w_dev, bias, B, H, W, Cin, Cout, ks, groups, epilogue, aux, mean, rstd, noise, noise_w, slope, out_dtype):
    """float64 reference and the per-element bound; x [B, H, W, Cin], w_dev the device layout, aux [B, H, W, Cy] (values as stored)"""
    D = torch.float64
    F = torch.nn.functional
    Cg = Cin // groups
    xi = x.to(D).permute(0, 3, 1, 2)
    wt = w_dev.to(D).view(ks, ks, Cout, Cg).permute(2, 3, 0, 1)
    acc = F.conv2d(xi, wt, bias.to(D), padding=ks // 2, groups=groups)
    S = F.conv2d(xi.abs(), wt.abs(), bias.to(D).abs(), padding=ks // 2, groups=groups)
    e = (ks * ks * Cg + 2) * U32 * S
    u = unit(out_dtype)
    if epilogue == 3:
        C = Cout // 2
        xn = (aux.to(D).permute(0, 3, 1, 2) - mean.to(D).view(B, C, 1, 1)) * rstd.to(D).view(B, C, 1, 1)
        g, b_ = acc[:, :C], acc[:, C:]
        nz = noise_w * noise.to(D).view(B, 1, H, W) if noise is not None else torch.zeros(1, dtype=D)
        t = xn * (1 + g) + b_ + nz
        y = F.leaky_relu(t, slope)
        A = xn.abs() * (1 + g).abs() + b_.abs() + nz.abs()
        bound = SLACK * (xn.abs() * e[:, :C] + e[:, C:] + 8 * U32 * A) + u * y.abs()
    else:
        y = acc
        if epilogue == 1:
            y = torch.relu(y)
        elif epilogue == 2:
            y = y + aux.to(D).permute(0, 3, 1, 2)
        bound = SLACK * e + 2 * U32 * y.abs() + u * y.abs()
    return y.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1) + 1e-30


def stats_reference(x, eps=1e-5):
    """x [B, HW, C] as stored -> mean, rstd in float64 and their bounds"""
    D = torch.float64
    xv = x.to(D)
    n = xv.shape[1]
    mean = xv.mean(1)
    var = ((xv - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    spread = (xv.max(1).values - xv.min(1).values)
    n_c = min(n, 1024) + (n + 1023) // 1024
    d_round = U32 * spread                              # one fp32 rounding of x - K
    mean_b = SLACK * ((n_c + 8) * U32 * spread + d_round) + 4 * U32 * mean.abs() + 1e-30
    var_b = SLACK * (2 * (n_c + 8) * U32 * spread ** 2 + 4 * spread * d_round + 2 * d_round ** 2)
    rstd_b = 0.5 * rstd ** 3 * var_b + 4 * U32 * rstd
    return mean, rstd, mean_b, rstd_b


def resize_reference(x, Hout, Wout, out_dtype):
    """x [B, H, W, C] as stored -> float64 bilinear and its bound"""
    D = torch.float64
    F = torch.nn.functional
    xi = x.to(D).permute(0, 3, 1, 2)
    y = F.interpolate(xi, size=(Hout, Wout), mode="bilinear", align_corners=False)
    # (the four taps are bounded by the plane's largest magnitude)
    bound = 16 * (1 + max(xi.shape[-2:])) * U32 * xi.abs().amax(dim=(2, 3), keepdim=True).expand_as(y) + unit(out_dtype) * y.abs() + 1e-30
    return y.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1)


def worst_ratio(got, ref, bound):
    return float(((got.double().cpu() - ref).abs() / bound).max())


def rel_err(got, ref):
    """worst relative error of a tensor: max|got - ref| / max|ref|"""
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


# ---------------------------------------------------------------------------------------------- guarded device buffers
GUARD = 4096          # floats of guard on either side of a buffer (tests/test_match_kernels_gpu.py::Guarded)


class Guarded:
    """alloc(name, shape, dtype) -> a 16-byte aligned device view between two guards; check(): everything outside the views kept its bits"""

    def __init__(self, device="cuda"):
        self.items, self.device = [], device

    def __call__(self, name, shape, dtype, fill=None):
        n_bytes = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
        n_f = (n_bytes + 3) // 4
        whole = torch.full((n_f + 2 * GUARD,), 4096.0, device=self.device)
        whole[1::2] = -4096.0
        view = whole[GUARD:GUARD + n_f].view(torch.uint8)[:n_bytes].view(dtype).view(*shape)
        if fill is not None:
            view.copy_(fill)
        self.items.append((name, whole, whole.clone(), n_bytes))
        return view

    def check(self, unchanged=()):
        """unchanged: names whose VIEW must have kept its bits too (refused calls)"""
        for name, whole, before, n_bytes in self.items:
            w, b = whole.view(torch.uint8), before.view(torch.uint8)
            lo = GUARD * 4
            assert torch.equal(w[:lo], b[:lo]) and torch.equal(w[lo + n_bytes:], b[lo + n_bytes:]), f"{name}: storage outside the view was written"
            if name in unchanged:
                assert torch.equal(w[lo:lo + n_bytes], b[lo:lo + n_bytes]), f"{name}: a refused call wrote"
        self.items = []
