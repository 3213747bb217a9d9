"""The image generator on the device: the frozen SPADE decoder of the reference (image_generator/src/layers.py:Generator, deployed by
tasks/sample_images.py:52-67) that turns a grid of codes into pixels, written over the `ops` object (HipOps on the device; the tests'
restatement on the host), as match.py is.  Forward only.

Per residual block (ref layers.py:93-113), NHWC, r = the block's input side:
    stats(x) -> SPADE1 = conv3x3(relu(conv3x3(y_r))) with the modulation, the noise and the LeakyReLU in the second conv's epilogue
    -> x2 bilinear -> conv1 -> stats -> SPADE2 -> conv2 with the residual branch (x2 bilinear of x, 1x1 conv) added in its epilogue
    -> ToRGB conv (3 channels) -> upsampled into the fp32 [B, 3, T, T] sum; tanh with the last block.
y_r is the style map resized to the block's resolution (once per resolution).  The bottleneck (1x1 conv + tanh over the code rows) is
xl_gemm with the tanh epilogue.  Spectral norm is folded once at load with the eval-mode meaning (fold_spectral_norm); the weights are
repacked once into the device layout of include/xlxmert_hip.h ("image generator").  Nothing in a call synchronises with the host."""
import math

import torch

from .ops import CONV_ADD, CONV_NONE, CONV_RELU, CONV_SPADE, EPI_TANH

NHIDDEN = 128                   # SPADE's hidden width (ref layers.py:23: "Yes, hardcoded")
SLOPE = 0.2


def fold_spectral_norm(weight_orig, u, v):
    """eval-mode torch.nn.utils.spectral_norm: W = weight_orig / (u . (weight_orig.flatten(1) @ v)), u and v as stored"""
    sigma = torch.dot(u, torch.mv(weight_orig.flatten(1), v))
    return weight_orig / sigma


def resolution_channels(res, base_dim):
    """ref layers.py:161-175 (its table has 7..224 and 8..256 by doubling; any other side takes the 512 cap of the small ones)"""
    return min({112: 256, 224: 128, 128: 256, 256: 128}.get(res, 512), base_dim)


def pack_conv(w):
    """torch [Cout, Cin/groups, kh, kw] -> device [kh*kw, Cout, Cin/groups]"""
    return w.permute(2, 3, 0, 1).contiguous()


class Generator:
    def __init__(self, emb_dim=2048, mod_dim=128, base_dim=64, n_channel=3, target_size=16, extra_layers=0, init_H=8, init_W=8,
                 norm_type="spade_in", SN=True, codebook_dim=256, *, device=None, dtype=torch.bfloat16, ops=None, chunk_images=64):
        if norm_type != "spade_in":
            raise KeyError(norm_type)                               # (the reference's dict lookup, layers.py:74-76)
        if init_H != init_W:
            raise ValueError(f"init_H = {init_H}, init_W = {init_W}: the device path renders square grids")
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"dtype {dtype}: bfloat16 or float32")
        if codebook_dim % 4 or base_dim % 4:
            raise ValueError("codebook_dim and base_dim must be multiples of 4 (the init convolutions have 4 groups)")
        self.emb_dim, self.base_dim, self.codebook_dim, self.target_size = emb_dim, base_dim, codebook_dim, target_size
        self.init_H, self.init_W, self.SN, self.norm_type, self.extra_layers = init_H, init_W, bool(SN), norm_type, extra_layers
        self.device = torch.device(device if device is not None else "cuda")
        self.dtype, self.chunk_images = dtype, int(chunk_images)
        if self.chunk_images < 1:
            raise ValueError(f"chunk_images {chunk_images!r}: at least 1")
        if ops is None:
            from .ops import HipOps
            ops = HipOps(dtype)
        self.ops = ops
        self.mod = base_dim                                         # (ref layers.py:182: mod_dim = n_init)
        # (side in, side out, channels in, channels out) per residual block
        self.blocks = []
        res = init_H
        for _ in range(int(math.log2(target_size // init_H))):
            self.blocks.append((res, res * 2, resolution_channels(res, base_dim), resolution_channels(res * 2, base_dim)))
            res *= 2
        for _ in range(extra_layers):
            c = resolution_channels(res, base_dim)
            self.blocks.append((res, res, c, c))
        if not self.blocks:
            raise ValueError("a generator without a residual block (target_size / init_H < 2 and no extra layers)")
        self.keep_blocks = False            # tests: keep a copy of every block's output (self.block_out) and of the pre-tanh sum
        self.block_out, self.pre_tanh = [], None
        self._bufs = {}
        g = torch.Generator().manual_seed(0)
        self._sd = {}
        for k, shape in self._shapes().items():
            if k.endswith("bias") or k.endswith("noise1.weight") or k.endswith("noise2.weight"):
                t = torch.zeros(shape)
            elif k.endswith("weight_u") or k.endswith("weight_v"):
                t = torch.nn.functional.normalize(torch.randn(shape, generator=g), dim=0)
            else:
                t = torch.randn(shape, generator=g) / math.sqrt(max(1, math.prod(shape[1:])))
            self._sd[k] = t
        self._pack()

    # ------------------------------------------------------------------ parameters
    def _conv_keys(self, prefix, cout, cin_g, ks, sn):
        d = {}
        if sn:
            d[prefix + ".weight_orig"] = (cout, cin_g, ks, ks)
            d[prefix + ".bias"] = (cout,)
            d[prefix + ".weight_u"] = (cout,)
            d[prefix + ".weight_v"] = (cin_g * ks * ks,)
        else:
            d[prefix + ".weight"] = (cout, cin_g, ks, ks)
            d[prefix + ".bias"] = (cout,)
        return d

    def _shapes(self):
        """the reference's state_dict: key -> shape"""
        sn, d = self.SN, {}
        d.update(self._conv_keys("bottleneck_emb.0", self.codebook_dim, self.emb_dim, 1, False))
        d.update(self._conv_keys("learned_init_conv.0", self.base_dim, self.codebook_dim // 4, 3, sn))
        d.update(self._conv_keys("style_init_conv.0", self.mod, self.codebook_dim // 4, 3, sn))
        for i, (_, _, n_in, n_out) in enumerate(self.blocks):
            p = f"resblocks.{i}"
            for name, c in (("cbn1", n_in), ("cbn2", n_out)):
                d.update(self._conv_keys(f"{p}.{name}.shared.0", NHIDDEN, self.mod, 3, False))
                d.update(self._conv_keys(f"{p}.{name}.gamma", c, NHIDDEN, 3, False))
                d.update(self._conv_keys(f"{p}.{name}.beta", c, NHIDDEN, 3, False))
            d.update(self._conv_keys(f"{p}.conv1", n_out, n_in, 3, sn))
            d.update(self._conv_keys(f"{p}.conv2", n_out, n_out, 3, sn))
            d.update(self._conv_keys(f"{p}.res_branch.1", n_out, n_in, 1, sn))
            d[f"{p}.noise1.weight"] = (1,)
            d[f"{p}.noise2.weight"] = (1,)
            d.update(self._conv_keys(f"to_RGB_blocks.{i}.conv", 3, n_out, 3, False))
        return d

    def state_dict(self):
        return {k: v.clone() for k, v in self._sd.items()}

    def load_state_dict(self, state_dict, strict=True):
        shapes = self._shapes()
        missing = [k for k in shapes if k not in state_dict]
        unexpected = [k for k in state_dict if k not in shapes]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Generator.load_state_dict: missing keys {missing}, unexpected keys {unexpected}")
        for k, shape in shapes.items():
            if k in state_dict:
                t = torch.as_tensor(state_dict[k]).detach().to("cpu", torch.float32)
                if tuple(t.shape) != tuple(shape):
                    raise RuntimeError(f"Generator.load_state_dict: {k} has shape {tuple(t.shape)}, expected {tuple(shape)}")
                self._sd[k] = t.clone()
        self._pack()
        return missing, unexpected

    def _weight(self, prefix):
        sd = self._sd
        if prefix + ".weight_orig" in sd:
            return fold_spectral_norm(sd[prefix + ".weight_orig"], sd[prefix + ".weight_u"], sd[prefix + ".weight_v"])
        return sd[prefix + ".weight"]

    def _pack(self):
        """fold the spectral norms and repack every weight into the device layout, once"""
        dev, dt, sd = self.device, self.dtype, self._sd
        w = lambda t: t.to(dt).to(dev)                     # noqa: E731
        f = lambda t: t.to(torch.float32).to(dev)          # noqa: E731
        P = {"bott.w": w(sd["bottleneck_emb.0.weight"].reshape(self.codebook_dim, self.emb_dim).contiguous()),
             "bott.b": f(sd["bottleneck_emb.0.bias"])}
        for name, key in (("init", "learned_init_conv.0"), ("style", "style_init_conv.0")):
            P[name + ".w"], P[name + ".b"] = w(pack_conv(self._weight(key))), f(sd[key + ".bias"])
        self.noise_w = []
        for i in range(len(self.blocks)):
            p = f"resblocks.{i}"
            for name in ("cbn1", "cbn2"):
                q = f"{p}.{name}"
                P[q + ".shared.w"], P[q + ".shared.b"] = w(pack_conv(sd[q + ".shared.0.weight"])), f(sd[q + ".shared.0.bias"])
                P[q + ".gb.w"] = w(pack_conv(torch.cat([sd[q + ".gamma.weight"], sd[q + ".beta.weight"]], 0)))
                P[q + ".gb.b"] = f(torch.cat([sd[q + ".gamma.bias"], sd[q + ".beta.bias"]], 0))
            for name in ("conv1", "conv2", "res_branch.1"):
                P[f"{p}.{name}.w"], P[f"{p}.{name}.b"] = w(pack_conv(self._weight(f"{p}.{name}"))), f(sd[f"{p}.{name}.bias"])
            P[f"rgb.{i}.w"], P[f"rgb.{i}.b"] = w(pack_conv(sd[f"to_RGB_blocks.{i}.conv.weight"])), f(sd[f"to_RGB_blocks.{i}.conv.bias"])
            self.noise_w.append((float(sd[f"{p}.noise1.weight"]), float(sd[f"{p}.noise2.weight"])))
        self.P = P

    # ------------------------------------------------------------------ buffers
    def _buf(self, name, numel, dtype=None):
        dtype = self.dtype if dtype is None else dtype
        key = (name, dtype)
        if key not in self._bufs or self._bufs[key].numel() < numel:
            self._bufs[key] = torch.zeros(numel, dtype=dtype, device=self.device)
        return self._bufs[key][:numel]

    def noise_shapes(self, B):
        """[B, 1, h, w] of every NoiseInjection in call order"""
        out = []
        for r_in, r_out, _, _ in self.blocks:
            out += [(B, 1, r_in, r_in), (B, 1, r_out, r_out)]
        return out

    # ------------------------------------------------------------------ forward
    def __call__(self, emb, train=True, **kw):
        return self.forward(emb, train, **kw)

    def forward(self, emb, train=True, *, noise=None, noise_seed=None):
        """emb [B, emb_dim, H, W] or [B, H, W, emb_dim] -> [B, 3, T, T] fp32 in (-1, 1) on the device"""
        B = emb.shape[0]
        if tuple(emb.shape[1:]) != (self.init_H, self.init_W, self.emb_dim):
            if tuple(emb.shape[1:]) != (self.emb_dim, self.init_H, self.init_W):
                raise ValueError(f"emb {tuple(emb.shape)}: [B, {self.emb_dim}, {self.init_H}, {self.init_W}] or channels last")
            emb = emb.permute(0, 2, 3, 1)
        rows = emb.to(device=self.device, dtype=self.dtype).reshape(B * self.init_H * self.init_W, self.emb_dim).contiguous()
        return self.render_rows(rows, B, train, noise, noise_seed)

    def render_codes(self, code, B):
        """the samplers' code rows [B * init_H * init_W, emb_dim] (already channels last) -> the image on the device; noise on, as the
        reference's samplers call G(x)"""
        return self.render_rows(code.to(self.dtype).reshape(B * self.init_H * self.init_W, self.emb_dim).contiguous(), B, True, None, None)

    def render_rows(self, rows, B, train=True, noise=None, noise_seed=None):
        ops, T = self.ops, self.target_size
        planes = None
        if train:
            shapes = self.noise_shapes(B)
            if noise is not None:
                if len(noise) != len(shapes) or any(tuple(n.shape) != s for n, s in zip(noise, shapes)):
                    raise ValueError(f"noise: {len(shapes)} planes of shapes {shapes}")
                planes = [n.to(device=self.device, dtype=torch.float32).reshape(B, -1).contiguous() for n in noise]
            else:
                if noise_seed is None:
                    noise_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                planes = []
                for site, s in enumerate(shapes):
                    pl = self._buf(f"noise{site}", B * s[2] * s[3], torch.float32).view(B, s[2] * s[3])
                    ops.normal_planes(pl, int(noise_seed), site, B, s[2] * s[3])
                    planes.append(pl)
        acc = torch.empty(B, 3, T, T, dtype=torch.float32, device=self.device)
        out = torch.empty(B, 3, T, T, dtype=torch.float32, device=self.device)
        self.block_out = []
        for b0 in range(0, B, self.chunk_images):
            Bc = min(self.chunk_images, B - b0)
            self._chunk(rows, b0, Bc, None if planes is None else [p[b0:b0 + Bc] for p in planes], acc[b0:b0 + Bc], out[b0:b0 + Bc])
        self.pre_tanh = acc
        return out

    def _conv(self, x, key, y, B, r, cin, cout, ks=3, groups=1, **kw):
        self.ops.conv2d_nhwc(x, self.P[key + ".w"], self.P[key + ".b"], y, B, r, r, cin, cout, ks, groups, **kw)

    def _chunk(self, rows, b0, Bc, planes, acc, out):
        ops, P, r0, mod, T = self.ops, self.P, self.init_H, self.mod, self.target_size
        n0 = Bc * r0 * r0
        emb = self._buf("emb", n0 * self.codebook_dim)
        ops.gemm(rows[b0 * r0 * r0:], P["bott.w"], emb, P["bott.b"], None, None, n0, self.codebook_dim, self.emb_dim, self.emb_dim, self.emb_dim,
                 self.codebook_dim, epilogue=EPI_TANH)
        x = self._buf("x0", n0 * self.base_dim)
        y0 = self._buf("y0", n0 * mod)
        self._conv(emb, "init", x, Bc, r0, self.codebook_dim, self.base_dim, groups=4)
        self._conv(emb, "style", y0, Bc, r0, self.codebook_dim, mod, groups=4)
        styles = {r0: y0}

        def style(r):
            if r not in styles:
                styles[r] = self._buf(f"y{r}", Bc * r * r * mod)
                ops.resize_bilinear_nhwc(y0, styles[r], Bc, r0, r0, r, r, mod)
            return styles[r]

        def spade(x, key, r, c, plane, nw, dst):
            mean, rstd = self._buf("mean", Bc * c, torch.float32), self._buf("rstd", Bc * c, torch.float32)
            ws = self._buf("stats_ws", ops.instnorm_ws_floats(Bc, r * r, c), torch.float32)
            ops.instnorm_stats(x, mean, rstd, ws, Bc, r * r, c, c)
            actv = self._buf("actv", Bc * r * r * NHIDDEN)
            self._conv(style(r), key + ".shared", actv, Bc, r, mod, NHIDDEN, epilogue=CONV_RELU)
            self._conv(actv, key + ".gb", dst, Bc, r, NHIDDEN, 2 * c, epilogue=CONV_SPADE, aux=x, ldaux=c, mean=mean, rstd=rstd, noise=plane,
                       noise_w=nw if plane is not None else 0.0, slope=SLOPE)

        keep = []
        for i, (r, R, n_in, n_out) in enumerate(self.blocks):
            p = f"resblocks.{i}"
            nw1, nw2 = self.noise_w[i]
            h = self._buf("h", Bc * r * r * n_in)
            spade(x, p + ".cbn1", r, n_in, None if planes is None else planes[2 * i], nw1, h)
            if R != r:
                hu, xu = self._buf("hu", Bc * R * R * n_in), self._buf("xu", Bc * R * R * n_in)
                ops.resize_bilinear_nhwc(h, hu, Bc, r, r, R, R, n_in)
                ops.resize_bilinear_nhwc(x, xu, Bc, r, r, R, R, n_in)
            else:
                hu, xu = h, x
            h1 = self._buf("h1", Bc * R * R * n_out)
            self._conv(hu, p + ".conv1", h1, Bc, R, n_in, n_out)
            h2 = self._buf("h2", Bc * R * R * n_out)
            spade(h1, p + ".cbn2", R, n_out, None if planes is None else planes[2 * i + 1], nw2, h2)
            res = self._buf("res", Bc * R * R * n_out)
            self._conv(xu, p + ".res_branch.1", res, Bc, R, n_in, n_out, ks=1)
            x = self._buf(f"out{i % 2}", Bc * R * R * n_out)            # (two buffers in turn: the next block reads this one as its x)
            self._conv(h2, p + ".conv2", x, Bc, R, n_out, n_out, epilogue=CONV_ADD, aux=res, ldaux=n_out)
            if self.keep_blocks:
                keep.append(x.view(Bc, R, R, n_out).clone())
            rgb = self._buf("rgb", Bc * R * R * 3)
            self._conv(x, f"rgb.{i}", rgb, Bc, R, n_out, 3)
            last = i + 1 == len(self.blocks)
            ops.torgb_accum(rgb, acc, out if last else None, Bc, R, T, 3, first=i == 0)
        if self.keep_blocks:
            self.block_out.append(keep)
