"""TEST INFRASTRUCTURE: an independent float64 restatement of the reference generator's forward (image_generator/src/layers.py:Generator)
in torch.nn.functional, NCHW, straight from a reference state_dict.  tests/golden/generator_tiny*.npz pin it; it is the reference for
every shape the fixtures are too small for.  The product package never imports it.

emulate=True is the yardstick of the bf16 device path (the pattern of oracle/lxmert_oracle.EMU): the same float64 arithmetic with the
weights and every activation that the device STORES in bf16 rounded to bf16 at that point -- the code rows, the bottleneck output, the
two init maps, every resized map, SPADE's hidden activation and its output, conv1 / res_branch / conv2 outputs, the ToRGB conv output.
Statistics, biases, noise, and the RGB sum stay unrounded (fp32 on the device)."""
import math

import torch
import torch.nn.functional as F


def _cap(res):
    return {112: 256, 224: 128, 128: 256, 256: 128}.get(res, 512)


def make_state_dict(cfg, seed, rgb_scale=0.004, bias_std=0.1, noise_w=0.3):
    """random parameters with the reference's key set and shapes (u / v chosen so that sigma is O(1))"""
    g = torch.Generator().manual_seed(seed)
    base, cd, emb = cfg["base_dim"], cfg["codebook_dim"], cfg["emb_dim"]
    sd = {}

    def conv(prefix, cout, cin_g, ks, sn):
        w = torch.randn(cout, cin_g, ks, ks, generator=g, dtype=torch.float64) / math.sqrt(cin_g * ks * ks)
        if sn:          # v random, u = the normalised image of v: sigma = |W v| is O(1), the folded weight keeps w's scale
            v = F.normalize(torch.randn(cin_g * ks * ks, generator=g, dtype=torch.float64), dim=0)
            u = F.normalize(torch.mv(w.flatten(1), v), dim=0)
            sd[prefix + ".weight_orig"] = w.float()
            sd[prefix + ".weight_u"], sd[prefix + ".weight_v"] = u.float(), v.float()
        else:
            sd[prefix + ".weight"] = w.float()
        sd[prefix + ".bias"] = (torch.randn(cout, generator=g, dtype=torch.float64) * bias_std).float()

    conv("bottleneck_emb.0", cd, emb, 1, False)
    conv("learned_init_conv.0", base, cd // 4, 3, True)
    conv("style_init_conv.0", base, cd // 4, 3, True)
    for i, (r, R, n_in, n_out) in enumerate(blocks(cfg)):
        p = f"resblocks.{i}"
        for name, c in (("cbn1", n_in), ("cbn2", n_out)):
            conv(f"{p}.{name}.shared.0", 128, base, 3, False)
            conv(f"{p}.{name}.gamma", c, 128, 3, False)
            conv(f"{p}.{name}.beta", c, 128, 3, False)
        conv(f"{p}.conv1", n_out, n_in, 3, True)
        conv(f"{p}.conv2", n_out, n_out, 3, True)
        conv(f"{p}.res_branch.1", n_out, n_in, 1, True)
        sd[f"{p}.noise1.weight"] = torch.full((1,), noise_w)
        sd[f"{p}.noise2.weight"] = torch.full((1,), noise_w)
        conv(f"to_RGB_blocks.{i}.conv", 3, n_out, 3, False)
        sd[f"to_RGB_blocks.{i}.conv.weight"] *= rgb_scale * math.sqrt(n_out * 9)
    return sd


def blocks(cfg):
    out, res = [], cfg["init_H"]
    for _ in range(int(math.log2(cfg["target_size"] // cfg["init_H"]))):
        out.append((res, res * 2, min(_cap(res), cfg["base_dim"]), min(_cap(res * 2), cfg["base_dim"])))
        res *= 2
    for _ in range(cfg.get("extra_layers", 0)):
        out.append((res, res, min(_cap(res), cfg["base_dim"]), min(_cap(res), cfg["base_dim"])))
    return out


def forward(sd, cfg, x, noise=None, emulate=False):
    """x [B, emb_dim, H, W]; noise: None (train=False) or the list of [B, 1, h, w] planes in call order.
    -> {"h": [per-block output], "pre_tanh", "image"} in float64"""
    D = torch.float64
    sd = {k: torch.as_tensor(v).to(D) for k, v in sd.items()}
    rnd = (lambda t: t.to(torch.bfloat16).to(D)) if emulate else (lambda t: t)

    def weight(prefix):
        if prefix + ".weight_orig" in sd:
            wo = sd[prefix + ".weight_orig"]
            if emulate:         # the host folds in fp32 before it rounds to bf16
                wo32, u32, v32 = wo.float(), sd[prefix + ".weight_u"].float(), sd[prefix + ".weight_v"].float()
                return rnd((wo32 / torch.dot(u32, torch.mv(wo32.flatten(1), v32))).to(D))
            return wo / torch.dot(sd[prefix + ".weight_u"], torch.mv(wo.flatten(1), sd[prefix + ".weight_v"]))
        return rnd(sd[prefix + ".weight"])

    def conv(t, prefix, pad, groups=1):
        return F.conv2d(t, weight(prefix), sd[prefix + ".bias"], padding=pad, groups=groups)

    def resize(t, size):
        if t.shape[-1] == size and t.shape[-2] == size:
            return t
        return rnd(F.interpolate(t, size=(size, size), mode="bilinear", align_corners=False))

    def spade(t, y, prefix, plane, nw):
        normalized = F.instance_norm(t, eps=1e-5)
        actv = rnd(torch.relu(conv(resize(y, t.shape[-1]), prefix + ".shared.0", 1)))
        out = normalized * (1 + conv(actv, prefix + ".gamma", 1)) + conv(actv, prefix + ".beta", 1)
        if plane is not None:
            out = out + nw * plane.to(D)
        return rnd(F.leaky_relu(out, 0.2))

    emb = rnd(torch.tanh(conv(rnd(x.to(D)), "bottleneck_emb.0", 0)))
    h = rnd(conv(emb, "learned_init_conv.0", 1, 4))
    y = rnd(conv(emb, "style_init_conv.0", 1, 4))
    T = cfg["target_size"]
    total, hs = torch.zeros(x.shape[0], 3, T, T, dtype=D), []
    for i, (r, R, n_in, n_out) in enumerate(blocks(cfg)):
        p = f"resblocks.{i}"
        planes = (None, None) if noise is None else (noise[2 * i], noise[2 * i + 1])
        t = spade(h, y, p + ".cbn1", planes[0], sd[p + ".noise1.weight"])
        t = rnd(conv(resize(t, R), p + ".conv1", 1))
        t = spade(t, y, p + ".cbn2", planes[1], sd[p + ".noise2.weight"])
        res = rnd(conv(resize(h, R), p + ".res_branch.1", 0))
        h = rnd(conv(t, p + ".conv2", 1) + res)
        hs.append(h)
        rgb = rnd(conv(h, f"to_RGB_blocks.{i}.conv", 1))
        total = total + (rgb if R == T else F.interpolate(rgb, size=(T, T), mode="bilinear", align_corners=False))
    return {"h": hs, "pre_tanh": total, "image": torch.tanh(total)}
