"""Writes tests/golden/generator_tiny*.npz and generator_tiny7*.npz from the REFERENCE generator (image_generator/src/layers.py of the
reference tree, path in argv[1]).  Run by hand where the reference is available; never by a test.

Per fixture NAME: NAME.npz holds the key list, the input, the noise planes and the reference's outputs (per-block h, the pre-tanh RGB
sum and the image, with train=False and with train=True); the state_dict (eval mode, weight_orig / _u / _v included) goes into
NAME_sd0.npz, NAME_sd1.npz ... shards of at most SHARD_BYTES so that no committed file passes 1 MiB.

What is done to the parameters, and why: biases ~ N(0, 0.1) and every NoiseInjection.weight = 0.3 (the reference initialises both to
0, which would hide errors); the ToRGB conv weights are scaled by 0.004 after the reference's orthogonal init (otherwise the
pre-tanh sum has std ~ 48 and tanh hides everything)).  u / v are the constructor's fresh pair (no power iteration has run), so
sigma is arbitrary; where the pre-tanh sum still has std > 1 the ToRGB weights are scaled once more, to std 0.78.
Asserted: at most 10 % of pixels with |pre-tanh| > 2; the noise moves the pre-tanh sum by more than 0.05 somewhere; feeding the recorded planes back reproduces the train=True output bit for bit."""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
SHARD_BYTES = 900 * 1024
CONFIGS = {
    "generator_tiny": dict(emb_dim=32, codebook_dim=16, base_dim=16, init_H=8, init_W=8, target_size=32, extra_layers=0),
    "generator_tiny7": dict(emb_dim=32, codebook_dim=16, base_dim=16, init_H=7, init_W=7, target_size=28, extra_layers=1),
}
B = 2


def reference_layers(ref_root):
    for name in ("torchvision", "torchvision.models"):          # layers.py imports torchvision at the top; the Generator never uses it
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.path.insert(0, os.path.join(ref_root, "image_generator", "src"))
    import layers
    return layers


def run(G, x, train, seed, planes_out=None):
    """the reference forward with per-block h and the pre-tanh sum recorded; train=True draws the noise after torch.manual_seed(seed)"""
    hs = []
    hooks = [blk.register_forward_hook(lambda m, i, o: hs.append(o.detach().clone())) for blk in G.resblocks]
    pre = []
    hooks.append(G.last.register_forward_hook(lambda m, i, o: pre.append(i[0].detach().clone())))
    torch.manual_seed(seed)
    with torch.no_grad():
        img = G(x, train=train)
    for h in hooks:
        h.remove()
    if planes_out is not None:
        torch.manual_seed(seed)
        for blk in G.resblocks:
            for h_in in (blk._noise_shapes):
                planes_out.append(torch.empty(h_in).normal_())
    return hs, pre[0], img


def main():
    layers = reference_layers(sys.argv[1])
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    for name, cfg in CONFIGS.items():
        torch.manual_seed(1234)
        G = layers.Generator(**cfg)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for k, p in G.named_parameters():
                if k.endswith("bias"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
                if k.endswith("noise1.weight") or k.endswith("noise2.weight"):
                    p.fill_(0.3)
                if k.startswith("to_RGB_blocks") and k.endswith("conv.weight"):
                    p.mul_(0.004)
        x = torch.randn(B, cfg["emb_dim"], cfg["init_H"], cfg["init_W"], generator=g)
        G.eval()
        # the shapes of the noise planes in call order: recorded by a hook on every NoiseInjection
        for blk in G.resblocks:
            blk._noise_shapes = []
            for ni in (blk.noise1, blk.noise2):
                ni.register_forward_hook(lambda m, i, o, blk=blk: blk._noise_shapes.append((i[0].shape[0], 1, i[0].shape[2], i[0].shape[3])))
        hs0, pre0, img0 = run(G, x, False, 0)
        if float(pre0.std()) > 1.0:         # sigma of a fresh u / v pair is arbitrary: three blocks can amplify far past what 0.004 tames
            with torch.no_grad():
                for k, p in G.named_parameters():
                    if k.startswith("to_RGB_blocks") and k.endswith("conv.weight"):
                        p.mul_(0.78 / float(pre0.std()))
            hs0, pre0, img0 = run(G, x, False, 0)
        for blk in G.resblocks:
            blk._noise_shapes = []
        planes = []
        hs1, pre1, img1 = run(G, x, True, 77, planes)
        # the recorded planes reproduce the train=True output bit for bit
        it = iter(planes)
        orig = layers.NoiseInjection.forward
        layers.NoiseInjection.forward = lambda self, image, noise=False: image + self.weight * next(it) if noise else image
        with torch.no_grad():
            again = G(x, train=True)
        layers.NoiseInjection.forward = orig
        assert torch.equal(again, img1), "the recorded noise planes do not reproduce the reference's train=True output"
        frac = float((pre0.abs() > 2).float().mean())
        moved = float((pre1 - pre0).abs().max())
        assert frac <= 0.10, frac
        assert moved > 0.05, moved
        # eval mode: the weight the reference convolves with equals the stored-u/v fold exactly
        for m in G.modules():
            if hasattr(m, "weight_orig"):
                W = m.weight_orig / torch.dot(m.weight_u, torch.mv(m.weight_orig.flatten(1), m.weight_v))
                assert float((m.weight - W).abs().max()) == 0.0
        sd = {k: v.detach().numpy().copy() for k, v in G.state_dict().items()}
        main_arrays = {"keys": np.array(list(sd.keys())), "input": x.numpy(), "n_blocks": np.int64(len(hs0)), "n_planes": np.int64(len(planes)),
                       "config": np.array([f"{k}={v}" for k, v in cfg.items()])}
        for i, p in enumerate(planes):
            main_arrays[f"noise{i}"] = p.numpy()
        for tag, hs, pre, img in (("eval", hs0, pre0, img0), ("train", hs1, pre1, img1)):
            for i, h in enumerate(hs):
                main_arrays[f"{tag}_h{i}"] = h.numpy()
            main_arrays[f"{tag}_pre_tanh"] = pre.numpy()
            main_arrays[f"{tag}_image"] = img.numpy()
        np.savez(os.path.join(out_dir, name + ".npz"), **main_arrays)
        shard, size, n = {}, 0, 0
        for k, v in sd.items():
            if shard and size + v.nbytes > SHARD_BYTES:
                np.savez(os.path.join(out_dir, f"{name}_sd{n}.npz"), **shard)
                shard, size, n = {}, 0, n + 1
            shard[k] = v
            size += v.nbytes
        np.savez(os.path.join(out_dir, f"{name}_sd{n}.npz"), **shard)
        print(f"{name}: {len(sd)} keys in {n + 1} shards, pre-tanh std {float(pre0.std()):.3f} max {float(pre0.abs().max()):.3f}, "
              f"|pre| > 2: {100 * frac:.2f} %, noise moves the sum by {moved:.3f}")


if __name__ == "__main__":
    main()
