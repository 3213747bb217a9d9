"""The whole generator on the device (xlxmert_amd.generator.Generator over HipOps): fp32 against the reference's fixtures under the CPU
test's bound, bf16 against the float64 oracle with the bf16-emulating oracle as the yardstick (the device's worst relative error per
tensor at most twice the emulation's), the deployed geometry once, noise seeds, chunking, and the ImggenModel route."""
import pytest
import torch

import generator_cases as GC
import generator_oracle as GO

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURES = ("generator_tiny", "generator_tiny7")
DEPLOYED = dict(emb_dim=2048, codebook_dim=256, base_dim=32, init_H=8, init_W=8, target_size=256, extra_layers=0)
_cache = {}


def fixture(name):
    if name not in _cache:
        _cache[name] = GC.load_fixture(name)
    return _cache[name]


def _gen(cfg, sd, dtype, **kw):
    from xlxmert_amd.ops import HipOps
    return GC.make_generator(cfg, sd, HipOps(dtype), DEV, dtype, **kw)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_matches_the_reference_fixture(name, train):
    cfg, sd, arrays = fixture(name)
    G = _gen(cfg, sd, torch.float32)
    got = GC.run_generator(G, torch.from_numpy(arrays["input"]), GC.fixture_planes(arrays) if train else None)
    excess = GC.worst_fixture_excess(got, GC.fixture_reference(arrays, "train" if train else "eval"), 1e-4)
    print(f"  device fp32 {name} train={train}: worst |got - ref| / bound = {excess:.4f}")
    assert excess <= 1.0


def _against_emulation(label, cfg, sd, x, planes):
    """bf16 device vs float64, with the bf16-emulating float64 oracle as the yardstick: per tensor, device error <= 2 x emulation error"""
    exact = GO.forward(sd, cfg, x, planes)
    emu = GO.forward(sd, cfg, x, planes, emulate=True)
    got = GC.run_generator(_gen(cfg, sd, torch.bfloat16), x, planes)
    names = [f"h{i}" for i in range(len(exact["h"]))] + ["pre_tanh", "image"]
    flat = lambda d: d["h"] + [d["pre_tanh"], d["image"]]          # noqa: E731
    bad = []
    for n, g, e, m in zip(names, flat(got), flat(exact), flat(emu)):
        dev_err, emu_err = GC.rel_err(g, e), GC.rel_err(m, e)
        print(f"  {label} {n}: device {dev_err:.3e}  emulation {emu_err:.3e}  ratio {dev_err / emu_err:.2f}")
        if dev_err > 2 * emu_err:
            bad.append((n, dev_err, emu_err))
    assert not bad, bad


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_within_twice_the_emulation(name, train):
    cfg, sd, arrays = fixture(name)
    _against_emulation(f"{name} train={train}", cfg, sd, torch.from_numpy(arrays["input"]), GC.fixture_planes(arrays) if train else None)


def test_bf16_deployed_geometry_within_twice_the_emulation():
    """base_dim 32, 2048 -> 256 codes, 8 -> 256 pixels, B = 2, random weights (ToRGB scaled), noise planes given"""
    sd = GO.make_state_dict(DEPLOYED, 11)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(2, 2048, 8, 8, generator=gen)
    planes = [torch.randn(2, 1, r, r, generator=gen) for blk in GO.blocks(DEPLOYED) for r in (blk[0], blk[1])]
    _against_emulation("deployed", DEPLOYED, sd, x, planes)


def test_noise_seed_reproduces_and_train_false_is_zero_noise():
    cfg, sd, arrays = fixture("generator_tiny")
    x = torch.from_numpy(arrays["input"])
    for dtype in (torch.float32, torch.bfloat16):
        G = _gen(cfg, sd, dtype)
        a, b, c = G(x, noise_seed=5), G(x, noise_seed=5), G(x, noise_seed=6)
        assert torch.equal(a, b) and not torch.equal(a, c)
        torch.manual_seed(3)
        d = G(x)
        torch.manual_seed(3)
        e = G(x)
        assert torch.equal(d, e) and not torch.equal(d, a)          # noise_seed=None: torch's default CPU generator governs
        zero = [torch.zeros(s) for s in G.noise_shapes(x.shape[0])]
        assert torch.equal(G(x, train=False), G(x, train=True, noise=zero))
        assert a.dtype == torch.float32 and a.is_cuda and float(a.abs().max()) < 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_chunks_of_one_equal_one_chunk_bit_for_bit(dtype):
    cfg, sd, arrays = fixture("generator_tiny7")
    x = torch.from_numpy(arrays["input"]).repeat(2, 1, 1, 1)[:3]
    x[2] += 0.25
    G = _gen(cfg, sd, dtype)
    whole = G(x, noise_seed=9)
    G.chunk_images = 1
    assert torch.equal(G(x, noise_seed=9), whole)
    G.chunk_images = 2
    assert torch.equal(G(x, noise_seed=9), whole)


def test_imggen_model_renders_with_the_native_generator():
    """sample_image_NAR with the native generator == denorm(G(features as NCHW fp32)) with the same object called through the generic
    callable route, bit for bit in fp32; a stock torch callable still takes the old route"""
    from test_modeling_gpu import _imggen_model, load_golden
    from xlxmert_amd.generator import Generator
    g = load_golden("sampler_tiny")
    m, grid = _imggen_model(g)
    F = m.config.visual_feat_dim
    G = Generator(emb_dim=F, codebook_dim=16, base_dim=16, init_H=grid, init_W=grid, target_size=grid * 4, device=DEV, dtype=torch.float32)
    sd = GO.make_state_dict(dict(emb_dim=F, codebook_dim=16, base_dim=16, init_H=grid, target_size=grid * 4), 3, rgb_scale=0.05)
    G.load_state_dict(sd, strict=True)
    ids = torch.from_numpy(g["in_input_ids"]).cuda()
    T = int(g["n_steps"])
    m.set_image_generator(G)
    torch.manual_seed(21)
    native = m.sample_image_NAR(ids, n_steps=T)
    m.set_image_generator(lambda x: G(x))                # the same object behind a plain callable: the generic route
    torch.manual_seed(21)
    generic = m.sample_image_NAR(ids, n_steps=T)
    assert native.device.type == "cpu" and tuple(native.shape) == (ids.shape[0], 3, grid * 4, grid * 4)
    assert torch.equal(native, generic)
    assert float(native.min()) >= 0.0 and float(native.max()) <= 1.0 and float(native.std()) > 1e-3
    seen = []
    m.set_image_generator(lambda x: (seen.append((x.dtype, tuple(x.shape))), x)[1])
    m.sample_image_NAR(ids, n_steps=T)
    assert seen == [(torch.float32, (ids.shape[0], F, grid, grid))]
