"""The image generator without a GPU: xlxmert_amd.generator.Generator over tests/fake_ops_generator.GeneratorFakeOps against the two
fixtures recorded from the reference (tests/golden/generator_tiny*.npz, generator_tiny7*.npz; tools/gen_generator_golden.py), the
state_dict contract, the spectral-norm fold, the float64 oracle against the same fixtures, one injected fault at a time, and
ImggenModel._image's untouched route for a stock torch generator."""
import pytest
import torch

import generator_cases as GC
import generator_oracle as GO
from fake_ops_generator import FAULTS, GeneratorFakeOps, power_iter_fold

FIXTURES = ("generator_tiny", "generator_tiny7")
FIX_REL = 1e-4          # the project's fp32 fixture bound, per tensor: 1e-4 * max(1, max|ref|)
_cache = {}


def fixture(name):
    if name not in _cache:
        _cache[name] = GC.load_fixture(name)
    return _cache[name]


def run(name, train, fault=None):
    cfg, sd, arrays = fixture(name)
    G = GC.make_generator(cfg, sd, GeneratorFakeOps(torch.float32, fault=fault), "cpu", torch.float32)
    got = GC.run_generator(G, torch.from_numpy(arrays["input"]), GC.fixture_planes(arrays) if train else None)
    return GC.worst_fixture_excess(got, GC.fixture_reference(arrays, "train" if train else "eval"), FIX_REL)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_runner_matches_the_reference_fixture(name, train):
    excess = run(name, train)
    print(f"  {name} train={train}: worst |got - ref| / bound = {excess:.4f}")
    assert excess <= 1.0


@pytest.mark.parametrize("name", FIXTURES)
def test_channels_last_input_and_chunks_give_the_same_image(name):
    cfg, sd, arrays = fixture(name)
    x = torch.from_numpy(arrays["input"])
    G = GC.make_generator(cfg, sd, GeneratorFakeOps(torch.float32), "cpu", torch.float32)
    a = G(x, train=False)
    b = G(x.permute(0, 2, 3, 1).contiguous(), train=False)
    G.chunk_images = 1
    c = G(x, train=False)
    # (bit equality of the chunks is the device test's: the host's convolution picks its algorithm by batch size)
    assert torch.equal(a, b) and float((a - c).abs().max()) < 1e-5
    assert a.dtype == torch.float32 and tuple(a.shape) == (x.shape[0], 3, cfg["target_size"], cfg["target_size"])


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_equal_the_reference_both_ways(name):
    from xlxmert_amd.generator import Generator
    cfg, sd, _ = fixture(name)
    G = Generator(**cfg, device="cpu", dtype=torch.float32, ops=GeneratorFakeOps(torch.float32))
    own = G.state_dict()
    assert set(own) == set(sd)
    assert all(tuple(own[k].shape) == tuple(sd[k].shape) for k in sd)
    G.load_state_dict(sd, strict=True)
    assert all(torch.equal(G.state_dict()[k], sd[k]) for k in sd)
    short = dict(sd)
    short.pop("resblocks.0.conv1.weight_u")
    with pytest.raises(RuntimeError, match="missing"):
        G.load_state_dict(short, strict=True)
    with pytest.raises(RuntimeError, match="unexpected"):
        G.load_state_dict({**sd, "resblocks.0.conv1.weight": sd["resblocks.0.conv1.weight_orig"]}, strict=True)


def test_unsupported_norm_type_raises():
    from xlxmert_amd.generator import Generator
    with pytest.raises(KeyError):
        Generator(emb_dim=32, codebook_dim=16, base_dim=16, target_size=32, norm_type="batch", device="cpu", dtype=torch.float32,
                  ops=GeneratorFakeOps(torch.float32))


def test_fold_uses_the_stored_u_and_v():
    from xlxmert_amd.generator import fold_spectral_norm
    _, sd, _ = fixture("generator_tiny")
    wo, u, v = (sd["resblocks.0.conv1." + k] for k in ("weight_orig", "weight_u", "weight_v"))
    W = fold_spectral_norm(wo, u, v)
    sigma = torch.dot(u, torch.mv(wo.flatten(1), v))
    assert torch.equal(W, wo / sigma)
    # another stored pair gives another weight; a power iteration does too: nothing is recomputed from weight_orig alone
    assert not torch.allclose(fold_spectral_norm(wo, u.flip(0), v), W)
    assert not torch.allclose(power_iter_fold(wo, u, v), W, rtol=1e-3)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_the_reference_fixture(name, train):
    cfg, sd, arrays = fixture(name)
    got = GO.forward(sd, cfg, torch.from_numpy(arrays["input"]), GC.fixture_planes(arrays) if train else None)
    excess = GC.worst_fixture_excess(got, GC.fixture_reference(arrays, "train" if train else "eval"), 1e-5)
    print(f"  oracle {name} train={train}: worst |got - ref| / bound = {excess:.4f}")
    assert excess <= 1.0


@pytest.mark.parametrize("fault", FAULTS)
def test_an_injected_fault_fails_the_fixture_check(fault, monkeypatch):
    """each wrong rule, alone, must push the runner outside the fixture bound on at least one fixture / mode"""
    if fault == "power_iter":
        import xlxmert_amd.generator as gen
        monkeypatch.setattr(gen, "fold_spectral_norm", power_iter_fold)
        fault = None
    worst = max(run(name, train, fault) for name in FIXTURES for train in (False, True))
    print(f"  worst excess under the fault: {worst:.1f}")
    assert worst > 1.0


def test_image_route_of_a_stock_torch_generator_is_untouched():
    """ImggenModel._image with a stand-in torch callable: [B, F, g, g] fp32 handed over, denorm, host -- today's calls"""
    from xlxmert_amd.modeling import ImggenModel
    seen = {}

    def G(x):
        seen["x"] = x
        return x[:, :3] * 2.0 - 0.5

    class Stub:
        grid_size = 2
    stub = Stub()
    stub.G = G
    stub.denorm = ImggenModel.denorm
    code = torch.arange(2 * 4 * 5, dtype=torch.bfloat16).view(8, 5) / 16
    out = ImggenModel._image(stub, code, 2)
    want_x = code.view(2, 4, -1).permute(0, 2, 1).reshape(2, -1, 2, 2).float()
    assert seen["x"].dtype == torch.float32 and tuple(seen["x"].shape) == (2, 5, 2, 2) and torch.equal(seen["x"], want_x)
    assert torch.equal(out, ((want_x[:, :3] * 2.0 - 0.5 + 1) / 2).clamp(0, 1)) and out.device.type == "cpu"
