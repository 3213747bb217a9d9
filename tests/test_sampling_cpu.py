"""Temperature sampling without a GPU: the quality of the restated noise function (tests/fake_ops_sampling.py restates
csrc/common.h gumbel_noise: integers bit for bit), the engine's sequencing over SamplingFakeOps, and the honest / injected-fault
pair of the bounds in tests/bounds_sampling.py.  The kernels themselves are held to the same bounds in test_sampling_gpu.py."""
import math

import pytest
import torch

import bounds as Bd
import bounds_sampling as BS
import fake_ops_sampling as FS
from _util import load_golden
from fake_ops import FakeOps
from fake_ops_sampling import EPI_ROWSAMPLE, SamplingFakeOps
from test_engine_cpu import make_sampler_engine
from xlxmert_amd.engine import Engine


# ---------------------------------------------------------------------------------------------------------------- noise function
def test_integer_part_known_words_and_grid_extremes():
    """lowbias32 maps 0 to 0: element (0, 0) under seed 0 is the smallest grid value; the grid's ends are finite and ordered"""
    assert int(FS.gumbel_bits(0, 0, 0)) == 0
    assert FS.launch_seed(3, 5) == (3 * 0x9E3779B97F4A7C15 + 5) % 2 ** 64 and FS.launch_seed(3, 5) != FS.launch_seed(3, 6)
    h = torch.tensor([0, 0xFFFFFFFF, 0x80000000, 0x1FF, 0x200])
    u = FS.uniform_from_bits(h)
    assert u.tolist() == [2.0 ** -24, 1 - 2.0 ** -24, 0.5 + 2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24]
    g64, g32 = FS.gumbel_from_bits(h, torch.float64), FS.gumbel_from_bits(h, torch.float32)
    assert torch.isfinite(g64).all() and abs(float(g64[0]) + math.log(24 * math.log(2))) < 1e-12
    assert abs(float(g64[1]) - 24 * math.log(2)) < 1e-6            # -log(-log(1 - 2^-24)) = log 2^24 - O(2^-25)
    Bd.check(g32, g64, BS.gumbel_bound(g64), "float32 restatement of the float part")
    # all 32 bits of the column, and the high half of the seed, reach the hash
    assert int(FS.gumbel_bits(7, 3, 5)) != int(FS.gumbel_bits(7, 3, 5 + 2 ** 31))
    assert int(FS.gumbel_bits(7, 3, 5)) != int(FS.gumbel_bits(7 + 2 ** 40, 3, 5))


def test_float_part_bound_over_a_dense_sample_of_the_grid():
    """float32 restatement against float64 on 2^20 words plus both ends of the grid (the device function: test_sampling_gpu.py)"""
    gen = torch.Generator().manual_seed(5)
    h = torch.cat([torch.randint(0, 2 ** 32, (2 ** 20,), generator=gen), torch.arange(0, 2 ** 14) << 9,
                   (2 ** 23 - 1 - torch.arange(0, 2 ** 14)) << 9])
    g64 = FS.gumbel_from_bits(h, torch.float64)
    Bd.check(FS.gumbel_from_bits(h, torch.float32), g64, BS.gumbel_bound(g64), "gumbel_from_bits fp32")
    assert float(g64.max()) > 16.6 and float(g64.min()) < -2.81


SEED_A, SEED_B = 20240607, 77


def _ids(seed, y, row0=0):
    M, N = y.shape
    g = FS.gumbel_noise(seed, torch.arange(row0, row0 + M)[:, None], torch.arange(N)[None, :])
    return FS.first_argmax(y + g)


def test_chi_square_uniform_and_known_softmax():
    """equal logits: every column equally often (256 columns x 4096 rows); a known softmax over 256 columns x 16 384 identical rows
    (logits within +-1: every expected count >= 5).  Thresholds: chi-square tail at 1e-9 (Wilson-Hilferty), fixed seeds."""
    thr = BS.chi2_threshold(255)
    assert 370 < thr < 420                                   # (chi2.isf(1e-9, 255) = 404.6)
    ids = _ids(FS.launch_seed(SEED_A, 0), torch.zeros(4096, 256, dtype=torch.float64))
    stat = BS.chi2_stat(ids, torch.full((256,), 4096 / 256, dtype=torch.float64))
    print(f"uniform: chi2 {stat:.1f} (threshold {thr:.1f})")
    assert stat < thr
    x = torch.rand(256, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 2 - 1
    p = torch.softmax(x, 0)
    assert float(p.min()) * 16384 >= 5
    for T in (1.0, 2.0):                                     # (tempered logits stay within +-1)
        pT = torch.softmax(x / T, 0)
        assert float(pT.min()) * 16384 >= 5
        ids = _ids(FS.launch_seed(SEED_A, 1), (x / T)[None, :].expand(16384, -1))
        stat = BS.chi2_stat(ids, pT * 16384)
        print(f"softmax T={T}: chi2 {stat:.1f} (threshold {thr:.1f})")
        assert stat < thr


def test_rows_steps_and_seeds_draw_independently():
    """two independent draws from p agree with probability sum p^2: adjacent rows, adjacent steps, two seeds"""
    x = torch.rand(256, dtype=torch.float64, generator=torch.Generator().manual_seed(2)) * 2 - 1
    p2 = float((torch.softmax(x, 0) ** 2).sum())
    y = x[None, :].expand(16384, -1)
    a = _ids(FS.launch_seed(SEED_A, 0), y)
    for what, pairs in (("adjacent rows", (a[0::2], a[1::2])),
                        ("adjacent steps", (a, _ids(FS.launch_seed(SEED_A, 1), y))),
                        ("two seeds", (a, _ids(FS.launch_seed(SEED_A + 1, 0), y))),
                        ("far seeds", (a, _ids(FS.launch_seed(SEED_B, 0), y)))):
        n = pairs[0].numel()
        agree = int((pairs[0] == pairs[1]).sum())
        lo, hi = BS.agreement_interval(p2, n)
        print(f"{what}: {agree} agreements of {n}, expected {n * p2:.1f} in [{lo:.1f}, {hi:.1f}]")
        assert lo <= agree <= hi, what


# ---------------------------------------------------------------------------------------------------------------- engine
def _nar(eng, n_steps, **kw):
    masks, ids = [], []

    def hook(i):
        masks.append(int(eng.vmask.sum()))
        ids.append(eng.row_argmax.clone())
    cid, _, prob = eng.sample_codes_nar(n_steps, on_step=hook, **kw)
    return cid.clone(), prob.clone(), masks, ids


def test_engine_nar_reproducible_seeded_and_greedy_unchanged():
    g = load_golden("sampler_tiny")
    T = int(g["n_steps"])
    eng, _ = make_sampler_engine(g, SamplingFakeOps(torch.float32))
    greedy = _nar(eng, T)
    calls_greedy = [c[0] if isinstance(c, tuple) else c for c in eng.ops.calls]
    eng.ops.calls.clear()
    none = _nar(eng, T, temperature=None, seed=5)
    assert torch.equal(greedy[0], none[0]) and torch.equal(greedy[1], none[1])
    assert [c[0] if isinstance(c, tuple) else c for c in eng.ops.calls] == calls_greedy
    assert not any(isinstance(c, tuple) and c[0] == "gemm" and c[-1] == EPI_ROWSAMPLE for c in eng.ops.calls)
    a, b = _nar(eng, T, temperature=1.0, seed=7), _nar(eng, T, temperature=1.0, seed=7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = _nar(eng, T, temperature=1.0, seed=8)
    assert not torch.equal(a[3][0], c[3][0])                 # another seed: another first-step draw
    assert a[2] == greedy[2] == c[2]                         # masked positions per step: the greedy schedule's
    assert ((a[1] > 0) & (a[1] <= 1)).all()
    # another step: the same inputs and user seed under step 0's and step 1's launch seed draw differently
    eng.head_forward()
    out = []
    for step in (0, 1):
        eng._predict_step(False, 1.0, Engine.sample_launch_seed(7, step))
        out.append(eng.row_argmax.clone())
    assert not torch.equal(out[0], out[1])
    # a low temperature approaches the greedy choice: at T = 1e-3 the draw is the mode wherever the mode leads by a margin
    cold = _nar(eng, 1, temperature=1e-3, seed=3)
    g1 = _nar(eng, 1)
    assert (cold[3][0] == g1[3][0]).float().mean() > 0.9


@pytest.mark.parametrize("mode", ["confidence", "tlbr", "random"])
def test_engine_ar_policies_unmask_one_position_per_step(mode):
    g = load_golden("sampler_ar_tiny")
    eng, _ = make_sampler_engine(g, SamplingFakeOps(torch.float32))
    B, V = eng.B, eng.V
    outs = []
    for seed in (11, 11, 12):
        trace = []
        cid, _, _ = eng.sample_codes_ar(None, mode, positions=g["random_positions"].tolist()[-V:], trace=trace, temperature=2.0, seed=seed)
        assert [int(m.sum()) for m in trace] == [B * (V - i - 1) for i in range(V)], mode
        assert all(int(m.view(B, V).sum(1).max()) == V - i - 1 for i, m in enumerate(trace))
        outs.append(cid.clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), 1e-4, 1e4])
def test_bad_temperatures_raise(bad):
    g = load_golden("sampler_tiny")
    eng, _ = make_sampler_engine(g, SamplingFakeOps(torch.float32))
    with pytest.raises(ValueError, match="temperature"):
        eng.sample_codes_nar(2, temperature=bad)
    with pytest.raises(ValueError, match="temperature"):
        eng.sample_codes_ar(2, temperature=bad)
    assert Engine.check_temperature(None) is None and Engine.check_temperature(1e3) == 1e3 and Engine.check_temperature(1e-3) == 1e-3
    assert (Engine.TEMPERATURE_MIN, Engine.TEMPERATURE_MAX) == (BS.T_MIN, BS.T_MAX)


def test_fused_and_unfused_paths_draw_the_same_bf16(monkeypatch):
    """bf16, B*V = 256: the codebook contraction ending in XL_EPI_ROWSAMPLE (no logits in memory) and the path over fp32 logits
    perturb every element identically: both first-step draws are admissible against the float64 z of the logits, and equal
    wherever a single column is admissible.  (The two paths round y differently: alpha acc + bias/T against (acc + bias) inv_T --
    a few U32 (|y| + |bias / T|), taken as 8 U32 of it.)"""
    import lxmert_oracle as O
    from _util import golden_cfg
    from xlxmert_amd.config import XLxmertConfig
    from xlxmert_amd.params import ParamStore
    g = load_golden("sampler_tiny")
    oc = golden_cfg(g)
    cfg = XLxmertConfig(**{k: getattr(oc, k) for k in ("vocab_size", "hidden_size", "num_attention_heads", "intermediate_size",
                                                      "max_position_embeddings", "type_vocab_size", "l_layers", "x_layers", "r_layers",
                                                      "visual_feat_dim", "visual_pos_dim", "num_clusters")})
    sd = O.make_state_dict(oc, int(g["seed"]))
    B, L, grid, T, seed = 4, 8, 8, 2.0, 9
    ids = torch.from_numpy(g["in_input_ids"])[:1].expand(B, -1).clone()
    pos = torch.from_numpy(O.box_position(grid)).unsqueeze(0).expand(B, -1, -1)
    outs = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("XL_FUSED_PREDICT", fused)
        store = ParamStore(cfg, "cpu", torch.bfloat16, task="vis_mask")
        store.load_named(sd)
        eng = Engine(cfg, store, SamplingFakeOps(torch.bfloat16), B, L, grid * grid, need_lang=False)
        eng.sync_compute_weights()
        eng.set_inputs(ids, ids > 0, None, pos, cluster_ids=torch.zeros(B, grid * grid, dtype=torch.long),
                       vis_mask=torch.ones(B, grid * grid, dtype=torch.bool))
        assert eng.fused_predict_available() == (fused == "1")
        first = {}
        cid, _, prob = eng.sample_codes_nar(3, temperature=T, seed=seed,
                                            on_step=lambda i: first.setdefault("ids", eng.row_argmax.clone()) if i == 0 else None)
        n_rs = sum(1 for c in eng.ops.calls if c[0] == "gemm" and c[-1] == EPI_ROWSAMPLE)
        assert n_rs == (3 if fused == "1" else 0)
        outs[fused] = (first["ids"], cid.clone(), eng)
        assert int(cid.max()) < cfg.num_clusters                 # never a pad column
    eng = outs["0"][2]
    # first-step logits of the unfused engine: rerun step 0's forward on an all-masked grid
    eng.vmask.fill_(1)
    eng.encoder_forward(want_pooled=False)
    eng.head_forward()
    y = eng.logits.view(eng.MV, eng.K).double() / T
    gz = FS.gumbel_noise(Engine.sample_launch_seed(seed, 0), torch.arange(eng.MV)[:, None], torch.arange(eng.K)[None, :])
    e = 8 * Bd.U32 * (y.abs() + (eng.hd["bc"][0].double().abs() / T)[None, :])
    n_f, _ = BS.check_draw(y, gz, e, outs["1"][0], "fused first step")
    n_u, _ = BS.check_draw(y, gz, e, outs["0"][0], "unfused first step")
    single = (n_f[:, 0] == 1)
    assert int(single.sum()) > 200
    assert torch.equal(outs["1"][0][single], outs["0"][0][single])


# ---------------------------------------------------------------------------------------------------------------- honest / faults
def _case(M=64, N=128, K=32, T=2.0, pad=40, gen_seed=3):
    gen = torch.Generator().manual_seed(gen_seed)
    A = (torch.randn(M, K, generator=gen)).bfloat16()
    Bm = (torch.randn(N, K, generator=gen) * 0.5).bfloat16()
    bias = torch.randn(N, generator=gen)
    Bm[N - pad:] = 0
    bias_T = (bias / T).float()
    bias_T[N - pad:] = BS.PAD_BIAS
    return A, Bm, bias_T, 1.0 / T


_reference = BS.tempered_reference


def _run(ops, A, Bm, bias_T, alpha, seed):
    M, K = A.shape
    N = Bm.shape[0]
    ws = torch.zeros((N // 64) * M * 4)
    ops.gemm(A, Bm, None, bias_T, None, ws, M, N, K, K, K, N, epilogue=EPI_ROWSAMPLE, alpha=alpha, seed=seed)
    p, lse, idx = torch.zeros(M), torch.zeros(M), torch.zeros(M, dtype=torch.int32)
    ops.rowsample_combine(ws, N // 64, M, seed, p, idx, lse)
    return ws, p, idx, lse


@pytest.mark.parametrize("noise", ["ok", "row", "seed", "u16"])
def test_bounds_accept_the_restatement_and_reject_wrong_noise(noise):
    """the float32 restatement passes every bound of bounds_sampling.py; a noise function that ignores the row, ignores the launch
    seed or draws 16-bit uniforms fails them"""
    A, Bm, bias_T, alpha = _case()
    seed = FS.launch_seed(123, 2)
    y, g, e = _reference(A, Bm, bias_T, alpha, seed)
    ws, p, idx, lse = _run(SamplingFakeOps(torch.bfloat16, torch.float32, noise=noise), A, Bm, bias_T, alpha, seed)

    def checks():
        BS.check_records(ws, y, g, e, "ROWSAMPLE")
        BS.check_rows(y, g, e, Bm.shape[0] // 64, p, idx, lse, "ROWSAMPLE + combine")
    if noise == "ok":
        checks()
    else:
        with pytest.raises(AssertionError, match="not admissible"):
            checks()


@pytest.mark.parametrize("noise", ["ok", "row", "seed", "u16"])
def test_sample_rows_restatement_within_bounds_and_faults_rejected(noise):
    M, K, ld, T = 37, 1000, 1008, 4.0
    gen = torch.Generator().manual_seed(8)
    logits = torch.randn(M, ld, generator=gen) * 3
    seed = FS.launch_seed(5, 1)
    y, g, e = BS.logits_reference(logits, K, 1.0 / T, seed)
    p, lse, idx = torch.zeros(M), torch.zeros(M), torch.zeros(M, dtype=torch.int32)
    SamplingFakeOps(torch.float32, torch.float32, noise=noise).sample_rows(logits, M, K, ld, 1.0 / T, seed, p, idx, lse)
    if noise == "ok":
        BS.check_rows(y, g, e, (K + 63) // 64 + 6, p, idx, lse, "sample_rows")
    else:
        with pytest.raises(AssertionError, match="not admissible"):
            BS.check_rows(y, g, e, (K + 63) // 64 + 6, p, idx, lse, "sample_rows")


def test_greedy_fake_ops_have_no_sampling_entry_points():
    """the keywords reach the library only through the new entry points: plain FakeOps (today's surface) lacks them"""
    assert not hasattr(FakeOps(torch.float32), "sample_rows") and not hasattr(FakeOps(torch.float32), "rowsample_combine")
