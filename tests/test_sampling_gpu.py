"""Temperature sampling on the device: xl_gumbel_from_bits, xl_gemm(XL_EPI_ROWSAMPLE) + xl_rowsample_combine, xl_sample_rows, the
engine loops and the ImggenModel surface, element by element under the float64 bounds of tests/bounds_sampling.py (derivations
there).  The noise reference is tests/fake_ops_sampling.py in float64: integers restated bit for bit, floats in float64."""
import pytest
import torch

import bounds as Bd
import bounds_sampling as BS
import fake_ops_sampling as FS
from _util import load_golden
from fake_ops_sampling import EPI_ROWSAMPLE

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096          # floats of guard on either side of a workspace, filled with +-2^12


def _ops(dtype=torch.bfloat16):
    from xlxmert_amd.ops import HipOps
    return HipOps(dtype)


def _table(rows, what):
    for name, r in rows:
        print(f"  {what:<34} {name:<22} {'exact' if r == 0 else f'headroom {1.0 / r:9.2f}x'}")


# ---------------------------------------------------------------------------------------------------------------- 1. noise
def test_gumbel_from_bits_within_g_abs_over_the_grid():
    """the hash words of the smallest, the largest and the middle grid value (and their neighbours), 2^20 random words"""
    gen = torch.Generator().manual_seed(17)
    edge = torch.tensor([0, 0x1FF, 0x200, 0xFFFFFFFF, 0xFFFFFE00, 0xFFFFFDFF, 0x80000000, 0x7FFFFFFF, 0x7FFFFE00, 0x80000200])
    ends = torch.cat([torch.arange(0, 4096) << 9, (2 ** 23 - 1 - torch.arange(0, 4096)) << 9])
    h = torch.cat([edge, ends, torch.randint(0, 2 ** 32, (2 ** 20,), generator=gen)])
    n = h.numel()
    h_dev = (h & 0xFFFFFFFF).to(torch.int64).to(DEV)
    h32 = torch.where(h_dev >= 2 ** 31, h_dev - 2 ** 32, h_dev).to(torch.int32)          # the uint32 bits in int32 storage
    g = torch.full((n + 64,), 4096.0, device=DEV)
    _ops().gumbel_from_bits(h32, g, n)
    torch.cuda.synchronize()
    assert bool((g[n:] == 4096.0).all())
    ref = FS.gumbel_from_bits(h_dev, torch.float64)
    r = Bd.check(g[:n], ref, BS.gumbel_bound(ref), "xl_gumbel_from_bits")
    print(f"xl_gumbel_from_bits: {n} words, g in [{float(ref.min()):.4f}, {float(ref.max()):.4f}], worst |err| / bound {r:.3f}")
    assert abs(float(g[0]) - float(ref[0])) < 1e-5 and float(g[3]) > 16.63


# ---------------------------------------------------------------------------------------------------------------- 2. fused path
def _fused_case(M, N, K, T, pad, gen_seed, zero_a=False, zero_bias=False):
    gen = torch.Generator().manual_seed(gen_seed)
    A = torch.randn(M, K, generator=gen).bfloat16()
    Bm = (torch.randn(N, K, generator=gen) * 0.5).bfloat16()
    bias = torch.randn(N, generator=gen)
    if zero_a:
        A.zero_()
    if zero_bias:
        bias.zero_()
    Bm[N - pad:] = 0
    bias_T = (bias / T).float()
    bias_T[N - pad:] = BS.PAD_BIAS                 # NOT divided by T (include/xlxmert_hip.h XL_EPI_ROWSAMPLE)
    return A.to(DEV), Bm.to(DEV), bias_T.to(DEV), 1.0 / T


def _guarded(n):
    """a workspace of n floats with GUARD floats on either side, everything filled with +-2^12; returns (whole, view, copy)"""
    whole = torch.full((n + 2 * GUARD,), 4096.0, device=DEV)
    whole[1::2] = -4096.0
    return whole, whole[GUARD:GUARD + n], whole.clone()


def _run_fused(ops, A, Bm, bias_T, alpha, seed):
    M, K = A.shape
    N = Bm.shape[0]
    n_seg = N // 64
    whole, ws, before = _guarded(n_seg * M * 4)
    ops.gemm(A, Bm, None, bias_T, None, ws, M, N, K, K, K, N, epilogue=EPI_ROWSAMPLE, alpha=alpha, seed=seed)
    out_w, out, out_b = _guarded(3 * M)
    p, lse = out[:M], out[M:2 * M]
    idx = out[2 * M:].view(torch.int32)
    ops.rowsample_combine(ws, n_seg, M, seed, p, idx, lse)
    torch.cuda.synchronize()
    for w, b, n in ((whole, before, n_seg * M * 4), (out_w, out_b, 3 * M)):      # bit-identical outside the records / the outputs
        assert torch.equal(w[:GUARD].view(torch.int32), b[:GUARD].view(torch.int32))
        assert torch.equal(w[GUARD + n:].view(torch.int32), b[GUARD + n:].view(torch.int32))
    return ws, p.clone(), idx.clone(), lse.clone()


@pytest.mark.parametrize("seed", [3, 2 ** 40 + 11])
@pytest.mark.parametrize("T", [0.5, 1.0, 4.0, BS.T_MAX])
def test_rowsample_gemm_and_combine_within_bounds(T, seed):
    """M = 256, N = 512, K = 128: two column tiles, 8 segments -- the lane merge, the segment merge and the cross-tile merge all happen;
    random bias, -1e30 in the last 100 columns"""
    M, N, K = 256, 512, 128
    A, Bm, bias_T, alpha = _fused_case(M, N, K, T, 100, 31)
    ls = FS.launch_seed(seed, 1)
    ws, p, idx, lse = _run_fused(_ops(), A, Bm, bias_T, alpha, ls)
    y, g, e = BS.tempered_reference(A, Bm, bias_T, alpha, ls)
    rows, n_adm_seg = BS.check_records(ws, y, g, e, "ROWSAMPLE")
    _table(rows, f"T={T} records")
    rows, n_adm = BS.check_rows(y, g, e, N // 64, p, idx, lse, "ROWSAMPLE + combine")
    _table(rows, f"T={T} rows")
    assert int(idx.max()) < N - 100 and int(idx.min()) >= 0                     # no padded index, ever
    print(f"  rows with more than one admissible column: {int((n_adm > 1).sum())} of {M}; distinct draws {idx.unique().numel()}")
    if T <= 4.0:
        assert idx.unique().numel() > 16                                        # a draw, not the mode of identical rows


def test_rowsample_exact_ties_choose_the_float64_argmax_of_the_noise():
    """M = 512, A = 0, no bias: every real logit is exactly 0, so the draw is the argmax of g alone"""
    M, N, K = 512, 512, 128
    A, Bm, bias_T, alpha = _fused_case(M, N, K, 1.0, 100, 32, zero_a=True, zero_bias=True)
    ls = FS.launch_seed(5, 0)
    ws, p, idx, lse = _run_fused(_ops(), A, Bm, bias_T, alpha, ls)
    y, g, e = BS.tempered_reference(A, Bm, bias_T, alpha, ls)
    assert bool((y[:, :N - 100] == 0).all()) and bool((e == 0).all())
    Bd.check_exact(idx.long(), FS.first_argmax(g[:, :N - 100]), "draw under exact ties")
    BS.check_records(ws, y, g, e, "ROWSAMPLE, exact ties")
    rows, _ = BS.check_rows(y, g, e, N // 64, p, idx, lse, "ROWSAMPLE + combine, exact ties")
    _table(rows, "exact ties")


# ---------------------------------------------------------------------------------------------------------------- 3. unfused path
@pytest.mark.parametrize("K", [10000, 1000])
def test_sample_rows_within_bounds(K):
    M, ld, T = 37, K + 8, 2.0
    gen = torch.Generator().manual_seed(40 + K)
    whole, lg, before = _guarded(M * ld)
    lg.view(M, ld)[:, :K] = (torch.randn(M, K, generator=gen) * 3).to(DEV)       # the row pads keep +-2^12
    before = whole.clone()
    ls = FS.launch_seed(9, 2)
    out_w, out, out_b = _guarded(3 * M)
    p, lse, idx = out[:M], out[M:2 * M], out[2 * M:].view(torch.int32)
    _ops(torch.float32).sample_rows(lg, M, K, ld, 1.0 / T, ls, p, idx, lse)
    torch.cuda.synchronize()
    assert torch.equal(whole.view(torch.int32), before.view(torch.int32))
    assert torch.equal(out_w[:GUARD], out_b[:GUARD]) and torch.equal(out_w[GUARD + 3 * M:], out_b[GUARD + 3 * M:])
    y, g, e = BS.logits_reference(lg.view(M, ld), K, 1.0 / T, ls)
    rows, n_adm = BS.check_rows(y, g, e, (K + 63) // 64 + 6, p, idx, lse, "sample_rows")
    _table(rows, f"K={K}")


def test_fused_and_unfused_paths_draw_the_same_from_the_same_logits():
    """logits that both paths see bit for bit: A, B hold multiples of 1/8 in [-2, 2], so A B^T (K = 64) is exact in fp32; no bias, 24
    pad columns.  y = logits * (1/T) in both kernels: the same admissible set, and equal ids wherever one column is admissible."""
    M, N, K, NR, T = 256, 1024, 64, 1000, 2.0
    gen = torch.Generator().manual_seed(50)
    A = (torch.randint(-16, 17, (M, K), generator=gen).float() / 8).bfloat16().to(DEV)
    Bm = (torch.randint(-16, 17, (N, K), generator=gen).float() / 8).bfloat16()
    Bm[NR:] = 0
    Bm = Bm.to(DEV)
    bias_T = torch.zeros(N, device=DEV)
    bias_T[NR:] = BS.PAD_BIAS
    ls = FS.launch_seed(21, 3)
    ws, p_f, idx_f, lse_f = _run_fused(_ops(), A, Bm, bias_T, 1.0 / T, ls)
    logits = (A.float() @ Bm.float().t()).contiguous()                          # exact
    assert torch.equal(logits.double(), A.double() @ Bm.double().t())
    Mu = 37
    p, lse, idx = torch.zeros(Mu, device=DEV), torch.zeros(Mu, device=DEV), torch.zeros(Mu, dtype=torch.int32, device=DEV)
    _ops(torch.float32).sample_rows(logits, Mu, NR, N, 1.0 / T, ls, p, idx, lse)
    torch.cuda.synchronize()
    y, g, e = BS.logits_reference(logits, NR, 1.0 / T, ls)
    _, n_f = BS.check_rows(y, g, e, N // 64, p_f, idx_f, lse_f, "fused on exact logits")
    _, n_u = BS.check_rows(y[:Mu], g[:Mu], e[:Mu], (NR + 63) // 64 + 6, p, idx, lse, "unfused on the same logits")
    assert torch.equal(n_f[:Mu], n_u)                                           # the same admissible set
    single = n_u == 1
    assert int(single.sum()) >= Mu - 3
    assert torch.equal(idx[single], idx_f[:Mu][single])


# ---------------------------------------------------------------------------------------------------------------- 4. distribution
def test_device_draws_follow_the_known_softmax():
    """16 384 identical rows x 256 columns through the fused GEMM (K = 64), logits within +-1: chi-square of the device's own ids
    against softmax of the float64 logits (threshold: the 1e-9 tail, as in test_sampling_cpu.py)"""
    M, N, K = 16384, 256, 64
    gen = torch.Generator().manual_seed(60)
    a = (torch.randint(-8, 9, (K,), generator=gen).float() / 8).bfloat16()
    Bm = (torch.randint(-8, 9, (N, K), generator=gen).float() / 64).bfloat16()
    alpha = float(torch.tensor(1.0 / float((Bm.double() @ a.double()).abs().max()), dtype=torch.float32))
    A = a[None, :].expand(M, -1).contiguous().to(DEV)
    ops = _ops()
    ws = torch.zeros((N // 64) * M * 4, device=DEV)
    ls = FS.launch_seed(77, 0)
    ops.gemm(A, Bm.to(DEV), None, None, None, ws, M, N, K, K, K, N, epilogue=EPI_ROWSAMPLE, alpha=alpha, seed=ls)
    idx = torch.zeros(M, dtype=torch.int32, device=DEV)
    p = torch.zeros(M, device=DEV)
    ops.rowsample_combine(ws, N // 64, M, ls, p, idx, None)
    torch.cuda.synchronize()
    y = alpha * (Bm.double() @ a.double())
    assert float(y.abs().max()) <= 1.0 + 1e-6
    prob = torch.softmax(y, 0)
    assert float(prob.min()) * M >= 5
    stat, thr = BS.chi2_stat(idx.cpu(), prob * M), BS.chi2_threshold(N - 1)
    print(f"device draws: chi2 {stat:.1f} over {N - 1} degrees of freedom (threshold {thr:.1f})")
    assert stat < thr
    # and the probability reported for a drawn code is that code's softmax probability
    assert float((p.cpu().double() - prob[idx.cpu().long()]).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- 5. engine
def _engine(g, dtype, B=None, grid=None):
    import lxmert_oracle as O
    from _util import golden_cfg
    from xlxmert_amd.config import XLxmertConfig
    from xlxmert_amd.engine import Engine
    from xlxmert_amd.params import ParamStore
    oc = golden_cfg(g)
    cfg = XLxmertConfig(**{k: getattr(oc, k) for k in ("vocab_size", "hidden_size", "num_attention_heads", "intermediate_size",
                                                      "max_position_embeddings", "type_vocab_size", "l_layers", "x_layers", "r_layers",
                                                      "visual_feat_dim", "visual_pos_dim", "num_clusters")})
    sd = O.make_state_dict(oc, int(g["seed"]))
    ids = torch.from_numpy(g["in_input_ids"])
    grid = int(g["grid"]) if grid is None else grid
    if B is not None:
        ids = ids[:1].expand(B, -1).clone()
        ids[1:, 2] = (ids[1:, 2] + torch.arange(1, B)) % (cfg.vocab_size - 1) + 1
    B, L = ids.shape
    V = grid * grid
    store = ParamStore(cfg, DEV, dtype, task="vis_mask")
    store.load_named(sd)
    eng = Engine(cfg, store, _ops(dtype), B, L, V, need_lang=False)
    eng.sync_compute_weights()
    pos = torch.from_numpy(O.box_position(grid)).unsqueeze(0).expand(B, -1, -1).float()
    eng.set_inputs(ids.to(DEV), (ids > 0).to(DEV), None, pos.to(DEV), cluster_ids=torch.zeros(B, V, dtype=torch.long, device=DEV),
                   vis_mask=torch.ones(B, V, dtype=torch.bool, device=DEV))
    return eng


def _grab(eng, snaps):
    """on_step hook: the kernel's own inputs of this step's draw (features or logits) and its outputs"""
    def hook(i):
        fused = eng.fused_predict_available()
        snaps.append({"fused": fused, "feat": eng.feat.clone() if fused else None, "logits": None if fused else eng.logits.clone(),
                      "ids": eng.row_argmax.clone(), "p": eng.row_maxprob.clone(), "lse": eng.row_lse.clone(),
                      "mask": int(eng.vmask.sum()), "cid": eng.cid.clone()})
    return hook


def _check_step(eng, s, T, launch_seed, what):
    """one step's ids / probability / lse on the kernel's own inputs against float64; returns the admissible counts per row"""
    if s["fused"]:
        Kq = eng.code_pred.w_pad.shape[0]
        y, g, e = BS.tempered_reference(s["feat"][:eng.MV].view(eng.MV, eng.F), eng.code_pred.w_pad, eng.code_pred.bias_pad_T, 1.0 / T, launch_seed)
        rows, n_adm = BS.check_rows(y, g, e, Kq // 64, s["p"], s["ids"], s["lse"], what)
        assert int(s["ids"].max()) < eng.K
    else:
        y, g, e = BS.logits_reference(s["logits"][:eng.MV].view(eng.MV, eng.K), eng.K, 1.0 / T, launch_seed)
        rows, n_adm = BS.check_rows(y, g, e, (eng.K + 63) // 64 + 6, s["p"], s["ids"], s["lse"], what)
    return n_adm


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_nar_sampling_properties_and_steps_admissible(dtype):
    from xlxmert_amd.engine import Engine
    g = load_golden("sampler_tiny")
    n_steps, T = int(g["n_steps"]), 1.0
    eng = _engine(g, dtype)
    plain = [x.clone() for x in eng.sample_codes_nar(n_steps)]
    g_snaps = []
    none = [x.clone() for x in eng.sample_codes_nar(n_steps, _grab(eng, g_snaps), temperature=None, seed=3)]
    assert all(torch.equal(a, b) for a, b in zip(plain, none))              # temperature=None: bit-identical ids, codes, probabilities
    runs = {}
    for key, seed in (("a", 7), ("b", 7), ("c", 8)):
        snaps = []
        cid, _, prob = eng.sample_codes_nar(n_steps, _grab(eng, snaps), temperature=T, seed=seed)
        runs[key] = (cid.clone(), prob.clone(), snaps)
    torch.cuda.synchronize()
    assert torch.equal(runs["a"][0], runs["b"][0]) and torch.equal(runs["a"][1], runs["b"][1])       # same seed: identical
    assert not torch.equal(runs["a"][2][0]["ids"], runs["c"][2][0]["ids"])                           # another seed: another draw
    assert [s["mask"] for s in runs["a"][2]] == [s["mask"] for s in g_snaps]                         # the greedy schedule's masks
    for i, s in enumerate(runs["a"][2]):
        _check_step(eng, s, T, Engine.sample_launch_seed(7, i), f"{dtype} step {i}")
        assert bool(((s["p"] > 0) & (s["p"] <= 1)).all())
    assert int(runs["a"][0].max()) < eng.K
    # another step: the same logits and user seed under step 0's and step 1's launch seed draw differently
    assert not eng.fused_predict_available()
    eng.head_forward()
    out = []
    for step in (0, 1):
        eng._predict_step(False, T, Engine.sample_launch_seed(7, step))
        out.append(eng.row_argmax.clone())
    assert not torch.equal(out[0], out[1])


@pytest.mark.parametrize("mode", ["confidence", "tlbr", "random"])
def test_engine_ar_sampling_policies(mode):
    from xlxmert_amd.engine import Engine
    g = load_golden("sampler_ar_tiny")
    eng = _engine(g, torch.float32)
    B, V = eng.B, eng.V
    pos = g["random_positions"].tolist()[-V:]
    plain = eng.sample_codes_ar(None, mode, positions=pos)[0].clone()
    assert torch.equal(plain, eng.sample_codes_ar(None, mode, positions=pos, temperature=None, seed=4)[0])
    outs = []
    for seed in (11, 11, 12):
        trace, snaps = [], []
        cid = eng.sample_codes_ar(None, mode, positions=pos, trace=trace, on_step=_grab(eng, snaps), temperature=2.0, seed=seed)[0].clone()
        assert [int(m.sum()) for m in trace] == [B * (V - i - 1) for i in range(V)]
        outs.append((cid, snaps))
    assert torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][0], outs[2][0])
    for i in (0, V // 2, V - 1):
        _check_step(eng, outs[0][1][i], 2.0, Engine.sample_launch_seed(11, i), f"AR {mode} step {i}")


def test_engine_bf16_fused_and_unfused_first_step_agree(monkeypatch):
    """bf16, B*V = 256: the first step's draw through XL_EPI_ROWSAMPLE + combine and, with XL_FUSED_PREDICT=0, through the fp32
    logits + xl_sample_rows: each admissible on its own inputs, equal wherever a single column is admissible for both"""
    from xlxmert_amd.engine import Engine
    g = load_golden("sampler_tiny")
    T, seed = 2.0, 13
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("XL_FUSED_PREDICT", fused)
        eng = _engine(g, torch.bfloat16, B=4, grid=8)
        assert eng.MV == 256 and eng.fused_predict_available() == (fused == "1")
        snaps = []
        eng.sample_codes_nar(2, _grab(eng, snaps), temperature=T, seed=seed)
        torch.cuda.synchronize()
        assert snaps[0]["fused"] == (fused == "1")
        n_adm = _check_step(eng, snaps[0], T, Engine.sample_launch_seed(seed, 0), f"fused={fused} step 0")
        _check_step(eng, snaps[1], T, Engine.sample_launch_seed(seed, 1), f"fused={fused} step 1")
        res[fused] = (snaps[0]["ids"], n_adm)
    single = (res["1"][1] == 1) & (res["0"][1] == 1)
    print(f"fused / unfused first step: {int(single.sum())} of 256 rows with a single admissible column")
    assert int(single.sum()) > 200
    assert torch.equal(res["1"][0][single], res["0"][0][single])


# ---------------------------------------------------------------------------------------------------------------- 6. public API
def test_imggen_model_sampling_keywords():
    """the same caption twice: at T = 1 the two rows' codes differ, greedy they are equal; sample_seed reproduces; torch.manual_seed
    governs the default seed; `seed` of sample_image_AR keeps meaning the position order"""
    from test_modeling_gpu import _imggen_model
    g = load_golden("sampler_tiny")
    m, grid = _imggen_model(g)
    ids = torch.from_numpy(g["in_input_ids"])[:1].expand(2, -1).contiguous().cuda()
    n = int(g["n_steps"])
    m.sample_image_NAR(ids, n_steps=n)
    greedy = m.code_ids.clone()
    assert torch.equal(greedy[0], greedy[1])
    m.sample_image_NAR(ids, n_steps=n, temperature=None, sample_seed=7)
    assert torch.equal(m.code_ids, greedy)
    img7 = m.sample_image_NAR(ids, n_steps=n, temperature=1.0, sample_seed=7)
    c7 = m.code_ids.clone()
    assert not torch.equal(c7[0], c7[1])
    assert torch.equal(m.sample_image_NAR(ids, n_steps=n, temperature=1.0, sample_seed=7), img7) and torch.equal(m.code_ids, c7)
    steps = m.sample_image_NAR(ids, n_steps=n, temperature=1.0, sample_seed=7, return_intermediate=True)
    assert len(steps) == n and torch.equal(steps[-1], img7)
    torch.manual_seed(5)
    m.sample_image_NAR(ids, n_steps=n, temperature=1.0)
    d1 = m.code_ids.clone()
    m.sample_image_NAR(ids, n_steps=n, temperature=1.0)
    d2 = m.code_ids.clone()
    torch.manual_seed(5)
    m.sample_image_NAR(ids, n_steps=n, temperature=1.0)
    assert torch.equal(m.code_ids, d1) and not torch.equal(d1, d2)
    for kw in ({}, dict(position_TLBR=True), dict(position_random=True, seed=7)):
        m.sample_image_AR(ids, temperature=1.0, sample_seed=3, **kw)
        a = m.code_ids.clone()
        assert not torch.equal(a[0], a[1])
        m.sample_image_AR(ids, temperature=1.0, sample_seed=3, **kw)
        assert torch.equal(m.code_ids, a)
    out, cid = m.sample_codes(ids, n_steps=n, grid_size=grid, temperature=1.0, seed=7)
    assert torch.equal(cid, c7)
    with pytest.raises(ValueError):
        m.sample_image_NAR(ids, n_steps=n, temperature=0.0)
    with pytest.raises(ValueError):
        m.sample_codes(ids, temperature=float("nan"))
