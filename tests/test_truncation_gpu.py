"""Truncated sampling on the device: xl_sample_rows_trunc, the engine loops and the ImggenModel surface under the checks of
tests/bounds_truncation.py (exact rank / candidates / min-p, bounded top-p, admissible draw against the kernel's own kept count;
derivations there).  Every kernel case: ldl = K + 24 with the pad columns at +2^12 (a kernel that reads them draws them), logits
and outputs embedded in guard storage that must stay bit-identical."""
import functools
import math

import pytest
import torch

import bounds_sampling as BS
import bounds_truncation as BT
import fake_ops_sampling as FS
import fake_ops_truncation as FT
from _util import load_golden
from test_sampling_gpu import _engine, _guarded, _ops, GUARD
from test_truncation_cpu import CHI2_SEED, chi2_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEG_INF = -math.inf
PAD = 24


def _lmp(min_p):
    return NEG_INF if min_p is None else math.log(min_p)


def _launch(values, K, T, seed, top_k=None, top_p=None, min_p=None):
    """values [M, K] (any device) -> the kernel's four outputs, and the logits [M, K + PAD] it read.  top_k / top_p None: 256 / 1."""
    M = values.shape[0]
    ld = K + PAD
    whole, lg, _ = _guarded(M * ld)
    lg = lg.view(M, ld)
    lg[:, K:] = 4096.0
    lg[:, :K] = values.to(DEV)
    before = whole.clone()
    out_w, out, out_b = _guarded(4 * M)
    p, lse = out[:M], out[M:2 * M]
    idx, kept = out[2 * M:3 * M].view(torch.int32), out[3 * M:].view(torch.int32)
    _ops(torch.float32).sample_rows_trunc(lg, M, K, ld, 1.0 / T, seed, 256 if top_k is None else top_k, 1.0 if top_p is None else top_p,
                                          _lmp(min_p), p, idx, lse, kept)
    torch.cuda.synchronize()
    assert torch.equal(whole.view(torch.int32), before.view(torch.int32))                      # the logits and their guards
    assert torch.equal(out_w[:GUARD].view(torch.int32), out_b[:GUARD].view(torch.int32))
    assert torch.equal(out_w[GUARD + 4 * M:].view(torch.int32), out_b[GUARD + 4 * M:].view(torch.int32))
    return lg, p.clone(), idx.clone(), lse.clone(), kept.clone()


def _check(lg, K, T, seed, top_k, top_p, min_p, outs, what):
    p, idx, lse, kept = outs
    res = BT.check_trunc(lg, K, 1.0 / T, seed, 256 if top_k is None else top_k, 1.0 if top_p is None else top_p, _lmp(min_p),
                         p, idx, lse, kept, what)
    print(f"  {what}: kept min/median/max {res['kept']}, undecided rows {100 * res['undecided']:.1f} %, largest top-p bound "
          f"{res['b_max']:.2e}, row_lse {res['row_lse']:.3f} row_prob {res['row_prob']:.3f} of their bounds")
    return res


@functools.lru_cache(maxsize=None)
def _gauss(std, K, M=512):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(1000 * std + K % 997)) * std


# ---------------------------------------------------------------------------------------------------------------- 1. kernel
@pytest.mark.parametrize("min_p", [None, 0.05])
@pytest.mark.parametrize("top_k", [None, 50])
@pytest.mark.parametrize("std,K,T,top_p", [(4, 10000, 1.0, 0.5), (4, 10000, 0.7, 0.9), (4, 1000, 1.0, 0.9), (2, 300, 1.0, 0.9)])
def test_gaussian_logits_top_p_within_bounds(std, K, T, top_p, top_k, min_p):
    seed = FS.launch_seed(41, K % 7)
    lg, *outs = _launch(_gauss(std, K), K, T, seed, top_k, top_p, min_p)
    res = _check(lg, K, T, seed, top_k, top_p, min_p, outs, f"std {std} K {K} T {T} top_p {top_p} top_k {top_k} min_p {min_p}")
    assert res["b_max"] < 1e-4
    assert res["undecided"] <= 0.10                             # not vacuous: at least 90 % of the rows have k_lo == k_hi


def test_candidate_cap_shows_in_row_kept():
    """std 2, T = 2, top_p = 0.5: the nucleus is wider than 256 codes in every row, so every row reports the cap"""
    K, T, seed = 10000, 2.0, FS.launch_seed(42, 0)
    lg, *outs = _launch(_gauss(2, K), K, T, seed, None, 0.5, None)
    _check(lg, K, T, seed, None, 0.5, None, outs, "cap")
    assert bool((outs[3] == 256).all())


@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("K", [10000, 257, 100])
@pytest.mark.parametrize("top_k", [1, 2, 50, 256])
def test_top_k_alone_is_exact(top_k, K, T):
    seed = FS.launch_seed(43, top_k)
    lg, *outs = _launch(_gauss(4, K, 64), K, T, seed, top_k, None, None)
    res = _check(lg, K, T, seed, top_k, None, None, outs, f"top_k {top_k} K {K} T {T}")
    assert bool((outs[3] == min(K, top_k)).all()) and res["undecided"] == 0.0               # K = 100 < 256: the clamp
    if top_k == 1:
        assert torch.equal(outs[1].long(), FS.first_argmax(res["ref"].y32))


@pytest.mark.parametrize("top_k,top_p", [(50, None), (256, 0.9), (7, None)])
def test_ties_across_the_candidate_boundary(top_k, top_p):
    """logits rounded to multiples of 0.5: the boundary of the candidate set cuts through groups of equal values"""
    K, seed = 10000, FS.launch_seed(44, top_k)
    vals = (_gauss(4, K, 128) * 2).round() / 2
    lg, *outs = _launch(vals, K, 1.0, seed, top_k, top_p, None)
    res = _check(lg, K, 1.0, seed, top_k, top_p, None, outs, f"ties top_k {top_k} top_p {top_p}")
    ys = res["ref"].y32.gather(1, res["ref"].order[:, :min(K, top_k) + 1])
    assert int((ys[:, -1] == ys[:, -2]).sum()) > 32             # the case is what it says: ties at the boundary in many rows


def test_all_equal_one_hot_and_signed_zero_rows():
    seed = FS.launch_seed(45, 0)
    lg, *outs = _launch(torch.full((64, 1000), 0.25), 1000, 1.0, seed, None, 0.1005, None)
    _check(lg, 1000, 1.0, seed, None, 0.1005, None, outs, "all equal")
    assert bool((outs[3] == 101).all()) and int(outs[1].max()) < 101            # off the 1 / K lattice: c_r = r / 1000 < 0.1005
    lg, *outs = _launch(torch.full((64, 1000), -3.0), 1000, 0.5, seed, 37, None, None)
    _check(lg, 1000, 0.5, seed, 37, None, None, outs, "all equal, top_k")
    assert bool((outs[3] == 37).all()) and int(outs[1].max()) < 37 and outs[1].unique().numel() > 20
    one_hot = torch.full((64, 300), -30.0)
    one_hot[torch.arange(64), torch.arange(64) * 4] = 5.0
    lg, *outs = _launch(one_hot, 300, 1.0, seed, None, 0.9, None)
    _check(lg, 300, 1.0, seed, None, 0.9, None, outs, "one hot")
    assert bool((outs[3] == 1).all()) and outs[1].tolist() == [4 * i for i in range(64)]
    zeros = torch.zeros(128, 640)
    zeros[:, ::2] = -0.0
    zeros[:, 400:] = -1.0
    lg, *outs = _launch(zeros, 640, 1.0, seed, 10, None, None)
    _check(lg, 640, 1.0, seed, 10, None, None, outs, "signed zeros")
    assert bool((outs[3] == 10).all()) and int(outs[1].max()) < 10 and outs[1].unique().numel() == 10


@pytest.mark.parametrize("K", [12288, 12289, 30522])
def test_large_rows(K):
    """the last row length whose keys stay in LDS, the first that is read again in every pass, and a 30 522-word vocabulary (M = 8:
    too few rows for the 90 % guard, which the Gaussian cases carry)"""
    seed = FS.launch_seed(46, K)
    vals = _gauss(3, K, 8)
    for top_k, top_p, min_p in ((50, None, None), (None, 0.8, 0.01)):
        lg, *outs = _launch(vals, K, 1.0, seed, top_k, top_p, min_p)
        _check(lg, K, 1.0, seed, top_k, top_p, min_p, outs, f"K {K} top_k {top_k} top_p {top_p}")
    vals = (vals * 2).round() / 2
    lg, *outs = _launch(vals, K, 1.0, seed, 100, None, None)
    _check(lg, K, 1.0, seed, 100, None, None, outs, f"K {K} ties")


@pytest.mark.parametrize("T,top_k,top_p,min_p", [(1.0, 50, None, None), (0.7, None, 0.9, None), (2.0, None, None, 0.05)])
def test_coupled_with_the_untruncated_draw(T, top_k, top_p, min_p):
    """rule 6: the same noise function, so xl_sample_rows' draw on the same logits and seed is the truncated draw wherever it lies in
    the kept set (and cannot be it elsewhere).  The two kernels round z differently (xl_sample_rows' compiled code contracts the
    multiply into the add, this kernel adds the noise to the rounded y), so equality is demanded wherever the float64 rule admits
    a single column -- all rows but a handful -- as test_sampling_gpu.py does for the fused and the unfused path."""
    K, M, seed = 1000, 512, FS.launch_seed(47, 1)
    lg, p, idx, lse, kept = _launch(_gauss(4, K), K, T, seed, top_k, top_p, min_p)
    res = _check(lg, K, T, seed, top_k, top_p, min_p, (p, idx, lse, kept), "coupling")
    pu, lu, iu = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV), torch.zeros(M, dtype=torch.int32, device=DEV)
    _ops(torch.float32).sample_rows(lg, M, K, K + PAD, 1.0 / T, seed, pu, iu, lu)
    torch.cuda.synchronize()
    order = FT.rank_order(FT.tempered_y32(lg, K, 1.0 / T))
    rank_u = (order == iu.long()[:, None]).to(torch.uint8).argmax(1)
    inside = rank_u < kept
    print(f"  coupling: {int(inside.sum())} of {M} untruncated draws inside the kept set")
    assert 50 < int(inside.sum()) < M
    single = inside & (res["n_adm"] == 1)
    assert int(single.sum()) >= int(inside.sum()) - 3
    assert torch.equal(idx[single], iu[single])
    assert bool((idx[~inside] != iu[~inside]).all())


def test_device_draws_follow_the_renormalised_top_k_softmax():
    """4 096 rows of one vector, top_k = 20, T = 1: chi-square of the device's own draws over the twenty live columns (dof 19)"""
    logits, live, expected = chi2_case()
    seed = FS.launch_seed(CHI2_SEED, 0)
    lg, p, idx, lse, kept = _launch(logits, 300, 1.0, seed, 20, None, None)
    cols = live.sort().values
    assert bool((kept == 20).all()) and bool(torch.isin(idx.cpu().long(), cols).all())
    stat, thr = BS.chi2_stat(torch.searchsorted(cols, idx.cpu().long()), expected[cols]), BS.chi2_threshold(19)
    print(f"device top-20 draws: chi2 {stat:.1f} over 19 degrees of freedom (threshold {thr:.1f})")
    assert stat < thr


def test_one_seed_reproduces_all_four_outputs():
    K, T = 10000, 0.9
    a = _launch(_gauss(4, K), K, T, FS.launch_seed(48, 0), None, 0.9, 0.01)[1:]
    b = _launch(_gauss(4, K), K, T, FS.launch_seed(48, 0), None, 0.9, 0.01)[1:]
    c = _launch(_gauss(4, K), K, T, FS.launch_seed(49, 0), None, 0.9, 0.01)[1:]
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert not torch.equal(a[1], c[1]) and torch.equal(a[3], c[3]) and torch.equal(a[2].view(torch.int32), c[2].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 2. engine
def _grab(eng, snaps):
    def hook(i):
        snaps.append({"logits": eng.logits.clone(), "ids": eng.row_argmax.clone(), "p": eng.row_maxprob.clone(), "lse": eng.row_lse.clone(),
                      "kept": eng.row_kept.clone() if getattr(eng, "row_kept", None) is not None else None, "mask": int(eng.vmask.sum())})
    return hook


def _check_step(eng, s, T, launch_seed, trunc, what):
    top_k, top_p, log_min_p = trunc
    return BT.check_trunc(s["logits"][:eng.MV].view(eng.MV, eng.K), eng.K, 1.0 / T, launch_seed, top_k, top_p, log_min_p, s["p"], s["ids"],
                          s["lse"], s["kept"], what)


def test_engine_nar_fp32_top_k_1_is_greedy_and_every_step_admissible():
    from xlxmert_amd.engine import Engine
    g = load_golden("sampler_tiny")
    n_steps = int(g["n_steps"])
    eng = _engine(g, torch.float32)
    g_snaps = []
    greedy = [x.clone() for x in eng.sample_codes_nar(n_steps, _grab(eng, g_snaps))]
    snaps = []
    eng.sample_codes_nar(n_steps, _grab(eng, snaps), top_k=1, seed=5)
    torch.cuda.synchronize()
    assert torch.equal(snaps[0]["ids"], g_snaps[0]["ids"])                       # step 0: the greedy loop's codes
    for i, s in enumerate(snaps):                                              # teacher-forced on the engine's own logits
        _check_step(eng, s, 1.0, Engine.sample_launch_seed(5, i), (1, 1.0, NEG_INF), f"top_k 1 step {i}")
        assert bool((s["kept"] == 1).all())
    runs = {}
    for key, seed in (("a", 7), ("b", 7), ("c", 8)):
        snaps = []
        cid, _, prob = eng.sample_codes_nar(n_steps, _grab(eng, snaps), temperature=1.5, seed=seed, top_k=20, top_p=0.9, min_p=0.01)
        runs[key] = (cid.clone(), prob.clone(), snaps)
    torch.cuda.synchronize()
    assert torch.equal(runs["a"][0], runs["b"][0]) and torch.equal(runs["a"][1], runs["b"][1])
    assert not torch.equal(runs["a"][2][0]["ids"], runs["c"][2][0]["ids"])
    assert [s["mask"] for s in runs["a"][2]] == [s["mask"] for s in g_snaps]
    trunc = Engine.check_truncation(20, 0.9, 0.01)
    for i, s in enumerate(runs["a"][2]):
        _check_step(eng, s, 1.5, Engine.sample_launch_seed(7, i), trunc, f"fp32 step {i}")
        assert bool(((s["p"] > 0) & (s["p"] <= 1)).all()) and int(s["kept"].max()) <= 20
    assert int(runs["a"][0].max()) < eng.K
    plain = [x.clone() for x in eng.sample_codes_nar(n_steps)]                  # and the greedy loop is what it was
    assert all(torch.equal(a, b) for a, b in zip(plain, greedy))


def test_engine_bf16_takes_the_logits_path_where_the_fused_path_is_available():
    from xlxmert_amd.engine import Engine
    g = load_golden("sampler_tiny")
    eng = _engine(g, torch.bfloat16, B=4, grid=8)
    assert eng.MV == 256 and eng.fused_predict_available()
    snaps = []
    eng.sample_codes_nar(2, _grab(eng, snaps), temperature=2.0, seed=13, top_k=50, top_p=0.9)
    torch.cuda.synchronize()
    trunc = Engine.check_truncation(50, 0.9, None)
    for i, s in enumerate(snaps):
        _check_step(eng, s, 2.0, Engine.sample_launch_seed(13, i), trunc, f"bf16 step {i}")


@pytest.mark.parametrize("mode", ["confidence", "tlbr", "random"])
def test_engine_ar_truncated_policies(mode):
    from xlxmert_amd.engine import Engine
    g = load_golden("sampler_ar_tiny")
    eng = _engine(g, torch.float32)
    B, V = eng.B, eng.V
    pos = g["random_positions"].tolist()[-V:]
    outs = []
    for seed in (11, 11, 12):
        trace, snaps = [], []
        cid = eng.sample_codes_ar(None, mode, positions=pos, trace=trace, on_step=_grab(eng, snaps), temperature=2.0, seed=seed, top_k=5)[0].clone()
        assert [int(m.sum()) for m in trace] == [B * (V - i - 1) for i in range(V)]      # one position per step, all visited after V
        outs.append((cid, snaps))
    assert torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][0], outs[2][0])
    for i in (0, V // 2, V - 1):
        _check_step(eng, outs[0][1][i], 2.0, Engine.sample_launch_seed(11, i), (5, 1.0, NEG_INF), f"AR {mode} step {i}")


# ---------------------------------------------------------------------------------------------------------------- 3. public API
def test_imggen_model_truncation_keywords():
    """the same caption twice through an identity generator: top_k = 1 is the greedy image whatever the seed; a truncated draw
    differs between the two rows, reproduces for a sample_seed, and reaches sample_codes and all three AR policies"""
    from test_modeling_gpu import _imggen_model
    g = load_golden("sampler_tiny")
    m, grid = _imggen_model(g)
    ids = torch.from_numpy(g["in_input_ids"])[:1].expand(2, -1).contiguous().cuda()
    n = int(g["n_steps"])
    img_g = m.sample_image_NAR(ids, n_steps=n)
    greedy = m.code_ids.clone()
    # (step 0 of top_k = 1 is the greedy step; later steps re-mask by the same confidences within rounding: compare step 0)
    first = m.sample_image_NAR(ids, n_steps=n, top_k=1, sample_seed=9, return_intermediate=True)[0]
    assert torch.equal(first, m.sample_image_NAR(ids, n_steps=n, return_intermediate=True)[0])
    img = m.sample_image_NAR(ids, n_steps=n, temperature=1.5, top_k=20, top_p=0.95, sample_seed=7)
    c7 = m.code_ids.clone()
    assert not torch.equal(c7[0], c7[1])
    assert torch.equal(m.sample_image_NAR(ids, n_steps=n, temperature=1.5, top_k=20, top_p=0.95, sample_seed=7), img)
    assert torch.equal(m.code_ids, c7)
    m.sample_image_NAR(ids, n_steps=n, min_p=0.01, sample_seed=7)                # temperature None: T = 1
    a = m.code_ids.clone()
    m.sample_image_NAR(ids, n_steps=n, temperature=1.0, min_p=0.01, sample_seed=7)
    assert torch.equal(m.code_ids, a) and not torch.equal(a[0], a[1])
    for kw in ({}, dict(position_TLBR=True), dict(position_random=True, seed=7)):
        m.sample_image_AR(ids, top_k=5, sample_seed=3, **kw)
        a = m.code_ids.clone()
        assert not torch.equal(a[0], a[1])
        m.sample_image_AR(ids, top_k=5, sample_seed=3, **kw)
        assert torch.equal(m.code_ids, a)
    out, cid = m.sample_codes(ids, n_steps=n, grid_size=grid, temperature=1.5, seed=7, top_k=20, top_p=0.95)
    assert torch.equal(cid, c7)
    m.sample_image_NAR(ids, n_steps=n)
    assert torch.equal(m.code_ids, greedy) and torch.equal(m.sample_image_NAR(ids, n_steps=n), img_g)
    with pytest.raises(ValueError, match="top_k"):
        m.sample_image_NAR(ids, n_steps=n, top_k=0)
    with pytest.raises(ValueError, match="top_p"):
        m.sample_image_AR(ids, top_p=1.5)
    with pytest.raises(ValueError, match="min_p"):
        m.sample_codes(ids, min_p=0.0)
