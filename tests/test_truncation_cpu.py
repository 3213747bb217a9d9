"""Truncated sampling (top-k / top-p / min-p) without a GPU: properties of the restatement in tests/fake_ops_truncation.py, the
argument checks, the engine's sequencing over TruncationFakeOps, and the honest / injected-fault pair of the bounds in
tests/bounds_truncation.py.  The kernel itself is held to the same bounds in test_truncation_gpu.py."""
import math

import pytest
import torch

import bounds_sampling as BS
import bounds_truncation as BT
import fake_ops_sampling as FS
import fake_ops_truncation as FT
from _util import load_golden
from fake_ops_sampling import EPI_ROWSAMPLE, SamplingFakeOps
from fake_ops_truncation import TruncationFakeOps
from test_engine_cpu import make_sampler_engine
from xlxmert_amd.engine import Engine

EPI_ROWMAX = 5
NEG_INF = -math.inf
CHI2_SEED = 20241018          # the seed of the chi-square cases here and on the device (the restatement passes with it)


def _run(ops, logits, K, T, seed, top_k=256, top_p=1.0, min_p=None):
    M, ld = logits.shape
    p, lse = torch.zeros(M), torch.zeros(M)
    idx, kept = torch.zeros(M, dtype=torch.int32), torch.zeros(M, dtype=torch.int32)
    ops.sample_rows_trunc(logits, M, K, ld, 1.0 / T, seed, top_k, top_p, NEG_INF if min_p is None else math.log(min_p), p, idx, lse, kept)
    return p, idx, lse, kept


def chi2_case(M=4096, K=300):
    """M rows of one logit vector: linspace(0, -2, 20), then -10; with top_k = 20 the draw follows the renormalised top-20 softmax"""
    x = torch.full((K,), -10.0)
    x[:20] = torch.linspace(0, -2, 20)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(3))
    row = torch.empty(K)
    row[perm] = x                                              # the twenty live columns anywhere in the row
    expected = torch.zeros(K, dtype=torch.float64)
    expected[perm[:20]] = torch.softmax(x[:20].double(), 0) * M
    return row[None, :].expand(M, -1).contiguous(), perm[:20], expected


# ---------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("seed", [0, 1, 7, 2 ** 40 + 3])
def test_top_k_1_is_the_first_argmax_for_every_seed(seed):
    gen = torch.Generator().manual_seed(1)
    logits = (torch.randn(64, 500, generator=gen) * 2).round()             # integers: plenty of tied maxima
    p, idx, lse, kept = _run(TruncationFakeOps(torch.float32), logits, 500, 1.0, FS.launch_seed(seed, 0), top_k=1)
    assert torch.equal(idx.long(), FS.first_argmax(logits)) and bool((kept == 1).all())
    assert torch.allclose(p.double(), torch.softmax(logits.double(), 1).amax(1), rtol=1e-5)      # the greedy confidence


@pytest.mark.parametrize("T,top_k,top_p,min_p", [(1.0, 50, 1.0, None), (0.7, 256, 0.9, None), (2.0, 256, 1.0, 0.05), (1.0, 20, 0.8, 0.02)])
def test_truncated_draw_equals_the_untruncated_draw_inside_the_kept_set(T, top_k, top_p, min_p):
    """rule 6: the noise is the same function, so wherever sample_rows' draw lies in the kept set both agree"""
    gen = torch.Generator().manual_seed(2)
    M, K = 512, 1000
    logits = torch.randn(M, K, generator=gen) * 4
    seed = FS.launch_seed(11, 2)
    ops = TruncationFakeOps(torch.float32)
    p, idx, lse, kept = _run(ops, logits, K, T, seed, top_k, top_p, min_p)
    pu, lu, iu = torch.zeros(M), torch.zeros(M), torch.zeros(M, dtype=torch.int32)
    ops.sample_rows(logits, M, K, K, 1.0 / T, seed, pu, iu, lu)
    order = FT.rank_order(FT.tempered_y32(logits, K, 1.0 / T))
    rank_u = (order == iu.long()[:, None]).to(torch.uint8).argmax(1)
    inside = rank_u < kept
    assert 50 < int(inside.sum()) < M                                       # both kinds of row occur
    assert torch.equal(idx[inside], iu[inside]) and torch.equal(p[inside], pu[inside])
    assert bool((idx[~inside] != iu[~inside]).all())
    assert torch.allclose(lse, lu, rtol=1e-6)


def test_all_equal_row_keeps_the_lowest_columns_and_small_k_clamps():
    ops = TruncationFakeOps(torch.float32)
    logits = torch.full((256, 1000), 0.25)
    p, idx, lse, kept = _run(ops, logits, 1000, 1.0, FS.launch_seed(5, 0), top_k=37)
    assert bool((kept == 37).all()) and int(idx.max()) < 37 and idx.unique().numel() > 20
    p, idx, lse, kept = _run(ops, logits, 1000, 1.0, FS.launch_seed(5, 0), top_p=0.1005)
    assert bool((kept == 101).all()) and int(idx.max()) < 101             # c_r = r / 1000 < 0.1005 for r <= 100
    logits = torch.randn(64, 100, generator=torch.Generator().manual_seed(4))
    p, idx, lse, kept = _run(ops, logits, 100, 1.0, FS.launch_seed(5, 1), top_k=256)           # K < top_k
    assert bool((kept == 100).all())
    one_hot = torch.full((8, 300), -30.0)
    one_hot[torch.arange(8), torch.arange(8) * 7] = 5.0
    p, idx, lse, kept = _run(ops, one_hot, 300, 1.0, FS.launch_seed(5, 2), top_p=0.9)
    assert bool((kept == 1).all()) and idx.tolist() == [i * 7 for i in range(8)]


def test_signed_zeros_rank_by_column():
    """-0 and +0 are one value: a row of mixed zeros is all ties, ranked by column alone"""
    M, K = 128, 64
    logits = torch.zeros(M, K)
    logits[:, ::2] = -0.0
    logits[:, 40:] = -1.0
    r = FT.restate(logits, K, 1.0, FS.launch_seed(9, 0), 10, 1.0, NEG_INF)
    assert torch.equal(r.order[:, :40], torch.arange(40)[None, :].expand(M, -1))
    assert bool((r.k_s == 10).all()) and int(r.s.max()) < 10 and r.s.unique().numel() == 10


def test_restated_draws_follow_the_renormalised_top_k_softmax():
    logits, live, expected = chi2_case()
    assert float(expected[live].min()) >= 60
    p, idx, lse, kept = _run(TruncationFakeOps(torch.float32), logits, 300, 1.0, FS.launch_seed(CHI2_SEED, 0), top_k=20)
    assert bool((kept == 20).all()) and bool(torch.isin(idx.long(), live).all())
    cols = live.sort().values                                  # the twenty cells of the statistic
    stat = BS.chi2_stat(torch.searchsorted(cols, idx.long()), expected[cols])
    thr = BS.chi2_threshold(19)
    print(f"restated top-20 draws: chi2 {stat:.1f} over 19 degrees of freedom (threshold {thr:.1f})")
    assert stat < thr


# ---------------------------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("kw", [dict(top_k=0), dict(top_k=257), dict(top_k=-1), dict(top_k=True), dict(top_k=5.0), dict(top_k="5"),
                                dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1), dict(top_p=float("nan")), dict(top_p=float("inf")),
                                dict(top_p=True), dict(top_p="0.5"),
                                dict(min_p=0.0), dict(min_p=1.0001), dict(min_p=-1.0), dict(min_p=float("nan")), dict(min_p=float("inf")),
                                dict(min_p=False), dict(top_k=5, top_p=2.0), dict(top_p=0.5, min_p=0.0)])
def test_bad_truncation_arguments_raise(kw):
    name = [k for k in ("top_k", "top_p", "min_p") if k in kw][-1] if len(kw) > 1 else next(iter(kw))
    with pytest.raises(ValueError, match=name):
        Engine.check_truncation(kw.get("top_k"), kw.get("top_p"), kw.get("min_p"))
    g = load_golden("sampler_tiny")
    eng, _ = make_sampler_engine(g, TruncationFakeOps(torch.float32))
    with pytest.raises(ValueError, match=name):
        eng.sample_codes_nar(2, **kw)
    with pytest.raises(ValueError, match=name):
        eng.sample_codes_ar(2, **kw)


def test_good_truncation_arguments():
    assert Engine.check_truncation(None, None, None) is None
    assert Engine.check_truncation(1, None, None) == (1, 1.0, NEG_INF)
    assert Engine.check_truncation(256, 1.0, 1.0) == (256, 1.0, 0.0)
    assert Engine.check_truncation(None, 0.9, None) == (Engine.TRUNC_MAX_CAND, 0.9, NEG_INF)
    assert Engine.check_truncation(None, None, 0.05) == (256, 1.0, math.log(0.05))
    assert Engine.TRUNC_MAX_CAND == FT.TRUNC_MAX_CAND


# ---------------------------------------------------------------------------------------------------------------- engine
def _names(ops):
    return [c[0] if isinstance(c, tuple) else c for c in ops.calls]


def _nar(eng, n_steps, **kw):
    masks, ids = [], []

    def hook(i):
        masks.append(int(eng.vmask.sum()))
        ids.append(eng.row_argmax.clone())
    cid, _, prob = eng.sample_codes_nar(n_steps, on_step=hook, **kw)
    return cid.clone(), prob.clone(), masks, ids


def test_engine_nar_truncated_reproducible_and_other_paths_unchanged():
    g = load_golden("sampler_tiny")
    T = int(g["n_steps"])
    eng, _ = make_sampler_engine(g, TruncationFakeOps(torch.float32))
    greedy = _nar(eng, T)
    assert "sample_rows_trunc" not in _names(eng.ops)
    calls_greedy = list(eng.ops.calls)
    eng.ops.calls.clear()
    _nar(eng, T, top_k=None, top_p=None, min_p=None)
    assert eng.ops.calls == calls_greedy                                    # none given: the greedy call list
    eng.ops.calls.clear()
    temp = _nar(eng, T, temperature=1.0, seed=7)
    assert "sample_rows_trunc" not in _names(eng.ops)                       # temperature alone: no truncation call
    eng.ops.calls.clear()
    a = _nar(eng, T, temperature=1.0, seed=7, top_k=5)
    assert _names(eng.ops).count("sample_rows_trunc") == T
    b = _nar(eng, T, temperature=1.0, seed=7, top_k=5)
    c = _nar(eng, T, temperature=1.0, seed=8, top_k=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[3][0], c[3][0])
    assert a[2] == greedy[2] == c[2]                                        # the greedy schedule's masks
    assert ((a[1] > 0) & (a[1] <= 1)).all() and bool(((eng.row_kept >= 1) & (eng.row_kept <= 5)).all())
    # top_k = 1 is the greedy sampler, whatever the seed; temperature None means T = 1
    one = _nar(eng, T, top_k=1, seed=3)
    assert torch.equal(one[0], greedy[0]) and torch.allclose(one[1], greedy[1], rtol=1e-5)
    eng.ops.calls.clear()
    d = _nar(eng, T, seed=7, top_k=5)
    assert torch.equal(d[0], a[0]) and [c for c in eng.ops.calls if c[0] == "sample_rows_trunc"][0][3:] == (5, 1.0, NEG_INF)
    # every keyword reaches the kernel as the C ABI takes it
    eng.ops.calls.clear()
    _nar(eng, 1, temperature=2.0, seed=1, top_p=0.9, min_p=0.05)
    assert [c for c in eng.ops.calls if c[0] == "sample_rows_trunc"][0][3:] == (256, 0.9, math.log(0.05))
    # where the untruncated draw is among the five best, the truncated step drew the same code (rule 6, through the engine)
    assert (a[3][0] == temp[3][0]).float().mean() > 0.2


@pytest.mark.parametrize("mode", ["confidence", "tlbr", "random"])
def test_engine_ar_truncated_policies_unmask_one_position_per_step(mode):
    g = load_golden("sampler_ar_tiny")
    eng, _ = make_sampler_engine(g, TruncationFakeOps(torch.float32))
    B, V = eng.B, eng.V
    outs = []
    for seed in (11, 11, 12):
        trace = []
        cid, _, _ = eng.sample_codes_ar(None, mode, positions=g["random_positions"].tolist()[-V:], trace=trace, temperature=2.0, seed=seed,
                                        top_k=5, top_p=0.95)
        assert [int(m.sum()) for m in trace] == [B * (V - i - 1) for i in range(V)], mode
        assert all(int(m.view(B, V).sum(1).max()) == V - i - 1 for i, m in enumerate(trace))
        outs.append(cid.clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    assert _names(eng.ops).count("sample_rows_trunc") == 3 * V


def test_truncated_call_takes_the_logits_path_where_the_fused_path_is_available():
    """bf16, B*V = 256: greedy and temperature-only loops end the codebook contraction in ROWMAX / ROWSAMPLE; a truncated loop issues
    neither and one sample_rows_trunc per step"""
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
    B, L, grid = 4, 8, 8
    ids = torch.from_numpy(g["in_input_ids"])[:1].expand(B, -1).clone()
    pos = torch.from_numpy(O.box_position(grid)).unsqueeze(0).expand(B, -1, -1)
    store = ParamStore(cfg, "cpu", torch.bfloat16, task="vis_mask")
    store.load_named(sd)
    eng = Engine(cfg, store, TruncationFakeOps(torch.bfloat16), B, L, grid * grid, need_lang=False)
    eng.sync_compute_weights()
    eng.set_inputs(ids, ids > 0, None, pos, cluster_ids=torch.zeros(B, grid * grid, dtype=torch.long),
                   vis_mask=torch.ones(B, grid * grid, dtype=torch.bool))
    assert eng.fused_predict_available()

    def epis():
        return [c[-1] for c in eng.ops.calls if c[0] == "gemm"]
    eng.sample_codes_nar(2)
    assert epis().count(EPI_ROWMAX) == 2
    eng.ops.calls.clear()
    eng.sample_codes_nar(2, temperature=1.0, seed=1)
    assert epis().count(EPI_ROWSAMPLE) == 2 and "sample_rows_trunc" not in _names(eng.ops)
    eng.ops.calls.clear()
    cid, _, prob = eng.sample_codes_nar(2, temperature=1.0, seed=1, top_k=50, top_p=0.9)
    assert EPI_ROWSAMPLE not in epis() and EPI_ROWMAX not in epis() and _names(eng.ops).count("sample_rows_trunc") == 2
    assert int(cid.max()) < cfg.num_clusters and bool(((eng.row_kept >= 1) & (eng.row_kept <= 50)).all())
    eng.ops.calls.clear()
    eng.sample_codes_ar(3, temperature=1.0, seed=1, min_p=0.1)
    assert EPI_ROWSAMPLE not in epis() and EPI_ROWMAX not in epis() and _names(eng.ops).count("sample_rows_trunc") == 3


def test_sampling_fake_ops_have_no_truncation_entry_point():
    """the keywords reach the library only through the new entry point"""
    assert not hasattr(SamplingFakeOps(torch.float32), "sample_rows_trunc")


# ---------------------------------------------------------------------------------------------------------------- honest / faults
def _fault_cases():
    """(logits, K, T, top_k, top_p, min_p) on which every injected fault shows"""
    gen = torch.Generator().manual_seed(6)
    M = 256
    gauss = torch.randn(M, 1024, generator=gen) * 4
    halves = (torch.randn(M, 1024, generator=gen) * 8).round() / 2                 # multiples of 0.5: ties across the boundary
    return [(gauss, 1000, 1.0, 50, 0.9, None), (gauss, 1000, 0.7, 256, 0.9, 0.05), (halves, 1000, 1.0, 50, 1.0, None),
            (torch.full((M, 512), 0.5), 500, 1.0, 20, 1.0, None)]


@pytest.mark.parametrize("fault", [None, "ties", "renorm", "all", "prob"])
def test_bounds_accept_the_restatement_and_reject_each_fault(fault):
    """the float32 restatement passes every check of bounds_truncation.py on every case; each injected fault fails on at least one"""
    failed = []
    for n, (logits, K, T, top_k, top_p, min_p) in enumerate(_fault_cases()):
        seed = FS.launch_seed(31, n)
        p, idx, lse, kept = _run(TruncationFakeOps(torch.float32, fault=fault), logits, K, T, seed, top_k, top_p, min_p)
        lmp = NEG_INF if min_p is None else math.log(min_p)
        try:
            res = BT.check_trunc(logits, K, 1.0 / T, seed, top_k, top_p, lmp, p, idx, lse, kept, f"case {n}")
            if top_p < 1:
                assert res["undecided"] <= 0.1 and res["b_max"] < 1e-4
        except AssertionError as err:
            assert fault is not None, err
            failed.append((n, str(err).split(";")[0]))
    print(fault, failed)
    assert (fault is None) == (not failed)
    expect = {"ties": "draw", "renorm": "kept counts", "all": "outside the kept set", "prob": "row_prob"}
    if fault is not None:
        assert any(expect[fault] in msg for _, msg in failed), failed


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_rejects_bad_arguments_before_any_launch_and_is_planable():
    """host-side checks of xl_sample_rows_trunc (XL_ERR_BAD_ARG with the values in the text), and its row in the plan table"""
    from xlxmert_amd._lib import XlError, get_lib
    lib = get_lib()

    def call(K=100, ldl=100, inv_T=1.0, top_k=50, top_p=0.9, lmp=-1.0, logits=16):
        lib.call("xl_sample_rows_trunc", logits, 4, K, ldl, inv_T, 1, top_k, top_p, lmp, None, None, None, None, None)
    for kw, text in ((dict(top_k=0), "top_k=0 "), (dict(top_k=257), "top_k=257 "), (dict(top_k=-3), "top_k=-3 "), (dict(top_p=0.0), "top_p=0 "),
                     (dict(top_p=-0.5), "top_p=-0.5 "), (dict(top_p=float("nan")), "top_p=nan "), (dict(lmp=0.5), "log_min_p=0.5 "),
                     (dict(lmp=float("nan")), "log_min_p=nan "), (dict(K=65537, ldl=65537), "K=65537 "), (dict(K=0), "K=0 "),
                     (dict(ldl=99), "ldl=99 "), (dict(inv_T=0.0), "inv_T=0"), (dict(inv_T=float("inf")), "inv_T=inf"), (dict(logits=None), "M=4 ")):
        with pytest.raises(XlError, match="xl_sample_rows_trunc.*" + text.replace("(", r"\(")):
            call(**kw)
    fid = lib._dll.xl_plan_fn_id(b"xl_sample_rows_trunc")
    assert fid >= 0 and lib._dll.xl_plan_fn_nargs(fid) == 14 == len(lib.protos["xl_sample_rows_trunc"][1])
