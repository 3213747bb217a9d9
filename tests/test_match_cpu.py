"""Caption-image matching on the host: match.MatchRunner over the restatement of the two new kernels (tests/fake_ops_match.MatchFakeOps)
against the oracle's matched forward on the explicitly materialised pairs, the restatement itself against the expected outputs of
tests/match_cases.py, and the injected faults that those checks must reject."""
import pytest
import torch

import match_cases as MC
from fake_ops_match import FAULTS, MatchFakeOps
from xlxmert_amd.match import MatchRunner
from xlxmert_amd.params import ParamStore

TOL = 1e-4          # the project's fp32 activation tolerance
N, M, LENS = 3, 2, (1, 8, 5)


def make_runner(ops, chunk_pairs, pack_lang=True, row_pad=4, task="matched", N=N, M=M, lens=LENS, **kw):
    cfg, oc, sd, inp = MC.tiny_case(N, M, lens)
    store = ParamStore(cfg, "cpu", torch.float32, task=task)
    store.load_named(sd)
    r = MatchRunner(cfg, store, ops, N, M, inp["input_ids"].shape[1], inp["cluster_ids"].shape[1], chunk_pairs=chunk_pairs,
                    pack_lang=pack_lang, **kw)
    for e in (r.lang_eng, r.vis_eng, r.chunk_eng):
        e.ROW_PAD = row_pad             # (tails of a few rows instead of the GEMM row tile: the pad rules at tiny sizes)
    r.sync_compute_weights()
    return r, inp


def run(r, inp, **kw):
    return r.run(inp["input_ids"], inp["attention_mask"], inp["token_type_ids"], cluster_ids=inp["cluster_ids"],
                 visual_pos=inp["visual_pos"], **kw)


def check_scores(ops, chunk_pairs, pack_lang=True):
    r, inp = make_runner(ops, chunk_pairs, pack_lang)
    out = run(r, inp)
    ref = MC.oracle_margin(N, M, LENS)
    err = (out["margin"].double() - ref).abs().max().item()
    assert err < TOL, (chunk_pairs, pack_lang, err, out["margin"].tolist(), ref.tolist())
    p = torch.sigmoid(ref)
    assert (out["prob"].double() - p).abs().max().item() < TOL
    return out


@pytest.mark.parametrize("pack_lang", [True, False])
@pytest.mark.parametrize("chunk_pairs", [None, 1, 4, 6])
def test_margin_matches_oracle_on_materialised_pairs(chunk_pairs, pack_lang):
    """N = 3 captions (lengths 1, L and 5) x M = 2 images: margin of the shared-stack path against the oracle's matched forward on the
    six explicit pairs, for chunks that divide the pairs, that do not, and a single chunk; packed and dense language rows"""
    ops = MatchFakeOps(torch.float32)
    check_scores(ops, chunk_pairs, pack_lang)
    B_c = 6 if chunk_pairs is None else chunk_pairs
    exp = [c for c in ops.calls if c[0] == "pair_expand"]
    assert len(exp) == (6 + B_c - 1) // B_c and all(c[5] == B_c for c in exp)
    assert _visn_fc(ops) == 1           # the feature encoder (the one contraction over F) ran once, however many chunks


def _visn_fc(ops):
    return sum(1 for c in ops.calls if c[0] == "gemm" and c[3] == 32 and c[2] == 64)


def _gemms(ops):
    return sum(1 for c in ops.calls if c[0] == "gemm")


def test_stacks_run_once_whatever_the_chunking():
    """contractions of six chunks minus those of one chunk = five times a chunk's; what is left is the two stacks, once: four per
    language layer and per visual layer, and the feature encoder's"""
    g = {}
    for cp in (1, 6):
        ops = MatchFakeOps(torch.float32)
        check_scores(ops, cp)
        g[cp] = _gemms(ops)
    per_chunk, rest = divmod(g[1] - g[6], 5)
    assert rest == 0 and g[6] - per_chunk == 4 * 2 + 4 * 2 + 1, g


def test_chunkings_agree():
    """(the host's matrix products block differently with the row count, so not bit for bit here: the device test holds that)"""
    outs = [check_scores(MatchFakeOps(torch.float32), cp)["margin"].clone() for cp in (1, 4, 6)]
    assert (outs[0] - outs[1]).abs().max().item() < 1e-6 and (outs[0] - outs[2]).abs().max().item() < 1e-6


def test_square_case_shares_one_stack_engine():
    """N == M: one engine runs both stacks; the scores still match the oracle"""
    lens = (1, 8, 5)
    r, inp = make_runner(MatchFakeOps(torch.float32), 4, N=3, M=3, lens=lens)
    assert r.lang_eng is r.vis_eng
    out = run(r, inp, top_k=2, image_of_caption=torch.arange(3), caption_of_image=torch.arange(3))
    ref = MC.oracle_margin(3, 3, lens)
    assert (out["margin"].double() - ref).abs().max().item() < TOL
    exp = MC.expected_ranking(out["margin"], 2, torch.arange(3), torch.arange(3))
    for key in ("topk_images", "topk_captions", "rank_t2i", "rank_i2t"):
        assert torch.equal(out[key], exp[key]), key
    hits = out["recall_hits"]
    for i, key in enumerate(("rank_t2i", "rank_i2t")):
        want = [int((exp[key] < kk).sum()) for kk in (1, 5, 10)] + [3]
        assert hits[i].tolist() == [float(x) for x in want]


def test_dropout_engines_and_state_untouched():
    """engines built with dropout give the scores of dropout-free ones; the store's gradients and parameters keep their bits"""
    r, inp = make_runner(MatchFakeOps(torch.float32), 4, train_dropout=True)
    assert r.chunk_eng.p_hid > 0
    st = r.store
    st.grad.normal_()
    before = [st.grad.clone(), st.master.clone()]
    seeds = [(e._seed, int(e.seed_dev.item())) for e in (r.lang_eng, r.vis_eng, r.chunk_eng)]
    out = run(r, inp)
    assert (out["margin"].double() - MC.oracle_margin(N, M, LENS)).abs().max().item() < TOL
    assert r.chunk_eng.p_hid > 0 and r.lang_eng.p_attn > 0                  # restored
    assert MC.same_bits(st.grad, before[0]) and MC.same_bits(st.master, before[1])
    assert seeds == [(e._seed, int(e.seed_dev.item())) for e in (r.lang_eng, r.vis_eng, r.chunk_eng)]
    assert not getattr(r.chunk_eng, "_x0_given", False)


def test_missing_head_and_bad_arguments():
    cfg, oc, sd, inp = MC.tiny_case()
    store = ParamStore(cfg, "cpu", torch.float32, task="vis_mask")
    with pytest.raises(AssertionError, match="matched head"):
        MatchRunner(cfg, store, MatchFakeOps(torch.float32), N, M, 8, 16)
    r, inp = make_runner(MatchFakeOps(torch.float32), 4)
    with pytest.raises(ValueError, match="top_k"):
        run(r, inp, top_k=3)                                                # > min(N, M)
    holes = inp["attention_mask"].clone()
    holes[1, 2] = False
    with pytest.raises(ValueError, match="prefix"):
        r.run(inp["input_ids"], holes, inp["token_type_ids"], cluster_ids=inp["cluster_ids"], visual_pos=inp["visual_pos"])
    with pytest.raises(ValueError, match="chunk_pairs"):
        make_runner(MatchFakeOps(torch.float32), 7)


def test_encoder_forward_without_the_flag_is_unchanged():
    """without _x0_given the engine issues exactly the calls it issued before: both stacks run, and the two reuse flags together
    are still refused"""
    r, inp = make_runner(MatchFakeOps(torch.float32), 6)
    e = r.chunk_eng
    big = MC.materialised(inp, N, M)
    e.set_inputs(big["input_ids"], big["attention_mask"], big["token_type_ids"], big["visual_pos"], cluster_ids=big["cluster_ids"])
    e.ops.calls.clear()
    e.encoder_forward(want_pooled=True)
    n_full = _gemms(e.ops)
    assert _visn_fc(e.ops) == 1 and n_full > 17
    rel = e.lang_heads.rel_fwd(e.pooled)
    mg = (rel[:, 1] - rel[:, 0]).view(N, M)
    assert (mg.double() - MC.oracle_margin(N, M, LENS)).abs().max().item() < TOL
    e.ops.calls.clear()
    e._x0_given = True
    e.encoder_forward(want_pooled=True)
    e._x0_given = False
    assert _gemms(e.ops) == n_full - 17 and _visn_fc(e.ops) == 0             # the flag: neither stack
    e._reuse_lang_stack = e._reuse_vis_stack = True
    with pytest.raises(AssertionError):
        e.encoder_forward(want_pooled=True)


# ---------------------------------------------------------------------------------------------- the restatement and its faults
EXPAND = dict(N=3, M=2, V=4, L=5, d=8, lens=(1, 5, 3))


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("B_c", [1, 4, 6])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_restated_expand_matches_index_select(dtype, B_c, packed):
    MC.check_expand(MatchFakeOps(dtype), "cpu", dtype, B_c=B_c, packed=packed, **EXPAND)
    MC.check_expand(MatchFakeOps(dtype), "cpu", torch.float32, B_c=B_c, packed=packed, two=True, **EXPAND)


@pytest.mark.parametrize("shape", [(5, 3, 1, 4), (5, 3, 3, 4), (5, 3, 3, 15), (1, 70, 1, 64), (1, 70, 32, 70), (70, 1, 32, 9)])
def test_restated_ranking_matches_stable_sort(shape):
    Nq, Mq, k, B_c = shape
    MC.check_rank(MatchFakeOps(torch.float32), "cpu", Nq, Mq, k, B_c)


def _rejected(fault):
    """the first check that refuses the fault"""
    ops = lambda: MatchFakeOps(torch.float32, fault=fault)                  # noqa: E731
    checks = [lambda: check_scores(ops(), 4), lambda: check_scores(ops(), 6),
              lambda: MC.check_expand(ops(), "cpu", torch.float32, B_c=4, packed=True, **EXPAND),
              lambda: MC.check_rank(ops(), "cpu", 5, 3, 3, 4)]
    for i, c in enumerate(checks):
        try:
            c()
        except (AssertionError, RuntimeError, IndexError):       # (a wrong index may also leave the restatement's buffers)
            return i
    return None


@pytest.mark.parametrize("fault", FAULTS)
def test_injected_fault_is_rejected(fault):
    assert _rejected(None) is None
    assert _rejected(fault) is not None, f"fault {fault!r} passed every check"
