"""The Mask-Predict caption sampler without a GPU: the restatement of xl_caption_step (tests/fake_ops_caption.py) against an
independent plain-torch statement (tests/caption_oracle.py) with one injected fault at a time, the engine's loop over the restatement
against the oracle's loop, the properties of the public entry points, the C ABI's argument checks, and the sharpness of the
admissible-argmax rule at the inputs of the device test.  The kernel itself is held to the restatement in test_caption_gpu.py."""
import math

import pytest
import torch

import bounds as BD
import caption_oracle as CO
import lxmert_oracle as O
from _util import golden_cfg, load_golden
from fake_ops_caption import FAULTS, CaptionFakeOps, n_mask_of, score_bound
from xlxmert_amd.config import XLxmertConfig
from xlxmert_amd.engine import Engine
from xlxmert_amd.params import ParamStore

CFG_KEYS = ("vocab_size", "hidden_size", "num_attention_heads", "intermediate_size", "max_position_embeddings", "type_vocab_size",
            "l_layers", "x_layers", "r_layers", "visual_feat_dim", "visual_pos_dim", "num_clusters")
# the specials of the tiny fixture vocabulary (100 ids; its sentences are [98 ... 99 0 0]) and a [MASK] of our own
PAD, MASK, CLS, SEP = 0, 97, 98, 99
BANNED = (PAD, MASK, CLS, SEP)
PREFIX = (11, 12, 13)
B_, L_ = 5, 20


def lengths_for(P, L=L_):
    """ragged, with the extremes 1 and L - 2 - P"""
    return [1, L - 2 - P, 7, 4, 10]


def tiny_model(seed_shift=0):
    g = load_golden("lang_tasks_tiny")
    oc = golden_cfg(g)
    cfg = XLxmertConfig(**{k: getattr(oc, k) for k in CFG_KEYS})
    return cfg, oc, O.make_cls_state_dict(oc, int(g["seed"]) + seed_shift)


def picture(oc, sd, B, seed=5, codes=True):
    """(cluster_ids or None, features [B, V, F], positions [B, V, 4]) of a 4 x 4 grid"""
    gen = torch.Generator().manual_seed(seed)
    V = 16
    pos = torch.from_numpy(O.box_position(4)).unsqueeze(0).expand(B, -1, -1).float()
    if codes:
        cid = torch.randint(0, oc.num_clusters, (B, V), generator=gen)
        return cid, O.codebook_features(sd, cid, None), pos
    return None, torch.randn(B, V, oc.visual_feat_dim, generator=gen), pos


def make_caption_engine(ops, cfg, sd, lengths, prefix=(), cid=None, feats=None, pos=None, device="cpu", dtype=torch.float32,
                        pack_lang=None, L=L_, task="word_mask"):
    B = len(lengths)
    dev = torch.device(device)
    store = ParamStore(cfg, device, dtype, task=task)
    store.load_named(sd)
    eng = Engine(cfg, store, ops, B, L, pos.shape[1], need_lang=True, pack_lang=pack_lang)
    eng.sync_compute_weights()
    tok, free, att = CO.layout(lengths, L, prefix, CLS, SEP, MASK)
    eng.set_inputs(tok.to(dev), att.to(dev), None, pos.to(dev), cluster_ids=None if cid is None else cid.to(dev),
                   visual_feats=None if cid is not None else feats.to(dev))
    return eng


def run_loop(eng, lengths, T, P, **kw):
    trace = []

    def hook(i):
        trace.append(dict(tokens=eng.cap_tokens.clone(), fed_ids=eng.ids.clone(), word_mask=eng.word_mask.clone(),
                          conf=eng.cap_conf.clone(), score=eng.cap_score.clone()))
    tok, score, conf = eng.sample_words_nar(lengths, T, P, hook, mask_token_id=MASK, banned_ids=BANNED, **kw)
    return tok.clone(), score.clone(), conf.clone(), trace


# ---------------------------------------------------------------------------------------------------------------- restatement
def make_step_case(gen, B, L, P, T, step, packed, sup):
    """arguments of one caption_step on B captions with ragged lengths (1 and L - 2 - P among them when B allows): random predictions
    and masks, four equal confidences in some rows, a prediction equal to the last prefix id at the first free position, a run of three
    equal predictions"""
    lengths = torch.tensor([L - 2 - P, 1, 55 if L == 64 else 7, 4, 10][:B] if B > 1 else [L - 2 - P], dtype=torch.int32)
    real = lengths.long() + P + 2
    off = torch.cat([torch.zeros(1, dtype=torch.long), real.cumsum(0)]).to(torch.int32)
    n_rows = (int(off[-1]) + 255) // 256 * 256 if packed else B * L
    row_prob = torch.rand(n_rows, generator=gen) * 0.98 + 0.01
    row_id = torch.randint(1, 90, (n_rows,), generator=gen, dtype=torch.int32)
    tok, free, att = CO.layout(lengths, L, tuple(range(11, 11 + P)), CLS, SEP, MASK)
    wm = free & (torch.rand(B, L, generator=gen) < 0.6)
    tok = torch.where(free & ~wm, torch.randint(1, 90, (B, L), generator=gen), tok)
    row = (lambda b, l: int(off[b]) + l) if packed else (lambda b, l: b * L + l)
    for b in (0, 2, 4):                                         # ties: four free positions of a row share one confidence
        if b < B:
            for l in (P + 2, P + 3, P + 5, P + 6)[:max(1, min(4, int(lengths[b]) - 1))]:
                row_prob[row(b, l)] = 0.25
    if P:                                                       # a repeat across the prefix boundary: the first free token = the last prefix id
        wm[0, P + 1] = True
        row_id[row(0, P + 1)] = int(tok[0, P])
        row_prob[row(0, P + 1)] = 0.99
    b = min(4, B - 1)
    for l in (P + 3, P + 4, P + 5):                             # a run of three equal tokens
        wm[b, l] = True
        row_id[row(b, l)] = 55
        row_prob[row(b, l)] = 0.97
    return dict(row_prob=row_prob, row_id=row_id, lang_off=off if packed else None, lengths=lengths, tokens=tok,
                word_mask=wm.to(torch.uint8), B=B, L=L, P=P, step=step, n_steps=T, suppress=sup)


def step_cases():
    """[(name, arguments of one caption_step)] with ties, n_b = 1, n_mask = 0 rows, repeats (one across the prefix boundary, one
    triple), dense and packed rows, L = 64 with T = 11 and n_b = 55 where the float schedule differs, and the last step"""
    gen = torch.Generator().manual_seed(12)
    return [(name, make_step_case(gen, B_, L, P, T, step, packed, sup)) for name, P, T, step, packed, sup, L in (
        ("dense", 3, 4, 0, False, False, L_), ("packed", 3, 4, 1, True, False, L_), ("repeats", 3, 4, 1, False, True, L_),
        ("packed repeats", 0, 7, 2, True, True, L_), ("float schedule", 0, 11, 4, False, False, 64), ("last step", 3, 4, 3, True, True, L_))]


def dense_pred(c):
    """row_prob / row_id as [B, L] for the independent statement (packed: gathered through the offsets, by this test)"""
    B, L = c["B"], c["L"]
    pos = torch.arange(L)[None, :]
    rows = (c["lang_off"][:-1].long()[:, None] if c["lang_off"] is not None else torch.arange(B)[:, None] * L) + pos
    rows = rows.clamp(max=c["row_prob"].numel() - 1)
    return c["row_prob"][rows], c["row_id"][rows]


def run_step(ops, c):
    tok, wm = c["tokens"].clone(), c["word_mask"].clone()
    B, L = c["B"], c["L"]
    fed, conf, score = torch.full((B, L), -7, dtype=torch.int64), torch.full((B, L), -7.0), torch.full((B,), -7.0)
    ops.caption_step(c["row_prob"], c["row_id"], c["lang_off"], c["lengths"], tok, fed, wm, conf, score, B, L, c["P"], c["step"],
                     c["n_steps"], MASK, c["suppress"])
    return tok, fed, wm, conf, score


def check_step(c, got, what=""):
    """the outputs of one caption_step against the independent plain-torch statement: integers and conf exact, score in its bound"""
    tok, fed, wm, conf, score = got
    pp, pi = dense_pred(c)
    r_tok, r_fed, r_wm, r_conf, r_score = CO.caption_update(pp, pi, c["lengths"], c["tokens"], c["word_mask"], c["L"], c["P"], c["step"],
                                                            c["n_steps"], MASK, c["suppress"])
    if c["step"] + 1 == c["n_steps"]:
        r_wm = c["word_mask"].bool()                               # the last step leaves the mask as the forward read it
        r_fed = torch.where(torch.arange(c["L"])[None, :] < c["P"] + c["lengths"].long()[:, None] + 2,
                            torch.where(r_wm, torch.full_like(r_tok, MASK), r_tok), torch.zeros_like(r_tok))
    BD.check_exact(tok.cpu(), r_tok, f"{what} tokens")
    BD.check_exact(conf.cpu().view(torch.int32).long(), r_conf.view(torch.int32).long(), f"{what} conf")
    BD.check_exact(wm.cpu().long(), r_wm.long(), f"{what} word_mask")
    BD.check_exact(fed.cpu(), r_fed, f"{what} fed_ids")
    n = c["lengths"].long().clamp(0, c["L"] - 2 - c["P"])
    logs = torch.where(r_conf > 0, torch.log(pp.double()).abs(), torch.zeros(1, dtype=torch.float64)).sum(1)
    for b in range(c["B"]):
        bound = score_bound(int(n[b]), float(logs[b]))
        assert abs(float(score[b]) - float(r_score[b])) <= bound, f"{what} score[{b}] {float(score[b])} vs {float(r_score[b])} (bound {bound:.2e})"


def test_float_schedule_differs_from_the_integer_one_in_the_cases():
    """the reference's int(ratio * n) is one short of (n (T - i - 1)) // T where the float product lands below the integer: for
    n <= 62 and T <= 14 that happens at T = 11, n = 55 only (6/11 * 55 = 29.999...) -- the case the "float" fault is caught on"""
    diff = [(T, n, i) for T in range(1, 15) for n in range(1, 63) for i in range(T) if int((T - i - 1) / T * n) != n_mask_of(n, i, T)]
    assert diff == [(11, 55, 4), (11, 55, 7)], diff
    assert any(c["n_steps"] == 11 and c["step"] == 4 and 55 in c["lengths"].tolist() for _, c in step_cases())


@pytest.mark.parametrize("fault", [None] + list(FAULTS))
def test_independent_statement_accepts_the_restatement_and_rejects_each_fault(fault):
    failed = []
    for name, c in step_cases():
        try:
            check_step(c, run_step(CaptionFakeOps(torch.float32, fault=fault), c), name)
        except AssertionError as err:
            assert fault is not None, err
            failed.append((name, str(err)[:60]))
    print(fault, failed)
    assert (fault is None) == (not failed)


def test_suppress_repeats_remasks_a_planted_repeat_first():
    """three equal tokens with the HIGHEST confidences of their row: without the flag they stay, with it the second and third are the
    first to be re-masked (the first of the run has a different left neighbour)"""
    name, c = [x for x in step_cases() if x[0] == "repeats"][0]
    P = c["P"]
    on = run_step(CaptionFakeOps(torch.float32), c)
    off = run_step(CaptionFakeOps(torch.float32), dict(c, suppress=False))
    assert on[3][4, P + 4] == -1 and on[3][4, P + 5] == -1 and on[3][4, P + 3] > 0
    assert on[2][4, P + 4] == 1 and on[2][4, P + 5] == 1
    assert off[2][4, P + 4] == 0 and off[2][4, P + 5] == 0 and float(off[3][4, P + 4]) == pytest.approx(0.97)
    assert on[3][0, P + 1] == -1 and on[2][0, P + 1] == 1             # the repeat of the last prefix id
    assert torch.equal(on[0], off[0]) and torch.equal(on[4], off[4])   # tokens and score do not depend on the flag


# ---------------------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("P,T", [(0, 4), (0, 7), (3, 4), (3, 7)])
def test_engine_loop_matches_the_oracle_loop_step_by_step(P, T):
    """fp32 engine over the restatement against the loop composed from the oracle's modules: tokens, masks and fed ids identical after
    every step, confidences to fp32 rounding, score within score_bound of the float64 mean (<= 64 fp32 log terms)"""
    cfg, oc, sd = tiny_model()
    prefix = PREFIX[:P]
    lengths = lengths_for(P)
    cid, feats, pos = picture(oc, sd, B_)
    r_tok, r_score, r_conf, r_trace = CO.sample_words_nar(sd, oc, feats, pos, lengths, T, L_, prefix, BANNED, CLS, SEP, MASK)
    eng = make_caption_engine(CaptionFakeOps(torch.float32), cfg, sd, lengths, prefix, cid, feats, pos)
    tok, score, conf, trace = run_loop(eng, lengths, T, P)
    assert len(trace) == T
    for i, (a, r) in enumerate(zip(trace, r_trace)):
        assert torch.equal(a["tokens"], r["tokens"]), i
        assert torch.equal(a["word_mask"].bool(), r["word_mask"] if i + 1 < T else r_trace[i - 1]["word_mask"] if i else CO.layout(lengths, L_, prefix, CLS, SEP, MASK)[1]), i
        if i + 1 < T:
            assert torch.equal(a["fed_ids"], r["fed_ids"]), i
        assert torch.allclose(a["conf"], r["conf"], rtol=1e-4, atol=1e-7), i
        n = torch.tensor(lengths)
        logs = torch.log(r["conf"].double().clamp(min=1e-300)).abs().sum(1)
        for b in range(B_):
            # the engine's confidences are the fp32 forward's, the oracle's too: both within 1e-4 relative of each other per term
            assert abs(float(a["score"][b]) - float(r["score"][b])) <= score_bound(int(n[b]), float(logs[b])) + 1e-4, (i, b)
    assert torch.equal(tok, r_tok)
    free = CO.layout(lengths, L_, prefix, CLS, SEP, MASK)[1]
    assert not torch.isin(tok[free], torch.tensor(BANNED)).any()                # banned ids never appear
    assert torch.equal(tok[~free], CO.layout(lengths, L_, prefix, CLS, SEP, MASK)[0][~free])
    masks = [int(t["word_mask"].sum()) for t in trace[:-1]]
    assert masks == [sum(n_mask_of(n, i, T) for n in lengths) for i in range(T - 1)]


def test_packed_and_dense_engines_and_the_reused_visual_stack_agree():
    cfg, oc, sd = tiny_model()
    lengths = lengths_for(3)
    cid, feats, pos = picture(oc, sd, B_, codes=False)
    outs = {}
    for pack in (True, False):
        for reuse in (True, False):
            eng = make_caption_engine(CaptionFakeOps(torch.float32), cfg, sd, lengths, PREFIX, None, feats, pos, pack_lang=pack)
            assert eng.packed == pack
            eng.reuse_vis_stack = reuse
            outs[pack, reuse] = run_loop(eng, lengths, 4, 3)
            n_visn = sum(1 for c in eng.ops.calls if c[0] == "gemm" and c[1:4] == (eng.MV, eng.d, eng.F))
            assert n_visn == (1 if reuse else 4)                                   # the feature encoder ran in step 0 only
            assert [c for c in eng.ops.calls if c[0] == "caption_step"][0][-1] == pack
    for pack in (True, False):                                                     # bit-identical with and without the reuse
        assert torch.equal(outs[pack, True][0], outs[pack, False][0]) and torch.equal(outs[pack, True][2], outs[pack, False][2])
        assert torch.equal(outs[pack, True][1], outs[pack, False][1])
    assert torch.equal(outs[True, True][0], outs[False, True][0])                  # packed and dense: the same tokens
    assert torch.allclose(outs[True, True][2], outs[False, True][2], rtol=1e-4, atol=1e-7)


def test_sampling_arguments_reach_the_loop():
    cfg, oc, sd = tiny_model()
    lengths = lengths_for(0)
    cid, feats, pos = picture(oc, sd, B_)
    eng = make_caption_engine(CaptionFakeOps(torch.float32), cfg, sd, lengths, (), cid, feats, pos)
    greedy = run_loop(eng, lengths, 1, 0)
    for seed in (0, 1, 7, 2 ** 40 + 3):                                            # top_k = 1 at T = 1 is the greedy step, whatever the seed
        one = run_loop(eng, lengths, 1, 0, top_k=1, seed=seed)
        assert torch.equal(one[0], greedy[0]) and torch.allclose(one[2], greedy[2], rtol=1e-5)
    a = run_loop(eng, lengths, 4, 0, temperature=1.5, seed=11)
    b = run_loop(eng, lengths, 4, 0, temperature=1.5, seed=11)
    c = run_loop(eng, lengths, 4, 0, temperature=1.5, seed=12)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not torch.equal(a[0], c[0])
    free = CO.layout(lengths, L_, (), CLS, SEP, MASK)[1]
    for out in (a, c, run_loop(eng, lengths, 4, 0, temperature=2.0, seed=3, top_k=20, top_p=0.95, min_p=0.01)):
        assert not torch.isin(out[0][free], torch.tensor(BANNED)).any()
        assert bool(((out[2][free] > 0) & (out[2][free] <= 1)).all())
    assert [x[0] for x in eng.ops.calls].count("sample_rows_trunc") == 4 + 4    # the four top_k = 1 steps and the truncated loop
    eng.ops.calls.clear()
    run_loop(eng, lengths, 2, 0, suppress_repeats=True)
    assert all(c[7] for c in eng.ops.calls if c[0] == "caption_step")


def test_bf16_engine_takes_the_fused_predict_and_truncation_the_logits():
    """bf16 and a row count that is a multiple of 256 (packed rows are rounded up to it): greedy / temperature end the decoder
    contraction in ROWMAX / ROWSAMPLE, a truncated loop issues neither; fp32 never does"""
    cfg, oc, sd = tiny_model()
    lengths = lengths_for(0)
    cid, feats, pos = picture(oc, sd, B_)
    eng = make_caption_engine(CaptionFakeOps(torch.bfloat16), cfg, sd, lengths, (), cid, feats, pos, dtype=torch.bfloat16)
    assert eng.packed and eng.ML == 256

    def epis():
        return [c[-1] for c in eng.ops.calls if c[0] == "gemm"]
    g = run_loop(eng, lengths, 2, 0)
    assert epis().count(5) == 2
    eng.ops.calls.clear()
    run_loop(eng, lengths, 2, 0, temperature=1.0, seed=1)
    assert epis().count(9) == 2
    eng.ops.calls.clear()
    t = run_loop(eng, lengths, 2, 0, top_k=1)
    assert 5 not in epis() and 9 not in epis() and [c[0] for c in eng.ops.calls].count("sample_rows_trunc") == 2
    free = CO.layout(lengths, L_, (), CLS, SEP, MASK)[1]
    assert not torch.isin(g[0][free], torch.tensor(BANNED)).any() and int(g[0].max()) < cfg.vocab_size
    assert (t[0] == g[0]).float().mean() > 0.9                                     # fused and logits path: the same greedy tokens (bf16 ties aside)


@pytest.mark.parametrize("kw,err", [(dict(lengths=[0, 1, 1, 1, 1]), "lengths"), (dict(lengths=[1, 1, 1, 1, 19]), "lengths"), (dict(lengths=[1, 1]), "lengths"),
                                    (dict(lengths=2.5), "lengths"), (dict(lengths=True), "lengths"), (dict(P=-1), "prefix_len"), (dict(P=18), "prefix_len"),
                                    (dict(T=0), "n_steps"), (dict(temperature=0.0), "temperature"), (dict(top_k=0), "top_k")])
def test_bad_arguments_raise(kw, err):
    cfg, oc, sd = tiny_model()
    cid, feats, pos = picture(oc, sd, B_)
    eng = make_caption_engine(CaptionFakeOps(torch.float32), cfg, sd, lengths_for(0), (), cid, feats, pos)
    kw = dict(kw)
    lengths, P, T = kw.pop("lengths", 3), kw.pop("P", 0), kw.pop("T", 2)
    with pytest.raises(ValueError, match=err):
        eng.sample_words_nar(lengths, T, P, mask_token_id=MASK, banned_ids=BANNED, **kw)


def test_long_text_and_stores_without_the_mlm_head_are_refused():
    cfg, oc, sd = tiny_model()
    cid, feats, pos = picture(oc, sd, 2)
    for task in ("matched", "vqa"):
        store = ParamStore(cfg, "cpu", torch.float32, task=task, **({"num_answers": 8} if task == "vqa" else {}))
        eng = Engine(cfg, store, CaptionFakeOps(torch.float32), 2, L_, 16, need_lang=True)
        with pytest.raises(RuntimeError, match="MLM head"):
            eng.sample_words_nar(3, 2)
    store = ParamStore(cfg, "cpu", torch.float32, task="word_mask")
    eng = Engine(XLxmertConfig(**{**{k: getattr(oc, k) for k in CFG_KEYS}, "max_position_embeddings": 128}), store, CaptionFakeOps(torch.float32),
                 2, 65, 16, need_lang=True)
    with pytest.raises(ValueError, match="text length 65"):
        eng.sample_words_nar(3, 2)
    eng = Engine(cfg, store, CaptionFakeOps(torch.float32), 2, L_, 16, need_lang=True)
    with pytest.raises(ValueError, match="banned_ids"):
        eng.sample_words_nar(3, 2, banned_ids=[100])


# ---------------------------------------------------------------------------------------------------------------- nn.Module
class _StubEngine:
    """stands in for the engine under XLxmertForPretraining.sample_caption_ids: records set_inputs, returns a fixed score per row"""

    def __init__(self, scores):
        self.scores = scores

    def set_inputs(self, ids, att, tt, pos, **kw):
        self.ids, self.att, self.kw = ids.clone(), att.clone(), kw

    def sample_words_nar(self, lengths, n_steps, P, on_step, **kw):
        self.lengths, self.P, self.loop_kw = lengths.clone(), P, kw
        self.cap_tokens = self.ids
        if on_step is not None:
            for i in range(n_steps):
                on_step(i)
        return self.ids, self.scores, torch.zeros(self.ids.shape)


def _stub_model(eng, mlm=True, vis_emb=True):
    from xlxmert_amd.modeling import XLxmertForPretraining
    m = XLxmertForPretraining.__new__(XLxmertForPretraining)
    torch.nn.Module.__init__(m)
    m.task_mask_lm, m.vis_emb = mlm, (object() if vis_emb else None)
    m.config = XLxmertConfig(vocab_size=100)
    m._step_engine = lambda B, L, V: eng
    return m


def test_candidate_lengths_return_the_best_scoring_row_per_image():
    B, C, L = 3, 4, 12
    scores = torch.tensor([-1.0, -0.5, -2.0, -0.7, -3.0, -2.5, -2.6, -2.4, -0.1, -0.9, -0.8, -0.05])
    eng = _StubEngine(scores)
    m = _stub_model(eng)
    cids = torch.arange(B * 16).view(B, 16) % 50
    tok, score, chosen, steps = m.sample_caption_ids(cluster_ids=cids, lengths=[2, 4, 5, 7], prefix_ids=[11, 12], n_steps=3, max_text_length=L,
                                                     return_intermediate=True, mask_token_id=MASK, cls_token_id=CLS, sep_token_id=SEP,
                                                     banned_ids=BANNED)
    best = scores.view(B, C).argmax(1)
    assert best.tolist() == [1, 3, 3]
    assert torch.equal(score, scores.view(B, C).max(1).values) and chosen.tolist() == [4, 7, 7]
    assert eng.ids.shape == (B * C, L) and eng.lengths.tolist() == [2, 4, 5, 7] * B and eng.P == 2 and len(steps) == 3
    assert torch.equal(eng.kw["cluster_ids"], cids.repeat_interleave(C, 0)) and eng.kw["visual_feats"] is None
    for b in range(B):
        n = int(chosen[b])
        assert tok[b].tolist() == [CLS, 11, 12] + [MASK] * n + [SEP] + [PAD] * (L - n - 4)
    assert eng.att.sum(1).tolist() == [n + 4 for n in [2, 4, 5, 7]] * B
    assert eng.kw["lang_off"].tolist() == [0] + torch.tensor([n + 4 for n in [2, 4, 5, 7]] * B).cumsum(0).tolist()
    assert eng.loop_kw["mask_token_id"] == MASK and "temperature" not in eng.loop_kw
    # one length for all, and one per row
    tok, score = m.sample_caption_ids(cluster_ids=cids, lengths=torch.tensor([1, 3, 9]), max_text_length=L, mask_token_id=MASK,
                                      cls_token_id=CLS, sep_token_id=SEP, banned_ids=BANNED)[:2]
    assert eng.ids.shape == (B, L) and eng.att.sum(1).tolist() == [3, 5, 11]
    m.sample_caption_ids(torch.zeros(B, 16, 32), lengths=5, max_text_length=L, temperature=0.8, seed=4, top_k=5)
    assert eng.kw["cluster_ids"] is None and eng.lengths.tolist() == [5] * B and eng.loop_kw["seed"] == 4 and eng.loop_kw["top_k"] == 5
    assert eng.loop_kw["banned_ids"].tolist() == list(range(100))                  # default: every id below 999 (here: the whole tiny vocabulary)


def test_module_argument_checks():
    eng = _StubEngine(torch.zeros(2))
    cids = torch.zeros(2, 16, dtype=torch.long)
    with pytest.raises(RuntimeError, match="task_mask_lm"):
        _stub_model(eng, mlm=False).sample_caption_ids(cluster_ids=cids, lengths=3)
    with pytest.raises(RuntimeError, match="codebook"):
        _stub_model(eng, vis_emb=False).sample_caption_ids(cluster_ids=cids, lengths=3)
    m = _stub_model(eng)
    for kw in (dict(lengths=0), dict(lengths=19), dict(lengths=[3, 19]), dict(lengths=torch.tensor([1, 2, 3])), dict(lengths=3, max_text_length=65),
               dict(lengths=3, prefix_ids=list(range(18)))):
        with pytest.raises(ValueError, match="lengths|max_text_length"):
            m.sample_caption_ids(cluster_ids=cids, **kw)
    with pytest.raises(ValueError, match="either"):
        m.sample_caption_ids(lengths=3)
    with pytest.raises(ValueError, match="square"):
        m.sample_caption_ids(cluster_ids=torch.zeros(2, 15, dtype=torch.long), lengths=3)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_rejects_bad_arguments_before_any_launch_and_is_planable():
    from xlxmert_amd._lib import XlError, get_lib, parse_header
    lib = get_lib()

    def call(B=5, L=20, P=3, step=0, T=4, null=None, mask_id=103):
        ptr = [16] * 9
        ptr[2] = None                                               # lang_off may be NULL
        if null is not None:
            ptr[null] = None
        lib.call("xl_caption_step", *ptr, B, L, P, step, T, mask_id, 0, None)
    for kw, text in ((dict(L=65), "L=65 "), (dict(P=-1), "P=-1 "), (dict(P=18), "P=18 "), (dict(step=4), "step=4 "), (dict(step=-1), "step=-1 "),
                     (dict(T=0), "n_steps=0"), (dict(B=0), "B=0 "), (dict(mask_id=-1), "mask_token_id=-1")):
        with pytest.raises(XlError, match=r"xl_caption_step.*\(-5\).*" + text.replace("(", r"\(")):
            call(**kw)
    for null in (0, 1, 3, 4, 5, 6, 7, 8):
        with pytest.raises(XlError, match=r"xl_caption_step.*\(-5\).*null argument"):
            call(null=null)
    fid = lib._dll.xl_plan_fn_id(b"xl_caption_step")
    assert fid >= 0 and lib._dll.xl_plan_fn_nargs(fid) == 17 == len(lib.protos["xl_caption_step"][1])
    assert "xl_caption_step" in parse_header(experimental=False) and hasattr(lib._dll, "xl_caption_step")


# ---------------------------------------------------------------------------------------------------------------- sharpness
SHARP_CFG = dict(vocab_size=1000, hidden_size=128, num_attention_heads=2, intermediate_size=256, max_position_embeddings=32,
                 visual_feat_dim=64, num_clusters=96, l_layers=2, x_layers=2, r_layers=2)
SHARP_B, SHARP_SEED = 12, 41                # 12 captions of L = 20: 240 dense rows, packed rows rounded up to 256 = the fused path
SHARP_BANNED = tuple(range(0, 20))
SHARP_MASK, SHARP_CLS, SHARP_SEP = 3, 1, 2
DEVICE_CAPS = (0.05, 2)       # sharpness caps of the device loop test, from the measurement below (see its docstring)


def sharp_lengths(P=0):
    return [1, L_ - 2 - P, 7, 4, 10, 3, 12, 9, 5, 15, 2, 8]


def sharp_model():
    oc = O.OracleConfig(**SHARP_CFG)
    return XLxmertConfig(**SHARP_CFG), oc, O.make_cls_state_dict(oc, SHARP_SEED)


def head_operands_bf16(sd, oc, lang):
    """(A, W, b) of the decoder contraction as the bf16 kernel reads them, in float64: LN(gelu(dense(lang))) rounded to bf16, the tied
    word embeddings rounded to bf16, the fp32 bias"""
    h = O._layer_norm(sd, "cls.predictions.transform.LayerNorm",
                      torch.nn.functional.gelu(O._linear(sd, "cls.predictions.transform.dense", lang)), 1e-12)
    return (h.to(torch.bfloat16).double(), sd["bert.embeddings.word_embeddings.weight"].to(torch.bfloat16).double(),
            sd["cls.predictions.bias"].double())


def test_admissible_argmax_rule_is_sharp_on_the_oracle_caption_step():
    """The admissible-argmax rule accepts every column within 2 SLACK E of the float64 maximum; it says nothing if many columns are.
    Measured here from the oracle alone (float64 forward of the device loop test's model and inputs -- SHARP_CFG, make_cls_state_dict(oc,
    41), 12 captions, all free positions masked = step 0 -- head operands rounded to bf16 as the kernel reads them, banned columns
    excluded): 0 of the 94 free rows (0.0 %) have more than one admissible column, at most 1 in a row (logit std 0.23, worst E
    1.8e-05, median top-1/top-2 gap 807 x the acceptance width).  Caps for the device test, which sees other steps' inputs too
    (DEVICE_CAPS): at most 5 % of the free rows -- 4 of 94, where none was measured -- with more than one admissible column, never
    more than 2 in a row (twice the measured 1).  The image sampler's caps (15 %, 4: measured 5.1 %, 2) would be slack here."""
    cfg, oc, sd64 = sharp_model()
    sd64 = {k: v.double() for k, v in sd64.items()}
    lengths = sharp_lengths()
    cid, feats, pos = picture(oc, sd64, SHARP_B)
    tok, free, att = CO.layout(lengths, L_, (), SHARP_CLS, SHARP_SEP, SHARP_MASK)
    with torch.no_grad():
        lang, _, _ = O.lxmert_model(sd64, oc, tok, feats.double(), pos.double(), att.long())
        A, W, b = head_operands_bf16(sd64, oc, lang[free])
    pre = A @ W.t() + b
    pre[:, list(SHARP_BANNED)] = -1e30
    e = BD.rowmax_logit_error(pre, A.abs() @ W.abs().t(), b.abs()[None, :], A.shape[1])
    live = torch.ones(pre.shape[1], dtype=torch.bool)
    live[list(SHARP_BANNED)] = False
    E = e[:, live].amax(-1)
    _, n_adm = BD.argmax_admissible(pre, pre.argmax(-1), E)
    share, most = BD.sharpness(n_adm)
    top2 = pre.topk(2, -1).values
    print(f"\ncaption sharpness: {int((n_adm > 1).sum())} of {n_adm.numel()} rows ({100 * share:.1f} %) with more than one admissible column, "
          f"at most {most} in a row; logit std {float(pre[:, live].std()):.2f}, worst E {float(E.max()):.2g}, median top-1/top-2 gap "
          f"{float(((top2[:, 0] - top2[:, 1]) / (2 * BD.SLACK * E)).median()):.1f} x the acceptance width")
    assert share == 0.0 and most == 1, (share, most)                                 # the measurement the caps are chosen from
    assert DEVICE_CAPS == (0.05, 2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_device_loop_checks_pass_over_the_host_restatement(dtype):
    """the device loop tests' own checks (test_caption_gpu._check_loop: admissible predictions on the head's own inputs, the six rules
    on the device's own predictions, the oracle where it is decisive), driven here by the host restatement at the same geometries"""
    import test_caption_gpu as G
    T, snaps = 4, []
    if dtype == torch.float32:
        cfg, oc, sd = tiny_model()
        lengths = lengths_for(3)
        cid, feats, pos = picture(oc, sd, B_)
        eng = make_caption_engine(CaptionFakeOps(dtype), cfg, sd, lengths, PREFIX, cid, feats, pos)
        eng.sample_words_nar(lengths, T, 3, G._grab(eng, snaps), mask_token_id=MASK, banned_ids=BANNED)
        G._check_loop(eng, snaps, sd, oc, feats, pos, lengths, PREFIX, T, BANNED, (CLS, SEP, MASK), 2.0 ** -12, (0.0, 1))
    else:
        eng, oc, sd, feats, pos, lengths = G._sharp_engine(dtype, CaptionFakeOps(dtype), "cpu")
        eng.sample_words_nar(lengths, T, 0, G._grab(eng, snaps), mask_token_id=SHARP_MASK, banned_ids=SHARP_BANNED)
        assert all(s["fused"] for s in snaps) and eng.ML == 256
        G._check_loop(eng, snaps, sd, oc, feats, pos, lengths, (), T, SHARP_BANNED, (SHARP_CLS, SHARP_SEP, SHARP_MASK), G.BF16_MARGIN, DEVICE_CAPS)


assert math.isfinite(score_bound(1, 0.0))
