"""The Mask-Predict caption sampler on the device: xl_caption_step against its restatement, the vocabulary shape (N = 30720, K = 768)
through the existing fused predict, the engine loop teacher-forced against the oracle, and the nn.Module entry point."""
import pytest
import torch

import bounds as Bd
import bounds_sampling as BS
import caption_oracle as CO
import fake_ops_sampling as FS
import test_caption_cpu as TC
from fake_ops_caption import CaptionFakeOps, n_mask_of, score_bound
from test_caption_cpu import BANNED, CLS, MASK, SEP

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64            # guard words on either side of every buffer of the caption step
BF16_MARGIN = 2.0 ** -6


def _ops(dtype=torch.float32):
    from xlxmert_amd.ops import HipOps
    return HipOps(dtype)


def _guard(t, fill):
    """(whole, view): a device copy of t with GUARD elements of `fill` on either side"""
    whole = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype, device=DEV)
    whole[GUARD:GUARD + t.numel()] = t.reshape(-1).to(DEV)
    return whole, whole[GUARD:GUARD + t.numel()].view(t.shape)


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
# (step, n_steps): with the lengths of make_step_case (1, 4, 7, 10, L - 2 - P, 55) n_mask = (n (T - step - 1)) // T takes the values
# n - 1 (step 0 of T = 64: n 63 // 64), 0 and 1 (step 8 of T = 10: n // 10), the mid-range ones (step 1 of T = 4), and the last step
# leaves the mask alone.  n_mask = n itself only exists in the host-written state before step 0.
STEPS = ((0, 64), (8, 10), (1, 4), (4, 11), (3, 4))


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("P", [0, 3])
@pytest.mark.parametrize("B,L", [(5, 20), (1, 20), (5, 64), (1, 64)])
def test_caption_step_equals_the_restatement(B, L, P, packed):
    ops, ref = _ops(), CaptionFakeOps(torch.float32, compute=torch.float64)
    gen = torch.Generator().manual_seed(100 * B + L + P)
    seen = set()
    for step, T in STEPS:
        for sup in (False, True):
            c = TC.make_step_case(gen, B, L, P, T, step, packed, sup)
            seen |= {(n_mask_of(int(n), step, T), int(n)) for n in c["lengths"]} if step + 1 < T else set()
            want = TC.run_step(ref, c)
            TC.check_step(c, want, "restatement")                  # (the restatement itself against the independent statement)
            bufs = {"row_prob": (c["row_prob"], 7.0), "row_id": (c["row_id"], -7), "lengths": (c["lengths"], 9),
                    "tokens": (c["tokens"], -7), "fed_ids": (torch.full((B, L), -7, dtype=torch.int64), -7),
                    "word_mask": (c["word_mask"], 7), "conf": (torch.full((B, L), -7.0), -7.0), "score": (torch.full((B,), -7.0), -7.0)}
            if packed:
                bufs["lang_off"] = (c["lang_off"], 9)
            dev = {k: _guard(t, fill) for k, (t, fill) in bufs.items()}
            before = {k: w.clone() for k, (w, _) in dev.items()}
            v = {k: x for k, (_, x) in dev.items()}
            ops.caption_step(v["row_prob"], v["row_id"], v.get("lang_off"), v["lengths"], v["tokens"], v["fed_ids"], v["word_mask"], v["conf"],
                             v["score"], B, L, P, step, T, MASK, sup)
            torch.cuda.synchronize()
            for k, (w, x) in dev.items():                              # guards untouched, inputs unchanged
                n = x.numel()
                assert torch.equal(w[:GUARD], before[k][:GUARD]) and torch.equal(w[GUARD + n:], before[k][GUARD + n:]), k
                if k in ("row_prob", "row_id", "lengths", "lang_off"):
                    assert torch.equal(w, before[k]), k
            what = f"B={B} L={L} P={P} packed={packed} step {step}/{T} suppress={sup}"
            Bd.check_exact(v["tokens"].cpu(), want[0], what + " tokens")
            Bd.check_exact(v["fed_ids"].cpu(), want[1], what + " fed_ids")
            Bd.check_exact(v["word_mask"].cpu().long(), want[2].long(), what + " word_mask")
            Bd.check_exact(v["conf"].cpu().view(torch.int32).long(), want[3].view(torch.int32).long(), what + " conf")
            n = c["lengths"].long()
            logs = torch.log(want[3].double().clamp(min=1e-300)).abs()
            for b in range(B):
                free = slice(P + 1, P + 1 + int(n[b]))
                pp = c["row_prob"][(int(c["lang_off"][b]) if packed else b * L) + P + 1:][:int(n[b])]
                bound = score_bound(int(n[b]), float(torch.log(pp.double()).abs().sum()))
                ref_score = float(torch.log(pp.double()).sum() / int(n[b]))
                assert abs(float(v["score"][b]) - ref_score) <= bound, (what, b, float(v["score"][b]), ref_score, bound)
                assert logs[b, free].numel() == int(n[b])
            TC.check_step(c, tuple(t.cpu() for t in (v["tokens"], v["fed_ids"], v["word_mask"], v["conf"], v["score"])), what)
    if B > 1:
        kinds = {"0" if k == 0 else "1" if k == 1 else "n-1" if k == n - 1 else "mid" for k, n in seen}
        assert {"0", "1", "n-1", "mid"} <= kinds, sorted(seen)


def test_caption_step_bad_arguments_do_not_launch():
    """XL_ERR_BAD_ARG before any launch: the buffers come back untouched"""
    from xlxmert_amd._lib import XlError
    ops = _ops()
    gen = torch.Generator().manual_seed(5)
    c = TC.make_step_case(gen, 5, 20, 3, 4, 1, False, False)
    v = {k: c[k].to(DEV) for k in ("row_prob", "row_id", "lengths", "tokens", "word_mask")}
    fed, conf, score = torch.full((5, 20), -7, dtype=torch.int64, device=DEV), torch.full((5, 20), -7.0, device=DEV), torch.full((5,), -7.0, device=DEV)
    tok0, wm0 = v["tokens"].clone(), v["word_mask"].clone()
    for kw in (dict(L=65), dict(P=-1), dict(P=18), dict(step=4), dict(step=-1), dict(T=0)):
        a = dict(L=20, P=3, step=1, T=4)
        a.update(kw)
        with pytest.raises(XlError, match=r"xl_caption_step.*\(-5\)"):
            ops.caption_step(v["row_prob"], v["row_id"], None, v["lengths"], v["tokens"], fed, v["word_mask"], conf, score, 5, a["L"], a["P"],
                             a["step"], a["T"], MASK)
    with pytest.raises(XlError, match="null argument"):
        ops.caption_step(v["row_prob"], v["row_id"], None, v["lengths"], v["tokens"], None, v["word_mask"], conf, score, 5, 20, 3, 1, 4, MASK)
    torch.cuda.synchronize()
    assert torch.equal(v["tokens"], tok0) and torch.equal(v["word_mask"], wm0)
    assert bool((fed == -7).all()) and bool((conf == -7.0).all()) and bool((score == -7.0).all())
    # out-of-range lengths are clamped, not refused: n = 99 behaves as L - 2 - P, n = -3 as 0
    c2 = dict(c, lengths=torch.tensor([99, -3, 7, 4, 10], dtype=torch.int32))
    want = TC.run_step(CaptionFakeOps(torch.float32), c2)
    ops.caption_step(v["row_prob"], v["row_id"], None, c2["lengths"].to(DEV), v["tokens"], fed, v["word_mask"], conf, score, 5, 20, 3, 1, 4, MASK)
    torch.cuda.synchronize()
    assert torch.equal(v["tokens"].cpu(), want[0]) and torch.equal(fed.cpu(), want[1]) and torch.equal(v["word_mask"].cpu(), want[2])
    assert float(score[1]) == 0.0 and int(v["word_mask"][1].sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- 2. vocabulary shape
VOCAB, VQ, D_MODEL, N_BANNED = 30522, 30720, 768, 999


def _vocab_case(T):
    """M = 256 head rows against the padded tied decoder: 30522 real columns of which the first 999 are banned (real embedding rows, bias
    -1e30), 198 pad columns (zero rows, bias -1e30); the -1e30 entries are NOT divided by T"""
    gen = torch.Generator().manual_seed(77)
    A = torch.randn(256, D_MODEL, generator=gen).bfloat16()
    Bm = (torch.randn(VQ, D_MODEL, generator=gen) * 0.05).bfloat16()
    Bm[VOCAB:] = 0
    bias = torch.randn(VQ, generator=gen) * 0.1
    bias_T = (bias / T).float()
    bias_T[:N_BANNED] = BS.PAD_BIAS
    bias_T[VOCAB:] = BS.PAD_BIAS
    return A.to(DEV), Bm.to(DEV), bias_T.to(DEV), 1.0 / T


def _live_error(y, e, bias_T):
    """the logit error with no allowance at the banned columns: a banned column is acc - 1e30 = -1e30 exactly in fp32 (|acc| is far
    below half an ulp of 1e30) and in float64, as a pad column is -- rowmax_logit_error only knows the pad columns' zero rows"""
    return torch.where(bias_T[None, :] < -1e29, torch.zeros_like(e), e)


def test_vocabulary_shape_through_the_fused_greedy_predict():
    """xl_gemm XL_EPI_ROWMAX at M = 256, N = 30720 (480 segments), K = 768 + xl_rowmax_combine against float64: every segment record,
    an admissible row argmax, row_lse, row_maxprob; no banned or pad column is ever returned"""
    from test_sampling_gpu import _guarded, _table
    ops = _ops(torch.bfloat16)
    A, Bm, bias, _ = _vocab_case(1.0)
    M, n_seg = 256, VQ // 64
    whole, ws, before = _guarded(n_seg * M * 4)
    ops.gemm(A, Bm, None, bias, None, ws, M, VQ, D_MODEL, D_MODEL, D_MODEL, VQ, epilogue=5)
    p, lse = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
    idx = torch.zeros(M, dtype=torch.int32, device=DEV)
    ops.rowmax_combine(ws, n_seg, M, p, idx, lse)
    torch.cuda.synchronize()
    G = (whole.numel() - n_seg * M * 4) // 2
    assert torch.equal(whole[:G], before[:G]) and torch.equal(whole[-G:], before[-G:])
    y, _, e = BS.tempered_reference(A, Bm, bias, 1.0, 0)
    e = _live_error(y, e, bias)
    rows, n_adm_seg = Bd.check_rowmax_records(ws, y, e, "vocabulary ROWMAX")
    _table(rows, "records")
    rows, n_adm = Bd.check_rowmax_rows(y, e, n_seg, p, idx, lse, "vocabulary ROWMAX + combine")
    _table(rows, "rows")
    assert int(idx.min()) >= N_BANNED and int(idx.max()) < VOCAB
    print(f"  rows with more than one admissible column: {int((n_adm > 1).sum())} of {M}; distinct tokens {idx.unique().numel()}")


@pytest.mark.parametrize("T", [1.0, 0.5])
def test_vocabulary_shape_through_the_fused_draw(T):
    """the same shape through XL_EPI_ROWSAMPLE + xl_rowsample_combine: records, an admissible draw, row_lse, row_prob"""
    from test_sampling_gpu import _run_fused, _table
    A, Bm, bias_T, alpha = _vocab_case(T)
    ls = FS.launch_seed(9, 2)
    ws, p, idx, lse = _run_fused(_ops(torch.bfloat16), A, Bm, bias_T, alpha, ls)
    y, g, e = BS.tempered_reference(A, Bm, bias_T, alpha, ls)
    e = _live_error(y, e, bias_T)
    rows, _ = BS.check_records(ws, y, g, e, "vocabulary ROWSAMPLE")
    _table(rows, f"T={T} records")
    rows, n_adm = BS.check_rows(y, g, e, VQ // 64, p, idx, lse, "vocabulary ROWSAMPLE + combine")
    _table(rows, f"T={T} rows")
    assert int(idx.min()) >= N_BANNED and int(idx.max()) < VOCAB
    assert idx.unique().numel() > 200                                   # a draw over a flat 29.5k-way distribution, not a mode


# ---------------------------------------------------------------------------------------------------------------- 3. the engine loop
def _grab(eng, snaps):
    lh = eng.lang_heads

    def hook(i):
        M = eng.ML
        fused = eng.cdtype == torch.bfloat16 and lh.fused_predict_available()
        snaps.append(dict(fused=fused, hn=lh.p_hn[:M].clone(), logits=None if fused else lh.p_scores[:M].clone(), ids=lh.row_id[:M].clone(),
                          p=lh.row_prob[:M].clone(), lse=lh.row_lse[:M].clone(), tokens=eng.cap_tokens.clone().cpu(),
                          fed_ids=eng.ids.clone().cpu(), word_mask=eng.word_mask.clone().cpu(), conf=eng.cap_conf.clone().cpu(),
                          score=eng.cap_score.clone().cpu(), loff=eng.loff.clone().cpu() if eng.packed else None))
    return hook


def _dense(s, x, B, L):
    """a per-head-row vector as [B, L] (packed rows through the offsets)"""
    pos = torch.arange(L)[None, :]
    rows = (s["loff"][:-1].long()[:, None] if s["loff"] is not None else torch.arange(B)[:, None] * L) + pos
    return x.cpu()[rows.clamp(max=x.numel() - 1)]


def _check_loop(eng, snaps, sd, oc, feats, pos, lengths, prefix, T, banned, specials, margin_rel, caps):
    """every step teacher-forced: (a) the predicted ids admissible on the kernel's own head inputs against float64, no position
    exempted, within the sharpness caps; (b) tokens / masks / fed ids / confidences exactly what the six rules make of the device's own
    predictions; (c) the oracle's forward on the ids the device fed: the same token wherever the oracle's best logit is decisive"""
    cls_id, sep_id, mask_id = specials
    B, L, P = len(lengths), eng.L, len(prefix)
    lh = eng.lang_heads
    tok0, free, att = CO.layout(lengths, L, prefix, cls_id, sep_id, mask_id)
    state = dict(tokens=tok0, word_mask=free, fed_ids=tok0)
    banned_t = torch.tensor(list(banned))
    for i, s in enumerate(snaps):
        M = s["ids"].numel()
        if s["fused"]:
            Vq = lh.word_pred.w_pad.shape[0]
            y, _, e = BS.tempered_reference(s["hn"], lh.word_pred.w_pad, lh.word_pred.bias_pad, 1.0, 0)
            e = torch.where(lh.word_pred.bias_pad[None, :] < -1e29, torch.zeros_like(e), e)
            _, n_adm = Bd.check_rowmax_rows(y, e, Vq // 64, s["p"], s["ids"], s["lse"], f"step {i} fused predict")
        else:
            y = s["logits"][:, :lh.Vn].double()                      # the kernel's own fp32 logits: exact inputs, the exact rule
            n_adm = Bd.check_admissible(y, s["ids"], torch.zeros(M, dtype=torch.float64, device=y.device), f"step {i} argmax")
            pr = torch.exp(y.amax(1) - torch.logsumexp(y, 1))
            assert torch.allclose(s["p"].double(), pr, rtol=1e-5), i
        fr = _dense(s, torch.arange(M), B, L)[free]                  # head rows of the free positions
        share, most = Bd.sharpness(n_adm.cpu()[fr])
        print(f"  step {i}: {100 * share:.1f} % of the free rows with more than one admissible column, at most {most}")
        assert share <= caps[0] and most <= caps[1], (i, share, most)
        pp, pi = _dense(s, s["p"], B, L), _dense(s, s["ids"], B, L)
        assert not torch.isin(pi[free], banned_t).any() and int(pi[free].max()) < lh.Vn
        r_tok, r_fed, r_wm, r_conf, r_score = CO.caption_update(pp, pi, lengths, state["tokens"], state["word_mask"], L, P, i, T, mask_id)
        if i + 1 == T:
            r_wm = state["word_mask"]
            r_fed = torch.where(att, torch.where(r_wm, torch.full_like(r_tok, mask_id), r_tok), torch.zeros_like(r_tok))
        assert torch.equal(s["tokens"], r_tok) and torch.equal(s["word_mask"].bool(), r_wm) and torch.equal(s["fed_ids"], r_fed), i
        assert torch.equal(s["conf"], r_conf), i
        n = torch.tensor(lengths)
        logs = torch.log(r_conf.double().clamp(min=1e-300)).abs().sum(1)
        for b in range(B):
            assert abs(float(s["score"][b]) - float(r_score[b])) <= score_bound(int(n[b]), float(logs[b])), (i, b)
        scores = CO.step_logits(sd, oc, state["fed_ids"], att, feats, pos, banned)
        top2 = scores.topk(2, dim=2).values
        gap, scale = top2[..., 0] - top2[..., 1], top2[..., 0].abs().clamp_min(1.0)
        decisive = free & (gap > scale * margin_rel)
        same = pi.long() == scores.argmax(2)
        print(f"  step {i}: oracle decisive at {int(decisive.sum())} of {int(free.sum())} free positions, same token at {int((same & decisive).sum())}"
              f" of them, {int((same & free).sum())} of all")
        assert int(decisive.sum()) >= 0.5 * int(free.sum()) and bool(same[decisive].all()), i
        state = dict(tokens=r_tok, word_mask=r_wm, fed_ids=r_fed)
    assert torch.equal(snaps[-1]["tokens"][~free], tok0[~free])


@pytest.mark.parametrize("P,T,pack", [(0, 4, True), (3, 7, True), (3, 4, False)])
def test_engine_loop_fp32_teacher_forced_against_the_oracle(P, T, pack):
    """fp32, the tiny fixture model, B = 5, L = 20, ragged lengths with 1 and L - 2 - P.  Decisive = the oracle's best logit leads by
    more than 2^-12 of its size (2000 fp32 ulps: the six-layer fp32 forward differs from the oracle's by a few ulps per contraction)"""
    cfg, oc, sd = TC.tiny_model()
    prefix, lengths = TC.PREFIX[:P], TC.lengths_for(P)
    cid, feats, pos = TC.picture(oc, sd, TC.B_)
    snaps = []
    runs = []
    for reuse in (True, False):
        eng = TC.make_caption_engine(_ops(), cfg, sd, lengths, prefix, cid, feats, pos, device=DEV, pack_lang=pack)
        eng.reuse_vis_stack = reuse
        tok, score, conf = eng.sample_words_nar(lengths, T, P, _grab(eng, snaps) if reuse else None, mask_token_id=MASK, banned_ids=BANNED)
        torch.cuda.synchronize()
        runs.append((tok.clone(), score.clone(), conf.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))             # the visual stack once or every step: bit-identical
    assert eng.packed == pack and len(snaps) == T
    _check_loop(eng, snaps, sd, oc, feats, pos, lengths, prefix, T, BANNED, (CLS, SEP, MASK), 2.0 ** -12, (0.0, 1))


def _sharp_engine(dtype, ops=None, device=DEV):
    """the bf16 loop test's engine: SHARP_CFG, 12 captions of L = 20 (240 dense rows: packed rows rounded up to 256 head rows)"""
    cfg, oc, sd = TC.sharp_model()
    lengths = TC.sharp_lengths()
    cid, feats, pos = TC.picture(oc, sd, TC.SHARP_B)
    from xlxmert_amd.engine import Engine
    from xlxmert_amd.params import ParamStore
    store = ParamStore(cfg, device, dtype, task="word_mask")
    store.load_named(sd)
    eng = Engine(cfg, store, _ops(dtype) if ops is None else ops, TC.SHARP_B, TC.L_, 16, need_lang=True)
    eng.sync_compute_weights()
    tok, free, att = CO.layout(lengths, TC.L_, (), TC.SHARP_CLS, TC.SHARP_SEP, TC.SHARP_MASK)
    eng.set_inputs(tok.to(device), att.to(device), None, pos.to(device), cluster_ids=cid.to(device))
    return eng, oc, sd, feats, pos, lengths


def test_engine_loop_bf16_fused_teacher_forced_against_the_oracle():
    """bf16 at the smallest geometry that takes the fused path: 12 captions of L = 20, packed rows rounded up to 256 head rows.  Same
    three checks per step; the sharpness caps are TC.DEVICE_CAPS, chosen from the measurement on the oracle in test_caption_cpu.
    Decisive = the oracle's best logit leads by more than BF16_MARGIN = 2^-6 (the logits here are O(1), so the image sampler's "1/64
    of the best logit" with its floor of 1).  Why that is safe: the head input is a LayerNorm output, O(1) per element, carrying the
    bf16 roundings of ~6 layers (2^-9 each, adding in quadrature: ~5e-3 per element); a logit is a 128-term sum against embedding
    weights of size ~0.02, so its error is about sqrt(128) x 5e-3 x 0.02 = 1e-3, the operand roundings of the decoder add 4e-4, and
    the difference of two logits about 2e-3: the margin is some eight of those"""
    eng, oc, sd, feats, pos, lengths = _sharp_engine(torch.bfloat16)
    T = 4
    snaps, runs = [], []
    for reuse in (True, False):
        eng.reuse_vis_stack = reuse
        out = eng.sample_words_nar(lengths, T, 0, _grab(eng, snaps) if reuse else None, mask_token_id=TC.SHARP_MASK, banned_ids=TC.SHARP_BANNED)
        torch.cuda.synchronize()
        runs.append([x.clone() for x in out])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert eng.packed and eng.ML == 256 and all(s["fused"] for s in snaps)
    _check_loop(eng, snaps, sd, oc, feats, pos, lengths, (), T, TC.SHARP_BANNED, (TC.SHARP_CLS, TC.SHARP_SEP, TC.SHARP_MASK), BF16_MARGIN,
                TC.DEVICE_CAPS)


def test_fused_and_logits_paths_agree_where_a_single_column_is_admissible(monkeypatch):
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("XL_FUSED_PREDICT", fused)
        eng, oc, sd, feats, pos, lengths = _sharp_engine(torch.bfloat16)
        assert eng.lang_heads is not None
        snaps = []
        eng.sample_words_nar(lengths, 1, 0, _grab(eng, snaps), mask_token_id=TC.SHARP_MASK, banned_ids=TC.SHARP_BANNED)
        torch.cuda.synchronize()
        s = snaps[0]
        assert s["fused"] == (fused == "1")
        lh = eng.lang_heads
        lh.word_pred.prepare()
        y, _, e = BS.tempered_reference(s["hn"], lh.word_pred.w_pad, lh.word_pred.bias_pad, 1.0, 0)
        e = torch.where(lh.word_pred.bias_pad[None, :] < -1e29, torch.zeros_like(e), e)
        n_adm = Bd.check_admissible(y, s["ids"], e.amax(-1), f"fused={fused}")
        res[fused] = (s["ids"], n_adm, s["tokens"])
    single = (res["1"][1] == 1) & (res["0"][1] == 1)
    print(f"fused / logits first step: {int(single.sum())} of {single.numel()} head rows with a single admissible column")
    assert int(single.sum()) > 0.9 * single.numel()
    assert torch.equal(res["1"][0][single], res["0"][0][single])


# ---------------------------------------------------------------------------------------------------------------- 4. nn.Module
def test_sample_caption_ids_through_the_module():
    from xlxmert_amd.modeling import XLxmertForPretraining
    cfg, oc, sd = TC.tiny_model()
    m = XLxmertForPretraining(cfg, device=DEV, dtype=torch.float32).eval()
    m.load_state_dict(sd)
    B = 3
    cid, feats, pos = TC.picture(oc, sd, B)
    kw = dict(max_text_length=TC.L_, n_steps=4, mask_token_id=MASK, cls_token_id=CLS, sep_token_id=SEP, banned_ids=BANNED)
    for pic in (dict(cluster_ids=cid.to(DEV)), dict(visual_feats=feats.to(DEV), visual_pos=pos.to(DEV))):
        lengths = torch.tensor([4, 9, 1])
        tok, score = m.sample_caption_ids(lengths=lengths, prefix_ids=[11, 12], **pic, **kw)
        tok2, score2 = m.sample_caption_ids(lengths=lengths, prefix_ids=[11, 12], **pic, **kw)
        assert torch.equal(tok, tok2) and torch.equal(score, score2)                    # greedy is deterministic
        r_tok, r_score, _, _ = CO.sample_words_nar(sd, oc, feats, pos, lengths.tolist(), 4, TC.L_, (11, 12), BANNED, CLS, SEP, MASK)
        assert torch.equal(tok.cpu(), r_tok) and torch.allclose(score.cpu().double(), r_score, atol=1e-4)
        one = m.sample_caption_ids(lengths=lengths, prefix_ids=[11, 12], top_k=1, seed=5, **pic, **kw)
        assert torch.equal(one[0], tok)                                                 # top_k = 1 is greedy
        a = m.sample_caption_ids(lengths=lengths, temperature=1.5, seed=21, **pic, **kw)
        b = m.sample_caption_ids(lengths=lengths, temperature=1.5, seed=21, **pic, **kw)
        c = m.sample_caption_ids(lengths=lengths, temperature=1.5, seed=22, **pic, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
        torch.manual_seed(3)
        d = m.sample_caption_ids(lengths=lengths, temperature=1.5, **pic, **kw)
        torch.manual_seed(3)
        e = m.sample_caption_ids(lengths=lengths, temperature=1.5, **pic, **kw)
        assert torch.equal(d[0], e[0])                                                  # seed=None: torch's default generator governs
        cand = [2, 5, 8]
        tok_c, score_c, chosen, steps = m.sample_caption_ids(lengths=cand, return_intermediate=True, **pic, **kw)
        per = [m.sample_caption_ids(lengths=n, **pic, **kw) for n in cand]
        all_scores = torch.stack([p_[1] for p_ in per], 1)                              # [B, C]
        best = all_scores.argmax(1)
        assert chosen.tolist() == [cand[int(j)] for j in best] and len(steps) == 4 and steps[0].shape == (B * 3, TC.L_)
        for b_ in range(B):
            assert torch.equal(tok_c[b_], per[int(best[b_])][0][b_])
            assert abs(float(score_c[b_]) - float(all_scores[b_, best[b_]])) < 1e-5
    m2 = XLxmertForPretraining(TC.XLxmertConfig(**{**{k: getattr(oc, k) for k in TC.CFG_KEYS}, "task_mask_lm": False}), device=DEV, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="task_mask_lm"):
        m2.sample_caption_ids(cluster_ids=cid.to(DEV), lengths=3)
