"""The float64 instrument of tests/test_kernel_bounds_gpu.py (its recording proxy and tests/bounds.py) pointed at everything else the
benchmark times: the masked-visual-token step in its DEFAULT reduction mode (deferred second stages, checked at the flushes), the
Mask-Predict and autoregressive samplers with the fused row-max head, the VQA / NLVR2 fine-tune steps, the word_mask / matched
language branches, the output_attentions forward, a temperature sampler (XL_EPI_ROWSAMPLE head) and the validation pass of the
codebook head and the tied decoder (Engine.evaluate_task: XL_EPI_ROWSCORE, and xl_score_rows with XL_FUSED_PREDICT=0).  One recorded bf16 step each at the geometry bench.py times (same
construction as bench.py other_workloads; weights from the oracle's make_*_state_dict), dropout on for the training steps, eager.
Every test prints its headroom table, fails on a numeric method without a checker, on any element beyond its bound, on a pending
column sum that no flush covered, and on a kernel of its "must have called" set that the step no longer reaches."""
import functools
import time

import pytest
import torch

import bounds as BD
import lxmert_oracle as O
from test_kernel_bounds_gpu import CFG_KEYS, Recorder, _rn, _table

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
# make_inputs seeds of the sampler tests.  The sharpness caps of the admissible-argmax rule (bounds.MAX_SHARE_AMBIGUOUS,
# MAX_ADMISSIBLE) are a condition on the INPUTS, computed from the float64 logits alone: at bs 256, T = 4, seed 23 has one row
# with 5 admissible columns at step 4 (5.3 ... 7.6 % of the rows with more than one); seeds 29, 37, 41, 43, 47 stay at <= 4 columns
# and <= 7.8 % at every step, seed 41 with the smallest shares (4.5 / 5.8 / 6.9 / 5.8 %).  The caps stay; the inputs are seed 41.
NAR_SEED, INPUT_SEED = 41, 23


def _cfgs(**kw):
    from xlxmert_amd.config import XLxmertConfig
    cfg = XLxmertConfig(**kw)
    return cfg, O.OracleConfig(**{k: getattr(cfg, k) for k in CFG_KEYS})


@functools.lru_cache(maxsize=2)
def _state_dict(kind, seed, num_answers=0):
    """oracle weights of the full-size model (cached: several workloads share one draw)"""
    _, oc = _cfgs()
    if kind == "vqa":
        return O.make_vqa_state_dict(oc, num_answers, seed)
    if kind == "nlvr2":
        return O.make_nlvr2_state_dict(oc, seed)
    if kind == "cls":
        return O.make_cls_state_dict(oc, seed)
    return O.make_state_dict(oc, seed)


def _recorder(ops=None):
    if ops is None:
        from xlxmert_amd.ops import HipOps
        ops = HipOps(BF)
    return Recorder(ops)


def _finish(rec, t0, must, extra=()):
    _table(rec.rows, time.time() - t0)
    print(f"methods called: {sorted(rec.called)}")
    assert not rec.unchecked, f"numeric methods without a checker: {sorted(rec.unchecked)}"
    assert not rec.failures, "\n".join(rec.failures)
    assert not rec.leftover(), f"column sums never checked: {rec.leftover()}"
    for m in must:
        assert m in rec.called, f"the step no longer calls {m}"
        assert m.startswith("flush_") or any(r[0] == m for r in rec.rows), f"{m} was called but none of its calls was checked"
    for what, ok in extra:
        assert ok, what


def _checked(rec, name, **match):
    """the checked calls of `name` whose arguments match (value, or a predicate)"""
    return [a for n, a in rec.checked if n == name and all((v(a[k]) if callable(v) else a[k] == v) for k, v in match.items())]


def _step(task, B, batch, sd, cfg, dev="cuda", ops=None, L=20, V=64, **kw):
    """one recorded training step (forward, backward, clip + AdamW), constructed as bench.py does"""
    from xlxmert_amd.params import ParamStore
    from xlxmert_amd.trainer import PretrainStep
    extra = {"num_answers": kw["num_answers"]} if "num_answers" in kw else {}
    store = ParamStore(cfg, dev, BF, task=task, **extra)
    store.load_named(sd)
    rec = _recorder(ops)
    tr = PretrainStep(cfg, B, L, V, dtype=BF, device=dev, store=store, task=task, train_dropout=True, total_steps=1000, lr=1e-4,
                      overlap_optimizer=True, plan=False, ops=rec, **kw)
    losses = tr.step({k: (v.to(dev) if torch.is_tensor(v) and k != "word_rows" else v) for k, v in batch.items()})
    tr.sync()
    assert all(torch.isfinite(torch.as_tensor(x)).all() for x in (losses if isinstance(losses, (tuple, list)) else [losses]) if x is not None)
    return rec, tr


# ---------------------------------------------------------------------------------------------------------------- deferred sums
def vis_mask_deferred(cfg, sd, B, dev="cuda", ops=None):
    from xlxmert_amd.trainer import synthetic_batch
    t0 = time.time()
    batch = synthetic_batch(cfg, B, 20, 8, seed=31)
    rec, tr = _step("vis_mask", B, batch, sd, cfg, dev, ops)
    for _ in range(3):              # a destination with two producers, the first unrecorded: both are recorded in another step
        if not rec.retry():
            break
        print("one more step: recording both producers of every shared destination", flush=True)
        tr.step({k: v.to(dev) for k, v in batch.items()})
        tr.sync()
    producers = sorted(n for n in ("gemm", "layernorm_bwd", "sdpa_bwd", "visn_ln_bwd", "colsum", "masked_colsum") if n in rec.called)
    at_flush = {r[0] for r in rec.rows if r[1].endswith("@flush")}
    _finish(rec, t0, ("gemm", "gemm_wgrad_group", "sdpa_bwd", "layernorm_bwd", "visn_ln_bwd", "flush_reductions", "adamw"),
            [("no flush was checked", rec.flushes_checked > 0)] +
            [(f"no pending sum of {n} was checked at a flush", n in at_flush) for n in producers if n not in ("colsum", "masked_colsum")])
    return rec


def test_vis_mask_step_with_deferred_reductions_checks_every_pending_sum_at_its_flush(monkeypatch):
    """the step the benchmark times: XL_DEFER_REDUCE unset, so the backward runs under xl_set_deferred_reduce(1) and every column
    sum (GEMM colsum, LayerNorm dgamma / dbeta / dbias_prev, the visual feature encoder's sums, the attention bias sums) is finished
    by reduce_partials_batched_kernel at a flush_reductions / flush_reductions_on.  Each pending destination is compared at the
    flush that covers it with (its content before the flush + the float64 contributions of the producers), within the producers'
    bounds.  Two producers into one destination (the shared cross-attention's q / k / v bias: one sdpa_bwd per direction) must
    both be recorded; where the first of them had passed unrecorded (its signature checked in an earlier layer), a second step
    records that signature at every call (Recorder.retry) -- nothing stays unchecked."""
    monkeypatch.delenv("XL_DEFER_REDUCE", raising=False)
    cfg, oc = _cfgs()
    vis_mask_deferred(cfg, _state_dict("base", 2718), 256)


# ---------------------------------------------------------------------------------------------------------------- samplers
def _sampler_engine(cfg, sd, B, ids, dev="cuda", ops=None, L=20, V=64):
    from xlxmert_amd.engine import Engine
    from xlxmert_amd.params import ParamStore
    store = ParamStore(cfg, dev, BF, task="vis_mask")
    store.load_named(sd)
    rec = _recorder(ops)
    eng = Engine(cfg, store, rec, B, L, V, need_lang=False)
    eng.sync_compute_weights()
    g = int(V ** 0.5)
    pos = torch.from_numpy(O.box_position(g)).unsqueeze(0).expand(B, -1, -1).float()
    eng.set_inputs(ids.to(dev), (ids > 0).to(dev), None, pos.to(dev), cluster_ids=torch.zeros(B, V, dtype=torch.long, device=dev),
                   vis_mask=torch.ones(B, V, dtype=torch.bool, device=dev))
    return rec, eng


def nar_sampler(cfg, oc, sd, B, T=4, dev="cuda", ops=None, seed=NAR_SEED):
    t0 = time.time()
    V = 64
    rec, eng = _sampler_engine(cfg, sd, B, O.make_inputs(oc, seed, B, 20, 8)["input_ids"], dev, ops)
    assert eng.fused_predict_available(), "the fused row-max head is not in use: the sampler would run the logits path"
    rec.mark(0)
    eng.sample_codes_nar(T, on_step=lambda i: rec.mark(i + 1))
    steps = set(range(T))
    n_masks = {a["n_mask"] for a in _checked(rec, "remask_lowest")}
    _finish(rec, t0, ("gemm", "rowmax_combine", "remask_lowest", "sampler_update", "codebook_gather"), [
        ("a ROWMAX gemm was not checked at every step", len(_checked(rec, "gemm", epilogue=BD.EPI_ROWMAX)) == T),
        ("rowmax_combine was not checked at every step", len(_checked(rec, "rowmax_combine")) == T),
        ("the composed check did not run at every step", {s[0] for s in rec.sharp} == steps),
        ("sampler_update was not checked at every step", len(_checked(rec, "sampler_update")) == T),
        (f"remask_lowest n_mask {sorted(n_masks)}", n_masks == {int((T - i) / T * V) for i in range(1, T)}),
        ("codebook_gather(vis_mask=None) not checked", len(_checked(rec, "codebook_gather", vis_mask=None)) >= 1),
        ("step 1 did not embed the text", rec.ncalls.get((0, "embed_ln_fwd"), 0) == 1),
        ("steps 2..T re-ran the language stack (_reuse_lang_stack)", all(rec.ncalls.get((i, "embed_ln_fwd"), 0) == 0 and
                                                                        rec.ncalls.get((i, "sdpa_fwd"), 0) > 0 for i in range(1, T)))])
    return rec


def test_nar_sampler_every_refinement_step_against_float64_logits():
    """Mask-Predict sampling at the timed geometry (bs 256, T = 4, 10k codebook padded to 10 240, fused head).  At EVERY step (the
    sampler ops and the ROWMAX gemm are keyed by the step index): the segment records against float64 logits, the combine on the
    kernel's own records (exact argmax), the composed row results (admissible argmax with no position exempted, row_lse,
    row_maxprob), remask_lowest (n_mask 48 / 32 / 16) and sampler_update exact; steps 2..T run the _reuse_lang_stack forward.
    The sharpness of the admissible-argmax rule is computed from the same float64 logits at every step and held to the caps that
    tests/test_bounds_cpu.py pins on the oracle (15 % of rows, 4 columns)."""
    cfg, oc = _cfgs()
    rec = nar_sampler(cfg, oc, _state_dict("base", 19), 256)
    for tag, share, most in rec.sharp:
        assert share <= BD.MAX_SHARE_AMBIGUOUS and most <= BD.MAX_ADMISSIBLE, (tag, share, most)


def ar_sampler(cfg, oc, sd, B, mode, n_steps, dev="cuda", ops=None, seed=INPUT_SEED):
    t0 = time.time()
    rec, eng = _sampler_engine(cfg, sd, B, O.make_inputs(oc, seed, B, 20, 8)["input_ids"], dev, ops)
    rec.mark(0)
    eng.sample_codes_ar(n_steps=n_steps, mode=mode, on_step=lambda i: rec.mark(i + 1))
    want = (lambda f: f >= 0) if mode == "tlbr" else (lambda f: f == -1)
    for tag, share, most in rec.sharp:
        assert share <= BD.MAX_SHARE_AMBIGUOUS and most <= BD.MAX_ADMISSIBLE, ("admissible-argmax rule not sharp", tag, share, most)
    _finish(rec, t0, ("sampler_ar_update", "rowmax_combine", "codebook_gather"), [
        ("sampler_ar_update was not checked at every step", len(_checked(rec, "sampler_ar_update", fixed_pos=want)) == n_steps),
        ("the final codebook_gather keeps the mask", len(_checked(rec, "codebook_gather", vis_mask="T")) >= 1)])
    return rec


@pytest.mark.parametrize("mode", ["confidence", "tlbr"])
def test_ar_sampler_steps_against_float64(mode):
    """autoregressive sampling, bs 64, three steps: sampler_ar_update with fixed_pos = -1 (most confident unvisited position, first
    index on ties) and with fixed_pos >= 0 (top-left to bottom-right), exact at every step, behind the same fused head checks"""
    cfg, oc = _cfgs()
    ar_sampler(cfg, oc, _state_dict("base", 19), 64, mode, 3)


def temperature_sampler(cfg, oc, sd, B, T=2, temperature=2.0, dev="cuda", ops=None, seed=NAR_SEED):
    """Mask-Predict sampling with a temperature: the head runs XL_EPI_ROWSAMPLE + xl_rowsample_combine instead of the row maximum"""
    t0 = time.time()
    rec, eng = _sampler_engine(cfg, sd, B, O.make_inputs(oc, seed, B, 20, 8)["input_ids"], dev, ops)
    assert eng.fused_predict_available(), "the fused head is not in use: the sampler would run the logits path"
    rec.mark(0)
    eng.sample_codes_nar(T, on_step=lambda i: rec.mark(i + 1), temperature=temperature, seed=5)
    _finish(rec, t0, ("gemm", "rowsample_combine", "remask_lowest", "sampler_update", "codebook_gather"), [
        ("a ROWSAMPLE gemm was not checked at every step", len(_checked(rec, "gemm", epilogue=9, alpha=1.0 / temperature)) == T),
        ("rowsample_combine was not checked at every step", len(_checked(rec, "rowsample_combine")) == T),
        ("the composed check did not run at every step", {s[0] for s in rec.sharp} == set(range(T))),
        ("sampler_update was not checked at every step", len(_checked(rec, "sampler_update")) == T),
        ("the row-maximum head ran", "rowmax_combine" not in rec.called)])
    return rec


def test_temperature_sampler_every_step_against_float64_logits():
    """T = 2, two steps, bs 4 (256 grid rows), bf16: the tempered segment records, the admissible draw and the tempered
    probability of the drawn code at every step, with the launch seed of that step"""
    cfg, oc = _cfgs()
    rec = temperature_sampler(cfg, oc, _state_dict("base", 19), 4)
    for tag, share, most in rec.sharp:
        assert share <= BD.MAX_SHARE_AMBIGUOUS and most <= BD.MAX_ADMISSIBLE, (tag, share, most)


def evaluate_tasks(cfg, oc, sds, B, fused, dev="cuda", ops=None, L=64, V=64):
    """Engine.evaluate_task("vis_mask") and ("word_mask") on one recorder each: the codebook head and the tied decoder through
    XL_EPI_ROWSCORE + xl_rowscore_combine (fused) or through fp32 logits and xl_score_rows (the caller sets XL_FUSED_PREDICT=0)"""
    from xlxmert_amd.engine import Engine
    from xlxmert_amd.params import ParamStore
    from xlxmert_amd.trainer import random_word_batch
    recs = []
    inp = O.make_inputs(oc, INPUT_SEED, B, L, int(V ** 0.5))
    for task, sd in zip(("vis_mask", "word_mask"), sds):
        t0 = time.time()
        store = ParamStore(cfg, dev, BF, task=task)
        store.load_named(sd)
        rec = _recorder(ops)
        eng = Engine(cfg, store, rec, B, L, V, need_lang=task != "vis_mask")
        eng.sync_compute_weights()
        ids, mask, pos = inp["input_ids"], inp["attention_mask"].to(dev), inp["visual_pos"].float().to(dev)
        if task == "vis_mask":
            labels = inp["cluster_ids"].clone()
            labels.view(-1)[::11] = -100
            eng.set_inputs(ids.to(dev), mask, None, pos, cluster_ids=inp["cluster_ids"].to(dev),
                           vis_mask=torch.ones(B, V, dtype=torch.bool, device=dev), obj_labels=labels.to(dev))
            out = eng.evaluate_task("vis_mask")
            key = "obj_loss"
        else:
            ids, wl = random_word_batch(ids, vocab_size=cfg.vocab_size, generator=torch.Generator().manual_seed(4242))
            eng.set_inputs(ids.to(dev), mask, None, pos, cluster_ids=inp["cluster_ids"].to(dev))
            out = eng.evaluate_task("word_mask", word_labels=wl.to(dev))
            key = "lm_loss"
        assert bool(torch.isfinite(out[key]).all()) and float(out[key + "_count"]) > 0
        must = ("gemm", "rowscore_combine") if fused else ("gemm", "score_rows")
        _finish(rec, t0, must, [
            ("the fused head did not run", not fused or len(_checked(rec, "gemm", epilogue=10)) >= 1),
            ("the totals were not checked", any(r[1] == "totals count" for r in rec.rows)),
            ("the other scores path ran too", ("score_rows" if fused else "rowscore_combine") not in rec.called)])
        recs.append(rec)
    return recs


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "logits"])
def test_evaluate_task_heads_within_bounds(fused, monkeypatch):
    """the validation pass of the codebook head and of the tied decoder at bs 4 (256 grid rows, 64 tokens a row), once through the fused scores epilogue and once
    (XL_FUSED_PREDICT=0) through fp32 logits and xl_score_rows"""
    if not fused:
        monkeypatch.setenv("XL_FUSED_PREDICT", "0")
    cfg, oc = _cfgs()
    evaluate_tasks(cfg, oc, (_state_dict("base", 19), _state_dict("cls", 41)), 4, fused)


# ---------------------------------------------------------------------------------------------------------------- fine-tune steps
def vqa_step(cfg, sd, B, A, dev="cuda", ops=None):
    from xlxmert_amd.trainer import synthetic_batch
    t0 = time.time()
    g = torch.Generator().manual_seed(4242)
    b = synthetic_batch(cfg, B, 20, 8, seed=7)
    tgt = torch.zeros(B, A)
    tgt[torch.arange(B), torch.randint(0, A, (B,), generator=g)] = 1.0
    feats = torch.randn(B, 64, cfg.visual_feat_dim, generator=g).relu()
    batch = {"input_ids": b["input_ids"], "visual_pos": b["visual_pos"], "visual_feats": feats, "targets": tgt}
    rec, tr = _step("vqa", B, batch, sd, cfg, dev, ops, num_answers=A)
    _finish(rec, t0, ("bce_logits_fwd_bwd", "visn_ln_fwd", "visn_ln_bwd", "gemm", "adamw"), [
        ("the BCE head did not see all answers", len(_checked(rec, "bce_logits_fwd_bwd", M=B, N=A)) == 1),
        ("the tanh pooler was not checked", len(_checked(rec, "gemm", epilogue=BD.EPI_TANH)) >= 1)])
    return rec


@pytest.mark.parametrize("B", [128, 512])
def test_vqa_step_within_bounds(B):
    """VQA fine-tune step, 3 129 answers, real 2048-d grid features in (visn_ln_fwd / visn_ln_bwd on features, not on the
    codebook), the BCE-with-logits head and its padded gradient, the answer head through the tanh pooler"""
    cfg, oc = _cfgs()
    vqa_step(cfg, _state_dict("vqa", 41, 3129), B, 3129)


def nlvr2_step(cfg, sd, P, dev="cuda", ops=None):
    from xlxmert_amd.trainer import synthetic_batch
    t0 = time.time()
    g = torch.Generator().manual_seed(4242)
    b = synthetic_batch(cfg, P, 20, 8, seed=8)
    batch = {"input_ids": b["input_ids"].repeat_interleave(2, 0), "visual_pos": b["visual_pos"][:, None].expand(-1, 2, -1, -1).contiguous(),
             "visual_feats": torch.randn(P, 2, 64, cfg.visual_feat_dim, generator=g).relu(), "labels": torch.randint(0, 2, (P,), generator=g)}
    rec, tr = _step("nlvr2", 2 * P, batch, sd, cfg, dev, ops)
    H = cfg.hidden_size
    _finish(rec, t0, ("gemm", "ce_fwd_bwd", "visn_ln_fwd", "visn_ln_bwd", "adamw"), [
        ("the pair head's first gemm (2 x hidden in) was not checked", len(_checked(rec, "gemm", M=P, K=2 * H)) >= 1),
        ("the 2-class CE of the pair head was not checked", len(_checked(rec, "ce_fwd_bwd", M=P, K=2)) == 1)])
    return rec


def test_nlvr2_step_within_bounds():
    """NLVR2 step: 128 statements x 2 images = 256 encoder rows, the pair head on the concatenated pooled rows"""
    cfg, oc = _cfgs()
    nlvr2_step(cfg, _state_dict("nlvr2", 41), 128)


def lang_step(cfg, sd, task, B, dev="cuda", ops=None):
    from xlxmert_amd.trainer import random_word_batch, synthetic_batch, word_rows_of
    t0 = time.time()
    g = torch.Generator().manual_seed(4242)
    b = synthetic_batch(cfg, B, 20, 8, seed=9)
    ids, wl = random_word_batch(b["input_ids"], vocab_size=cfg.vocab_size, generator=g)
    batch = {"input_ids": ids, "visual_pos": b["visual_pos"], "cluster_ids": b["cluster_ids"], "word_labels": wl,
             "matched_labels": torch.randint(0, 2, (B,), generator=g), "word_rows": word_rows_of(wl)}
    rec, tr = _step(task, B, batch, sd, cfg, dev, ops)
    Vc, H = cfg.vocab_size, cfg.hidden_size
    if task == "word_mask":
        must = ("gather_rows", "gather_labels", "ce_fwd_bwd", "embed_bwd", "gemm", "adamw")
        extra = [("the tied decoder's CE over the vocabulary was not checked", len(_checked(rec, "ce_fwd_bwd", K=Vc)) == 1),
                 ("the tied decoder's forward gemm was not checked", len(_checked(rec, "gemm", N=Vc, K=H)) >= 1),
                 ("the tied decoder's weight gradient into the word table was not checked",
                  any(r[0] in ("gemm", "gemm_wgrad_group") and (f"M={Vc} N={H}" in r[2] or f"{Vc}x{H}x" in r[1]) for r in rec.rows))]
    else:
        must = ("gemm", "tanh_bwd", "ce_fwd_bwd", "adamw")
        extra = [("the pooler's tanh epilogue was not checked", len(_checked(rec, "gemm", epilogue=BD.EPI_TANH)) >= 1),
                 ("the matched head's 2-class CE was not checked", len(_checked(rec, "ce_fwd_bwd", M=B, K=2)) == 1)]
    _finish(rec, t0, must, extra)
    return rec


@pytest.mark.parametrize("task", ["word_mask", "matched"])
def test_language_pretraining_step_within_bounds(task):
    """word_mask: the 30 522-way tied decoder on the gathered label rows (gather_rows / gather_labels), its CE and its weight
    gradient into the word table, embed_bwd; matched: the tanh pooler (EPI_TANH, tanh_bwd) and the 2-class head.  bs 256.
    The float64 reference of the decoder is computed for every gathered row (~750 x 30 522 x 768: no row subset was needed)."""
    cfg, oc = _cfgs()
    lang_step(cfg, _state_dict("cls", 41), task, 256)


# ---------------------------------------------------------------------------------------------------------------- attentions
def attentions_forward(cfg, oc, sd, B, dev="cuda", ops=None, L=20, V=64):
    from xlxmert_amd.engine import Engine
    from xlxmert_amd.params import ParamStore
    t0 = time.time()
    store = ParamStore(cfg, dev, BF, task="vis_mask")
    store.load_named(sd)
    rec = _recorder(ops)
    eng = Engine(cfg, store, rec, B, L, V, need_lang=True)
    eng.sync_compute_weights()
    inp = O.make_inputs(oc, 23, B, L, int(V ** 0.5))
    eng.set_inputs(inp["input_ids"].to(dev), inp["attention_mask"].to(dev), None, inp["visual_pos"].float().to(dev),
                   cluster_ids=inp["cluster_ids"].to(dev), vis_mask=inp["vis_mask"].to(dev))
    eng.encoder_forward()
    probs = eng.attention_probs()
    H = cfg.num_attention_heads
    _finish(rec, t0, ("attn_probs",), [
        ("language self-attention probabilities (packed) not checked", len(_checked(rec, "attn_probs", nq=L, nk=L, q_off="T")) >= 1),
        ("visual self-attention probabilities not checked", len(_checked(rec, "attn_probs", nq=V, nk=V)) >= 1),
        ("cross-attention probabilities not checked", len(_checked(rec, "attn_probs", nq=L, nk=V)) >= 1)])
    return rec, probs


def test_output_attentions_forward_within_bounds():
    """what LxmertModel.forward(output_attentions=True) (modeling.py) computes its attention tuples with: Engine.attention_probs()
    after an encoder forward with packed language rows -- attn_probs for the language / visual self-attention and the
    cross-attention, against exp(s - lse) in float64 from the forward's own lse"""
    cfg, oc = _cfgs()
    rec, _ = attentions_forward(cfg, oc, _state_dict("base", 19), 64)


# ---------------------------------------------------------------------------------------------------------------- edge cases
def _done(rec, t0, n_min):
    _table(rec.rows, time.time() - t0)
    assert not rec.unchecked, sorted(rec.unchecked)
    assert not rec.failures, "\n".join(rec.failures)
    assert len(rec.rows) >= n_min, len(rec.rows)


def test_rowmax_ragged_codebook_exact_tie_row_and_last_real_column():
    """the fused head off the sampler's data: 10 000 codes in 10 240 columns (segment 156 is 16 real + 48 padded columns, segments
    157..159 all padded), a constant bias so that row 0 -- an all-zero operand row -- is one exact tie over all real columns
    (expected argmax: column 0, in every segment its first column) and row 1's maximum sits in the last real column"""
    t0 = time.time()
    rec = _recorder()
    g = torch.Generator(device="cuda").manual_seed(21)
    M, K, n_real, N = 512, 2048, 10000, 10240
    A = _rn(g, M, K)
    W = torch.zeros(N, K, dtype=BF, device="cuda")
    W[:n_real] = _rn(g, n_real, K, scale=0.05)
    bias = torch.full((N,), -1e30, device="cuda")
    bias[:n_real] = 0.5
    A[0] = 0
    W[n_real - 1] = A[1] * 0.25
    ws = torch.zeros((N // 64) * M * 4, device="cuda")
    p, lse = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
    am = torch.zeros(M, dtype=torch.int32, device="cuda")
    rec.gemm(A, W, None, bias, None, ws, M, N, K, K, K, N, epilogue=BD.EPI_ROWMAX)
    rec.rowmax_combine(ws, N // 64, M, p, am, lse)
    _done(rec, t0, 9)
    assert int(am[0]) == 0 and int(am[1]) == n_real - 1, (int(am[0]), int(am[1]))
    idx = BD.rowmax_records(ws, N // 64, M)[2]
    assert torch.equal(idx[:, 0], torch.arange(N // 64, device="cuda") * 64)        # row 0: every segment's first column
    assert abs(float(p[0]) * n_real - 1.0) < 1e-5 and len(rec.sharp) == 1


def test_bce_padded_gradient_one_row_and_evaluation_call():
    """N = 3129 answers with ld_dlogits padded to 3136 (pre-filled with NaN: the kernel owns the pad columns), M = 1 and M = 5,
    logits out to |x| = 30 (both sigmoid branches, log1p of a denormal-range exp), soft targets; the dlogits=None call"""
    t0 = time.time()
    rec = _recorder()
    g = torch.Generator(device="cuda").manual_seed(22)
    N, ld = 3129, 3136
    for M in (1, 5):
        x = torch.randn(M, N, generator=g, device="cuda") * 8
        x[0, :4] = torch.tensor([30.0, -30.0, 0.0, 88.0], device="cuda")
        t = (torch.rand(M, N, generator=g, device="cuda") < 0.3).float() * torch.rand(M, N, generator=g, device="cuda")
        t[0, 0] = 1.0
        dl = torch.full((M, ld), float("nan"), dtype=BF, device="cuda")
        loss = torch.full((1,), 0.25, device="cuda")
        rec.bce_logits_fwd_bwd(x, t, dl, loss, M, N, N, N, ld)
        rec.bce_logits_fwd_bwd(x, t, None, loss, M, N, N, N, ld)
    _done(rec, t0, 6)


def test_remask_lowest_none_all_and_equal_confidences():
    t0 = time.time()
    rec = _recorder()
    g = torch.Generator(device="cuda").manual_seed(23)
    B, V = 37, 64
    prob = torch.rand(B, V, generator=g, device="cuda")
    prob[3] = 0.25
    prob[4, 7] = prob[4, 50] = 0.0
    for n_mask in (0, 1, 16, V):
        rec.mark(n_mask)
        vm = torch.full((B, V), 7, dtype=torch.uint8, device="cuda")
        rec.remask_lowest(prob, vm, B, V, n_mask)
        if 0 < n_mask < V:
            assert bool(vm[3, :n_mask].all()) and not bool(vm[3, n_mask:].any())       # equal confidences: the lowest indices
    _done(rec, t0, 8)


def test_attn_probs_with_an_all_masked_example():
    t0 = time.time()
    rec = _recorder()
    g = torch.Generator(device="cuda").manual_seed(24)
    B, H, dh, nq, nk = 4, 12, 64, 20, 64
    ld = 3 * H * dh
    q, kv = _rn(g, B * nq, ld), _rn(g, B * nk, ld)
    km = (torch.rand(B, nk, generator=g, device="cuda") > 0.3).to(torch.uint8)
    km[:, 0] = 1
    km[1] = 0
    o = torch.zeros(B * nq, H * dh, dtype=BF, device="cuda")
    lse = torch.zeros(B * H * nq, device="cuda")
    for p_drop in (0.0, 0.1):
        rec.sdpa_fwd(q, kv[:, H * dh:], kv[:, 2 * H * dh:], km, o, lse, B, H, nq, nk, dh, ld, ld, ld, H * dh, 0.125, p_drop=p_drop, seed=3)
        probs = torch.full((B, H, nq, nk), float("nan"), device="cuda")
        rec.attn_probs(q, kv[:, H * dh:], km, lse, probs, B, H, nq, nk, dh, ld, ld, 0.125, p_drop=p_drop, seed=3)
        assert not bool(probs[1].any())
    _done(rec, t0, 4)


def test_take_and_put_f32_of_the_sharded_optimizer():
    """only a multi-rank run reaches them: direct calls with indices inside and outside [own_lo, own_hi); an empty index list is
    refused by the library (the trainer never issues one) and leaves the destination alone"""
    from xlxmert_amd._lib import XlError
    t0 = time.time()
    rec = _recorder()
    g = torch.Generator(device="cuda").manual_seed(25)
    src = torch.randn(5000, generator=g, device="cuda")
    idx = torch.randperm(5000, generator=g, device="cuda")[:1300].to(torch.int32)
    dst = torch.full((1300,), float("nan"), device="cuda")
    rec.take_f32(src, idx, 1000, 3000, dst)
    own = (idx >= 1000) & (idx < 3000)
    assert 0 < int(own.sum()) < 1300 and not bool(dst[~own].any())
    back = torch.randn(5000, generator=g, device="cuda")
    keep = back.clone()
    rec.put_f32(back, idx, dst)
    untouched = torch.ones(5000, dtype=torch.bool, device="cuda")
    untouched[idx.long()] = False
    assert torch.equal(back[untouched], keep[untouched])
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    with pytest.raises(XlError):
        rec._ops.take_f32(src, empty, 0, 10, dst)
    with pytest.raises(XlError):
        rec._ops.put_f32(back, empty, dst)
    _done(rec, t0, 2)
