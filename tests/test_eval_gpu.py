"""Validation scores on the device: xl_gemm(XL_EPI_ROWSCORE) + xl_rowscore_combine, xl_score_rows, Engine.evaluate_task and
PretrainStep.evaluate, element by element under the float64 bounds of tests/bounds_eval.py (derivations there)."""
import math

import numpy as np
import pytest
import torch

import bounds as Bd
import bounds_eval as BE
from fake_ops_eval import EPI_ROWSCORE

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096          # floats of guard on either side of a buffer, filled with +-2^12
PAD_BIAS = -1e30
N_REAL = 412


def _ops(dtype=torch.bfloat16):
    from xlxmert_amd.ops import HipOps
    return HipOps(dtype)


def _table(rows, what):
    for name, r in rows:
        print(f"  {what:<30} {name:<22} {'exact' if r == 0 else f'headroom {1.0 / r:9.2f}x'}")


def _guarded(n):
    whole = torch.full((n + 2 * GUARD,), 4096.0, device=DEV)
    whole[1::2] = -4096.0
    return whole, whole[GUARD:GUARD + n], whole.clone()


def _same_guards(whole, before, n):
    assert torch.equal(whole[:GUARD].view(torch.int32), before[:GUARD].view(torch.int32))
    assert torch.equal(whole[GUARD + n:].view(torch.int32), before[GUARD + n:].view(torch.int32))


def _fused_case(M, N, K, pad, gen_seed, zero=False):
    gen = torch.Generator().manual_seed(gen_seed)
    A = torch.randn(M, K, generator=gen).bfloat16()
    Bm = (torch.randn(N, K, generator=gen) * 0.5).bfloat16()
    bias = torch.randn(N, generator=gen)
    if zero:
        A.zero_()
        bias.zero_()
    Bm[N - pad:] = 0
    bias[N - pad:] = PAD_BIAS
    labels = torch.randint(0, N - pad, (M,), generator=gen)
    labels[torch.randperm(M, generator=gen)[:M // 10]] = -100
    labels[:6] = torch.tensor([0, 63, 64, 255, 256, N - pad - 1])
    return A.to(DEV), Bm.to(DEV), bias.to(DEV), labels.to(DEV)


def _reference(A, Bm, bias):
    K = A.shape[1]
    pre = A.double() @ Bm.double().t() + bias.double()[None, :]
    e = Bd.rowmax_logit_error(pre, A.double().abs() @ Bm.double().abs().t(), bias.double().abs()[None, :], K)
    return pre, e


def _run_fused(ops, A, Bm, bias, labels, totals):
    M, K = A.shape
    N = Bm.shape[0]
    n_seg = N // 64
    whole, ws, before = _guarded(n_seg * M * 4)
    ops.gemm(A, Bm, None, bias, labels, ws, M, N, K, K, K, N, epilogue=EPI_ROWSCORE)
    out_w, out, out_b = _guarded(3 * M)
    nll, rmax, pred = out[:M], out[M:2 * M], out[2 * M:].view(torch.int32)
    ops.rowscore_combine(ws, n_seg, M, labels, N_REAL, nll, pred, rmax, totals)
    torch.cuda.synchronize()
    _same_guards(whole, before, n_seg * M * 4)
    _same_guards(out_w, out_b, 3 * M)
    return ws, nll.clone(), pred.clone(), rmax.clone()


def test_rowscore_gemm_and_combine_within_bounds():
    """M = 256, N = 512, K = 128: two column tiles, 8 segments; -1e30 in the last 100 columns; labels random in [0, 412) with -100
    in a tenth of the rows and the segment / tile edges 0, 63, 64, 255, 256, 411 forced"""
    M, N, K = 256, 512, 128
    A, Bm, bias, labels = _fused_case(M, N, K, N - N_REAL, 51)
    tw, totals, tb = _guarded(4)
    before = totals.clone()
    ops = _ops()
    ws, nll, pred, rmax = _run_fused(ops, A, Bm, bias, labels, totals)
    _same_guards(tw, tb, 4)
    pre, e = _reference(A, Bm, bias)
    _table(BE.check_rowscore_records(ws, pre, e, labels), "records")
    _table(BE.check_rowscore_rows(pre, e, N // 64, labels, N_REAL, nll, pred, rmax), "rows")
    assert int(pred.max()) < N_REAL and int(pred.min()) >= 0
    _table(BE.check_totals(before, totals, labels, N_REAL, nll, pred), "totals")
    mid = totals.clone()
    _, nll2, pred2, _ = _run_fused(ops, A, Bm, bias, labels, totals)
    assert torch.equal(nll2, nll) and torch.equal(pred2, pred)
    d1, d2 = mid.double() - before.double(), totals.double() - mid.double()
    assert d2[1] == d1[1] and d2[2] == d1[2]                                        # a second call doubles the totals
    BE.check_totals(mid, totals, labels, N_REAL, nll, pred, "second launch")
    _same_guards(tw, tb, 4)
    # reproducible: the same launch into a fresh accumulator, twice, bit for bit
    t1, t2 = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV)
    _run_fused(ops, A, Bm, bias, labels, t1)
    _run_fused(ops, A, Bm, bias, labels, t2)
    assert torch.equal(t1.view(torch.int32), t2.view(torch.int32))
    # every per-row output and the totals may be NULL
    n_seg = N // 64
    ops.rowscore_combine(ws, n_seg, M, labels, N_REAL, None, None, None, None)
    t3 = torch.zeros(4, device=DEV)
    ops.rowscore_combine(ws, n_seg, M, labels, N_REAL, None, None, None, t3)
    torch.cuda.synchronize()
    assert torch.equal(t3.view(torch.int32), t1.view(torch.int32))


def test_rowscore_exact_ties():
    """M = 512 (two row tiles), A = 0 and no bias: every real logit is exactly 0 -- the lowest column wins, nll = log(412), a hit
    exactly where the label is 0"""
    M, N, K = 512, 512, 128
    A, Bm, bias, labels = _fused_case(M, N, K, N - N_REAL, 52, zero=True)
    totals = torch.zeros(4, device=DEV)
    ws, nll, pred, rmax = _run_fused(_ops(), A, Bm, bias, labels, totals)
    pre, e = _reference(A, Bm, bias)
    assert bool((pre[:, :N_REAL] == 0).all()) and bool((e == 0).all())
    assert bool((pred == 0).all())
    _table(BE.check_rowscore_records(ws, pre, e, labels), "ties records")
    _table(BE.check_rowscore_rows(pre, e, N // 64, labels, N_REAL, nll, pred, rmax), "ties rows")
    valid = labels >= 0
    assert bool((nll[~valid] == 0).all()) and float((nll[valid] - math.log(N_REAL)).abs().max()) < 1e-5
    BE.check_totals(torch.zeros(4, device=DEV), totals, labels, N_REAL, nll, pred)
    assert float(totals[2]) == int((labels == 0).sum()) > 0 and float(totals[1]) == int(valid.sum())


@pytest.mark.parametrize("K,ldl", [(2, 8), (1000, 1000), (10000, 10000), (30522, 30528)])
def test_score_rows_within_bounds(K, ldl):
    """M = 70 (more than one block, a ragged last one); the columns >= K of every row hold +2^12 and are never read"""
    M = 70
    gen = torch.Generator().manual_seed(60 + K)
    whole, lg, _ = _guarded(M * ldl)
    lg.view(M, ldl)[:, :K] = (torch.randn(M, K, generator=gen) * 3).to(DEV)
    if ldl > K:
        lg.view(M, ldl)[:, K:] = 4096.0
    x = lg.view(M, ldl)[:, :K].double()
    x[3] = x[3, 0]                                                                  # a row of exact ties
    lg.view(M, ldl)[3, :K] = x[3].float()
    before = whole.clone()
    labels = torch.randint(0, K, (M,), generator=gen)
    labels[::9] = -100
    labels[1], labels[2] = 0, K - 1
    labels = labels.to(DEV)
    ops = _ops(torch.float32)
    out_w, out, out_b = _guarded(3 * M)
    nll, rmax, pred = out[:M], out[M:2 * M], out[2 * M:].view(torch.int32)
    totals = torch.tensor([2.0, 3.0, 1.0, -7.0], device=DEV)
    t0 = totals.clone()
    ops.score_rows(lg, M, K, ldl, labels, nll, pred, rmax, totals)
    torch.cuda.synchronize()
    assert torch.equal(whole.view(torch.int32), before.view(torch.int32))
    _same_guards(out_w, out_b, 3 * M)
    _table(BE.check_score_rows(x, labels, nll, pred, rmax), f"K={K}")
    assert int(pred[3]) == 0 and float(rmax.max()) < 4096.0
    _table(BE.check_totals(t0, totals, labels, K, nll, pred), f"K={K} totals")
    # labels = NULL: predictions and maxima only, nothing counted
    out2_w, out2, out2_b = _guarded(3 * M)
    t1 = torch.zeros(4, device=DEV)
    ops.score_rows(lg, M, K, ldl, None, out2[:M], out2[2 * M:].view(torch.int32), out2[M:2 * M], t1)
    torch.cuda.synchronize()
    _same_guards(out2_w, out2_b, 3 * M)
    assert torch.equal(out2[2 * M:].view(torch.int32), pred) and torch.equal(out2[M:2 * M], rmax)
    assert bool((out2[:M] == 0).all()) and bool((t1 == 0).all())


def test_fused_against_unfused_on_one_set_of_operands():
    M, N, K = 256, 512, 128
    A, Bm, bias, labels = _fused_case(M, N, K, N - N_REAL, 53)
    ops = _ops()
    _, nll_f, pred_f, _ = _run_fused(ops, A, Bm, bias, labels, None)
    logits = torch.zeros(M, N_REAL, device=DEV)
    ops.gemm(A, Bm, logits, bias, None, None, M, N_REAL, K, K, K, N_REAL, out_f32=True)
    nll_u, pred_u = torch.zeros(M, device=DEV), torch.zeros(M, dtype=torch.int32, device=DEV)
    ops.score_rows(logits, M, N_REAL, N_REAL, labels, nll_u, pred_u, None, None)
    torch.cuda.synchronize()
    pre, e = _reference(A, Bm, bias)
    _, b_f, _, _, E, _ = BE.rowscore_row_bounds(pre, e, N // 64, labels, N_REAL)
    # the unfused path: logits within e (+ their fp32 store) of float64, then xl_score_rows on them
    x = logits.double()
    _, b_rows, _, _, valid = BE.score_rows_bounds(x, labels)
    col = labels.clamp(0, N_REAL - 1)
    b_u = torch.where(valid, b_rows + Bd.SLACK * E + e.gather(1, col[:, None])[:, 0] + 2 * Bd.U32 * pre[:, :N_REAL].abs().amax(-1),
                      torch.zeros_like(b_rows))
    r = Bd.check(nll_f, nll_u.double(), b_f + b_u, "fused against unfused row_nll")
    print(f"  fused against unfused: worst |difference| / (sum of bounds) {r:.3f}")
    Bd.check_admissible(pre, pred_f, E, "fused row_pred")
    Bd.check_admissible(pre[:, :N_REAL], pred_u, E, "unfused row_pred")


# ---------------------------------------------------------------------------------------------------------------- engine
TINY = dict(vocab_size=100, hidden_size=64, num_attention_heads=4, intermediate_size=128, max_position_embeddings=64,
            visual_feat_dim=32, num_clusters=100, l_layers=2, x_layers=2, r_layers=1)


def _tiny_engine(task, dtype=torch.bfloat16, train_dropout=False, seed=7):
    from xlxmert_amd.config import XLxmertConfig
    from xlxmert_amd.engine import Engine
    from xlxmert_amd.ops import HipOps
    from xlxmert_amd.params import ParamStore
    from xlxmert_amd.trainer import init_reference_weights, synthetic_batch
    cfg = XLxmertConfig(**TINY)
    B, L, V = 4, 64, 64
    store = ParamStore(cfg, DEV, dtype, task=task)
    init_reference_weights(store, seed)
    gen = torch.Generator().manual_seed(seed)
    store.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=gen))
    for name in ("obj_predict_head.out_cluster.bias", "cls.predictions.bias"):
        if name in store.index:
            store.view(name).copy_(torch.randn(store.view(name).shape, generator=gen).to(DEV) * 0.5)
    eng = Engine(cfg, store, HipOps(dtype), B, L, V, need_lang=task != "vis_mask", train_dropout=train_dropout)
    eng.sync_compute_weights()
    batch = {k: v.to(DEV) for k, v in synthetic_batch(cfg, B, L, 8, seed=seed + 1).items()}
    return cfg, eng, batch


def _set_vis(eng, batch):
    vm = torch.ones_like(batch["vis_mask"], dtype=torch.bool)                        # all cells masked: 256 rows
    labels = batch["cluster_ids"].clone()
    labels.view(-1)[::11] = -100
    eng.set_inputs(batch["input_ids"], batch["attention_mask"], None, batch["visual_pos"], cluster_ids=batch["cluster_ids"],
                   vis_mask=vm, obj_labels=labels)
    return labels.reshape(-1)


def _set_word(eng, batch):
    wl = torch.full_like(batch["input_ids"], -1)
    wl[:, 1:7] = batch["input_ids"][:, 1:7]
    wl[batch["input_ids"] == 0] = -1
    eng.set_inputs(batch["input_ids"], batch["attention_mask"], None, batch["visual_pos"], cluster_ids=batch["cluster_ids"])
    return wl


def _head_check(key, out, x_in, W, bias, labels, n_cols, pred, Kq):
    """evaluate_task's totals against float64 over the head's own inputs x_in [M, K] (bf16), W [n_cols, K], bias"""
    M, K = x_in.shape
    Wp = torch.zeros(Kq, K, dtype=torch.float64, device=DEV)
    Wp[:n_cols] = W.double()
    bp = torch.full((Kq,), PAD_BIAS, dtype=torch.float64, device=DEV)
    bp[:n_cols] = bias.double()
    pre = x_in.double() @ Wp.t() + bp[None, :]
    e = Bd.rowmax_logit_error(pre, x_in.double().abs() @ Wp.abs().t(), bp.abs()[None, :], K)
    nll, b_nll, _, _, E, valid = BE.rowscore_row_bounds(pre, e, Kq // 64, labels, n_cols)
    Bd.check_admissible(pre, pred, E, f"{key} row_pred")
    assert int(pred.max()) < n_cols
    cnt = int(valid.sum())
    assert out[key + "_count"].item() == cnt > 0
    assert out[key + "_correct"].item() == int((valid & (pred.long() == labels)).sum())
    ref = nll.sum()
    b_sum = b_nll.sum() + Bd.sum_bound(nll.abs().sum(), M, ref)
    r = Bd.check(out[key + "_sum"], ref.reshape(1), b_sum.reshape(1), f"{key}_sum")
    b_mean = b_sum / cnt + Bd.U32 * (ref / cnt).abs() * Bd.SLACK
    Bd.check(out[key], (ref / cnt).reshape(1), b_mean.reshape(1), key)
    print(f"  {key}: {float(out[key]):.6f} (float64 {float(ref / cnt):.6f}), count {cnt}, |err| / bound {r:.3f}")
    # the logits path of task_forward(want_grad=False): fp32 logits (e + their store) and xl_ce_fwd_bwd's lse (bounds.ce_bounds),
    # one term per valid row, an M-deep fp32 sum scaled by 1 / count
    x = pre[:, :n_cols]
    b_lse, _ = Bd.ce_bounds(x, valid.double(), 0.0, torch.logsumexp(x, 1), torch.zeros_like(x), torch.float32)
    col = labels.clamp(0, n_cols - 1)
    per_row = (b_lse + Bd.SLACK * E + e.gather(1, col[:, None])[:, 0] + 2 * Bd.U32 * x.abs().amax(-1)) * valid
    b_tf = (per_row.sum() + Bd.sum_bound(nll.abs().sum(), M + 2, ref)) / cnt + Bd.SLACK * 2 * Bd.U32 * (ref / cnt).abs()
    return ref / cnt, b_mean, b_tf


@pytest.mark.parametrize("train_dropout", [False, True])
def test_engine_vis_mask_and_word_mask_bf16(train_dropout):
    cfg, eng, batch = _tiny_engine("all", train_dropout=train_dropout)
    _, plain, _ = _tiny_engine("all", train_dropout=False)
    st = eng.store
    # vis_mask: 256 masked rows, 100 codes padded to 256
    labels = _set_vis(eng, batch)
    out = {k: v.clone() for k, v in eng.evaluate_task("vis_mask").items()}
    torch.cuda.synchronize()
    pred = eng.eval_buf("pred_obj", 1, eng.MV, torch.int32).view(-1)
    ref, b_ev, b_tf = _head_check("obj_loss", out, eng.feat[:eng.MV], st.centroids_c, eng.hd["bc"][0], labels, cfg.num_clusters, pred, 256)
    _set_vis(plain, batch)
    tf = plain.task_forward("vis_mask", want_grad=False)
    torch.cuda.synchronize()
    Bd.check(out["obj_loss"], tf["obj_loss"].double(), (b_ev + b_tf).reshape(1), "obj_loss against task_forward(want_grad=False)")
    assert abs(out["feat_loss"].item() - tf["feat_loss"].item()) <= 1e-6 * max(1.0, abs(tf["feat_loss"].item()))
    # word_mask: 256 language rows, 100 words padded to 256
    wl = _set_word(eng, batch)
    out = {k: v.clone() for k, v in eng.evaluate_task("word_mask", word_labels=wl).items()}
    torch.cuda.synchronize()
    lh = eng.lang_heads
    lab = torch.where(wl < 0, torch.full_like(wl, -100), wl).reshape(-1)
    pred = eng.eval_buf("pred_lm", 1, eng.MLd, torch.int32).view(-1)
    ref, b_ev, b_tf = _head_check("lm_loss", out, lh.hn[:eng.MLd], st.cview("bert.embeddings.word_embeddings.weight"), lh.vb, lab,
                                  cfg.vocab_size, pred, 256)
    _set_word(plain, batch)
    tf = plain.task_forward("word_mask", word_labels=wl, want_grad=False)
    torch.cuda.synchronize()
    Bd.check(out["lm_loss"], tf["lm_loss"].double(), (b_ev + b_tf).reshape(1), "lm_loss against task_forward(want_grad=False)")


def test_engine_unfused_paths_agree_with_fused(monkeypatch):
    """XL_FUSED_PREDICT=0 and an fp32 engine go through the logits and xl_score_rows: the same counts, losses within bf16 noise"""
    cfg, eng, batch = _tiny_engine("all")
    labels = _set_vis(eng, batch)
    fused = {k: v.clone() for k, v in eng.evaluate_task("vis_mask", feat_loss=False).items()}
    monkeypatch.setenv("XL_FUSED_PREDICT", "0")
    unfused = eng.evaluate_task("vis_mask", feat_loss=False)
    torch.cuda.synchronize()
    assert fused["obj_loss_count"].item() == unfused["obj_loss_count"].item() == int((labels >= 0).sum())
    assert abs(fused["obj_loss"].item() - unfused["obj_loss"].item()) < 1e-4 * max(1.0, abs(unfused["obj_loss"].item()))


def _golden(name):
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("task", ["matched", "qa", "vqa", "nlvr2"])
def test_engine_small_heads_fp32_against_fixtures(task):
    """the heads that go through xl_score_rows, in fp32 against the reference fixtures (weights: the fixtures' state-dict recipe)"""
    import test_engine_cpu as TE
    ops = _ops(torch.float32)
    if task == "vqa":
        g = _golden("vqa_tiny")
        eng, inp = TE.make_vqa_engine(g, ops, DEV)
        out = eng.evaluate_task("vqa", targets=inp["targets"].to(DEV))
        logit = torch.from_numpy(g["logit"])
        assert abs(out["loss"].item() - float(g["loss"])) < 2e-5
        assert torch.equal(out["pred"].long().cpu(), logit.argmax(1)) and (out["score"].cpu() - logit.max(1).values).abs().max() < 5e-5
    elif task == "nlvr2":
        g = _golden("nlvr2_tiny")
        eng, inp = TE.make_nlvr2_engine(g, ops, DEV)
        out = eng.evaluate_task("nlvr2", labels=inp["labels"].to(DEV))
        logit = torch.from_numpy(g["logit"])
        assert abs(out["loss"].item() - float(g["loss"])) < 2e-5
        assert torch.equal(out["pred"].long().cpu(), logit.argmax(1))
        assert out["loss_count"].item() == 3 and out["loss_correct"].item() == int((logit.argmax(1) == inp["labels"]).sum())
    elif task == "matched":
        g = _golden("lang_tasks_tiny")
        eng, inp = TE.make_lang_task_engine(g, "matched", ops, DEV)
        out = eng.evaluate_task("matched", matched_labels=inp["matched_labels"].to(DEV))
        assert abs(out["matched_loss"].item() - float(g["matched:loss"])) < 2e-5 and out["matched_loss_count"].item() == 3
    else:
        g = _golden("qa_tasks_tiny")
        eng, inp = TE.make_qa_engine(g, "qa", ops, DEV)
        x = {k: v.to(DEV) for k, v in inp.items()}
        eng.set_inputs(x["input_ids"], x["attention_mask"], x["token_type_ids"], x["visual_pos"], cluster_ids=x["cluster_ids"])
        out = eng.evaluate_task("qa", qa_labels=x["qa_labels"])
        assert abs(out["qa_loss"].item() - float(g["qa:qa_loss"])) < 2e-5
        assert (out["qa_pred"].cpu().numpy() == g["qa:qa_pred"]).all()


@pytest.mark.parametrize("plan", [True, False])
def test_step_evaluate_step_equals_step_step(plan):
    from xlxmert_amd.config import XLxmertConfig
    from xlxmert_amd.trainer import PretrainStep, synthetic_batch
    cfg = XLxmertConfig(**TINY)
    B, L = 4, 64
    batches = [{k: v.to(DEV) for k, v in synthetic_batch(cfg, B, L, 8, seed=300 + i).items()} for i in range(4)]
    finals = []
    for with_eval in (True, False):
        tr = PretrainStep(cfg, B, L, 64, dtype=torch.bfloat16, device=DEV, seed=11, plan=plan, train_dropout=True, total_steps=10,
                          lr=1e-3)
        cent = torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=torch.Generator().manual_seed(2))
        tr.set_centroids(cent)
        for i in range(3):                                  # (plan mode: a warm step, a recorded step, a replayed step)
            tr.step(batches[i % 2])
            if with_eval and i >= 0:
                out = tr.evaluate(batches[3])
                assert out["obj_loss_count"].item() > 0
        tr.sync()
        torch.cuda.synchronize()
        assert tr.t == 3 and tr.micro == 3
        finals.append((tr.store.master.clone(), tr.store.exp_avg.clone()))
        tr.close()
    assert torch.equal(finals[0][0], finals[1][0]) and torch.equal(finals[0][1], finals[1][1])


# ---------------------------------------------------------------------------------------------------------------- module surface
def test_module_evaluate_and_predict():
    """XLxmertForPretraining.evaluate = the no_grad forward of an eval() model (losses), from a model left in train(); VQAModel /
    NLVR2Model.predict = logit.max(1) of their eval() forward; the training flag is restored"""
    from xlxmert_amd.config import XLxmertConfig
    from xlxmert_amd.modeling import NLVR2Model, VQAModel, XLxmertForPretraining
    from xlxmert_amd.trainer import synthetic_batch
    cfg = XLxmertConfig(**TINY)
    B, L = 4, 64
    b = {k: v.to(DEV) for k, v in synthetic_batch(cfg, B, L, 8, seed=21).items()}
    m = XLxmertForPretraining(cfg, device=DEV, dtype=torch.float32)
    m.set_visual_embedding(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=torch.Generator().manual_seed(3)))
    m.train()
    kw = dict(input_ids=b["input_ids"], visual_pos=b["visual_pos"], attention_mask=b["attention_mask"], cluster_ids=b["cluster_ids"],
              vis_mask=b["vis_mask"], label_dict={"obj_labels": b["obj_labels"]}, task="vis_mask")
    out = m.evaluate(**kw)
    assert m.training
    with torch.no_grad():
        ref = m.eval()(**kw)
    m.train()
    torch.cuda.synchronize()
    valid = b["obj_labels"] != -100
    assert out["obj_loss_count"].item() == int(valid.sum())
    assert abs(out["obj_loss"].item() - ref["obj_loss"].item()) < 1e-5 * max(1.0, abs(ref["obj_loss"].item()))
    gen = torch.Generator().manual_seed(5)
    feats = torch.randn(B, 64, cfg.visual_feat_dim, generator=gen).to(DEV)
    for model, f, p, ids in ((VQAModel(cfg, 37, dtype=torch.float32), feats, b["visual_pos"], b["input_ids"]),
                             (NLVR2Model(cfg, dtype=torch.float32), feats.view(2, 2, 64, -1), b["visual_pos"].view(2, 2, 64, 4), b["input_ids"])):
        model.train()
        score, pred = model.predict(ids, f, p, b["attention_mask"])
        assert model.training
        with torch.no_grad():
            logit = model.eval()(ids, f, p, b["attention_mask"])["logit"]
        torch.cuda.synchronize()
        assert torch.equal(pred, logit.argmax(1)) and torch.equal(score, logit.max(1).values)
