"""Validation pass on the host: Engine.evaluate_task / PretrainStep.evaluate / EvalMeter over the restatement of the new kernels
(tests/fake_ops_eval.EvalFakeOps) against the reference fixtures and the oracle, their effect on training state, dropout, the
dispatch of the heads, and the injected faults that tests/bounds_eval.py must reject."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import bounds as Bd
import bounds_eval as BE
import lxmert_oracle as O
from _util import golden_cfg, golden_inputs, load_golden
from fake_ops_eval import EPI_ROWSCORE, FAULTS, EvalFakeOps
from test_engine_cpu import make_lang_task_engine, make_nlvr2_engine, make_qa_engine, make_vqa_engine
from test_trainer_cpu import TINY, _free_port, oracle_cfg
from xlxmert_amd.config import XLxmertConfig
from xlxmert_amd.engine import Engine
from xlxmert_amd.params import ParamStore
from xlxmert_amd.trainer import EvalMeter, PretrainStep, synthetic_batch

CFG_KEYS = ("vocab_size", "hidden_size", "num_attention_heads", "intermediate_size", "max_position_embeddings", "type_vocab_size",
            "l_layers", "x_layers", "r_layers", "visual_feat_dim", "visual_pos_dim", "num_clusters")


def counts(logits, labels):
    """(#labels != -100, #(argmax == label) among them) over the oracle's logits"""
    lg, lab = logits.reshape(-1, logits.shape[-1]), labels.reshape(-1)
    valid = lab != -100
    return int(valid.sum()), int((valid & (lg.argmax(-1) == lab)).sum())


def check_key(out, key, loss, n, hits, tol):
    assert abs(out[key].item() - float(loss)) < tol, (key, out[key].item(), float(loss))
    assert out[key + "_count"].item() == n and out[key + "_correct"].item() == hits, (key, out[key + "_count"], n, out[key + "_correct"], hits)
    assert abs(out[key + "_sum"].item() - float(loss) * max(n, 1)) < tol * max(n, 1)


# ---------------------------------------------------------------------------------------------- oracle parity, fp32
def test_vis_mask_fixture_inputs_match_oracle():
    """tests/golden/vismask_tiny.npz inputs through the vis_mask branch: obj_loss / feat_loss of the oracle (the tolerance
    tests/test_trainer_cpu.py holds these keys to), hits and counts over the oracle's logits; masked rows only and all rows"""
    g = load_golden("vismask_tiny")
    oc = golden_cfg(g)
    cfg = XLxmertConfig(**{k: getattr(oc, k) for k in CFG_KEYS})
    sd = O.make_state_dict(oc, int(g["seed"]))
    inp = golden_inputs(g)
    ref = O.xlxmert_vis_mask_forward(sd, oc, inp["input_ids"], inp["visual_pos"], inp["attention_mask"], inp["cluster_ids"],
                                     inp["vis_mask"], inp["obj_labels"], token_type_ids=inp["token_type_ids"], return_all=True)
    n, hits = counts(ref["obj"], inp["obj_labels"])
    assert n > 0
    B, L = inp["input_ids"].shape
    V = inp["cluster_ids"].shape[1]
    for row_pad in (4, 256):                    # 4: the masked-row list is shorter than B*V; 256: padded up to all rows
        store = ParamStore(cfg, "cpu", torch.float32, task="vis_mask")
        store.load_named(sd)
        eng = Engine(cfg, store, EvalFakeOps(torch.float32), B, L, V, need_lang=False)
        eng.ROW_PAD = row_pad
        eng.sync_compute_weights()
        eng.set_inputs(inp["input_ids"], inp["attention_mask"], inp["token_type_ids"], inp["visual_pos"],
                       cluster_ids=inp["cluster_ids"], vis_mask=inp["vis_mask"], obj_labels=inp["obj_labels"])
        out = eng.evaluate_task("vis_mask")
        check_key(out, "obj_loss", ref["obj_loss"], n, hits, 3e-5)
        assert abs(out["feat_loss"].item() - ref["feat_loss"].item()) < 3e-5
        head = [c for c in eng.ops.calls if c[0] == "score_rows"]
        assert len(head) == 1 and (head[0][1] < B * V) == (row_pad == 4), head
        fwd = eng.task_forward("vis_mask", want_grad=False)
        assert abs(fwd["obj_loss"].item() - out["obj_loss"].item()) < 1e-6


@pytest.mark.parametrize("task", ["word_mask", "matched"])
def test_language_tasks_match_fixture(task):
    g = load_golden("lang_tasks_tiny")
    eng, inp = make_lang_task_engine(g, task, EvalFakeOps(torch.float32))
    oc = golden_cfg(g)
    sd = O.make_cls_state_dict(oc, int(g["seed"]))
    if task == "word_mask":
        ref = O.xlxmert_word_mask_forward(sd, oc, inp["input_ids"], inp["visual_pos"], inp["attention_mask"], inp["cluster_ids"],
                                          inp["word_labels"], inp["token_type_ids"])
        n, hits = counts(ref["scores"], inp["word_labels"])
        rows = (inp["word_labels"].reshape(-1) >= 0).nonzero().reshape(-1).to(torch.int32)
        for word_rows in (None, rows):
            out = eng.evaluate_task("word_mask", word_labels=inp["word_labels"], word_rows=word_rows)
            check_key(out, "lm_loss", g["word_mask:loss"], n, hits, 5e-6)
    else:
        ref = O.xlxmert_matched_forward(sd, oc, inp["input_ids"], inp["visual_pos"], inp["attention_mask"], inp["cluster_ids"],
                                        inp["matched_labels"], inp["token_type_ids"])
        n, hits = counts(ref["score"], inp["matched_labels"])
        out = eng.evaluate_task("matched", matched_labels=inp["matched_labels"])
        check_key(out, "matched_loss", g["matched:loss"], n, hits, 5e-6)


@pytest.mark.parametrize("task", ["qa", "vis_mask", "word_mask", "matched"])
def test_qa_model_tasks_match_fixture(task):
    g = load_golden("qa_tasks_tiny")
    eng, inp = make_qa_engine(g, task, EvalFakeOps(torch.float32))
    base = (inp["input_ids"], inp["attention_mask"], inp["token_type_ids"], inp["visual_pos"])
    kw = {"qa_labels": inp["qa_labels"]}
    if task == "vis_mask":
        eng.set_inputs(*base, cluster_ids=inp["cluster_ids"], vis_mask=inp["vis_mask"], obj_labels=inp["obj_labels"])
    else:
        eng.set_inputs(*base, cluster_ids=inp["cluster_ids"])
        if task == "word_mask":
            kw["word_labels"] = inp["word_labels"]
        elif task == "matched":
            kw["matched_labels"] = inp["matched_labels"]
    out = eng.evaluate_task(task, **kw)
    assert abs(out["qa_loss"].item() - float(g[task + ":qa_loss"])) < 1e-5
    assert (out["qa_pred"].numpy() == g[task + ":qa_pred"]).all()
    valid = inp["qa_labels"] != -100
    assert out["qa_loss_count"].item() == int(valid.sum())
    assert out["qa_loss_correct"].item() == int((valid & (torch.from_numpy(g[task + ":qa_pred"]) == inp["qa_labels"])).sum())
    for key in ("obj_loss", "feat_loss", "lm_loss", "matched_loss"):
        if f"{task}:{key}" in g:
            assert abs(out[key].item() - float(g[f"{task}:{key}"])) < 1e-5, key


def test_vqa_and_nlvr2_match_fixture():
    g = load_golden("vqa_tiny")
    eng, inp = make_vqa_engine(g, EvalFakeOps(torch.float32))
    out = eng.evaluate_task("vqa", targets=inp["targets"])
    logit = torch.from_numpy(g["logit"])
    assert abs(out["loss"].item() - float(g["loss"])) < 2e-6
    assert torch.equal(out["pred"].long(), logit.argmax(1)) and (out["score"] - logit.max(1).values).abs().max() < 5e-5
    assert abs(out["loss_correct"].item() - inp["targets"].gather(1, logit.argmax(1)[:, None]).sum().item()) < 1e-6
    g = load_golden("nlvr2_tiny")
    eng, inp = make_nlvr2_engine(g, EvalFakeOps(torch.float32))
    out = eng.evaluate_task("nlvr2", labels=inp["labels"])
    logit = torch.from_numpy(g["logit"])
    n, hits = counts(logit, inp["labels"])
    check_key(out, "loss", g["loss"], n, hits, 2e-6)
    assert torch.equal(out["pred"].long(), logit.argmax(1)) and (out["score"] - logit.max(1).values).abs().max() < 5e-5


# ---------------------------------------------------------------------------------------------- training state
def make_step(cfg, B, L, grid, ops=None, **kw):
    store = ParamStore(cfg, "cpu", torch.float32, task="vis_mask")
    store.load_named(O.make_state_dict(oracle_cfg(cfg), 3))
    kw.setdefault("visual_losses", "obj,feat")
    return PretrainStep(cfg, B, L, grid * grid, dtype=torch.float32, device="cpu", store=store,
                        ops=ops or EvalFakeOps(torch.float32), total_steps=10, lr=1e-2, **kw)


def snapshot(tr):
    st = tr.store
    bufs = [st.grad.clone(), st.master.clone()] + [getattr(st, n).clone() for n in ("m", "v", "exp_avg", "exp_avg_sq") if
                                                   isinstance(getattr(st, n, None), torch.Tensor)]
    return bufs, (tr.t, tr.micro, tr._accum_pending, tr.engine._seed, int(tr.engine.seed_dev.item()),
                  getattr(tr.engine, "accumulate", None), getattr(tr.engine, "dw_overwrite", None), dict(tr.engine._gen))


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1] and len(a[0]) == len(b[0]) >= 3


def state_sequences(world_tag=""):
    """step / evaluate / step == step / step; evaluate leaves every byte of the training state; an evaluate inside an
    accumulation window changes nothing"""
    cfg = XLxmertConfig(**TINY)
    B, L, grid = 2, 8, 4
    rank = dist.get_rank() if dist.is_initialized() else 0
    b = [synthetic_batch(cfg, B, L, grid, seed=700 + 10 * rank + i) for i in range(4)]
    a, c = make_step(cfg, B, L, grid, train_dropout=True), make_step(cfg, B, L, grid, train_dropout=True)
    a.step(b[0]); c.step(b[0])
    before = snapshot(a)
    out = a.evaluate(b[2])
    assert out["obj_loss_count"].item() > 0
    assert same(before, snapshot(a)), "evaluate changed training state"
    a.step(b[1]); c.step(b[1])
    assert torch.equal(a.store.master, c.store.master) and a.t == c.t == 2 and a.micro == c.micro
    # accumulation window
    a.step(b[2], update=False); c.step(b[2], update=False)
    before = snapshot(a)
    a.evaluate(b[3])
    assert same(before, snapshot(a)) and a._accum_pending
    a.step(b[3]); c.step(b[3])
    assert torch.equal(a.store.master, c.store.master) and torch.equal(a.store.grad, c.store.grad)
    return a.store.master.clone()


def test_evaluate_leaves_training_state_alone():
    state_sequences()


def _state_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    torch.save(state_sequences(), os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_leaves_training_state_alone_world2_gloo(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_state_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert torch.equal(torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt"))


def test_dropout_is_off_for_the_call():
    cfg = XLxmertConfig(**TINY)
    B, L, grid = 2, 8, 4
    batch = synthetic_batch(cfg, B, L, grid, seed=41)
    wet, dry = make_step(cfg, B, L, grid, train_dropout=True), make_step(cfg, B, L, grid, train_dropout=False)
    assert wet.engine.p_hid > 0 and wet.engine.p_attn > 0
    o1 = {k: v.clone() for k, v in wet.evaluate(batch).items()}
    o2 = {k: v.clone() for k, v in wet.evaluate(batch).items()}
    o3 = dry.evaluate(batch)
    assert wet.engine.p_hid > 0 and wet.engine.p_attn > 0              # restored
    for k in o1:
        assert torch.equal(o1[k], o2[k]) and torch.equal(o1[k], o3[k]), k
    with pytest.raises(AssertionError):                                 # ... also when the call raises
        wet.engine.evaluate_task("nonsense")
    assert wet.engine.p_hid > 0


def test_eval_meter_adds_on_the_device():
    cfg = XLxmertConfig(**TINY)
    B, L, grid = 2, 8, 4
    tr = make_step(cfg, B, L, grid)
    meter, s, n, h = EvalMeter(), 0.0, 0.0, 0.0
    for i in range(3):
        out = tr.evaluate(synthetic_batch(cfg, B, L, grid, seed=900 + i))
        s, n, h = s + out["obj_loss_sum"].item(), n + out["obj_loss_count"].item(), h + out["obj_loss_correct"].item()
        meter.add(out)
    res = meter.result()
    assert abs(res["obj_loss"] - s / n) < 1e-5 and abs(res["obj_accuracy"] - h / n) < 1e-7 and res["obj_loss_count"] == n
    assert "feat_loss" in res


# ---------------------------------------------------------------------------------------------- dispatch
def bf16_engine(task, B=4, L=64, V=64, fused="1", monkeypatch=None, dtype=torch.bfloat16):
    monkeypatch.setenv("XL_FUSED_PREDICT", fused)
    cfg = XLxmertConfig(**dict(TINY, max_position_embeddings=64, num_clusters=100))
    store = ParamStore(cfg, "cpu", dtype, task=task)
    store.load_named(O.make_cls_state_dict(oracle_cfg(cfg), 5) if task != "vis_mask" else O.make_state_dict(oracle_cfg(cfg), 5))
    eng = Engine(cfg, store, EvalFakeOps(dtype), B, L, V, need_lang=task != "vis_mask", pack_lang=False)
    eng.sync_compute_weights()
    return cfg, eng


@pytest.mark.parametrize("fused,dtype", [("1", torch.bfloat16), ("0", torch.bfloat16), ("1", torch.float32)])
def test_head_dispatch_vis_mask(monkeypatch, fused, dtype):
    cfg, eng = bf16_engine("vis_mask", fused=fused, monkeypatch=monkeypatch, dtype=dtype)
    B, V = 8, 64
    cfg, eng = bf16_engine("vis_mask", B=B, fused=fused, monkeypatch=monkeypatch, dtype=dtype)
    batch = synthetic_batch(cfg, B, 64, 8, seed=3)
    vm = torch.zeros(B, V, dtype=torch.bool)
    vm.view(-1)[torch.randperm(B * V, generator=torch.Generator().manual_seed(1))[:200]] = True        # 200 masked rows -> 256
    labels = batch["cluster_ids"].clone()
    labels[~vm] = -100
    eng.set_inputs(batch["input_ids"], batch["attention_mask"], None, batch["visual_pos"], cluster_ids=batch["cluster_ids"],
                   vis_mask=vm, obj_labels=labels)
    out = eng.evaluate_task("vis_mask", feat_loss=False)
    assert out["obj_loss_count"].item() == 200
    calls = eng.ops.calls
    score = [c for c in calls if c[0] == "gemm" and c[-1] == EPI_ROWSCORE]
    logits = [c for c in calls if c[0] == "gemm" and c[2] == cfg.num_clusters]
    if fused == "1" and dtype == torch.bfloat16:
        assert len(score) == 1 and score[0][1] == 256 and score[0][2] == 256 and not logits        # M = padded masked rows, not B*V
        assert not [c for c in calls if c[0] == "score_rows"] and [c for c in calls if c[0] == "rowscore_combine"] == [("rowscore_combine", 4, 256, 100)]
    else:
        assert not score and len(logits) == 1 and logits[0][1] == 256
        assert [c for c in calls if c[0] == "score_rows"] == [("score_rows", 256, 100, 100)]
    ref = eng.task_forward("vis_mask", want_grad=False, feat_loss=False)
    assert abs(ref["obj_loss"].item() - out["obj_loss"].item()) < (2e-2 if dtype == torch.bfloat16 else 1e-5)


def test_head_dispatch_word_mask(monkeypatch):
    outs = {}
    for fused in ("1", "0"):
        cfg, eng = bf16_engine("word_mask", fused=fused, monkeypatch=monkeypatch)
        batch = synthetic_batch(cfg, 4, 64, 8, seed=4)
        wl = torch.full((4, 64), -1, dtype=torch.int64)
        wl[:, 1:9] = batch["input_ids"][:, 1:9]
        eng.set_inputs(batch["input_ids"], batch["attention_mask"], None, batch["visual_pos"], cluster_ids=batch["cluster_ids"])
        outs[fused] = eng.evaluate_task("word_mask", word_labels=wl)
        score = [c for c in eng.ops.calls if c[0] == "gemm" and c[-1] == EPI_ROWSCORE]
        assert (len(score) == 1 and score[0][1:3] == (256, 256)) == (fused == "1")          # 100-word vocabulary padded to 256
        assert bool([c for c in eng.ops.calls if c[0] == "score_rows"]) == (fused == "0")
    assert outs["1"]["lm_loss_count"].item() == outs["0"]["lm_loss_count"].item() == int((wl >= 0).sum())
    assert abs(outs["1"]["lm_loss"].item() - outs["0"]["lm_loss"].item()) < 1e-4


# ---------------------------------------------------------------------------------------------- the checks reject injected faults
def fused_case(seed=0, M=256, N=512, K=128, n_real=412, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, K, generator=g) * 0.5).bfloat16()
    Bm = (torch.randn(N, K, generator=g) * 0.5).bfloat16()
    Bm[n_real:] = 0
    bias = torch.randn(N, generator=g) + shift
    bias[n_real:] = -1e30
    labels = torch.randint(0, n_real, (M,), generator=g)
    labels[torch.randperm(M, generator=g)[:M // 10]] = -100
    labels[:6] = torch.tensor([0, 63, 64, 255, 256, n_real - 1])
    pre = A.double() @ Bm.double().t() + bias.double()[None, :]
    e = Bd.rowmax_logit_error(pre, A.double().abs() @ Bm.double().abs().t(), bias.double().abs()[None, :], K)
    return A, Bm, bias, labels, pre, e


def run_fused(ops, A, Bm, bias, labels, n_real, totals):
    M, K = A.shape
    N = Bm.shape[0]
    ws = torch.zeros((N // 64) * M * 4)
    nll, rmax, pred = torch.zeros(M), torch.zeros(M), torch.zeros(M, dtype=torch.int32)
    ops.gemm(A, Bm, None, bias, labels, ws, M, N, K, K, K, N, epilogue=EPI_ROWSCORE)
    ops.rowscore_combine(ws, N // 64, M, labels, n_real, nll, pred, rmax, totals)
    return ws, nll, pred, rmax


def all_checks(ops, shift=0.0, ties=False):
    n_real = 412
    A, Bm, bias, labels, pre, e = fused_case(shift=shift)
    if ties:
        A.zero_(); bias[:n_real] = 0
        pre = A.double() @ Bm.double().t() + bias.double()[None, :]
        e = torch.zeros_like(pre)
    totals = torch.tensor([1.5, 7.0, 3.0, -2.0])
    before = totals.clone()
    ws, nll, pred, rmax = run_fused(ops, A, Bm, bias, labels, n_real, totals)
    BE.check_rowscore_records(ws, pre, e, labels)
    BE.check_rowscore_rows(pre, e, 8, labels, n_real, nll, pred, rmax)
    BE.check_totals(before, totals, labels, n_real, nll, pred)
    mid = totals.clone()
    run_fused(ops, A, Bm, bias, labels, n_real, totals)
    BE.check_totals(mid, totals, labels, n_real, nll, pred, "second launch")
    x = pre[:70, :n_real].float()
    t2 = torch.zeros(4)
    n2, m2, p2 = torch.zeros(70), torch.zeros(70), torch.zeros(70, dtype=torch.int32)
    if ties:
        x = torch.zeros_like(x)
    ops.score_rows(x, 70, n_real, n_real, labels[:70], n2, p2, m2, t2)
    BE.check_score_rows(x.double(), labels[:70], n2, p2, m2)
    BE.check_totals(torch.zeros(4), t2, labels[:70], n_real, n2, p2, "score_rows totals")


@pytest.mark.parametrize("compute", [torch.float32, torch.float64])
def test_restatement_passes_its_own_checks(compute):
    all_checks(EvalFakeOps(torch.bfloat16, compute))
    all_checks(EvalFakeOps(torch.bfloat16, compute), ties=True)
    all_checks(EvalFakeOps(torch.bfloat16, compute), shift=-40.0)


@pytest.mark.parametrize("fault", FAULTS)
def test_checks_reject_injected_faults(fault):
    """one fault at a time; each must be caught on at least one of the cases (random logits, exact ties, all real logits negative:
    the case in which a pad column's bare 0 would win)"""
    caught = 0
    for kw in ({}, {"ties": True}, {"shift": -40.0}):
        try:
            all_checks(EvalFakeOps(torch.bfloat16, torch.float32, fault=fault), **kw)
        except AssertionError:
            caught += 1
    assert caught >= 1, fault
    assert set(FAULTS) >= {"label_neighbour", "tie_high", "ignored_counted", "pad_wins", "correct_ignored", "totals_overwrite"}
