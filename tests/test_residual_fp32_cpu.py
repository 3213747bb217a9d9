"""The fp32 residual stream of the bf16 path (Engine residual_dtype="fp32"), checked on the CPU: the real
Engine over the host restatement of the kernels (tests/fake_ops_res.FakeOpsRes in bf16 storage) against the exact-fp32 oracle, next
to the oracle's own storage-precision emulation (lxmert_oracle.EMU "bf16" / "bf16_fp32res")."""
import math

import pytest
import torch

import lxmert_oracle as O
from _util import golden_cfg, golden_inputs, load_golden, maxdiff
from fake_ops_res import FakeOpsRes
from test_precision_emulation_cpu import _errors, _grads
from xlxmert_amd.config import XLxmertConfig
from xlxmert_amd.engine import Engine
from xlxmert_amd.params import ParamStore

CFG_KEYS = ("vocab_size", "hidden_size", "num_attention_heads", "intermediate_size", "max_position_embeddings",
            "type_vocab_size", "l_layers", "x_layers", "r_layers", "visual_feat_dim", "visual_pos_dim", "num_clusters")


def _rms(rel):
    return math.sqrt(sum(v * v for v in rel.values()) / len(rel))


def engine_grads(oc, sd, inp, residual_dtype, device="cpu", ops=None):
    """every gradient of one vis_mask step of the real Engine (bf16 compute, dropout off), as float64 on the CPU"""
    cfg = XLxmertConfig(**{k: getattr(oc, k) for k in CFG_KEYS})
    B, L = inp["input_ids"].shape
    V = inp["cluster_ids"].shape[1]
    store = ParamStore(cfg, device, torch.bfloat16, task="vis_mask")
    store.load_named(sd)
    ops = ops if ops is not None else FakeOpsRes(torch.bfloat16)
    eng = Engine(cfg, store, ops, B, L, V, need_lang=False, residual_dtype=residual_dtype)
    eng.sync_compute_weights()
    t = {k: v.to(device) for k, v in inp.items()}
    rows = (inp["vis_mask"].reshape(-1) != 0).nonzero().reshape(-1)
    eng.set_inputs(t["input_ids"], t["attention_mask"], t["token_type_ids"], t["visual_pos"], cluster_ids=t["cluster_ids"],
                   vis_mask=t["vis_mask"], obj_labels=t["obj_labels"], masked_rows=rows)
    losses = eng.vis_mask_forward_backward()
    if device != "cpu":
        torch.cuda.synchronize()
    return eng, float(losses[:2].sum()), {k: store.gview(k).double().cpu().reshape(-1) for k in store.index}


def stream_criterion(oc, sd, inp, run):
    """the criterion of the mode, shared with the device test: run(residual_dtype) -> {name: gradient}.  Prints every figure."""
    torch.manual_seed(0)
    loss0, ref = _grads(None, oc, sd, inp)
    _, gb = _grads("bf16", oc, sd, inp)
    _, gr = _grads("bf16_fp32res", oc, sd, inp)
    ref = {k: v.reshape(-1) for k, v in ref.items()}
    emu_b, _, emu_wb, _ = _errors({k: v.reshape(-1) for k, v in gb.items()}, ref)
    emu_r, _, emu_wr, _ = _errors({k: v.reshape(-1) for k, v in gr.items()}, ref)
    r_emu = _rms(emu_r) / _rms(emu_b)
    eb, er = run("bf16"), run("fp32")
    missing = [k for k in ref if k not in eb]
    assert not missing, missing
    rel_b, worst_b, wb, _ = _errors(eb, ref)
    rel_r, worst_r, wr, _ = _errors(er, ref)
    rms_b, rms_r = _rms(rel_b), _rms(rel_r)
    limit = (1 + r_emu) / 2
    print(f"oracle emulation   : rms bf16 {_rms(emu_b):.5f} -> fp32 stream {_rms(emu_r):.5f} (ratio r_emu {r_emu:.3f}); worst tensor "
          f"{emu_wb:.4f} -> {emu_wr:.4f}; {len(emu_b)} tensors")
    print(f"engine             : rms bf16 {rms_b:.5f} -> fp32 stream {rms_r:.5f} (ratio {rms_r / rms_b:.3f}, required <= {limit:.3f}, "
          f"i.e. rms <= {limit * rms_b:.5f}); worst tensor {worst_b} {wb:.4f} -> {worst_r} {wr:.4f}")
    assert len(rel_b) == len(rel_r) >= 150
    assert rms_r / rms_b <= limit, (rms_r, rms_b, limit)
    assert wr <= wb, (worst_r, wr, worst_b, wb)
    return dict(r_emu=r_emu, rms_b=rms_b, rms_r=rms_r, worst_b=wb, worst_r=wr)


def test_fp32_stream_engine_realises_half_of_the_emulated_improvement():
    """full architecture (9/5/5, d 768, 10k codebook), B 4, ragged text: every gradient of the engine in both modes against the
    exact-fp32 oracle (relative L2 per tensor, rms over tensors).  r_emu = what the oracle's storage emulation predicts for the
    fp32 stream (rms ratio, ~0.68); the engine must realise at least half of that improvement, and its worst tensor must not get
    worse.  The half is the margin for what the emulation does not model (summation order, the attention's internal roundings)."""
    torch.set_num_threads(8)
    oc = O.OracleConfig()
    sd = O.make_state_dict(oc, 7)
    inp = O.make_inputs(oc, 11, 4, 20, 8)
    stream_criterion(oc, sd, inp, lambda mode: engine_grads(oc, sd, inp, mode)[2])


def _tiny(dtype, residual_dtype, ops=None, **env):
    g = load_golden("tiny_222")
    oc = golden_cfg(g)
    cfg = XLxmertConfig(**{k: getattr(oc, k) for k in CFG_KEYS})
    sd = O.make_state_dict(oc, int(g["seed"]))
    inp = golden_inputs(g)
    B, L = inp["input_ids"].shape
    V = inp["cluster_ids"].shape[1]
    store = ParamStore(cfg, "cpu", dtype, task="vis_mask")
    store.load_named(sd)
    eng = Engine(cfg, store, ops if ops is not None else FakeOpsRes(dtype), B, L, V, need_lang=False, residual_dtype=residual_dtype)
    eng.ROW_PAD = 1
    eng.sync_compute_weights()
    eng.set_inputs(inp["input_ids"], inp["attention_mask"], inp["token_type_ids"], inp["visual_pos"],
                   cluster_ids=inp["cluster_ids"], vis_mask=inp["vis_mask"], obj_labels=inp["obj_labels"])
    return eng, cfg


def _stream_tensors(eng):
    out = [eng.emb_y, eng.vis0, eng.GA, eng.GB] + eng.lang_mid + eng.lang_out + eng.vis_mid + eng.vis_out + eng.X + eng.XY + eng.XS
    out += [blk.z for pair in eng.lang_layers + eng.vis_layers for blk in pair]
    for b in eng.x_layers:
        out += [b[k].z for k in ("cross", "sa_v", "ffn_v", "sa_l", "ffn_l") if k in b]
    return out


def test_bf16_mode_allocates_no_fp32_stream_and_calls_nothing_new():
    eng, cfg = _tiny(torch.bfloat16, None)
    assert eng.residual_dtype == "bf16" and not eng.res32
    eng.vis_mask_forward_backward()
    assert all(isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 for t in _stream_tensors(eng))
    assert eng.emb_pre32 is None and eng.xv32 is None
    assert all(t.dtype == torch.bfloat16 for t in eng._tmp.values())
    called = {c[0] for c in eng.ops.calls}
    assert not called & set(FakeOpsRes.NEW_METHODS), called
    res = [c for c in eng.ops.calls if c[0] == "gemm_residual"]
    assert res and all(c[1:4] == (torch.bfloat16, torch.bfloat16, False) for c in res)
    # the same geometry in fp32-stream mode needs more activation memory; the default needs none of it
    eng32, _ = _tiny(torch.bfloat16, "fp32")
    assert eng32.act_bytes > eng.act_bytes


def test_fp32_mode_routes_every_residual_epilogue_and_chain_layernorm_through_the_fp32_stream():
    eng, cfg = _tiny(torch.bfloat16, "fp32")
    assert eng.res32
    eng.vis_mask_forward_backward()
    calls = eng.ops.calls
    # every residual epilogue of the encoder (N = d); the one other XL_EPI_RESIDUAL launch of the step adds d(feat) of the feature
    # loss inside the codebook head (N = F): not a stream value, bf16 as before
    assert cfg.visual_feat_dim != cfg.hidden_size
    res = [c for c in calls if c[0] == "gemm_residual" and c[4] == cfg.hidden_size]
    assert res and all(c[1:4] == (torch.float32, torch.float32, True) for c in res), res
    other = [c for c in calls if c[0] == "gemm_residual" and c[4] != cfg.hidden_size]
    assert other == [("gemm_residual", torch.bfloat16, torch.bfloat16, False, cfg.visual_feat_dim)], other
    n_blocks = 2 * (cfg.l_layers + cfg.r_layers) + sum(
        sum(1 for k in ("cross", "sa_v", "ffn_v", "sa_l", "ffn_l") if k in b) for b in eng.x_layers)
    # forward: every block's LayerNorm + the embeddings' through the dual-output entry point; the plain one only in the head's
    # transform (not a stream value).  backward: every block's + the embeddings' through the fp32 one, the head's plain.
    assert sum(1 for c in calls if c[0] == "layernorm_fwd_res") == n_blocks + 1
    assert sum(1 for c in calls if c[0] == "layernorm_fwd") == 1
    assert sum(1 for c in calls if c[0] == "layernorm_bwd_res") == n_blocks + 1
    assert sum(1 for c in calls if c[0] == "layernorm_bwd") == 1
    for t in _stream_tensors(eng):
        f = t.f if hasattr(t, "f") else t
        assert f.dtype == torch.float32
    lang, vis = eng.hidden_states()
    assert all(t.dtype == torch.float32 for t in lang + vis)
    # the bf16 copy of a stream value is the rounding of its fp32 value
    for t in eng.X + eng.XY + eng.XS:
        assert torch.equal(t.h, t.f.to(torch.bfloat16))


def test_switch_changes_nothing_with_fp32_compute():
    out = {}
    for mode in ("bf16", "fp32"):
        eng, _ = _tiny(torch.float32, mode)
        assert not eng.res32
        losses = eng.vis_mask_forward_backward()
        out[mode] = (losses.clone(), eng.store.grad.clone())
        assert not {c[0] for c in eng.ops.calls} & set(FakeOpsRes.NEW_METHODS)
    assert torch.equal(out["bf16"][0], out["fp32"][0]) and torch.equal(out["bf16"][1], out["fp32"][1])


def test_unknown_value_and_unsupported_switch_raise(monkeypatch):
    with pytest.raises(ValueError, match="residual_dtype"):
        _tiny(torch.bfloat16, "fp16")
    monkeypatch.setenv("XL_RESIDUAL", "float32")
    with pytest.raises(ValueError, match="XL_RESIDUAL"):
        _tiny(torch.bfloat16, None)
    monkeypatch.setenv("XL_RESIDUAL", "fp32")
    assert _tiny(torch.bfloat16, None)[0].res32                   # the environment selects the mode when the keyword is unset
    assert not _tiny(torch.bfloat16, "bf16")[0].res32             # ... and the keyword wins
    monkeypatch.setenv("XL_PAIR_BLOCKS", "1")
    with pytest.raises(ValueError, match="XL_PAIR_BLOCKS"):
        _tiny(torch.bfloat16, "fp32")
    assert _tiny(torch.bfloat16, "bf16")[0].pair_blocks           # (still available in the default mode)


TINY = dict(vocab_size=60, hidden_size=64, num_attention_heads=4, intermediate_size=128, max_position_embeddings=32, l_layers=2,
            x_layers=2, r_layers=2, visual_feat_dim=32, num_clusters=24)


@pytest.mark.parametrize("source", ["keyword", "env"])
def test_pretrain_step_runs_every_task_in_fp32_stream_mode(source, monkeypatch):
    """PretrainStep(residual_dtype="fp32") / XL_RESIDUAL=fp32 over the host restatement, dropout on: two optimizer steps of
    vis_mask, one each of word_mask, matched and vqa -- finite losses, a changed parameter vector, the fp32-stream entry points called"""
    from xlxmert_amd.trainer import PretrainStep, synthetic_batch
    cfg = XLxmertConfig(**TINY)
    oc = O.OracleConfig(**{k: getattr(cfg, k) for k in CFG_KEYS})
    B, L, grid, A = 4, 10, 4, 7
    kw = {"residual_dtype": "fp32"} if source == "keyword" else {}
    if source == "env":
        monkeypatch.setenv("XL_RESIDUAL", "fp32")
    for task, steps in (("vis_mask", 2), ("word_mask", 1), ("matched", 1), ("vqa", 1)):
        store = ParamStore(cfg, "cpu", torch.bfloat16, task=task, num_answers=A if task == "vqa" else 0)
        store.load_named(O.make_vqa_state_dict(oc, A, 5) if task == "vqa" else O.make_state_dict(oc, 5) if task == "vis_mask"
                         else O.make_cls_state_dict(oc, 5))
        tr = PretrainStep(cfg, B, L, grid * grid, dtype=torch.bfloat16, device="cpu", lr=1e-3, total_steps=10, task=task, plan=False,
                          train_dropout=True, ops=FakeOpsRes(torch.bfloat16), store=store, num_answers=A if task == "vqa" else 0, **kw)
        assert tr.engine.res32
        p0 = tr.store.master.clone()
        for i in range(steps):
            if task == "vqa":
                batch = O.make_vqa_inputs(oc, A, 600 + i, B, L, grid)
            else:
                batch = synthetic_batch(cfg, B, L, grid, seed=3 + i)
                if task in ("word_mask", "matched"):
                    wl, ml = O.make_lang_task_labels(oc, batch["input_ids"], 800 + i)
                    batch.update(word_labels=wl, matched_labels=ml)
            losses = tr.step(batch)
            assert all(torch.isfinite(torch.as_tensor(x)).all() for x in losses if x is not None), (task, losses)
        assert not torch.equal(p0, tr.store.master), task
        assert {c[0] for c in tr.ops.calls} >= set(FakeOpsRes.NEW_METHODS), task
