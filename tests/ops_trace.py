"""TEST INFRASTRUCTURE: a recording proxy over the fake ops and the two scenario sets whose library-call traces are pinned:
scenarios() -- the sampler loops and the two big heads' validation (tests/test_sampler_call_trace_cpu.py, tests/golden/
sampler_call_trace.json) -- and engine_scenarios() -- the training steps, the nn.Module entry points and the rest of the validation
pass (tests/test_engine_call_trace_cpu.py, tests/golden/engine_call_trace.json).  tools/sampler_call_trace.py prints either in full.

A trace line is one `ops` call of the engine: the method name, every int / float / bool / str argument by value, every tensor
argument by dtype only (None stays None); keyword arguments carry their names.  Calls the fake ops make among themselves are not
the engine's and are not recorded.  The proxy forwards everything else (hasattr included: the engine gates on it)."""
import contextlib
import hashlib
import os
from collections import Counter

import torch

import lxmert_oracle as O
from _util import golden_cfg, load_golden
from fake_ops_eval import EvalFakeOps
from fake_ops_inpaint import InpaintFakeOps
from xlxmert_amd.config import XLxmertConfig
from xlxmert_amd.engine import Engine
from xlxmert_amd.params import ParamStore


def _canon(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    if isinstance(v, torch.Tensor):
        return str(v.dtype)
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(_canon(x) for x in v) + "]"
    return "<" + type(v).__name__ + ">"


class RecordingOps:
    """forwards every attribute to `inner`; calls of its methods are appended to `trace` first"""

    def __init__(self, inner):
        object.__setattr__(self, "inner", inner)
        object.__setattr__(self, "trace", [])

    def __getattr__(self, name):
        attr = getattr(self.inner, name)                           # AttributeError for what the inner ops do not have
        if not callable(attr):
            return attr

        def call(*args, **kw):
            parts = [_canon(a) for a in args] + [f"{k}={_canon(v)}" for k, v in sorted(kw.items())]
            self.trace.append(f"{name}({', '.join(parts)})")
            return attr(*args, **kw)
        return call

    def __setattr__(self, name, value):
        setattr(self.inner, name, value)


def summary(trace):
    """what the golden file keeps of one scenario's trace"""
    return {"calls": len(trace), "methods": dict(sorted(Counter(line.split("(", 1)[0] for line in trace).items())),
            "sha256": hashlib.sha256("\n".join(trace).encode()).hexdigest()}


@contextlib.contextmanager
def env(**switches):
    """environment switches for the duration of a scenario; nothing is left in os.environ"""
    old = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def fused_env(value):
    return env(XL_FUSED_PREDICT=value)


CFG_KEYS = ("vocab_size", "hidden_size", "num_attention_heads", "intermediate_size", "max_position_embeddings", "type_vocab_size",
            "l_layers", "x_layers", "r_layers", "visual_feat_dim", "visual_pos_dim", "num_clusters")
SAMPLING = {"greedy": {}, "temperature": dict(temperature=0.7, seed=3), "top_k": dict(top_k=5, seed=3)}
WORD_SAMPLING = {"greedy": {}, "temperature": dict(temperature=0.7, seed=3), "top_p": dict(top_p=0.9, seed=3)}
# (dtype, XL_FUSED_PREDICT): fp32 never fuses, bf16 at B*V = 256 does unless switched off
VARIANTS = {"fp32": (torch.float32, "1"), "bf16_fused": (torch.bfloat16, "1"), "bf16_unfused": (torch.bfloat16, "0")}


def image_engine(dtype):
    """the B*V = 256 engine of test_truncation_cpu: bf16 reaches the fused predict path"""
    g = load_golden("sampler_tiny")
    oc = golden_cfg(g)
    cfg = XLxmertConfig(**{k: getattr(oc, k) for k in CFG_KEYS})
    B, L, grid = 4, 8, 8
    ids = torch.from_numpy(g["in_input_ids"])[:1].expand(B, -1).clone()
    pos = torch.from_numpy(O.box_position(grid)).unsqueeze(0).expand(B, -1, -1)
    store = ParamStore(cfg, "cpu", dtype, task="vis_mask")
    store.load_named(O.make_state_dict(oc, int(g["seed"])))
    eng = Engine(cfg, store, RecordingOps(InpaintFakeOps(dtype)), B, L, grid * grid, need_lang=False)
    eng.sync_compute_weights()
    eng.set_inputs(ids, ids > 0, None, pos, cluster_ids=torch.zeros(B, grid * grid, dtype=torch.long),
                   vis_mask=torch.ones(B, grid * grid, dtype=torch.bool))
    return eng


def caption_engine(dtype, packed):
    """the five ragged captions of test_caption_cpu: packed bf16 rows round up to 256 = the fused predict path"""
    import test_caption_cpu as C
    cfg, oc, sd = C.tiny_model()
    lengths = C.lengths_for(0)
    cid, feats, pos = C.picture(oc, sd, C.B_)
    eng = C.make_caption_engine(RecordingOps(InpaintFakeOps(dtype)), cfg, sd, lengths, (), cid, feats, pos, dtype=dtype, pack_lang=packed)
    assert eng.packed == packed
    return eng, lengths, dict(mask_token_id=C.MASK, banned_ids=C.BANNED)


def eval_engine(task, dtype):
    """test_eval_cpu's dispatch geometry, 8 x (64 + 64) rows: the fused scoring path at 512 rows and at a 256-row list"""
    from test_trainer_cpu import TINY, oracle_cfg
    from xlxmert_amd.trainer import synthetic_batch
    B, L, V = 8, 64, 64
    cfg = XLxmertConfig(**dict(TINY, max_position_embeddings=64, num_clusters=100))
    store = ParamStore(cfg, "cpu", dtype, task=task)
    store.load_named(O.make_cls_state_dict(oracle_cfg(cfg), 5) if task != "vis_mask" else O.make_state_dict(oracle_cfg(cfg), 5))
    eng = Engine(cfg, store, RecordingOps(EvalFakeOps(dtype)), B, L, V, need_lang=task != "vis_mask", pack_lang=False)
    eng.sync_compute_weights()
    return eng, synthetic_batch(cfg, B, L, 8, seed=3)


def _image(kind, variant, sampling, **kw):
    dtype, env = VARIANTS[variant]

    def run():
        with fused_env(env):
            eng = image_engine(dtype)
            B, V = eng.B, eng.V
            if kind == "nar":
                eng.sample_codes_nar(2, **SAMPLING[sampling])
            elif kind == "ar":
                eng.sample_codes_ar(3, kw["mode"], positions=[5, 17, 40] if kw["mode"] == "random" else None, **SAMPLING[sampling])
            else:
                gen = torch.Generator().manual_seed(2)
                free = torch.rand(B, V, generator=gen) < 0.5
                init = torch.randint(0, eng.K, (B, V), generator=gen)
                eng.inpaint_codes(init, free, kw["n_steps"], kw["mode"], **SAMPLING[sampling])
        return eng.ops.trace
    return run


def _words(variant, packed, sampling):
    dtype, env = VARIANTS[variant]

    def run():
        with fused_env(env):
            eng, lengths, kw = caption_engine(dtype, packed)
            eng.sample_words_nar(lengths, 2, 0, **kw, **WORD_SAMPLING[sampling])
        return eng.ops.trace
    return run


def _evaluate(task, variant, rows):
    dtype, env = VARIANTS[variant]

    def run():
        with fused_env(env):
            eng, batch = eval_engine(task, dtype)
            B, L, V = eng.B, eng.L, eng.V
            if task == "vis_mask":
                vm = torch.ones(B, V, dtype=torch.bool)
                if rows:                                           # 200 masked rows -> a row list padded to 256
                    vm.zero_()
                    vm.view(-1)[torch.randperm(B * V, generator=torch.Generator().manual_seed(1))[:200]] = True
                labels = batch["cluster_ids"].clone()
                labels[~vm] = -100
                eng.set_inputs(batch["input_ids"], batch["attention_mask"], None, batch["visual_pos"], cluster_ids=batch["cluster_ids"],
                               vis_mask=vm, obj_labels=labels)
                eng.evaluate_task("vis_mask")
            else:
                wl = torch.full((B, L), -1, dtype=torch.int64)
                wl[:, 1:9] = batch["input_ids"][:, 1:9]
                eng.set_inputs(batch["input_ids"], batch["attention_mask"], None, batch["visual_pos"], cluster_ids=batch["cluster_ids"])
                eng.evaluate_task("word_mask", word_labels=wl, word_rows=(wl.view(-1) >= 0).nonzero().view(-1) if rows else None)
        return eng.ops.trace
    return run


def scenarios():
    """{name: callable returning the trace}: every mode of every sampler loop and of the two big heads' validation"""
    out = {}
    for v in VARIANTS:
        for s in SAMPLING:
            out[f"nar/{v}/{s}"] = _image("nar", v, s)
            for mode in ("confidence", "tlbr", "random"):
                out[f"ar/{mode}/{v}/{s}"] = _image("ar", v, s, mode=mode)
            out[f"inpaint/nar/{v}/{s}"] = _image("inpaint", v, s, mode="nar", n_steps=2)
            out[f"inpaint/confidence/{v}/{s}"] = _image("inpaint", v, s, mode="confidence", n_steps=3)
        for packed in (False, True):
            for s in WORD_SAMPLING:
                out[f"words/{'packed' if packed else 'dense'}/{v}/{s}"] = _words(v, packed, s)
        for task in ("vis_mask", "word_mask"):
            for rows in (False, True):
                out[f"evaluate/{task}/{'rows' if rows else 'all'}/{v}"] = _evaluate(task, v, rows)
    return out


# ---------------------------------------------------------------- engine_scenarios(): training steps, nn.Module entry points, validation
# (compute dtype, packed language rows, dropout, residual stream)
ENGINE_VARIANTS = {"fp32/dense": (torch.float32, False, False, "bf16"),
                   "bf16/packed/drop": (torch.bfloat16, True, True, "bf16"),
                   "bf16/packed/drop/res32": (torch.bfloat16, True, True, "fp32")}
# the switches an Engine reads when it is built, at their defaults: a scenario overrides what it is about
ENGINE_ENV = dict(XL_COMPACT_HEAD="1", XL_COMPACT_LAST_FFN="1", XL_PAIR_BLOCKS="0", XL_PAIR_SIDE="0")
TINY_B, TINY_L, TINY_GRID = 4, 8, 4
# Row-list granule of the scenarios, set on the engine after it is built (the language row capacity MLc keeps the 256 it was sized
# with): 22 masked rows -> 24 of 64, so the row-subset paths run at this size.  Production uses 256, at which a 64-row batch pads up to
# all rows and no row subset would exist: the pinned traces cover the code paths, not a granule that is deployed.
TINY_ROW_PAD = 8
NUM_QA = 9


def fake_ops_for(dtype, res32, evaluate=False):
    from fake_ops import FakeOps
    from fake_ops_res import FakeOpsRes
    return EvalFakeOps(dtype) if evaluate else FakeOpsRes(dtype) if res32 else FakeOps(dtype)


def tiny_engine(task, variant, qa=False, need_lang=None, evaluate=False, make_ops=fake_ops_for, device="cpu", wrap=None):
    """the smallest engine that still takes every branch: test_trainer_cpu.TINY, B=4, L=8, V=16, row lists padded to 8.
    task: the store's task; qa: a task_qa store (NUM_QA answers).  Returns (engine, batch on `device`).
    make_ops / device / wrap (here and in the scenario callables): nothing in the repository passes them; they let the same scenarios
    run over HipOps on a device under a recorder that also renders streams (profiles/engine_split/gpu_trace_equivalence.txt).
    wrap=None is this module's RecordingOps AS BOUND WHEN THE SCENARIO RUNS: tests/test_stream_audit_cpu.py puts an access-checking
    proxy under it for every scenario, also those that take no keyword."""
    from test_trainer_cpu import TINY, oracle_cfg
    wrap = wrap or RecordingOps
    from xlxmert_amd.trainer import synthetic_batch
    dtype, packed, drop, residual = ENGINE_VARIANTS[variant]
    cfg = XLxmertConfig(**dict(TINY, max_position_embeddings=64, num_clusters=100))
    oc = oracle_cfg(cfg)
    store = ParamStore(cfg, device, dtype, task=task, num_answers=NUM_QA if qa else 0)
    store.load_named(O.make_qa_state_dict(oc, NUM_QA, 5) if qa else O.make_cls_state_dict(oc, 5))
    res32 = residual == "fp32" and dtype == torch.bfloat16
    need_lang = (task != "vis_mask" or qa) if need_lang is None else need_lang
    eng = Engine(cfg, store, wrap(make_ops(dtype, res32, evaluate)), TINY_B, TINY_L, TINY_GRID * TINY_GRID, need_lang=need_lang,
                 train_dropout=drop, pack_lang=packed, residual_dtype=residual)
    eng.ROW_PAD = TINY_ROW_PAD
    eng.sync_compute_weights()
    eng.set_step_seed(11)
    batch = synthetic_batch(cfg, TINY_B, TINY_L, TINY_GRID, seed=3, device=device)
    batch["qa_labels"] = O.make_qa_labels(NUM_QA, TINY_B, 3).to(device) if qa else None
    return eng, batch


def stage(eng, batch, task, all_ones=False, word_rows=True):
    """set_inputs for one task; returns the task's keyword arguments of task_forward / evaluate_task"""
    from xlxmert_amd.trainer import random_word_batch, word_order_of, word_rows_of
    B, L, V = eng.B, eng.L, eng.V
    base = dict(attention_mask=batch["attention_mask"], token_type_ids=batch["token_type_ids"], visual_pos=batch["visual_pos"],
                cluster_ids=batch["cluster_ids"], lang_rows=batch["lang_rows"], lang_off=batch["lang_off"])
    kw = {"qa_labels": batch["qa_labels"]}
    if task == "vis_mask":
        vm = torch.ones(B, V, dtype=torch.bool, device=batch["cluster_ids"].device)
        if not all_ones:                                       # every third flat position: 22 of 64 rows
            vm.zero_()
            vm.view(-1)[::3] = True
        labels = batch["cluster_ids"].clone()
        labels[~vm] = -100
        eng.set_inputs(batch["input_ids"], vis_mask=vm, obj_labels=labels, word_order=batch["word_order"], **base)
    elif task == "word_mask":
        ids, wl = random_word_batch(batch["input_ids"].cpu(), mask_token_id=min(103, eng.cfg.vocab_size - 3),
                                    vocab_size=eng.cfg.vocab_size, mlm_probability=0.3, generator=torch.Generator().manual_seed(4))
        assert 0 < int((wl >= 0).sum()) < B * L
        eng.set_inputs(ids.to(eng.dev), word_order=word_order_of(ids).to(eng.dev), **base)
        kw.update(word_labels=wl.to(eng.dev), word_rows=word_rows_of(wl) if word_rows else None)
    else:
        eng.set_inputs(batch["input_ids"], word_order=batch["word_order"], **base)
        if task == "matched":
            kw["matched_labels"] = (torch.arange(B, device=eng.dev) % 2).to(torch.int64)
    return kw


def _step(task, variant, qa=False, switches=None, **stage_kw):
    def run(**engine_kw):
        with env(**dict(ENGINE_ENV, **(switches or {}))):
            eng, batch = tiny_engine(task, variant, qa=qa, **engine_kw)
            kw = stage(eng, batch, task, **stage_kw)
            if task == "vis_mask":
                eng.vis_mask_forward_backward(qa_labels=kw["qa_labels"])
            else:
                eng._task_step(task, **kw)
        return eng.ops.trace
    return run


def _finetune(task, dtype):
    def run(make_ops=fake_ops_for, device="cpu", wrap=None):
        import test_engine_cpu as E
        wrap = wrap or RecordingOps
        make = E.make_vqa_engine if task == "vqa" else E.make_nlvr2_engine
        with env(**ENGINE_ENV):
            eng, inp = make(load_golden(task + "_tiny"), wrap(make_ops(dtype, False, False)), device=device, dtype=dtype)
            if task == "vqa":
                eng.vqa_forward_backward(inp["targets"].to(device))
            else:
                eng.nlvr2_forward_backward(inp["labels"].to(device))
        return eng.ops.trace
    return run


def _backward_from_outputs(which, variant):
    def run():
        with env(**ENGINE_ENV):
            eng, batch = tiny_engine("all", variant, need_lang=True)
            stage(eng, batch, "matched")
            eng.encoder_forward()
            gen = torch.Generator().manual_seed(6)
            grads = {"d_lang": torch.randn(eng.MLd, eng.d, generator=gen), "d_vis": torch.randn(eng.MV, eng.d, generator=gen),
                     "d_pooled": torch.randn(eng.B, eng.d, generator=gen)}
            eng.backward_from_outputs(**{k: v for k, v in grads.items() if which in (k, "all")})
        return eng.ops.trace
    return run


def _head_forward(want_logits):
    def run():
        with env(**ENGINE_ENV):
            eng, batch = tiny_engine("all", "fp32/dense", need_lang=True)
            stage(eng, batch, "vis_mask")
            eng.encoder_forward()
            eng.head_forward(want_logits=want_logits)
        return eng.ops.trace
    return run


def _evaluate_small(task, variant_or_dtype):
    def run():
        import test_engine_cpu as E
        with env(**ENGINE_ENV):
            if task == "vqa":
                eng, inp = E.make_vqa_engine(load_golden("vqa_tiny"), RecordingOps(EvalFakeOps(variant_or_dtype)), dtype=variant_or_dtype)
                eng.evaluate_task("vqa", targets=inp["targets"])
            elif task == "nlvr2":
                eng, inp = E.make_nlvr2_engine(load_golden("nlvr2_tiny"), RecordingOps(EvalFakeOps(variant_or_dtype)), dtype=variant_or_dtype)
                eng.evaluate_task("nlvr2", labels=inp["labels"])
            else:
                eng, batch = tiny_engine(task, variant_or_dtype, qa=task == "qa", evaluate=True)
                eng.evaluate_task(task, **stage(eng, batch, task))
        return eng.ops.trace
    return run


STEP_TASKS = ("vis_mask", "word_mask", "matched")


def engine_scenarios():
    """{name: callable returning the trace}: every training step, nn.Module entry point and small-head validation of the engine"""
    out = {}
    for v in ENGINE_VARIANTS:
        for task in STEP_TASKS:
            out[f"step/{task}/{v}"] = _step(task, v)
    for v in ("fp32/dense", "bf16/packed/drop"):
        for task in STEP_TASKS + ("qa",):
            out[f"step/{task}/qa_store/{v}"] = _step(task, v, qa=True)
        out[f"step/vis_mask/compact_head_off/{v}"] = _step("vis_mask", v, switches={"XL_COMPACT_HEAD": "0"})
        out[f"step/vis_mask/compact_last_ffn_off/{v}"] = _step("vis_mask", v, switches={"XL_COMPACT_LAST_FFN": "0"})
        out[f"step/vis_mask/all_ones/{v}"] = _step("vis_mask", v, all_ones=True)
        out[f"step/word_mask/no_rows/{v}"] = _step("word_mask", v, word_rows=False)
        for task in ("matched", "qa"):
            out[f"evaluate/{task}/{v}"] = _evaluate_small(task, v)
    out["step/vis_mask/pair_blocks/fp32/dense"] = _step("vis_mask", "fp32/dense", switches={"XL_PAIR_BLOCKS": "1"})
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        for task in ("vqa", "nlvr2"):
            out[f"step/{task}/{name}"] = _finetune(task, dtype)
            out[f"evaluate/{task}/{name}"] = _evaluate_small(task, dtype)
    for v in ("fp32/dense", "bf16/packed/drop/res32"):
        for which in ("d_lang", "d_vis", "d_pooled", "all"):
            out[f"module/backward_from_outputs/{which}/{v}"] = _backward_from_outputs(which, v)
    for want in (True, False):
        out[f"module/head_forward/{'logits' if want else 'no_logits'}/fp32/dense"] = _head_forward(want)
    return out
