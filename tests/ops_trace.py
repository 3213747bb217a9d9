"""TEST INFRASTRUCTURE: a recording proxy over the fake ops and the sampler / validation scenarios whose library-call traces
tests/test_sampler_call_trace_cpu.py pins (tests/golden/sampler_call_trace.json) and tools/sampler_call_trace.py prints in full.

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
def fused_env(value):
    old = os.environ.get("XL_FUSED_PREDICT")
    os.environ["XL_FUSED_PREDICT"] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ["XL_FUSED_PREDICT"]
        else:
            os.environ["XL_FUSED_PREDICT"] = old


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
