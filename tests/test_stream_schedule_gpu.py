"""Happens-before audit of the multi-stream schedule on the device.  Each scenario runs ONCE, exactly as it runs without the audit
(tests/stream_trace.py forwards every call unchanged and never synchronises); the recorded launches, accesses and ordering events
are then analysed on the host (tests/stream_audit.py):
  - the unmodified trace has no pair of conflicting accesses on two streams without a happens-before path;
  - the audit is not blind: for every ordered pair of streams (a -> b) with an ordering edge, deleting all a -> b edges FROM THE MODEL
    produces a conflict, and every stream of the trace appears in such a pair;
  - every single edge (one per call site and stream pair) is classified needed / implied -- reported, not asserted.
Nothing is removed from what the device executes.  The report blocks printed here are kept in profiles/stream_audit.txt."""
import time
from collections import Counter

import pytest
import torch

import stream_audit as SA
import stream_trace as ST

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16
B, L, GRID = 8, 20, 8
V = GRID * GRID
NQ = 9


def tiny_cfg(layers=(2, 2, 2)):
    from xlxmert_amd.config import XLxmertConfig
    return XLxmertConfig(vocab_size=200, hidden_size=128, num_attention_heads=2, intermediate_size=256, max_position_embeddings=32,
                         visual_feat_dim=64, num_clusters=96, l_layers=layers[0], x_layers=layers[1], r_layers=layers[2])


@pytest.fixture(autouse=True)
def _process_streams_reserved():
    """the engine's side streams are created and first used once per process (engine.reserve_streams, a host synchronisation behind
    it): process set-up, whichever scenario comes first, not part of any scenario's schedule"""
    from xlxmert_amd.engine import reserve_streams
    reserve_streams(DEV)


class Audit:
    """one traced scenario: `with Audit(monkeypatch) as au:` runs the body under the tracer; au.check(...) analyses"""

    def __init__(self, monkeypatch):
        self.tracer = ST.Tracer()
        self.tracer.patch_torch_ordering(monkeypatch)
        self.tracer.patch_plans(monkeypatch)
        self.mode = ST.TorchOps(self.tracer)

    def ops(self, dtype=BF):
        return ST.tracing_hipops(dtype, self.tracer)

    def mark(self, label):
        self.tracer.trace.mark(label)

    def __enter__(self):
        self.t0 = time.time()
        self.mode.__enter__()
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
        self.mode.__exit__(*exc)
        self.t_trace = time.time() - self.t0
        return False

    # ---- analysis
    def scratch_reused(self, eng):
        """a backward-scratch tensor (Engine.tmp) written by a chain stream, read by a companion stream, written again by a chain
        stream -- inside one step (between two marks)"""
        scratch = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in eng._tmp.values())
        companions = {s.cuda_stream for s in eng._dw.values()}
        state, found = {}, 0
        for ev in self.tracer.trace.events:
            if isinstance(ev, SA.Mark):
                state = {}
            if not isinstance(ev, SA.Launch):
                continue
            for region, mode, _ in ev.accesses:
                lo, hi = SA.bounds(region)
                for slo, shi in scratch:
                    if slo <= lo and hi <= shi:
                        st = state.get(slo, 0)
                        if ev.stream in companions:
                            if st == 1 and mode == "r":
                                state[slo] = 2
                        elif mode in ("w", "rw"):
                            if st == 2:
                                found += 1
                            state[slo] = 1
                        break
        return found

    def check(self, name, single_stream_ok=False):
        tr = self.tracer
        trace = tr.trace
        t0 = time.time()
        rep = SA.analyse(trace)
        edges = SA.edges(trace)
        device_edges = [e for e in edges if e.kind != "host_sync"]
        lines = [f"== {name}", f"launches {tr.n_abi} through the C ABI + {tr.n_torch} torch-side ops"
                 + (f" + {getattr(tr, 'n_replayed', 0)} replayed plans" if getattr(tr, "n_replayed", 0) else "")
                 + f" ({rep.launches} in the trace), streams {len(rep.streams)}, "
                 f"ordering edges {len(device_edges)} on the device + {len(edges) - len(device_edges)} host synchronisations",
                 f"cross-stream dependent access pairs checked: {rep.pairs_checked}"]
        try:
            assert rep.ok, rep.describe()
            if len(rep.streams) == 1:
                assert single_stream_ok, "a single stream: this scenario was expected to use several"
                assert not device_edges
                lines.append("single stream: nothing to order")
                return rep
            # the audit is not blind
            pairs = sorted({(e.src, e.dst) for e in device_edges})
            for a, b in pairs:
                gone = SA.analyse(SA.without(trace, [e for e in device_edges if (e.src, e.dst) == (a, b)]))
                n = sum(1 for e in device_edges if (e.src, e.dst) == (a, b))
                lines.append(f"without the {n} edges {a:#x} -> {b:#x}: {len(gone.conflicts)} distinct conflicts")
                assert not gone.ok, f"deleting every {a:#x} -> {b:#x} edge changes nothing: the tracer does not see what these waits protect, or they are dead"
            in_pairs = {s for p in pairs for s in p}
            assert rep.streams <= in_pairs, f"streams without any ordering edge: {[hex(s) for s in rep.streams - in_pairs]}"
            # single-edge removal, one representative per (call site, stream pair)
            groups = {}
            for e in device_edges:
                groups.setdefault((e.site, e.src, e.dst), []).append(e)
            needed, implied, together = [], [], []
            for (site, a, b), es in sorted(groups.items()):
                if not SA.analyse(SA.without(trace, [es[0]])).ok:
                    needed.append((site, a, b, len(es)))
                elif len(es) > 1 and not SA.analyse(SA.without(trace, es)).ok:
                    together.append((site, a, b, len(es)))          # each covered by its neighbours, the group as a whole is not
                else:
                    implied.append((site, a, b, len(es)))
            lines.append(f"edges by call site and stream pair: {len(needed)} needed, {len(together)} implied singly but needed as a group, "
                         f"{len(implied)} implied")
            for tag, rows in (("needed", needed), ("needed as a group", together), ("implied", implied)):
                by_site = Counter()
                for site, a, b, n in rows:
                    by_site[site] += n
                lines.append(f"  {tag}: " + ", ".join(f"{s} x{n}" for s, n in sorted(by_site.items())))
            return rep
        finally:
            lines.append(f"wall time: trace {self.t_trace:.2f} s, analysis {time.time() - t0:.2f} s")
            print("\n".join(lines), flush=True)


def batches(cfg, n, seed=40):
    from xlxmert_amd.trainer import synthetic_batch
    return [{k: v.to(DEV) for k, v in synthetic_batch(cfg, B, L, GRID, seed=seed + i).items()} for i in range(n)]


def trainer(au, cfg, **kw):
    from xlxmert_amd.trainer import PretrainStep
    kw.setdefault("plan", False)
    kw.setdefault("drop_grads", True)
    tr = PretrainStep(cfg, B, L, V, dtype=BF, device=DEV, seed=5, lr=1e-3, total_steps=100, train_dropout=True, overlap_optimizer=True,
                      ops=au.ops(), **kw)
    g = torch.Generator().manual_seed(3)
    tr.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=g).relu())
    assert tr.opt_stream is not None and tr.engine.side is not None and tr.engine._dw is not None
    return tr


# the starred scenarios: scratch sets must be REUSED inside a backward, or the guards (_gen_guard, wgrad_sync) are never exercised
REUSE = [pytest.param((2, 2, 2), 2, id="222-ngen2"), pytest.param((2, 2, 2), 3, id="222-ngen3"), pytest.param((5, 3, 3), None, id="533-ngen8")]


def vis_mask_steps(au, monkeypatch, layers, ngen, n_steps, **kw):
    from xlxmert_amd.engine import Engine
    if ngen is not None:
        monkeypatch.setattr(Engine, "NGEN", ngen)
    cfg = tiny_cfg(layers)
    with au:
        tr = trainer(au, cfg, visual_losses="obj,feat", **kw)
        bs = batches(cfg, n_steps)
        for i in range(n_steps):
            au.mark(f"step {i}")
            tr.step(bs[i])
        au.mark("end")
        tr.sync()
    assert tr.engine.NGEN == (ngen or 8)
    return tr


@pytest.mark.parametrize("layers,ngen", REUSE)
def test_vis_mask_pretraining_three_steps(monkeypatch, layers, ngen):
    """first-backward overwrite mode, AdamW of step t on the optimizer stream under the forward of step t + 1, drop_grads, the
    step-seed fill between steps"""
    au = Audit(monkeypatch)
    tr = vis_mask_steps(au, monkeypatch, layers, ngen, 3)
    assert au.scratch_reused(tr.engine) > 0, "no scratch set was rewritten behind a companion-stream read: the guards are not exercised"
    au.check(f"vis_mask obj,feat x3, layers {layers}, NGEN {tr.engine.NGEN}")


@pytest.mark.parametrize("layers,ngen", REUSE)
def test_vis_mask_pretraining_fp32_residual_stream_two_steps(monkeypatch, layers, ngen):
    au = Audit(monkeypatch)
    tr = vis_mask_steps(au, monkeypatch, layers, ngen, 2, residual_dtype="fp32")
    assert tr.engine.res32
    assert au.scratch_reused(tr.engine) > 0, "no scratch set was rewritten behind a companion-stream read: the guards are not exercised"
    au.check(f"vis_mask obj,feat x2, fp32 residual stream, layers {layers}, NGEN {tr.engine.NGEN}")


def lang_batch(cfg, b, seed):
    from xlxmert_amd.trainer import random_word_batch, word_rows_of
    g = torch.Generator().manual_seed(seed)
    ids, wl = random_word_batch(b["input_ids"].cpu(), vocab_size=cfg.vocab_size, generator=g)
    out = dict(b, input_ids=ids.to(DEV), word_labels=wl.to(DEV), matched_labels=torch.randint(0, 2, (B,), generator=g).to(DEV))
    out["word_rows"] = word_rows_of(wl)
    return out


def test_task_round_robin_with_an_evaluation_between_two_steps(monkeypatch):
    """task="all": vis_mask, word_mask, [evaluate matched], matched, qa back to back on one parameter set; the evaluation forward
    reads weights that the optimizer stream may still be writing"""
    au = Audit(monkeypatch)
    cfg = tiny_cfg()
    with au:
        tr = trainer(au, cfg, task="all", num_answers=NQ, visual_losses="obj,feat", drop_grads=False)
        bs = batches(cfg, 5)
        qa = torch.randint(0, NQ, (B,), generator=torch.Generator().manual_seed(1)).to(DEV)
        bs = [dict(b, qa_labels=qa) for b in bs]        # (a model with an answer head adds the qa loss in every branch)
        au.mark("vis_mask")
        tr.step(bs[0], task="vis_mask")
        au.mark("word_mask")
        tr.step(lang_batch(cfg, bs[1], 11), task="word_mask")
        au.mark("evaluate matched")
        tr.evaluate(lang_batch(cfg, bs[2], 12), task="matched")
        au.mark("matched")
        tr.step(lang_batch(cfg, bs[3], 13), task="matched")
        au.mark("qa")
        tr.step(bs[4], task="qa")
        au.mark("end")
        tr.sync()
    au.check("task=all: vis_mask, word_mask, evaluate(matched), matched, qa")


def test_vqa_two_steps(monkeypatch):
    au = Audit(monkeypatch)
    cfg = tiny_cfg()
    A = 24
    with au:
        tr = trainer(au, cfg, task="vqa", num_answers=A)
        g = torch.Generator().manual_seed(4)
        for i, b in enumerate(batches(cfg, 2)):
            tgt = torch.zeros(B, A)
            tgt[torch.arange(B), torch.randint(0, A, (B,), generator=g)] = 1.0
            feats = torch.randn(B, V, cfg.visual_feat_dim, generator=g).relu()
            au.mark(f"step {i}")
            tr.step({"input_ids": b["input_ids"], "visual_pos": b["visual_pos"], "visual_feats": feats.to(DEV), "targets": tgt.to(DEV)})
        au.mark("end")
        tr.sync()
    au.check("vqa x2")


def test_nlvr2_two_steps(monkeypatch):
    from xlxmert_amd.trainer import PretrainStep, synthetic_batch
    au = Audit(monkeypatch)
    cfg = tiny_cfg()
    P = B // 2
    with au:
        tr = PretrainStep(cfg, 2 * P, L, V, dtype=BF, device=DEV, seed=5, lr=1e-3, total_steps=100, train_dropout=True,
                          overlap_optimizer=True, plan=False, task="nlvr2", ops=au.ops())
        g = torch.Generator().manual_seed(4)
        for i in range(2):
            b = synthetic_batch(cfg, P, L, GRID, seed=60 + i)
            batch = {"input_ids": b["input_ids"].repeat_interleave(2, 0), "visual_pos": b["visual_pos"][:, None].expand(-1, 2, -1, -1).contiguous(),
                     "visual_feats": torch.randn(P, 2, V, cfg.visual_feat_dim, generator=g).relu(), "labels": torch.randint(0, 2, (P,), generator=g)}
            au.mark(f"step {i}")
            tr.step({k: v.to(DEV) for k, v in batch.items()})
        au.mark("end")
        tr.sync()
    au.check("nlvr2 x2")


def test_gradient_accumulation_two_updates(monkeypatch):
    au = Audit(monkeypatch)
    cfg = tiny_cfg()
    with au:
        tr = trainer(au, cfg, visual_losses="obj,feat")
        for i, b in enumerate(batches(cfg, 4)):
            au.mark(f"micro-batch {i}")
            tr.step(b, update=i % 2 == 1)
        au.mark("end")
        tr.sync()
    au.check("vis_mask, update_freq 2, two updates")


def test_launch_plan_record_and_two_replays(monkeypatch):
    """step 1 warms up, step 2 records (recording also executes), steps 3 and 4 replay: the recorded step's C-ABI events are spliced
    in where LaunchPlan.run is called; only the torch-side staging is seen live during a replay"""
    au = Audit(monkeypatch)
    cfg = tiny_cfg()
    with au:
        tr = trainer(au, cfg, visual_losses="obj,feat", plan=True)
        assert tr.plan_mode
        bs = batches(cfg, 1) * 4              # one batch: one launch geometry, one plan
        for i in range(4):
            au.mark(f"step {i}")
            tr.step(bs[i])
        au.mark("end")
        tr.sync()
    assert len(tr._plans) == 1 and getattr(au.tracer, "n_replayed", 0) == 2
    plan = next(iter(tr._plans.values()))
    assert plan.n_segments == 1 and sum(isinstance(e, SA.Launch) for e in plan._audit_events) > 100
    au.check("vis_mask with a launch plan: eager, record, replay, replay")


# ---------------------------------------------------------------- inference loops
def sampler_engine(au, cfg):
    import lxmert_oracle as O
    from xlxmert_amd.engine import Engine
    from xlxmert_amd.params import ParamStore
    from xlxmert_amd.trainer import init_reference_weights, synthetic_batch
    store = ParamStore(cfg, DEV, BF, task="vis_mask")
    init_reference_weights(store, 5)
    store.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=torch.Generator().manual_seed(3)).relu())
    eng = Engine(cfg, store, au.ops(), B, L, V, need_lang=False)
    eng.sync_compute_weights()
    ids = synthetic_batch(cfg, B, L, GRID, seed=7)["input_ids"].to(DEV)
    pos = torch.from_numpy(O.box_position(GRID)).unsqueeze(0).expand(B, -1, -1).float().to(DEV)
    eng.set_inputs(ids, ids > 0, None, pos, cluster_ids=torch.zeros(B, V, dtype=torch.long, device=DEV),
                   vis_mask=torch.ones(B, V, dtype=torch.bool, device=DEV))
    return eng


def test_nar_sampler_two_steps(monkeypatch):
    au = Audit(monkeypatch)
    with au:
        eng = sampler_engine(au, tiny_cfg())
        eng.sample_codes_nar(2)
    au.check("NAR sampler, T = 2", single_stream_ok=True)


def test_ar_sampler(monkeypatch):
    au = Audit(monkeypatch)
    with au:
        eng = sampler_engine(au, tiny_cfg())
        eng.sample_codes_ar(3, "confidence")
    au.check("AR sampler, 3 cells by confidence", single_stream_ok=True)


def test_inpainting_loop(monkeypatch):
    au = Audit(monkeypatch)
    with au:
        eng = sampler_engine(au, tiny_cfg())
        g = torch.Generator().manual_seed(2)
        free = (torch.rand(B, V, generator=g) < 0.5).to(DEV)
        init = torch.randint(0, eng.K, (B, V), generator=g).to(DEV)
        eng.inpaint_codes(init, free, 2, "nar")
    au.check("in-painting, NAR, T = 2", single_stream_ok=True)


def test_caption_sampler(monkeypatch):
    import test_caption_cpu as TC
    from test_caption_gpu import _sharp_engine
    au = Audit(monkeypatch)
    with au:
        eng, oc, sd, feats, pos, lengths = _sharp_engine(BF, ops=au.ops())
        eng.sample_words_nar(lengths, 2, 0, mask_token_id=TC.SHARP_MASK, banned_ids=TC.SHARP_BANNED)
    au.check("caption sampler, T = 2", single_stream_ok=True)


def test_caption_image_matching(monkeypatch):
    import match_cases as MC
    from xlxmert_amd.match import MatchRunner
    from xlxmert_amd.params import ParamStore
    au = Audit(monkeypatch)
    N, M, lens = 3, 2, (1, 8, 5)
    with au:
        cfg, oc, sd, inp = MC.tiny_case(N, M, lens)
        store = ParamStore(cfg, DEV, torch.float32, task="matched")
        store.load_named(sd)
        r = MatchRunner(cfg, store, au.ops(torch.float32), N, M, 8, 16, chunk_pairs=4)
        r.sync_compute_weights()
        x = {k: v.to(DEV) for k, v in inp.items()}
        r.run(x["input_ids"], x["attention_mask"], x["token_type_ids"], cluster_ids=x["cluster_ids"], visual_pos=x["visual_pos"])
    au.check("caption-image matching, 3 x 2 pairs in chunks of 4", single_stream_ok=True)


def test_image_generator(monkeypatch):
    import generator_cases as GC
    au = Audit(monkeypatch)
    with au:
        cfg, sd, arrays = GC.load_fixture("generator_tiny")
        G = GC.make_generator(cfg, sd, au.ops(torch.float32), DEV, torch.float32)
        GC.run_generator(G, torch.from_numpy(arrays["input"]), None)
    au.check("image generator, tiny fixture", single_stream_ok=True)
