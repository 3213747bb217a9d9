"""The stream audit without a device: the analyser (tests/stream_audit.py) on hand-written traces -- every hazard kind once failing
and once fixed -- and the tracer's access table (tests/stream_trace.ACCESS) against what the fake ops really touch in every engine
scenario of tests/ops_trace.py."""
import inspect

import pytest
import torch

import ops_trace
import stream_audit as SA
import stream_trace as ST
from xlxmert_amd._lib import parse_header
from xlxmert_amd.ops import HipOps

MAIN, SIDE, DW = 0x10, 0x20, 0x30           # three non-blocking streams; 0 is the default stream
X, Y = SA.rng(0x1000, 0x1100), SA.rng(0x2000, 0x2100)


def kinds(rep):
    return sorted(c.kind for c in rep.conflicts)


def two_streams(first_mode, second_mode, ordered):
    t = SA.Trace()
    t.launch(MAIN, [(X, first_mode, "x")], "producer", "engine.py:1")
    if ordered:
        t.record("e", MAIN, "engine.py:2")
        t.wait("e", SIDE, "engine.py:3")
    t.launch(SIDE, [(X, second_mode, "x")], "consumer", "engine.py:4")
    return t


@pytest.mark.parametrize("first,second,kind", [("w", "r", "RAW"), ("r", "w", "WAR"), ("w", "w", "WAW"), ("rw", "rw", "WAW")])
def test_each_hazard_is_reported_without_the_wait_and_not_with_it(first, second, kind):
    rep = SA.analyse(two_streams(first, second, ordered=False))
    assert kinds(rep) == [kind]
    c = rep.conflicts[0]
    assert (c.first.name, c.first.site, c.first.stream, c.first.arg) == ("producer", "engine.py:1", MAIN, "x")
    assert (c.second.name, c.second.site, c.second.stream) == ("consumer", "engine.py:4", SIDE)
    assert "engine.py:1" in rep.describe() and "engine.py:4" in rep.describe()
    rep = SA.analyse(two_streams(first, second, ordered=True))
    assert rep.ok and rep.pairs_checked == 1


def test_reads_on_two_streams_need_no_order_but_the_next_write_needs_both():
    t = SA.Trace()
    t.launch(MAIN, [(X, "w", "x")])
    t.fork(MAIN, SIDE)
    t.fork(MAIN, DW)
    t.launch(SIDE, [(X, "r", "x")], "read_side")
    t.launch(DW, [(X, "r", "x")], "read_dw")
    assert SA.analyse(t).ok
    t.fork(SIDE, MAIN)
    t.launch(MAIN, [(X, "w", "x")], "rewrite")              # ordered after the side read only
    rep = SA.analyse(t)
    assert [(c.kind, c.first.name) for c in rep.conflicts] == [("WAR", "read_dw")]


def test_same_stream_accesses_are_ordered_by_issue_order():
    t = SA.Trace()
    for m in ("w", "r", "rw", "w"):
        t.launch(MAIN, [(X, m, "x")])
    assert SA.analyse(t).ok


def test_transitive_order_through_a_third_stream():
    t = SA.Trace()
    t.launch(MAIN, [(X, "w", "x")])
    t.fork(MAIN, SIDE)
    t.launch(SIDE, [(Y, "w", "y")])
    t.fork(SIDE, DW)
    t.launch(DW, [(X, "r", "x"), (Y, "r", "y")])
    assert SA.analyse(t).ok


def test_a_wait_binds_to_the_record_that_precedes_it_at_enqueue_time():
    """the HIP rule the 512-entry fork ring relies on: re-recording an event does not move a wait that is already queued"""
    t = SA.Trace()
    t.launch(MAIN, [(X, "w", "x")], "first")
    t.record("e", MAIN)
    t.wait("e", SIDE)                                       # binds to the snapshot after `first`
    t.launch(MAIN, [(Y, "w", "y")], "second")
    t.record("e", MAIN)                                     # re-record: covers `second` too, but the queued wait does not see it
    t.launch(SIDE, [(X, "r", "x")], "reads_first")
    assert SA.analyse(t).ok
    t.launch(SIDE, [(Y, "r", "y")], "reads_second")
    rep = SA.analyse(t)
    assert [(c.kind, c.first.name, c.second.name) for c in rep.conflicts] == [("RAW", "second", "reads_second")]
    t.events.insert(len(t.events) - 1, SA.Wait("e", SIDE, ""))          # a wait enqueued AFTER the re-record binds to the new snapshot
    assert SA.analyse(t).ok


def test_a_wait_on_a_never_recorded_event_orders_nothing():
    t = SA.Trace()
    t.launch(MAIN, [(X, "w", "x")])
    t.wait("never", SIDE)
    t.launch(SIDE, [(X, "r", "x")])
    assert kinds(SA.analyse(t)) == ["RAW"]
    assert SA.edges(t) == []


def guard_ring(fresh_event):
    """the _guard_event story: generation 0's guard refers to an event recorded behind the companion-stream launch that read its
    scratch.  Before the chain comes back to generation 0 the ring hands the SAME event to a cross-stream combine, which re-records
    it on the language stream: the chain's wait then binds to that record and no longer covers the companion-stream read."""
    S0, S1 = SA.rng(0x10000, 0x10400), SA.rng(0x20000, 0x20400)
    t = SA.Trace()
    t.launch(MAIN, [(S0, "w", "dz")], "layernorm_bwd", "blocks.py:10")
    t.fork(MAIN, DW, "engine.py:700")
    t.launch(DW, [(S0, "r", "dY0")], "gemm_wgrad_group", "engine.py:702")
    t.record("ring0", DW, "engine.py:709")                  # generation 0's guard
    t.launch(MAIN, [(S1, "w", "dz")], "layernorm_bwd", "blocks.py:10")
    t.launch(SIDE, [(Y, "w", "dgamma")], "flush_reductions", "engine.py:624")
    t.record("ring1" if fresh_event else "ring0", SIDE, "engine.py:625")    # the combine's event: a live one passed over, or not
    t.wait("ring1" if fresh_event else "ring0", MAIN, "engine.py:626")
    t.wait("ring0", MAIN, "engine.py:722")                  # wgrad_sync of generation 0
    t.launch(MAIN, [(S0, "w", "dz")], "layernorm_bwd", "blocks.py:10")
    return t


def test_a_ring_event_re_recorded_while_a_guard_still_refers_to_it():
    rep = SA.analyse(guard_ring(fresh_event=False))
    assert [(c.kind, c.first.name, c.first.site, c.second.site) for c in rep.conflicts] == [("WAR", "gemm_wgrad_group", "engine.py:702", "blocks.py:10")]
    assert SA.analyse(guard_ring(fresh_event=True)).ok


def test_accumulations_commute_with_each_other_only():
    t = SA.Trace()
    t.launch(MAIN, [(X, "acc", "dW")], "wgrad_a")
    t.launch(SIDE, [(X, "acc", "dW")], "wgrad_b")
    assert SA.analyse(t).ok
    t.launch(DW, [(X, "r", "g")], "sumsq")
    rep = SA.analyse(t)
    assert sorted((c.kind, c.first.name) for c in rep.conflicts) == [("RAW", "wgrad_a"), ("RAW", "wgrad_b")]
    t.events[-1:-1] = [SA.Fork(MAIN, DW, ""), SA.Fork(SIDE, DW, "")]
    assert SA.analyse(t).ok
    t.launch(MAIN, [(X, "acc", "dW")], "next_step")          # an accumulation after a read is a write after a read
    assert kinds(SA.analyse(t)) == ["WAR"]


def test_equal_pitch_rectangles_overlap_exactly():
    """q | k | v column blocks of one [rows, 3d] buffer: ld = 3d"""
    d, rows, es = 128, 40, 2
    base, pitch = 0x40000, 3 * d * es
    q, k, v = (SA.rect(base + i * d * es, rows, d * es, pitch) for i in range(3))
    assert q[0] == "rect"
    assert not SA.overlap(q, k) and not SA.overlap(k, v) and not SA.overlap(q, v)
    assert SA.overlap(q, SA.rect(base + d * es - 2, rows, 4, pitch))          # straddles the q / k boundary
    assert not SA.overlap(q, SA.rect(base + rows * pitch, rows, d * es, pitch))    # the rows behind
    assert SA.overlap(v, SA.rect(base + pitch - 2, 1, 8, pitch)) and SA.overlap(q, SA.rect(base + pitch - 2, 1, 8, pitch))   # wraps into the next row
    t = SA.Trace()
    t.launch(MAIN, [(q, "w", "dq")], "sdpa_bwd")
    t.launch(SIDE, [(k, "w", "dk")], "sdpa_bwd")
    assert SA.analyse(t).ok
    t.launch(DW, [(SA.rect(base, rows, 2 * d * es, pitch), "r", "dqk")], "gemm_wgrad_group")
    assert len(SA.analyse(t).conflicts) == 2


def test_other_pairs_fall_back_to_the_bounding_range():
    a = SA.rect(0x1000, 4, 8, 32)
    b = SA.rect(0x1008, 4, 8, 64)                           # other pitch: disjoint bytes in truth, bounding ranges meet
    assert SA.overlap(a, b)
    assert SA.overlap(a, SA.rng(0x1008, 0x1010))            # a byte range in the gap of a rectangle
    assert not SA.overlap(a, SA.rng(0x1068, 0x1070))        # beyond its last row
    assert SA.rect(0x1000, 4, 32, 32) == SA.rng(0x1000, 0x1080) and SA.rect(0x1000, 1, 8, 32) == SA.rng(0x1000, 0x1008)
    t = SA.Trace()
    t.launch(MAIN, [(a, "w", "a")])
    t.launch(SIDE, [(b, "w", "b")])
    assert kinds(SA.analyse(t)) == ["WAW"]


def test_host_sync_of_one_stream_and_of_all():
    def build(sync):
        t = SA.Trace()
        t.launch(MAIN, [(X, "w", "x")])
        t.launch(SIDE, [(Y, "w", "y")])
        if sync is not None:
            t.host_sync(sync, "trainer.py:294")
        t.launch(DW, [(X, "r", "x"), (Y, "r", "y")], "reader")
        return t
    assert len(SA.analyse(build(None)).conflicts) == 2
    rep = SA.analyse(build(MAIN))
    assert [(c.first.arg) for c in rep.conflicts] == ["y"]
    assert SA.analyse(build(SA.ALL)).ok
    # work queued on the synchronised stream AFTER the host came back is not covered
    t = build(MAIN)
    t.launch(MAIN, [(Y, "r", "y")], "late")
    assert sorted(c.second.name for c in SA.analyse(t).conflicts) == ["late", "reader"]


def test_host_wait_for_an_event_covers_what_the_event_holds():
    t = SA.Trace()
    t.launch(MAIN, [(X, "w", "x")])
    t.record("e", MAIN)
    t.launch(MAIN, [(Y, "w", "y")])
    t.host_sync(SA.EventRef("e"))
    t.launch(SIDE, [(X, "r", "x")])
    assert SA.analyse(t).ok
    t.launch(SIDE, [(Y, "r", "y")])
    assert kinds(SA.analyse(t)) == ["RAW"]


def test_the_default_stream_orders_nothing():
    t = SA.Trace()
    t.launch(0, [(X, "w", "x")], "fill_")
    t.launch(SIDE, [(X, "r", "x")], "dropout")
    assert kinds(SA.analyse(t)) == ["RAW"]
    t = SA.Trace()
    t.launch(SIDE, [(X, "w", "x")])
    t.launch(0, [(Y, "w", "y")])                            # work on the default stream between two streams is no barrier
    t.launch(DW, [(X, "r", "x")])
    assert kinds(SA.analyse(t)) == ["RAW"]


def test_without_turns_a_clean_trace_into_a_conflicting_one():
    t = two_streams("w", "r", ordered=True)
    e = SA.edges(t)
    assert [(x.kind, x.src, x.dst, x.site) for x in e] == [("wait", MAIN, SIDE, "engine.py:3")]
    assert SA.analyse(t).ok
    assert kinds(SA.analyse(SA.without(t, e))) == ["RAW"]
    assert SA.analyse(t).ok                                 # the recorded trace itself is untouched


def test_memory_reuse_is_an_address_like_any_other():
    """scratch used on a side stream, freed, and handed to the main stream at the same address"""
    t = SA.Trace()
    t.fork(MAIN, SIDE)
    t.launch(SIDE, [(X, "w", "tmp")], "aten.mul")
    t.launch(MAIN, [(X, "w", "other_tmp")], "aten.zeros")
    assert kinds(SA.analyse(t)) == ["WAW"]


# ---------------------------------------------------------------- the reviewer's sensitivity check
def three_layer_backward(ngen=2):
    """a three-layer backward with `ngen` scratch sets as engine.wgrad_flush / wgrad_sync schedule it: the chain (MAIN) writes layer i's
    scratch into set i % ngen, the companion stream (DW) reads it for the weight gradients behind a fork and records the set's guard;
    before the chain writes a set again it waits for that guard"""
    t = SA.Trace()
    sets = [SA.rng(0x100000 * (g + 1), 0x100000 * (g + 1) + 0x8000) for g in range(ngen)]
    grads = [SA.rng(0x900000 + 0x1000 * i, 0x900000 + 0x1000 * (i + 1)) for i in range(3)]
    guard = {}
    for i in range(3):
        g = i % ngen
        if g in guard:
            t.wait(guard.pop(g), MAIN, "engine.py:722")                 # wgrad_sync
        t.launch(MAIN, [(sets[g], "w", "dz")], "layernorm_bwd", "blocks.py:120")
        t.fork(MAIN, DW, "engine.py:700")
        t.launch(DW, [(sets[g], "r", "dY0"), (grads[i], "rw", "dW0")], "gemm_wgrad_group", "engine.py:702")
        t.record(("guard", i), DW, "engine.py:709")
        guard[g] = ("guard", i)
    t.fork(DW, MAIN, "engine.py:728")                                   # wgrad_sync_all
    t.launch(MAIN, [(r, "r", "g") for r in grads], "sumsq", "trainer.py:888")
    return t


def test_three_layer_backward_with_two_scratch_sets_needs_its_wgrad_sync():
    t = three_layer_backward()
    assert SA.analyse(t).ok
    sync = [e for e in SA.edges(t) if e.site == "engine.py:722"]
    assert len(sync) == 1
    rep = SA.analyse(SA.without(t, sync))
    assert [(c.kind, c.first.name, c.first.site, c.first.arg, c.second.name, c.second.site) for c in rep.conflicts] == \
        [("WAR", "gemm_wgrad_group", "engine.py:702", "dY0", "layernorm_bwd", "blocks.py:120")]
    text = rep.describe()
    assert "engine.py:702" in text and "blocks.py:120" in text and "WAR" in text
    # every other edge is needed too, each for its own reason; with three sets the guard wait does not exist
    for e in SA.edges(t):
        assert not SA.analyse(SA.without(t, [e])).ok, e
    assert not [e for e in SA.edges(three_layer_backward(3)) if e.site == "engine.py:722"]


# ---------------------------------------------------------------- the access table
def test_every_hipops_method_that_takes_a_tensor_is_in_the_access_table():
    """Which methods take device memory is read off the C header: a pointer parameter that is neither a stream nor an event.  The table
    must have an entry per such parameter, and as many read-only ones as the prototype has const pointers."""
    protos = parse_header()
    methods = ST.public_methods(HipOps)
    assert set(ST.ACCESS) <= set(methods)
    not_memory = ("stream", "event", "after_stream", "producer_stream", "launch_stream", "from_stream", "to_stream")
    different = {"gemm_wgrad_group", "gemm_pair", "wgrad_group_one_writer", "gemm_trace", "set_step_seed_ptr",
                 "comm_allreduce", "comm_reduce_scatter", "comm_allgather"}       # argument lists that do not map one to one
    for m in methods:
        proto = protos.get("xl_" + m)
        params = inspect.signature(getattr(HipOps, m)).parameters
        if proto is None:
            # no entry point of its name: the memset (in the table), and methods whose parameters are sizes, streams and devices
            assert m in ST.ACCESS or m in ("bound", "forget_binding", "rebind", "new_event", "gemm_workspace", "instnorm_ws_floats",
                                           "sumsq_scratch"), m
            continue
        ptrs = [(t, n) for t, n in proto[1] if "*" in t and n not in not_memory]
        if m in ST.ORDERING or m in ("comm_wait", "flush_reductions", "flush_reductions_on"):
            assert not ptrs
            continue
        if not ptrs:
            assert m not in ST.ACCESS, m
            continue
        assert m in ST.ACCESS, f"{m} takes device memory and has no ACCESS entry"
        assert set(ST.ACCESS[m]) <= set(params), (m, set(ST.ACCESS[m]) - set(params))
        if m in different:
            continue
        assert len(ST.ACCESS[m]) == len(ptrs), (m, sorted(ST.ACCESS[m]), [n for _, n in ptrs])
        n_const = sum(1 for t, _ in ptrs if "const" in t)
        n_read = sum(1 for v in ST.ACCESS[m].values() if v == "r" or (callable(v) and m == "sdpa_bwd"))
        assert n_read == n_const, (m, n_read, n_const)
    for m, table in ST.ACCESS.items():
        for mode in table.values():
            assert callable(mode) or mode in ("r", "w", "rw", "-"), (m, mode)       # "acc" needs the kernel line of its atomic add


def test_deferred_destinations_are_the_bound_checks_list():
    """one list of column-sum outputs whose second stage xl_set_deferred_reduce(1) postpones: the float64 recorder checks on the device
    that their producers leave them untouched until the flush"""
    import residual_checks  # noqa: F401  (adds layernorm_bwd_res to the recorder's list)
    import test_kernel_bounds_gpu as KB
    assert {k: tuple(v) for k, v in KB.REDUCE_OUTS.items()} == ST.REDUCE_OUTS


class DeferringOps:
    """The library's deferred column reductions on top of the fake ops, which always reduce at once: while deferred, a producer with a
    workspace leaves its REDUCE_OUTS destinations as they were and the next flush adds what it would have added."""

    def __init__(self, inner, bind):
        object.__setattr__(self, "_inner", inner)
        object.__setattr__(self, "_bind", bind)              # (name, fn, args, kw) -> arguments by HipOps' names
        object.__setattr__(self, "_on", False)
        object.__setattr__(self, "_held", [])
        object.__setattr__(self, "flushed", [])

    def __setattr__(self, k, v):
        setattr(self._inner, k, v)

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr) or name.startswith("_"):
            return attr
        if name == "set_deferred_reduce":
            def setter(on):
                object.__setattr__(self, "_on", bool(on))
                return attr(on)
            return setter
        if name in ("flush_reductions", "flush_reductions_on"):
            def flush(*args):
                del self.flushed[:]
                for t, delta in self._held:
                    t.add_(delta)
                    self.flushed.append((t.data_ptr(), bool((delta != 0).any())))
                del self._held[:]
                return attr(*args)
            return flush
        if name == "gemm_pair":                                 # by contract the two gemm calls: each defers on its own
            def pair(c0, c1):
                self.gemm(*c0.a, **c0.kw)
                self.gemm(*c1.a, **c1.kw)
            return pair
        if name in ST.REDUCE_OUTS:
            def producer(*args, **kw):
                a = self._bind(name, attr, args, kw)
                if not self._on or a.get("ws") is None or (name == "gemm" and a.get("colsum") is None):
                    return attr(*args, **kw)
                dests = [a[k] for k in ST.REDUCE_OUTS[name] if a.get(k) is not None]
                before = [t.clone() for t in dests]
                r = attr(*args, **kw)
                for t, b in zip(dests, before):
                    self._held.append((t, t - b))
                    t.copy_(b)
                return r
            return producer
        return attr


def _bytes(t):
    return torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage())


def _inside(off, region):
    if region[0] == "range":
        return (off >= region[1]) & (off < region[2])
    _, base, rows, rb, pitch = region
    rel = off - base
    return (rel >= 0) & (torch.div(rel, pitch, rounding_mode="floor") < rows) & (rel % pitch < rb)


class HonestTracer(ST.Tracer):
    """checks every call's declared accesses against the bytes that changed: a byte that changed lies inside a region declared w / rw
    (so an argument declared r is bit-unchanged, and so is a deferred destination under its producer); a flush changes every
    destination it was handed a non-zero sum for"""

    def __init__(self):
        super().__init__(stream_of=lambda: 0)
        self.calls = self.flush_dests = self.deferred_producers = 0
        self.problems = []
        self.shim = None

    def accesses_of(self, name, a):
        out, dests = super().accesses_of(name, a)
        ts = [v for v in a.values() if isinstance(v, torch.Tensor)]
        for v in a.values():
            if isinstance(v, (list, tuple)):
                ts += [x for pr in v if isinstance(pr, (list, tuple)) for x in pr if isinstance(x, torch.Tensor)]
            elif hasattr(v, "a") and hasattr(v, "kw"):                      # ops.GemmCall
                ts += [x for x in list(v.a) + list(v.kw.values()) if isinstance(x, torch.Tensor)]
        self._tensors = ts
        return out, dests

    def invoke(self, name, a, accesses, dests, run):
        self.calls += 1
        if "_pending" in a:
            tensors = [t for t, _ in self.shim._held]
        else:
            tensors = self._tensors
        stores = {}
        for t in tensors:
            stores.setdefault(t.untyped_storage().data_ptr(), t)
        before = {p: _bytes(t).clone() for p, t in stores.items()}
        r = run()
        written = [reg for reg, mode, _ in accesses if mode in ("w", "rw", "acc")]
        for p, t in stores.items():
            changed = (_bytes(t) != before[p]).nonzero().view(-1) + p
            if changed.numel() == 0:
                continue
            ok = torch.zeros_like(changed, dtype=torch.bool)
            for reg in written:
                ok |= _inside(changed, reg)
            if not bool(ok.all()):
                bad = int(changed[~ok][0])
                who = [n for reg, _, n in accesses + [(rg, "", f"{n} (deferred)") for rg, n in dests] if bool(_inside(torch.tensor([bad]), reg))]
                self.problems.append(f"{name}: byte {bad:#x} changed outside every region declared written (inside: {who or 'no declared region'})")
        if dests:
            self.deferred_producers += 1
        if "_pending" in a:
            nonzero = dict(self.shim.flushed)
            for reg, mode, n in accesses:
                if mode != "rw":
                    continue
                self.flush_dests += 1
                lo, hi = SA.bounds(reg)
                if nonzero.get(lo) and not any(bool(_inside((_bytes(t) != before[p]).nonzero().view(-1) + p, reg).any()) for p, t in stores.items()):
                    self.problems.append(f"{name}: destination {n} was handed a sum and did not change")
        return r


SCENARIOS = ops_trace.engine_scenarios()


@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
def test_access_table_is_honest_about_what_the_fake_ops_touch(scenario, monkeypatch):
    tracer = HonestTracer()
    recording = ops_trace.RecordingOps

    def wrap(inner):
        tracer.shim = DeferringOps(inner, tracer.bind)
        return recording(ST.TracingProxy(tracer.shim, tracer))
    monkeypatch.setattr(ops_trace, "RecordingOps", wrap)
    SCENARIOS[scenario]()
    assert tracer.calls > 10
    assert not tracer.problems, "\n".join(tracer.problems[:20])
    assert not tracer.pending.get(0), "column sums left pending at the end of the scenario"
    if scenario.startswith("step/") or "backward" in scenario:
        assert tracer.deferred_producers > 0 and tracer.flush_dests > 0, (tracer.deferred_producers, tracer.flush_dests)
    rep = SA.analyse(tracer.trace)                              # one stream on the CPU: nothing to order, nothing to report
    assert rep.ok and rep.launches > 10 and rep.pairs_checked == 0
