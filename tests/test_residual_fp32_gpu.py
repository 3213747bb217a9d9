"""The fp32 residual stream (Engine residual_dtype="fp32" / XL_RESIDUAL=fp32) on the device.

(a) the criterion of tests/test_residual_fp32_cpu.py with the real kernels: both modes against the exact-fp32 oracle, the fp32
    stream must realise at least half of the improvement the oracle's storage emulation predicts;
(b) every numeric library call of one eager fp32-stream training step at the benchmarked geometry within its float64 bound
    (the recording proxy of tests/test_kernel_bounds_gpu.py with the checkers of tests/residual_checks.py);
(c)-(e) the EXISTING device tests of the bf16 path -- bit reproducibility, the bs-256 step against the oracle, the other tasks
    and the sampler at their benchmarked sizes -- run once more with XL_RESIDUAL=fp32 in the environment: the same code, the same
    ceilings, the engines they build read the mode from the environment.  Each asserts that the fp32-stream kernels really ran."""
import time

import pytest
import torch

import lxmert_oracle as O
import test_engine_gpu as EG
import test_kernel_bounds_gpu as KB
from residual_checks import RecorderRes
from test_residual_fp32_cpu import engine_grads, stream_criterion

pytestmark = pytest.mark.gpu


@pytest.fixture
def fp32_stream(monkeypatch):
    """XL_RESIDUAL=fp32 for the engines the test builds, and a count of the fp32-stream launches they issue"""
    from xlxmert_amd.ops import HipOps
    monkeypatch.setenv("XL_RESIDUAL", "fp32")
    n = {"fwd": 0, "bwd": 0}
    fwd, bwd = HipOps.layernorm_fwd_res, HipOps.layernorm_bwd_res

    def count_fwd(self, *a, **kw):
        n["fwd"] += 1
        return fwd(self, *a, **kw)

    def count_bwd(self, *a, **kw):
        n["bwd"] += 1
        return bwd(self, *a, **kw)
    monkeypatch.setattr(HipOps, "layernorm_fwd_res", count_fwd)
    monkeypatch.setattr(HipOps, "layernorm_bwd_res", count_bwd)
    return n


def test_fp32_stream_engine_realises_half_of_the_emulated_improvement_on_the_device():
    """(a) full architecture, B 4, the inputs of the emulation test; HipOps; both modes in one test"""
    from bench import usable_cores
    from xlxmert_amd.ops import HipOps
    torch.set_num_threads(usable_cores())
    oc = O.OracleConfig()
    sd = O.make_state_dict(oc, 7)
    inp = O.make_inputs(oc, 11, 4, 20, 8)
    fig = stream_criterion(oc, sd, inp, lambda mode: engine_grads(oc, sd, inp, mode, device="cuda", ops=HipOps(torch.bfloat16))[2])
    print(f"device figures: {fig}")


def test_every_numeric_call_of_an_fp32_stream_training_step_is_within_its_bound(monkeypatch):
    """(b) tests/test_kernel_bounds_gpu.py's step test in fp32-stream mode: bs 256, dropout on, eager, optimizer in line.  A numeric
    method without a checker fails; deferred column sums are checked at their flush (the default of a step's backward)."""
    t0 = time.time()
    from xlxmert_amd.config import XLxmertConfig
    from xlxmert_amd.ops import HipOps
    from xlxmert_amd.params import ParamStore
    from xlxmert_amd.trainer import PretrainStep, synthetic_batch
    cfg = XLxmertConfig()
    oc = O.OracleConfig(**{k: getattr(cfg, k) for k in KB.CFG_KEYS})
    sd = O.make_state_dict(oc, 2718)
    B = 256
    store = ParamStore(cfg, "cuda", torch.bfloat16)
    store.load_named(sd)
    rec = RecorderRes(HipOps(torch.bfloat16))
    tr = PretrainStep(cfg, B, 20, 64, dtype=torch.bfloat16, device="cuda", store=store, lr=1e-4, total_steps=1000, warmup_ratio=0.0,
                      plan=False, drop_grads=False, overlap_optimizer=False, train_dropout=True, ops=rec, residual_dtype="fp32")
    assert tr.engine.res32
    batch = synthetic_batch(cfg, B, 20, 8, seed=31)
    dev = {k: v.cuda() for k, v in batch.items()}
    for _ in range(3):                  # (a destination shared with an unrecorded call: recorded from then on, the step run again)
        losses = tr.step(dev)
        tr.sync()
        KB._sync()
        if not rec.retry():
            break
    assert tr.engine.packed
    assert all(torch.isfinite(torch.as_tensor(x)).all() for x in losses if x is not None)
    KB._table(rec.rows, time.time() - t0)
    assert not rec.unchecked, f"numeric methods without a checker: {sorted(rec.unchecked)}"
    assert not rec.failures, "\n".join(rec.failures)
    assert not rec.leftover(), rec.leftover()
    assert rec.flushes_checked > 0
    for must in ("gemm", "gemm_wgrad_group", "sdpa_fwd", "sdpa_bwd", "layernorm_fwd_res", "layernorm_bwd_res", "layernorm_fwd",
                 "visn_ln_fwd", "visn_ln_bwd", "cast_to_f32", "cast_from_f32", "dropout", "gather_rows", "scatter_rows", "embed_bwd",
                 "ce_fwd_bwd", "sumsq", "adamw"):
        assert must in rec.called, must
    res = [a for name, a in rec.checked if name == "gemm" and a["epilogue"] == 2]
    assert res and all(a["out_f32"] for a in res), "a residual epilogue of the step ran with a bf16 stream"
    print(f"methods called: {sorted(rec.called)}; run time {time.time() - t0:.1f} s")


@pytest.mark.parametrize("plan", [False, True])
def test_fp32_stream_training_step_is_bit_reproducible(plan, fp32_stream):
    """(c)"""
    EG.test_training_step_is_bit_reproducible(plan)
    assert fp32_stream["fwd"] > 0 and fp32_stream["bwd"] > 0


def test_fp32_stream_benchmark_geometry_bs256_step_matches_oracle(monkeypatch, fp32_stream):
    """(d) the existing ceilings (loss 5e-3, worst norm 6 %, worst tensor 15.4 %, median 5 %), first in the bf16 mode, then in the
    fp32-stream mode: the two lines the runs print are the figures of the two modes side by side"""
    monkeypatch.setenv("XL_RESIDUAL", "bf16")
    print("bf16 stream:")
    EG.test_benchmark_geometry_bs256_step_matches_oracle()
    assert fp32_stream["fwd"] == 0
    monkeypatch.setenv("XL_RESIDUAL", "fp32")
    print("fp32 stream:")
    EG.test_benchmark_geometry_bs256_step_matches_oracle()
    assert fp32_stream["fwd"] > 0 and fp32_stream["bwd"] > 0


@pytest.mark.parametrize("task", ["word_mask", "matched", "vqa", "nlvr2"])
def test_fp32_stream_next_rows_at_bench_geometry_match_oracle(task, fp32_stream):
    """(e) under the ceilings of their bf16 runs"""
    EG.test_next_rows_at_bench_geometry_match_oracle(task)
    assert fp32_stream["fwd"] > 0 and fp32_stream["bwd"] > 0


def test_fp32_stream_sampler_first_step_at_bench_geometry(fp32_stream):
    """(e) forward only"""
    EG.test_sampler_first_step_at_bench_geometry_matches_oracle_where_decisive()
    assert fp32_stream["fwd"] > 0 and fp32_stream["bwd"] == 0
