"""The predict tail -- xl_gemm with XL_EPI_ROWMAX / XL_EPI_ROWSAMPLE / XL_EPI_ROWSCORE, xl_rowmax_combine / xl_rowsample_combine /
xl_rowscore_combine, xl_sample_rows / xl_score_rows: what every sampler, caption, validation loss and in-painting step ends in -- at
the edges of its dispatch, element by element under the float64 bounds of tests/bounds.py, bounds_sampling.py and bounds_eval.py
through the recording proxy of tests/test_kernel_bounds_gpu.py.  The calls are those of tests/predict_edge_cases.py: K below and off 64,
tight and padded leading dimensions with poisoned pads, alpha 1 and 0.5, a NULL bias, logits spread to +-60, planted exact ties, labels
at every edge, more than 256 tiles with and without a slab workspace, the GEMM switches, synthetic records for the combines, the
grid caps of the scores kernels and their ticket sets.

One test per family x switch set, a fresh library context each.  Every test ends with: no unchecked op, no failure, one checked call
and one "outside view" row per issued call, the kernel labels it expects present and the ones it must not reach absent."""
import time

import pytest
import torch

import predict_edge_cases as PE
from test_gemm_edges_bounds_gpu import labels
from test_kernel_bounds_gpu import Recorder, _table
from test_rowop_edges_bounds_gpu import _summary

pytestmark = pytest.mark.gpu

PP = "ping-pong 256x256 "
ROW_LABELS = [PP + "ROWMAX epilogue", PP + "ROWSAMPLE epilogue", PP + "ROWSCORE epilogue", "rowmax_combine_kernel",
              "rowsample_combine_kernel", "rowscore_combine_kernel + totals"]
SWITCH_SETS = {"mfma_128_only": (("set_gemm_pingpong", 0),), "duo_everywhere": (("set_gemm_duo", 2),),
               "wgrad_slabs": (("set_gemm_wgrad_slabs", 1), ("gemm_workspace", 256))}
TAIL = " + tail split 16x2"


def _rec(ops=None, switches=()):
    if ops is None:
        from xlxmert_amd.ops import HipOps
        ops = HipOps(torch.bfloat16)
    rec = Recorder(ops, every_call=True)
    for name, v in switches:
        getattr(rec, name)(*(v if isinstance(v, tuple) else (v,)))
    return rec


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _done(rec, t0, n_calls, expect, absent=()):
    _table(rec.rows, time.time() - t0)
    _summary(rec)
    assert not rec.unchecked, sorted(rec.unchecked)
    assert not rec.failures, "\n".join(rec.failures)
    assert not rec.leftover(), rec.leftover()
    assert len(rec.checked) == n_calls, (len(rec.checked), n_calls)
    assert sum(w.endswith("outside view") for _, w, _, _, _ in rec.rows) == n_calls
    assert len(rec.rows) >= 2 * n_calls, len(rec.rows)
    got = labels(rec)
    print("kernel labels:", *sorted(got), sep="\n  ")
    for e in expect:
        assert any(e in k for k in got), (e, sorted(got))
    for e in absent:
        assert not any(e in k for k in got), (e, sorted(got))


def _composed(rec, n_gemm):
    """every combine behind a checked launch was also held to the float64 logits of the whole row"""
    n = sum(w in ("composed row argmax admissible", "composed row draw admissible", "composed row_max") for _, w, _, _, _ in rec.rows)
    assert n == n_gemm, (n, n_gemm)


# The bodies take (ops, dev) so that tests/test_bounds_cpu.py runs the same code over the host restatement: the labels depend on
# the arguments and the switches only, so the label assertions hold there as they do here.
def run_fused(ops=None, dev="cuda", **kw):
    t0 = time.time()
    rec = _rec(ops)
    n = PE.fused(rec, dev, _gen(301), **kw)
    if kw:
        return rec, n
    _done(rec, t0, n, ROW_LABELS, ("tail split", "duo", "MFMA 128x128", "second pass"))
    _composed(rec, n // 2)
    gemms = [a for nm, a in rec.checked if nm == "gemm"]
    assert {a["alpha"] for a in gemms if a["epilogue"] != PE.EPI_ROWSAMPLE} == {1.0, 0.5}
    assert {a["alpha"] for a in gemms if a["epilogue"] == PE.EPI_ROWSAMPLE} == {2.0, 1.0, 0.25}
    assert {a["seed"] for a in gemms if a["epilogue"] == PE.EPI_ROWSAMPLE} == set(PE.SEEDS)
    assert all(any(a["epilogue"] == epi and a["bias"] is None for a in gemms) for epi in PE.EPIS)
    assert max(share for _, share, _ in rec.sharp) <= PE.MAX_AMBIGUOUS + 4 / 256, rec.sharp     # (the planted rows count here)


def run_rounds(tail, ops=None, dev="cuda", **kw):
    """tail: a slab workspace on the stream and set_gemm_tail_split(64, 1024).  XL_EPI_ROWSAMPLE and XL_EPI_ROWSCORE run whole tiles
    either way (csrc/gemm.hip excludes them from the tail split); XL_EPI_ROWMAX is not excluded, and may not need to be: the last
    arriver of a split tile holds the whole sum of the K slices in its registers (gemm_pp_kernel.h pp_tile, slab_exchange), sets
    `first`, loads the bias and runs the ordinary epilogue over them -- so with the workspace its label carries the tail split, and
    its records are held to the same bounds"""
    t0 = time.time()
    rec = _rec(ops, (("set_gemm_tail_split", (64, 1024)), ("gemm_workspace", 256)) if tail else ())
    keep = []
    n = PE.rounds(rec, dev, _gen(302), keep=keep, **kw)
    epis = kw.get("epis", PE.EPIS)
    expect = [PP + "ROWMAX epilogue" + (TAIL if tail else "")]
    expect += [PP + "ROWSAMPLE epilogue", PP + "ROWSCORE epilogue"] if len(epis) == 3 else []
    _done(rec, t0, n, expect)
    _composed(rec, n // 2)
    got = {a["epilogue"]: a["_kernel"] for nm, a in rec.checked if nm == "gemm"}
    assert got[PE.EPI_ROWMAX] == PP + "ROWMAX epilogue" + (TAIL if tail else ""), got
    assert all("tail split" not in k for e, k in got.items() if e != PE.EPI_ROWMAX), got
    if tail and ops is None:
        _tail_tiles_differ(keep, dev)
    return rec, n


def _tail_tiles_differ(keep, dev):
    """on the device, the tail-split run against the same launches without a workspace: XL_EPI_ROWSAMPLE and XL_EPI_ROWSCORE leave
    the same bits (whole tiles both times); the XL_EPI_ROWMAX records differ -- two K slices are summed in another order than one
    K loop -- in at most 16 of the 272 tiles and in at least one: the split that the label restates did run, on the last round only"""
    base, want = _rec(), []
    PE.rounds(base, dev, _gen(302), keep=want)
    assert not base.failures, base.failures
    (M, N, _), _ = PE.ROUNDS_SHAPE
    for i in (4, 8):                                   # aux of the ROWSAMPLE and of the ROWSCORE arm
        assert torch.equal(Recorder._raw(keep[i]), Recorder._raw(want[i])), "whole-tile launches differ between the two runs"
    diff = (keep[0].view(N // 64, M, 4) != want[0].view(N // 64, M, 4)).any(-1)            # [segment, row]
    tiles = diff.view(N // 256, 4, M // 256, 256).any(3).any(1)
    print(f"ROWMAX records that differ between the tail-split run and the two-round run: {int(diff.sum())} in {int(tiles.sum())} tiles")
    assert 1 <= int(tiles.sum()) <= 16, int(tiles.sum())


def run_switches(sw, ops=None, ops_default=None, dev="cuda"):
    """the (512, 768, 200) launches under a switch set against the same launches under the library's defaults: the epilogues force
    the ping-pong kernel on 256x256 tiles whatever the switches say, so every output is bit-identical"""
    t0 = time.time()
    base = _rec(ops_default)
    n0, want = PE.switch_calls(base, dev, _gen(303))
    rec = _rec(ops, SWITCH_SETS[sw])
    n, got = PE.switch_calls(rec, dev, _gen(303))
    _done(rec, t0, n, ROW_LABELS, ("tail split", "duo", "MFMA 128x128", "slabs"))
    assert not base.failures and len(base.checked) == n0 == n and len(want) == len(got)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(Recorder._raw(a), Recorder._raw(b)), f"output {i} differs from the default switches' bits"


def run_combines(ops=None, dev="cuda", **kw):
    t0 = time.time()
    rec = _rec(ops)
    n = PE.combines(rec, dev, _gen(304), **kw)
    if kw:
        return rec, n
    _done(rec, t0, n, ["rowmax_combine_kernel", "rowsample_combine_kernel", "rowscore_combine_kernel + totals",
                       "rowscore_combine_kernel second pass + totals"], ("ping-pong",))
    assert "rowscore_combine_kernel" in labels(rec)                            # (totals = NULL)
    for nm, outs in (("rowmax_combine", ("row_maxprob", "row_argmax", "row_lse")), ("rowsample_combine", ("row_prob", "row_id", "row_lse")),
                     ("rowscore_combine", ("row_nll", "row_pred", "row_max", "totals"))):
        calls = [a for k, a in rec.checked if k == nm]
        for o in outs:                                                          # each optional output absent and present
            assert any(a[o] is None for a in calls) and any(a[o] is not None for a in calls), (nm, o)


def run_logits(ops=None, dev="cuda", **kw):
    t0 = time.time()
    rec = _rec(ops)
    n = PE.logits(rec, dev, _gen(305), **kw)
    if kw:
        return rec, n
    _done(rec, t0, n, ["score_rows_kernel + totals", "score_rows_kernel second pass + totals", "score_rows_kernel + totals no labels",
                       "sample_rows_kernel"])
    assert {a["inv_T"] for nm, a in rec.checked if nm == "sample_rows"} == {1e-3, 1.0, 1e3}


def run_rejected(ops=None, ops_f32=None, dev="cuda", error=None):
    if ops is None:
        from xlxmert_amd.ops import HipOps, XlError
        ops, ops_f32, error = HipOps(torch.bfloat16), HipOps(torch.float32), XlError
    n = PE.rejected(ops, dev, _gen(306), error, ops_f32)
    print(f"{n} calls refused")
    assert n == 3 * 16 + 1 + 3 + 8, n        # 16 per epilogue, p_drop for two, the labels for one; 8 of the combines and logits kernels


# ---------------------------------------------------------------------------------------------------------------------- tests
def test_predict_gemm_epilogues_with_their_combines_within_bounds():
    run_fused()


@pytest.mark.parametrize("tail", [False, True], ids=["two_rounds", "tail_split"])
def test_predict_gemm_epilogues_past_256_tiles_within_bounds(tail):
    """(4352, 4096, 1096): 272 tiles.  Pins the answer to what XL_EPI_ROWMAX does with a slab workspace on its stream: its last 16
    tiles run as two K slices each and the records pass; XL_EPI_ROWSAMPLE and XL_EPI_ROWSCORE stay on whole tiles."""
    run_rounds(tail)


@pytest.mark.parametrize("sw", list(SWITCH_SETS))
def test_predict_gemm_epilogues_ignore_the_gemm_switches_bit_for_bit(sw):
    run_switches(sw)


def test_predict_combines_over_synthetic_records_within_bounds():
    run_combines()


def test_predict_logits_kernels_within_bounds():
    run_logits()


def test_predict_rejected_calls_raise_and_write_nothing():
    run_rejected()
