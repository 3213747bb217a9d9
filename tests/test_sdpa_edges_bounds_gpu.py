"""xl_sdpa_fwd, xl_sdpa_bwd and xl_attn_probs on the on-chip path (nq, nk <= 64, csrc/sdpa.hip) at the edges of their dispatch,
element by element under the float64 bounds of tests/bounds.py through the recording proxy of tests/test_kernel_bounds_gpu.py.  The
calls are those of tests/sdpa_edge_cases.py: both sides of every fragment boundary at dh 16 / 32 / 64 with and without a key mask
and through the three backward instantiations, with the LDS transpose read on and off; every condition of mfma_eligible broken
alone (the bf16 generic kernels) and the same shapes in fp32; packed rows with lengths of 0, 1, 32, 33, the capacity and beyond it
and pads of 0, 1 and 37 rows; the bias gradient through fused partials and through column sums, across the workspace limit and
with deferred second stages; seeds above 2^32 and the step seed; scores of +-60; xl_attn_probs; the calls the entry points refuse.

Operands are fused as the engine's are and sit in +-2^12, outputs in a sentinel: an element read or written one row, one head or
one query too far fails a bound or the row "outside view", which holds every storage involved -- inputs included -- to its earlier
bits outside the logical views.  The keep_bits buffer is compared bit for bit with the layout documented at struct KeepBits.

One test per family (x head size / switch / type), a fresh library context each.  Every test ends with: no unchecked op, no
failure, one checked call per issued call, one outside-view row per checked call, and the kernel labels it expects -- a sweep
that lands on one kernel fails."""
import time

import pytest
import torch

import sdpa_edge_cases as SE
from test_gemm_edges_bounds_gpu import _gen, _summary, labels
from test_kernel_bounds_gpu import Recorder, _table

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
FRAGS = ("1x1", "1x2", "2x1", "2x2")
BIAS_LABELS = ("fused bias", "separate colsum", "separate colsum no workspace")


def _rec(ops, dtype=torch.bfloat16, tr_read=1):
    if ops is None:
        from xlxmert_amd.ops import HipOps
        ops = HipOps(dtype)
    rec = Recorder(ops)
    if not tr_read:
        rec.set_lds_transpose_read(0)
    return rec


def _done(rec, t0, n_calls, expect, absent=(), flushes=0):
    """every issued call was checked (its signature was new) and has its outside-view row; every label of `expect` is part of a
    kernel label produced, none of `absent` is.  Returns (rec, n_calls) for the host runs that count failures."""
    _table(rec.rows, time.time() - t0)
    _summary(rec)
    got = labels(rec)
    print("kernel labels:", *sorted(got), sep="\n  ")
    if getattr(rec._ops, "fault", None) is not None:          # (the host twin with a planted fault asserts on the failures itself)
        return rec, n_calls
    assert not rec.unchecked, sorted(rec.unchecked)
    assert not rec.failures, "\n".join(rec.failures)
    assert not rec.leftover(), rec.leftover()
    assert len(rec.checked) == n_calls, (len(rec.checked), n_calls)
    assert sum(w == "outside view" for _, w, _, _, _ in rec.rows) == n_calls
    assert flushes is None or rec.flushes_checked == flushes, (rec.flushes_checked, flushes)
    for e in expect:
        assert any(e in k for k in got), (e, sorted(got))
    for e in absent:
        assert not any(e in k for k in got), (e, sorted(got))
    return rec, n_calls


# The bodies take (ops, dev) so that tests/test_bounds_cpu.py runs the same code over the host restatement: the labels depend on
# the arguments and the switches only, so the label assertions hold there as they do here.
def run_fragments(dh, tr_read, ops=None, dev="cuda", **subset):
    t0 = time.time()
    rec = _rec(ops, tr_read=tr_read)
    n = SE.fragments(rec, dev, _gen(301), dhs=(dh,), **subset)
    expect = [] if subset else [f"sdpa_{d}_mfma {f}{s}" for d in ("fwd", "bwd") for f in FRAGS for s in ("", " + dropout", " + dropout keep_bits")]
    return _done(rec, t0, n, expect, ["generic", "flash", "long"])


def run_eligibility(dtype, ops=None, dev="cuda", **subset):
    t0 = time.time()
    rec = _rec(ops, dtype)
    n = SE.eligibility(rec, dev, _gen(302), dtype, **subset)
    return _done(rec, t0, n, ["sdpa_fwd_generic", "sdpa_bwd_generic"], ["mfma", "flash", "long"])


def run_packed(dtype, path, ops=None, dev="cuda", **subset):
    t0 = time.time()
    rec = _rec(ops, dtype)
    n = SE.packed(rec, dev, _gen(303), dtype, path, **subset)
    kind = "mfma" if (path == "mfma" and dtype == torch.bfloat16) else "generic"
    other = "generic" if kind == "mfma" else "mfma"
    return _done(rec, t0, n, [f"sdpa_fwd_{kind}", f"sdpa_bwd_{kind}", "packed"] + ([" + dropout keep_bits packed"] if kind == "mfma" else []),
                 [other, "flash", "long"])


def run_bias_gradients(ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(ops)
    n = SE.bias_gradients(rec, dev, _gen(304))
    rec_, n = _done(rec, t0, n, ["sdpa_bwd_mfma 1x2 + dropout fused bias", "sdpa_bwd_mfma 1x2 separate colsum no workspace",
                                 "sdpa_bwd_generic + dropout separate colsum", "sdpa_bwd_generic separate colsum no workspace",
                                 "sdpa_bwd_mfma 1x2 + dropout packed fused bias", "sdpa_bwd_generic packed separate colsum",
                                 "sdpa_bwd_mfma 1x1 fused bias", "sdpa_bwd_mfma 1x1 separate colsum"],
                     flushes=2 if dev == "cuda" else None)   # (the host restatement reduces at once)
    if getattr(rec._ops, "fault", None) is None:
        got = {next(b for b in BIAS_LABELS[::-1] if k.endswith(b)) for k in labels(rec)}
        assert got == set(BIAS_LABELS), got
        assert sum(w.startswith("bias ") for _, w, _, _, _ in rec.rows) == 3 * n
    return rec_, n


def run_dropout(ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(ops)
    n = SE.dropout(rec, dev, _gen(305))
    rec_, n = _done(rec, t0, n, ["sdpa_fwd_mfma 2x2 + dropout keep_bits", "sdpa_bwd_mfma 1x2 + dropout", "sdpa_bwd_mfma 2x1 + dropout keep_bits",
                                 "sdpa_fwd_mfma 1x1 keep_bits"])
    if getattr(rec._ops, "fault", None) is None:
        assert sum(w == "keep_bits" for _, w, _, _, _ in rec.rows) == 3          # every forward that saves its decisions
    return rec_, n


def run_extremes(ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(ops)
    n = SE.extremes(rec, dev, _gen(306))
    return _done(rec, t0, n, ["sdpa_fwd_mfma 2x2", "sdpa_bwd_mfma 2x1 + dropout", "sdpa_fwd_generic", "sdpa_bwd_generic + dropout"])


def run_attn_probs(dtype, ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(ops, dtype)
    n = SE.attn_probs(rec, dev, _gen(307), dtype)
    return _done(rec, t0, n, ["attn_probs_kernel", "attn_probs_kernel + dropout packed", "attn_probs_kernel packed"])


def run_rejected(dtype, ops=None, dev="cuda", error=None):
    if ops is None:
        from xlxmert_amd.ops import HipOps
        ops = HipOps(dtype)
    if error is None:
        from xlxmert_amd._lib import XlError as error
    assert SE.rejected(ops, dev, _gen(308), dtype, error) == 24 + 7 + 2 + (7 if dtype == torch.bfloat16 else 2)
    if hasattr(ops, "dt"):                                     # an element type the library does not have
        c = SE.Case(_gen(309), dev, 2, 2, 4, 4, 16, dtype)
        was, ops.dt = ops.dt, 7
        try:
            with pytest.raises(error):
                c.fwd(ops)
            with pytest.raises(error):
                c.bwd(ops)
            with pytest.raises(error):
                c.probs(ops)
        finally:
            ops.dt = was
        assert bool((c.o[:c.rq * c.ld["ldo"]] == SE.SENTINEL).all()) and bool((c.lse == SE.SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("tr_read", [1, 0], ids=["transpose_read", "plain_lds_read"])
@pytest.mark.parametrize("dh", [16, 32, 64])
def test_attention_fragment_boundaries_masks_and_backward_instantiations_within_bounds(dh, tr_read):
    run_fragments(dh, tr_read)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_attention_generic_kernels_for_every_single_ineligibility_within_bounds(dt):
    run_eligibility(DTYPES[dt])


@pytest.mark.parametrize("dt,path", [("bf16", "mfma"), ("bf16", "generic"), ("fp32", "mfma")], ids=["mfma", "bf16_generic_odd_ld", "fp32"])
def test_attention_packed_rows_lengths_and_pads_within_bounds(dt, path):
    run_packed(DTYPES[dt], path)


def test_attention_bias_gradients_fused_separate_and_across_the_workspace_limit_within_bounds():
    run_bias_gradients()


def test_attention_dropout_seeds_step_seed_and_saved_keep_bits_within_bounds():
    run_dropout()


def test_attention_scores_of_sixty_and_strongly_negative_rows_within_bounds():
    run_extremes()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_attention_probabilities_packed_masked_dropped_and_odd_strides_within_bounds(dt):
    run_attn_probs(DTYPES[dt])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_attention_rejected_calls_raise_and_write_nothing(dt):
    run_rejected(DTYPES[dt])
