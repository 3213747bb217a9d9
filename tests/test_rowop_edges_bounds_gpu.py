"""The row kernels and the optimizer kernels (csrc/rowops.hip, csrc/optim.hip) at the edges of their dispatch, element by element
under the float64 bounds of tests/bounds.py through the recording proxy of tests/test_kernel_bounds_gpu.py.  The calls are those of
tests/rowop_edge_cases.py: every NIT of the LayerNorm family with whole and ragged last vectors, the grid caps and their ragged
second pass, the boundary of the DMA backward, LDS and generic feature-encoder kernels, sorted and scanning embedding backward
with runs across the 32-candidate chunks, column sums across the slab doubling, all four cross-entropy kernels and each reason
for the scalar one, deferred and batched second stages, the optimizer's loops, tails, flags and schedule branches.  Operand pads
and guards hold +-2^12, so an element read outside the logical extents fails its bound; every output is a view between guards and
its storage outside the view is held bit-identical (the row "outside view").

One test per family x library element type, a fresh recorder each.  Every test ends with: no unchecked op, no failure, one checked
call and one "outside view" row per issued call, and the kernel labels (rowop_kernel: the restatement of the launchers' dispatch)
the family is meant to reach -- a sweep that lands on one kernel fails -- and none it must not reach."""
import time

import pytest
import torch

import rowop_edge_cases as RE
from residual_checks import RecorderRes
from test_gemm_edges_bounds_gpu import labels
from test_kernel_bounds_gpu import Recorder, _sync, _table

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = {"bf16": BF, "fp32": F32}


def _rec(dtype, ops=None, cls=Recorder):
    if ops is None:
        from xlxmert_amd.ops import HipOps
        ops = HipOps(dtype)
    return cls(ops)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _summary(rec):
    """the smallest headroom (bound / worst |err|) per kernel label and output, with the number of rows it is the smallest of"""
    best = {}
    for _, what, shape, kern, ratio in rec.rows:
        n, r, s = best.get((kern, what), (0, -1.0, ""))
        best[(kern, what)] = (n + 1, ratio, shape) if ratio > r else (n + 1, r, s)
    print(f"\n{'kernel':<76} | {'output':<28} | {'rows':>5} | {'min headroom':>13} | at")
    for (kern, what), (n, r, shape) in sorted(best.items()):
        print(f"{kern:<76} | {what:<28} | {n:>5} | {'exact' if r == 0 else f'{1.0 / r:12.3f}x':>13} | {shape}")


def _done(rec, t0, n_calls, expect, absent=()):
    """no unchecked op, no failure, every issued call checked (its signature was new) with one "outside view" row, every label of
    `expect` is part of a kernel label produced, none of `absent` is"""
    _table(rec.rows, time.time() - t0)
    _summary(rec)
    assert not rec.unchecked, sorted(rec.unchecked)
    assert not rec.failures, "\n".join(rec.failures)
    assert not rec.leftover(), rec.leftover()
    assert len(rec.checked) == n_calls, (len(rec.checked), n_calls)
    assert sum(w == "outside view" for _, w, _, _, _ in rec.rows) == n_calls
    assert len(rec.rows) >= 2 * n_calls, len(rec.rows)
    got = labels(rec)
    print("kernel labels:", *sorted(got), sep="\n  ")
    for e in expect:
        assert any(e in k for k in got), (e, sorted(got))
    for e in absent:
        assert not any(e in k for k in got), (e, sorted(got))


def _tn(dtype):
    return "bf16" if dtype == BF else "f32"


# The bodies take (ops, dev) so that tests/test_bounds_cpu.py runs the same code over the host restatement: the labels depend on
# the arguments only, so the label assertions hold there as they do here.
def run_layernorm(dtype, ops=None, dev="cuda", **kw):
    t0 = time.time()
    rec = _rec(dtype, ops)
    n = RE.layernorm(rec, dev, _gen(201), dtype, **kw)
    if kw:
        return rec, n
    t = _tn(dtype)
    expect = [f"ln_fwd_kernel<{t}> NIT={k}" for k in (1, 2, 4, 8)]
    expect += [f"ln_bwd_kernel<{t}> NIT={k} {how}" for k in (1, 2, 4, 8) for how in ("workspace", "atomics", "grid-capped workspace",
                                                                                       "grid-capped atomics")]
    if dtype == BF:     # (8191, 512): a row short of the DMA variant; (8192, 1032): past its two 1 KiB vectors
        expect += ["ln_bwd_dma_kernel<1> grid-capped workspace", "ln_bwd_dma_kernel<1> grid-capped atomics",
                   "ln_bwd_dma_kernel<2> grid-capped workspace", "ln_bwd_dma_kernel<2> grid-capped atomics"]
        dma = {(a["M"], a["N"]): a["_kernel"] for nm, a in rec.checked if nm == "layernorm_bwd" and a["M"] > 8000 and a["ws"] is not None}
        assert {mn: k.split(" ")[0] for mn, k in dma.items()} == {
            (8191, 512): "ln_bwd_kernel<bf16>", (8192, 512): "ln_bwd_dma_kernel<1>", (8192, 520): "ln_bwd_dma_kernel<2>",
            (8192, 1024): "ln_bwd_dma_kernel<2>", (8192, 1032): "ln_bwd_kernel<bf16>", (8200, 264): "ln_bwd_dma_kernel<1>"}, dma
    _done(rec, t0, n, expect, () if dtype == BF else ("ln_bwd_dma_kernel", "bf16"))
    # dbias_prev was checked with and without dropout
    for p_on in (True, False):
        assert any(nm == "layernorm_bwd" and a["dbias_prev"] is not None and (a["p_drop"] > 0) == p_on for nm, a in rec.checked), p_on
    assert sum(w == "dbias_prev" for _, w, _, _, _ in rec.rows) == sum(nm == "layernorm_bwd" and a["dbias_prev"] is not None
                                                                       for nm, a in rec.checked)


def run_layernorm_res(ops=None, dev="cuda", **kw):
    t0 = time.time()
    rec = _rec(BF, ops, RecorderRes)
    n = RE.layernorm_res(rec, dev, _gen(202), **kw)
    if kw:
        return rec, n
    expect = [f"ln_fwd_res_kernel NIT={k}" for k in (1, 2, 3, 4, 8)]
    expect += [f"ln_bwd_res_kernel NIT={k} {how}" for k in (1, 2, 3, 4, 8) for how in ("workspace", "atomics", "grid-capped workspace",
                                                                                        "grid-capped atomics")]
    _done(rec, t0, n, expect)


def run_visn_ln(dtype, ops=None, dev="cuda", **kw):
    t0 = time.time()
    rec = _rec(dtype, ops)
    n = RE.visn_ln(rec, dev, _gen(203), dtype, **kw)
    if kw:
        return rec, n
    t = _tn(dtype)
    expect = [f"visn_ln_fwd_lds_kernel<{t}> NIT={k}" for k in (1, 2)] + [f"visn_ln_fwd_kernel<{t}> NIT={k}" for k in (1, 2, 4)]
    for how in ("workspace", "atomics", "grid-capped workspace", "grid-capped atomics"):
        expect += [f"visn_ln_bwd_lds_kernel<{t}> NIT={k} {how}" for k in (1, 2)]
        expect += [f"visn_ln_bwd_kernel<{t}> NIT={k} {how}" for k in (1, 2, 4)]
    _done(rec, t0, n, expect, ("NIT=8",))
    # P <= 4 beyond 128 VEC columns runs the generic kernels: at the largest N no LDS kernel
    big = max(RE.VISN_N[dtype])
    assert all("lds" not in a["_kernel"] for nm, a in rec.checked if a["N"] == big)


def run_embeddings(dtype, ops=None, dev="cuda", **kw):
    t0 = time.time()
    rec = _rec(dtype, ops)
    n = RE.embeddings(rec, dev, _gen(204), dtype, **kw)
    if kw:
        return rec, n
    t = _tn(dtype)
    passes = (1, 2) if dtype == BF else (1, 2, 4)
    expect = [f"embed_ln_fwd_kernel<{t}> NIT={k}" for k in (1, 2, 4, 8)]
    expect += [f"embed_bwd_sorted_kernel<{t}> passes={k} + type kernel + pos kernel" for k in passes]
    expect += [f"embed_bwd_kernel<{t}> passes={k} + pos kernel" for k in passes]
    expect += [f"embed_bwd_sorted_kernel<{t}> passes=1 + pos kernel", f"embed_bwd_kernel<{t}> passes=1 + type kernel + pos kernel"]
    _done(rec, t0, n, expect, () if dtype == F32 else ("passes=4",))
    assert sum(w == "rows 0 frozen" for _, w, _, _, _ in rec.rows) == sum(nm == "embed_bwd" for nm, _ in rec.checked)


def run_colsums(dtype, ops=None, dev="cuda", **kw):
    t0 = time.time()
    rec = _rec(dtype, ops)
    n = RE.colsums(rec, dev, _gen(205), dtype, **kw)
    if kw:
        return rec, n
    t = _tn(dtype)
    expect = [f"colsum_kernel<{t}>{m} {how}" for m in ("", " masked") for how in (
        "rows_per_block=128 slabs=1 workspace", "rows_per_block=128 slabs=2 workspace", "rows_per_block=128 slabs=128 workspace",
        "rows_per_block=256 slabs=65 workspace", "rows_per_block=128 slabs=129 atomics", "rows_per_block=128 slabs=1 atomics")]
    _done(rec, t0, n, expect, ("slabs=129 workspace",))


def run_deferred(dtype, ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(dtype, ops)
    rec.set_deferred_reduce(1)
    n, dests, keep, groups = RE.deferred(rec, dev, _gen(206), dtype)
    # the flush reaches both cuts: the alias after one entry, then a full batch of kBatch = 6, then the last producer alone
    assert RE.flush_batches(groups) == [1, 6, 1], RE.flush_batches(groups)
    rec.flush_reductions()
    _sync()
    del keep
    rec.set_deferred_reduce(0)
    t = _tn(dtype)
    _done(rec, t0, n, [f"ln_bwd_kernel<{t}> NIT=1 workspace", f"ln_bwd_kernel<{t}> NIT=1 grid-capped workspace", f"colsum_kernel<{t}>",
                       f"visn_ln_bwd_lds_kernel<{t}> NIT=1 workspace", f"visn_ln_bwd_lds_kernel<{t}> NIT=2 grid-capped workspace"])
    if dev != "cpu":
        # every column sum was completed by the flush, none by its producer; the shared dgamma / dbeta took two contributions
        whats = [w for _, w, _, _, _ in rec.rows]
        assert rec.flushes_checked == 1 and sum("@flush" in w for w in whats) == len(dests), whats
        assert sum("x2 @flush" in w for w in whats) == 2, whats
    # the same calls, each second stage at once: the same bits (the batched kernel adds the same slices in the same order)
    n2, dests2, _, _ = RE.deferred(rec._ops, dev, _gen(206), dtype)
    _sync()
    assert n2 == n and len(dests2) == len(dests)
    if dev != "cpu":
        for i, (a, b) in enumerate(zip(dests, dests2)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"destination {i}: deferred and immediate second stages differ"


def run_cross_entropy(dtype, ops=None, dev="cuda", **kw):
    t0 = time.time()
    rec = _rec(dtype, ops)
    n = RE.cross_entropy(rec, dev, _gen(207), dtype, **kw)
    if kw:
        return rec, n
    t = _tn(dtype)
    expect = [f"{k}{loop} dlogits {d}" for k in ("ce_row_kernel<2,256>", "ce_row_kernel<5,256>", "ce_row_kernel<4,1024>")
              for loop, d in (("", t), ("", "none"), (" row loop", t))] + [f"ce_kernel (scalar) dlogits {t}", "ce_kernel (scalar) dlogits none"]
    _done(rec, t0, n, expect, ("dlogits bf16",) if dtype == F32 else ("dlogits f32",))
    scalar = [a for nm, a in rec.checked if a["_kernel"].startswith("ce_kernel")]
    assert len(scalar) == len(RE.CE_PATTERNS) + 4 and sum(a["K"] == 1003 for a in scalar) == 4, len(scalar)   # K8 > 32768, and each fallback
    # slots K .. K8 of dlogits: checked as zeros wherever a register kernel ran with K off 8
    assert sum("slots K..K8 zero" in w for _, w, _, _, _ in rec.rows) == sum(
        a["dlogits"] is not None and a["K"] % 8 != 0 and a["_kernel"].startswith("ce_row_kernel") for nm, a in rec.checked)
    # valid labels without a gradient store still give a loss; without labels a loss_out stays as it was
    whats = [w for _, w, _, _, _ in rec.rows]
    assert whats.count("loss untouched") == sum(a["labels"] is None and a["loss_out"] is not None for nm, a in rec.checked) > 0
    assert any(a["labels"] is not None and a["dlogits"] is None and a["row_lse"] is not None for nm, a in rec.checked)
    # the argmax rule is sharp: on the float64 logits alone every row admits ONE column, but for the one planted tie per call
    with_am = [a for nm, a in rec.checked if a["row_argmax"] is not None]
    assert len(with_am) == len(rec.sharp)
    for a, (_, share, most) in zip(with_am, rec.sharp):
        assert round(share * a["M"]) == 1 and most == 2, (a["M"], a["K"], share, most)


def run_elementwise(dtype, ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(dtype, ops)
    n = RE.elementwise(rec, dev, _gen(208), dtype)
    t = _tn(dtype)
    _done(rec, t0, n, [f"dropout_kernel<{t}>", f"gelu_bwd_kernel<{t}>", f"tanh_bwd_kernel<{t}>", f"bce_logits_kernel dlogits {t}",
                       "bce_logits_kernel (no gradient)", f"move_rows_kernel<{t}> gather", f"move_rows_kernel<{t}> scatter",
                       "gather_labels_kernel", f"codebook_gather_kernel<{t}> masked", "mask_counts_kernel", f"featloss_kernel<{t}> rows centroids",
                       f"featloss_kernel<{t}> targets"])


def run_optimizer(dtype, ops=None, dev="cuda", **kw):
    t0 = time.time()
    rec = _rec(dtype, ops)
    n = RE.optimizer(rec, dev, _gen(209), dtype, **kw)
    if kw:
        return rec, n
    t = _tn(dtype)
    _done(rec, t0, n, ["sumsq_kernel grid=1 tail", "sumsq_kernel grid=1 single", "sumsq_kernel grid=1 single tail", "sumsq_kernel grid=512 single tail",
                       "sumsq_kernel grid=512 unrolled single tail", "adamw_kernel passes=1 compute copy none",
                       f"adamw_kernel passes=1 compute copy {t} flags chunk_steps clip zero_grad", f"adamw_kernel passes=2 compute copy {t} flags clip zero_grad",
                       "adamw_kernel passes=2 compute copy none flags chunk_steps clip", f"adamw_kernel passes=2 compute copy {t} clip",
                       "schedule_step_kernel warm-up", "schedule_step_kernel decay", "schedule_step_kernel decay clamped",
                       f"cast_from_f32_kernel<{t}>", f"cast_to_f32_kernel<{t}>", "take_f32_kernel", "put_f32_kernel"])
    whats = [w for _, w, _, _, _ in rec.rows]
    assert sum(w == "p skipped (bit 1)" for w in whats) == 2 and sum(w == "g kept (bit 2)" for w in whats) == 1, whats


def run_rejected(dtype, ops=None, dev="cuda", error=None):
    if ops is None:
        from xlxmert_amd.ops import HipOps
        ops = HipOps(dtype)
    if error is None:
        from xlxmert_amd._lib import XlError as error
    assert RE.rejected(ops, dev, _gen(210), dtype, error) == 8


# ---------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("dt", list(DTYPES))
def test_layernorm_every_nit_ragged_rows_grid_cap_and_dma_boundary_within_bounds(dt):
    run_layernorm(DTYPES[dt])


def test_residual_stream_layernorm_every_nit_and_grid_cap_within_bounds():
    run_layernorm_res()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_feature_encoder_lds_and_generic_kernels_within_bounds(dt):
    run_visn_ln(DTYPES[dt])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_embedding_forward_and_sorted_scanning_type_and_position_backward_within_bounds(dt):
    run_embeddings(DTYPES[dt])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_column_sums_across_the_slab_doubling_within_bounds(dt):
    run_colsums(DTYPES[dt])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_deferred_batched_second_stages_equal_the_immediate_ones_bit_for_bit(dt):
    run_deferred(DTYPES[dt])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_cross_entropy_register_and_scalar_kernels_within_bounds(dt):
    run_cross_entropy(DTYPES[dt])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_elementwise_copy_mask_and_loss_kernels_off_their_block_within_bounds(dt):
    run_elementwise(DTYPES[dt])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_optimizer_loops_tails_flags_and_schedule_branches_within_bounds(dt):
    run_optimizer(DTYPES[dt])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_launchers_reject_bad_rows_and_bases_without_writing(dt):
    run_rejected(DTYPES[dt])
