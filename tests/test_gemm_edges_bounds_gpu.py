"""xl_gemm and xl_gemm_wgrad_group at the edges of their dispatch (csrc/gemm.hip), element by element under the float64 bounds of
tests/bounds.py through the recording proxy of tests/test_kernel_bounds_gpu.py.  The calls are those of tests/gemm_edge_cases.py
(K below 8 and 64 and off 8, every layout, tight / padded / odd leading dimensions and a shifted base, all epilogues through the
templated, the generic and the scalar path, fused and separate column sums, K splits by atomics and by slabs, the tail split, the
duo tile, grouped and ungrouped weight gradients); operand pads hold +-2^12, so a pad element that leaks in as a K term fails its
bound, and every output's storage outside its [M, N] view is held to its earlier bits ("C outside view").

One test per switch set x family, a fresh library context each.  Every test ends with: no unchecked op, no failure, one checked
call per issued call, and the kernel labels (the restatement of the dispatch: gemm_kernel / wgrad_group_kernel) it expects --
a sweep that lands on one kernel fails."""
import time

import pytest
import torch

import gemm_edge_cases as GE
from test_kernel_bounds_gpu import Recorder, _table

pytestmark = pytest.mark.gpu

SWITCH_SETS = {"default": (), "pingpong_forced": (("set_gemm_pingpong", 2),), "mfma_128_only": (("set_gemm_pingpong", 0),),
               "transpose_read_off": (("set_lds_transpose_read", 0),)}


def _rec(ops, switches=(), slabs=False, workspace=False):
    if ops is None:
        from xlxmert_amd.ops import HipOps
        ops = HipOps(torch.bfloat16)
    rec = Recorder(ops)
    for name, v in switches:
        getattr(rec, name)(*(v if isinstance(v, tuple) else (v,)))
    if slabs:
        rec.set_gemm_wgrad_slabs(1)
    if workspace or slabs:
        rec.gemm_workspace(256)
    return rec


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def labels(rec):
    return {k for _, _, _, k, _ in rec.rows}


def _summary(rec):
    """the smallest headroom (bound / worst |err|) per kernel label and output, with the number of rows it is the smallest of"""
    best = {}
    for _, what, shape, kern, ratio in rec.rows:
        k = (kern, "dW" if what.startswith("dW[") else what)
        n, r, s = best.get(k, (0, -1.0, ""))
        best[k] = (n + 1, ratio, shape) if ratio > r else (n + 1, r, s)
    print(f"\n{'kernel':<72} {'output':<16} {'rows':>5} {'min headroom':>13}  at")
    for (kern, what), (n, r, shape) in sorted(best.items()):
        print(f"{kern:<72} {what:<16} {n:>5} {'exact' if r == 0 else f'{1.0 / r:12.3f}x':>13}  {shape}")


def _done(rec, t0, n_calls, expect, absent=()):
    """as test_kernel_bounds_gpu._done, and: every issued call was checked (its signature was new), every label of `expect` is the
    prefix of a kernel label produced, none of `absent` is"""
    _table(rec.rows, time.time() - t0)
    _summary(rec)
    assert not rec.unchecked, sorted(rec.unchecked)
    assert not rec.failures, "\n".join(rec.failures)
    assert len(rec.checked) == n_calls, (len(rec.checked), n_calls)
    assert len(rec.rows) >= 2 * n_calls, len(rec.rows)
    assert sum(w == "C outside view" for _, w, _, _, _ in rec.rows) == n_calls
    got = labels(rec)
    print("kernel labels:", *sorted(got), sep="\n  ")
    for e in expect:
        assert any(e in k for k in got), (e, sorted(got))
    for e in absent:
        assert not any(e in k for k in got), (e, sorted(got))


# The bodies take (ops, dev) so that tests/test_bounds_cpu.py runs the same code over the host restatement: the labels depend on
# the arguments and the switches only, so the label assertions hold there as they do here.
def run_shapes(sw, ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(ops, SWITCH_SETS[sw])
    # the generic-kernel policies do not depend on the switches: with the default set only
    n = GE.shapes(rec, dev, _gen(101), lds=GE.LD_MFMA + (GE.LD_GENERIC if sw == "default" else ()))
    expect = {"default": ["generic 64x64", "MFMA 128x128 + scalar edge epilogue"],
              "pingpong_forced": ["ping-pong 256x256 + scalar edge epilogue", "MFMA 128x128 + scalar edge epilogue"],   # (K % 8 != 0)
              "mfma_128_only": ["MFMA 128x128 + scalar edge epilogue"],
              "transpose_read_off": ["MFMA 128x128 plain LDS read + generic epilogue"]}[sw]
    absent = {"default": ["ping-pong"], "pingpong_forced": [], "mfma_128_only": ["ping-pong", "generic 64x64"],
              "transpose_read_off": ["ping-pong", "generic 64x64"]}[sw]
    _done(rec, t0, n, expect, absent)


def run_epilogues(sw, ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(ops, SWITCH_SETS[sw])
    n = GE.epilogues(rec, dev, _gen(102))
    base = {"default": "MFMA 128x128", "pingpong_forced": "ping-pong 256x256", "mfma_128_only": "MFMA 128x128",
            "transpose_read_off": "MFMA 128x128 plain LDS read"}[sw]
    expect = [base + " + scalar epilogue", base + " + generic epilogue"]
    if sw != "transpose_read_off":
        expect.append(base + " + scalar edge epilogue")
    _done(rec, t0, n, expect)
    # GELU_DG with b_kmajor = 0 and MULAUX with b_kmajor = 1 have no templated instance: generic also with 16-byte rows
    for epi, bk in ((GE.BD.EPI_GELU_DG, 0), (GE.BD.EPI_MULAUX, 1)):
        ks = {a["_kernel"] for nm, a in rec.checked if nm == "gemm" and a["epilogue"] == epi and a["b_kmajor"] == bk}
        assert ks and all("scalar epilogue" in k or "generic epilogue" in k for k in ks), (epi, bk, ks)


def run_colsums(sw, ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(ops, SWITCH_SETS[sw])
    n = GE.colsums(rec, dev, _gen(103))
    base = "ping-pong 256x256" if sw == "pingpong_forced" else "MFMA 128x128"
    _done(rec, t0, n, [base + " + fused colsum", base + " + scalar edge epilogue + separate colsum"])
    assert sum(w == "colsum" for _, w, _, _, _ in rec.rows) == n


def run_ksplits(sw, slabs, ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(ops, SWITCH_SETS[sw], slabs=slabs)
    n = GE.ksplits(rec, dev, _gen(104))
    base = "ping-pong 256x256" if sw == "pingpong_forced" else "MFMA 128x128"
    how = "slabs" if (slabs and sw == "pingpong_forced") else "atomics"       # (slabs: the ping-pong kernel only)
    _done(rec, t0, n, [f"{base} split-K 2 {how}", f"{base} split-K 4 {how}"], ["slabs"] if how == "atomics" else ["atomics"])


def run_tail_split(ops=None, dev="cuda", shape=GE.TAIL_SHAPE, label="tail split 16x2"):
    t0 = time.time()
    rec = _rec(ops, (("set_gemm_tail_split", (64, 1024)),), workspace=True)
    n = GE.tail_split(rec, dev, _gen(105), shape)
    _done(rec, t0, n, [f"ping-pong 256x256 + {label} + scalar edge epilogue"])
    assert all("tail split" in k for k in labels(rec)), labels(rec)


def run_duo(ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(ops, (("set_gemm_duo", 2),))
    n = GE.duo(rec, dev, _gen(106))
    _done(rec, t0, n, ["duo 128x192"])
    assert labels(rec) == {"duo 128x192"}, labels(rec)


def run_wgrad_groups(slabs, ops=None, dev="cuda"):
    t0 = time.time()
    rec = _rec(ops, slabs=slabs)
    n = GE.wgrad_groups(rec, dev, _gen(107))
    how = "slabs" if slabs else "atomics"
    _table(rec.rows, time.time() - t0)
    _summary(rec)
    assert not rec.unchecked and not rec.failures, "\n".join(rec.failures)
    assert len(rec.checked) == n and sum(w == "C outside view" for _, w, _, _, _ in rec.rows) == n
    assert len(rec.rows) == 3 * 4 + 1 + n, len(rec.rows)
    got = labels(rec)
    print("kernel labels:", *sorted(got), sep="\n  ")
    for e in (f"grouped ping-pong 256x256 split-K 8 {how}", f"grouped ping-pong 256x256 split-K 8 {how} + scalar edge epilogue",
              "ungrouped MFMA 128x128 split-K", "ungrouped MFMA 128x128 += atomics", "ungrouped ping-pong 256x256 split-K 4 " + how):
        assert any(e in k for k in got), (e, sorted(got))


# ---------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("sw", list(SWITCH_SETS))
def test_gemm_shapes_layouts_and_leading_dimensions_within_bounds(sw):
    run_shapes(sw)


@pytest.mark.parametrize("sw", list(SWITCH_SETS))
def test_gemm_epilogues_templated_generic_and_scalar_within_bounds(sw):
    run_epilogues(sw)


@pytest.mark.parametrize("sw", ["default", "pingpong_forced"])
def test_gemm_column_sums_fused_and_separate_within_bounds(sw):
    run_colsums(sw)


@pytest.mark.parametrize("slabs", [False, True], ids=["atomics", "slabs"])
@pytest.mark.parametrize("sw", ["default", "pingpong_forced"])
def test_gemm_k_splits_with_short_last_slice_within_bounds(sw, slabs):
    run_ksplits(sw, slabs)


def test_gemm_tail_split_with_ragged_m_and_n_within_bounds():
    """(4300, 4090, 1096): 272 tiles, the 16 of the last round split in two K slices that meet in slabs.  The whole output is
    checked, no row subset."""
    run_tail_split()


def test_gemm_duo_tiles_within_bounds():
    run_duo()


@pytest.mark.parametrize("slabs", [False, True], ids=["atomics", "slabs"])
def test_grouped_weight_gradients_ragged_mixed_overwrite_within_bounds(slabs):
    run_wgrad_groups(slabs)
