"""Every numeric library call of one real bf16 training step, checked element by element against the float64 restatement
(tests/fake_ops.FakeOps(..., compute=torch.float64), run on the device) within the bounds of tests/bounds.py.

The step: the benchmarked geometry (bs 256, 20 text tokens packed, 64 grid tokens, 9/5/5 layers, d 768, 10k codebook, canonical
visual_losses="obj"), dropout on, eager (no launch plan), optimizer in line.  Its HipOps is wrapped by a recording proxy: the first
call of every kernel-selecting signature is run on snapshots of its operands and compared; a numeric method without a checker
fails the test.

Deferred reductions.  With xl_set_deferred_reduce(1) (the default of a training step's backward) a producer's column sums are
not final at its own call: the recorder keeps, per producing stream, a pending list of (destination, float64 contribution,
bound) and checks every destination when flush_reductions / flush_reductions_on combines that stream; a pending entry that no
flush covers, or a destination that also received an unrecorded contribution, fails the test (Recorder.leftover()).

Stray stores.  Around every gemm / gemm_wgrad_group call the whole storage of every output (C, a written aux, the column-sum
target) is held bit for bit -- as integers -- to its content before the call everywhere outside the logical views the call may
write: the row "C outside view".  A store into a pad column of C or past row M-1 lands in a neighbouring tensor.  The launches without a
C (XL_EPI_ROWMAX / ROWSAMPLE / ROWSCORE) hold the storage of aux outside its (N / 64) M records of four floats: "aux outside view".

The predict tail.  Those three epilogues are checked record by record against the float64 logits alpha A B^T + bias (alpha and a NULL
bias included), their combines and the logits twins xl_sample_rows / xl_score_rows on what they read, and a combine behind a checked
launch once more against the float64 logits of the whole row ("composed" rows).  Recorder(ops, every_call=True) checks every call,
whether or not its signature was seen: alpha, seeds and temperatures are no part of a signature (tests/predict_edge_cases.py).

Kernel labels.  The recorder remembers the GEMM switches it forwards (set_gemm_pingpong / _duo / _wgrad_slabs / _tail_split,
set_lds_transpose_read, the slab workspace registered per stream); gemm_kernel / wgrad_group_kernel restate the dispatch of
csrc/gemm.hip under them, and the label is part of a call's signature: the same arguments after a switch change are checked again.

What the proxy switches off.  PretrainStep gates four paths on isinstance(self.ops, HipOps) (trainer.py): (1) a separate bf16
HipOps for a bf16 gradient exchange and (2) the library's RCCL binding -- both only with more than one rank, no numeric call of
a one-GPU step; (3) plan mode -- a recorded launch plan replays the same C-ABI calls without passing through Python, so these
tests run with plan=False by construction; (4) the side stream of the overlapped optimizer -- with the proxy the same grouped
sumsq / adamw calls are issued in the same order on the main stream, placement only.  None of them hides a numeric call of the
product path, so the proxy does not pretend to be a HipOps.  Engine gates nothing on the type (fused_predict_available asks
hasattr(ops, "rowmax_combine"), which the proxy forwards)."""
import inspect
import time

import pytest
import torch

import bounds as BD
import bounds_eval as BE
import bounds_sampling as BS
import lxmert_oracle as O
from fake_ops import FakeOps, ce_in_regs, keep_scale
from fake_ops_eval import EPI_ROWSCORE
from fake_ops_sampling import EPI_ROWSAMPLE, gumbel_noise

pytestmark = pytest.mark.gpu

CFG_KEYS = ("vocab_size", "hidden_size", "num_attention_heads", "intermediate_size", "max_position_embeddings",
            "type_vocab_size", "l_layers", "x_layers", "r_layers", "visual_feat_dim", "visual_pos_dim", "num_clusters")

# library calls that compute nothing a later call reads as a number of this step's result: memsets, stream / event plumbing,
# switches, size queries, workspace registration
NON_NUMERIC = {"zero", "stream_fork", "new_event", "event_record", "stream_wait", "set_step_seed_ptr", "set_deferred_reduce",
               "workspace_floats", "gemm_workspace", "sumsq_scratch", "sdpa_keep_bits_bytes", "wgrad_group_one_writer",
               "rebind", "bound", "forget_binding", "gemm_trace"}


# sampler ops: the signature also carries the step index (Recorder.mark), so that every refinement step is checked
STEP_KEYED = {"rowmax_combine", "rowsample_combine", "remask_lowest", "sampler_update", "sampler_ar_update"}
# the column-sum outputs whose second stage xl_set_deferred_reduce(1) postpones to the next flush of the producing stream
REDUCE_OUTS = {"gemm": ("colsum",), "layernorm_bwd": ("dgamma", "dbeta", "dbias_prev"), "sdpa_bwd": ("bias_grad",),
               "visn_ln_bwd": ("dgv", "dbv", "dgb", "dbb", "dwbox", "dbbox", "dbias_visn"), "colsum": ("out",),
               "masked_colsum": ("out",)}


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _is_setter(name):
    return name.startswith("set_")


def _al16(t):
    return None if t is None else t.data_ptr() % 16 == 0


def _v2(t, r, c, ld):
    return torch.as_strided(t, (r, c), (ld, 1))


# the xl_gemm switches of a library context and their library defaults (csrc/common.h Ctx; the XL_GEMM_* environment variables
# give the initial values): what Recorder remembers of the setters it forwards, and what gemm_kernel reads
def gemm_switches():
    import os
    e = lambda k, d: int(os.environ.get(k, d))                  # noqa: E731
    return dict(pingpong=e("XL_GEMM_PP", 1), tr_read=True, duo=e("XL_GEMM_DUO", 1), slabs=e("XL_GEMM_WGRAD_SLABS", 0),
                tail_max=e("XL_GEMM_TAIL_MAX", 64), tail_min_k=e("XL_GEMM_TAIL_MIN_K", 4096), ws_slabs=0)


def _ws_holds(sw, tiles, slabs):
    """slab_workspace(): the stream has a registered workspace with 4096 tickets in front of `ws_slabs` slabs"""
    return sw["ws_slabs"] > 0 and tiles * 4 <= 16384 and slabs <= sw["ws_slabs"]


ROW_EPILOGUES = {5: "ROWMAX", 9: "ROWSAMPLE", 10: "ROWSCORE"}      # no C: segment records in aux (include/xlxmert_hip.h)


def _tail_split(sw, tiles, K):
    """the tail split of a ping-pong launch of 256x256 tiles: more than one round, a last round of at most tail_max tiles, K >=
    tail_min_k, and a slab workspace on the stream that holds the remainder's slices -> the label suffix, "" without a split"""
    if tiles > 256 and 0 < tiles % 256 <= sw["tail_max"] and K >= sw["tail_min_k"]:
        rem = tiles % 256
        S = min(256 // rem, K // 512, 8)
        if S >= 2:
            kper_t = ((K + S - 1) // S + 63) // 64 * 64
            S = (K + kper_t - 1) // kper_t
            if S >= 2 and _ws_holds(sw, rem, rem * S):
                return f" + tail split {rem}x{S}"
    return ""


def gemm_vec_epi(C, ldc, out_f32, epilogue, residual=None, ldr=0, aux=None, ldx=0):
    """p.vec_epi of xl_gemm: 16-byte rows of C and of the epilogue's operand"""
    v = bool(_al16(C)) and (ldc % 4 == 0 if out_f32 else ldc % 8 == 0)
    if epilogue == BD.EPI_RESIDUAL:
        v = v and bool(_al16(residual)) and (ldr % 4 == 0 if residual.dtype == torch.float32 else ldr % 8 == 0)
    if epilogue in (BD.EPI_GELU, BD.EPI_DGELU, BD.EPI_GELU_DG, BD.EPI_MULAUX):
        v = v and bool(_al16(aux)) and ldx % 8 == 0
    return v


def gemm_kernel(M, N, K, lda, ldb, A, B, out_f32, epilogue, a_kmajor=1, b_kmajor=1, accumulate=0, vec_epi=True, bias_al16=True,
                colsum=False, res32=False, sw=None):
    """the kernel xl_gemm's dispatch (csrc/gemm.hip) selects for these arguments under the switches `sw` (gemm_switches(): the
    library defaults):
      generic 64x64         operands the MFMA loader does not take (fp32, a leading dimension off 8, a pointer off 16 bytes)
      ping-pong 256x256     pingpong 2, or 1 and >= 48 tiles of 256x256 (x K splits); needs the LDS transpose read and K % 8 == 0
      duo 128x192           forward / dX layouts, M % 128 == N % 192 == 0, a fast epilogue; duo 1: at most 64 tiles of 256x256
      MFMA 128x128          otherwise (" plain LDS read": the instance without the transpose read)
    suffixes: " split-K S atomics" / " split-K S slabs" (fp32 out, EPI_NONE, K >= 1024, too few tiles; slabs: the ping-pong kernel
    with set_gemm_wgrad_slabs and a registered workspace), " += atomics" (accumulate without a split), " + tail split RxS",
    " + scalar epilogue" (vec_epi == 0: every element through the scalar store), " + generic epilogue" (aligned rows but no
    templated epilogue -- template argument EPIK = -1: TANH, an unaligned bias, GELU_DG with b_kmajor = 0, MULAUX with b_kmajor = 1,
    every launch with a_kmajor = 0, the instance without the transpose read), " + scalar edge epilogue" (a templated epilogue whose
    ragged edge tiles take the scalar store), " + fused colsum" / " + separate colsum".  Held against the kernel names of a
    rocprofv3 --kernel-trace run of tests/test_gemm_edges_bounds_gpu.py once: profiles/bounds_gemm_edges.txt."""
    sw = dict(gemm_switches(), **(sw or {}))
    if epilogue in ROW_EPILOGUES:
        # XL_EPI_ROWMAX / ROWSAMPLE / ROWSCORE: the preconditions leave bf16 K-major operands on whole 256x256 tiles, and use_pp is
        # forced whatever set_gemm_pingpong says; no duo / 192-wide tile, no K split.  ROWMAX alone is not excluded from the tail split
        # (its siblings are, and assert tail_tiles == 0): the last tiles run as K slices whose last arriver runs the epilogue
        name = f"ping-pong 256x256 {ROW_EPILOGUES[epilogue]} epilogue"
        return name + (_tail_split(sw, (M // 256) * (N // 256), K) if epilogue == BD.EPI_ROWMAX else "")
    mfma = A.dtype == torch.bfloat16 and lda % 8 == 0 and ldb % 8 == 0 and bool(_al16(A)) and bool(_al16(B))
    may_split = mfma and out_f32 and epilogue == BD.EPI_NONE
    t256 = ((M + 255) // 256) * ((N + 255) // 256)
    pp_ok = mfma and sw["tr_read"] and K % 8 == 0 and (M if a_kmajor else K) * lda < 1e9 and (N if b_kmajor else K) * ldb < 1e9
    blocks = t256 * max(1, min(256 // t256, K // 512)) if (may_split and t256 < 256 and K >= 1024) else t256
    pp = pp_ok and (sw["pingpong"] == 2 or (sw["pingpong"] == 1 and blocks >= 48))
    tile = 256 if pp else 128 if mfma else 64
    tiles = ((M + tile - 1) // tile) * ((N + tile - 1) // tile)
    want = 256 if pp else 768
    split = 1
    if may_split and tiles < want and K >= 1024:
        split = max(1, min(want // tiles if pp else (want + tiles - 1) // tiles, K // 512))
    kstep = 64 if mfma else 16
    kper = ((K + split - 1) // split + kstep - 1) // kstep * kstep
    split = (K + kper - 1) // kper
    atomic = bool(accumulate) or split > 1
    slabs = pp and split > 1 and sw["slabs"] and _ws_holds(sw, tiles, tiles * split)
    epik = epilogue if (vec_epi and not atomic and epilogue != BD.EPI_TANH and bias_al16) else -1
    if (epilogue == BD.EPI_GELU_DG and not b_kmajor) or (epilogue == BD.EPI_MULAUX and b_kmajor):
        epik = -1
    duo = bool(pp_ok and sw["pingpong"] and sw["duo"] and a_kmajor and M % 128 == 0 and N % 192 == 0 and (not out_f32 or res32)
               and not accumulate and epik >= 0 and not colsum and epilogue != BD.EPI_TANH and split == 1
               and M * lda < 1e9 and (sw["duo"] == 2 or t256 <= 64))
    if not mfma:
        name = "generic 64x64"
    elif duo:
        name, tile = "duo 128x192", None
    elif pp:
        name = "ping-pong 256x256"
    else:
        name = "MFMA 128x128" + ("" if sw["tr_read"] else " plain LDS read")
    if split > 1:
        name += f" split-K {split} " + ("slabs" if slabs else "atomics")
    elif accumulate:
        name += " += atomics"
    if pp and not duo and split == 1 and not atomic:
        name += _tail_split(sw, tiles, K)
    ragged = tile is not None and (M % tile or N % tile)
    if mfma and not atomic:
        if not vec_epi:
            name += " + scalar epilogue"
        elif epik < 0 or not a_kmajor or (not sw["tr_read"] and not pp):
            name += " + generic epilogue"
        elif ragged:
            name += " + scalar edge epilogue"
    if colsum:
        fused = mfma and epik >= 0 and split == 1 and a_kmajor and M % tile == 0 and N % tile == 0
        name += " + fused colsum" if fused else " + separate colsum"
    return name


def wgrad_group_kernel(problems, overwrite_mask=0, sw=None):
    """xl_gemm_wgrad_group (csrc/gemm.hip): problems of (A, B, C, M, N, K, lda, ldb, ldc).  One launch of the grouped ping-pong
    kernel when every member is bf16 with 16-byte rows and K % 8 == 0, there is more than one, the ping-pong family and the transpose
    read are on and the launch puts up >= 96 workgroups; otherwise one xl_gemm per member.  -> (label of the launch, [label per
    member])"""
    sw = dict(gemm_switches(), **(sw or {}))
    grouped = len(problems) > 1 and sw["pingpong"] != 0 and sw["tr_read"]
    total, max_split = 0, 1 << 20
    for A, B, C, M, N, K, lda, ldb, ldc in problems:
        grouped = grouped and A.dtype == torch.bfloat16 and lda % 8 == 0 and ldb % 8 == 0 and bool(_al16(A)) and bool(_al16(B)) \
            and K % 8 == 0 and K * lda < 1e9 and K * ldb < 1e9
        total += ((M + 255) // 256) * ((N + 255) // 256)
        max_split = min(max_split, max(1, K // 512))
    split = 1 if total >= 256 else max(1, min(256 // total, max_split))
    if grouped and total * split < 96:
        grouped = False
    if not grouped:
        return "ungrouped: one xl_gemm per member", ["ungrouped " + gemm_kernel(M, N, K, lda, ldb, A, B, True, BD.EPI_NONE, 0, 0,
                                                        accumulate=0 if (overwrite_mask >> i) & 1 else 1,
                                                        vec_epi=gemm_vec_epi(C, ldc, True, BD.EPI_NONE), sw=sw)
                             for i, (A, B, C, M, N, K, lda, ldb, ldc) in enumerate(problems)]
    ranges = [(C.data_ptr(), C.data_ptr() + ((M - 1) * ldc + N) * 4) for _, _, C, M, N, _, _, _, ldc in problems]
    disjoint = all(not (a0 < b1 and b0 < a1) for i, (a0, a1) in enumerate(ranges) for b0, b1 in ranges[i + 1:])
    slabs = disjoint and sw["slabs"] and _ws_holds(sw, total, total * split)
    how = "slabs" if slabs else "one writer per tile" if (disjoint and split == 1) else "atomics"
    name = f"grouped ping-pong 256x256 split-K {split} {how}" if split > 1 else f"grouped ping-pong 256x256 {how}"
    return name, [name + (" + scalar edge epilogue" if (M % 256 or N % 256 or not (_al16(C) and ldc % 4 == 0)) else "")
                  for _, _, C, M, N, _, _, _, ldc in problems]


def sdpa_kernel(direction, nq, nk, dh, lds, aligned, tr_read=True, dtype=torch.bfloat16, long_mfma=None):
    """the kernel xl_sdpa_fwd / xl_sdpa_bwd (csrc/sdpa.hip) selects: direction "fwd" or "bwd"; lds the leading dimensions the
    entry point tests (fwd: q, k, v, o; bwd: those and dq, dk, dv), `aligned` the 16-byte alignment of the pointers it tests (fwd:
    q, k, v, o; bwd: q, k, v, dout, dq, dk, dv), tr_read the xl_set_lds_transpose_read switch, long_mfma the XL_SDPA_LONG_MFMA
    environment switch (None: read it).  Returns (name, n_kblk, n_qblk): the block counts the bounds need, 1 on the on-chip kernels.
      sdpa_*_mfma QFxKF   nq, nk <= 64, bf16, dh 16 / 32 / 64, every ld a multiple of 8, every pointer 16-byte aligned
      sdpa_*_generic      nq, nk <= 64 otherwise
      sdpa_*_flash        nq or nk in 65..512, the mfma conditions and the transpose read on (bwd: sdpa_bwd_flash_q + _k)
      sdpa_*_long         nq or nk in 65..512 otherwise (bwd: sdpa_bwd_long_q + _k)"""
    assert direction in ("fwd", "bwd")
    if long_mfma is None:
        import os
        e = os.environ.get("XL_SDPA_LONG_MFMA")
        long_mfma = e is None or (e.strip().lstrip("+-").isdigit() and int(e) != 0)
    mfma = dtype == torch.bfloat16 and dh in (16, 32, 64) and all(ld % 8 == 0 for ld in lds) and all(bool(x) for x in aligned)
    if nq > 64 or nk > 64:
        name = f"sdpa_{direction}_flash" if (mfma and tr_read and long_mfma) else f"sdpa_{direction}_long"
        return name, (nk + 63) // 64, (nq + 63) // 64
    if mfma:
        return f"sdpa_{direction}_mfma {(nq + 31) // 32}x{(nk + 31) // 32}", 1, 1
    return f"sdpa_{direction}_generic", 1, 1


SDPA_KERNELS = tuple(f"sdpa_{d}_{k}" for d in ("fwd", "bwd") for k in ("mfma", "flash", "long", "generic"))


# ------------------------------------------------------------------------------------------- row kernels and optimizer: dispatch
def _env_int(k, d):
    import os
    e = os.environ.get(k)
    try:
        return int(e) if e not in (None, "") else d
    except ValueError:
        return 0                                          # (atoi)


def _tn(t):
    return "none" if t is None else {torch.bfloat16: "bf16", torch.float32: "f32"}.get(t.dtype, str(t.dtype))


def _vec(t):
    return 8 if t.dtype == torch.bfloat16 else 4


def _cdiv(a, b):
    return -(-a // b)


def _nit(N, per, steps=(1, 2, 4, 8)):
    """DISPATCH_NIT / DISPATCH_NIT_RES: ceil(N / per) rounded up to the next instantiated count; None: XL_ERR_BAD_SHAPE"""
    n = _cdiv(N, per)
    return next((k for k in steps if n <= k), None)


def _ws(a, key="ws"):
    return " workspace" if a.get(key) is not None else " atomics"


def _k_layernorm_bwd(a):
    M, N, x = a["M"], a["N"], a["x"]
    blocks = _cdiv(M, 8)
    dma = (_env_int("XL_LN_BWD_DMA", 1) and x.dtype == torch.bfloat16 and N <= 1024 and N % 8 == 0
           and M >= _env_int("XL_LN_BWD_DMA_MIN_ROWS", 2 * 512 * 8) and M * N * 2.0 < 2.0e9 and _al16(a["dy"]) and _al16(x))
    name = f"ln_bwd_dma_kernel<{1 if N <= 512 else 2}>" if dma else f"ln_bwd_kernel<{_tn(x)}> NIT={_nit(N, 64 * _vec(x))}"
    return name + (" grid-capped" if blocks > 512 else "") + _ws(a)


def _k_visn(direction):
    def f(a):
        M, N, P, xv = a["M"], a["N"], a["P"], a["xv"]
        lds = P <= 4 and N <= 128 * _vec(xv)
        cap = 512 if (direction == "fwd" and lds) else 256 if direction == "bwd" else None
        blocks = _cdiv(M, 8 if lds else 4)
        name = (f"visn_ln_{direction}_lds_kernel<{_tn(xv)}> NIT={1 if N <= 64 * _vec(xv) else 2}" if lds
                else f"visn_ln_{direction}_kernel<{_tn(xv)}> NIT={_nit(N, 64 * _vec(xv))}")
        name += " grid-capped" if (cap is not None and blocks > cap) else ""
        return name + (_ws(a) if direction == "bwd" else "")
    return f


def _k_embed_bwd(a):
    d = a["dpre"]
    passes = _nit(a["N"], 64 * _vec(d), (1, 2, 4))
    return (f"embed_bwd_{'sorted_' if a['order'] is not None else ''}kernel<{_tn(d)}> passes={passes}"
            + (" + type kernel" if (a["tt"] is not None and a["n_types"] > 1) else "") + " + pos kernel")


def _k_colsum(masked):
    def f(a):
        M, rpb = a["M"], 128
        if a["ws"] is not None:
            while _cdiv(M, rpb) > 128:
                rpb *= 2
        return f"colsum_kernel<{_tn(a['x'])}>{' masked' if masked else ''} rows_per_block={rpb} slabs={_cdiv(M, rpb)}" + _ws(a)
    return f


def _k_ce(a):
    M, K, dl = a["M"], a["K"], a["dlogits"]
    K8 = (K + 7) // 8 * 8
    if not ce_in_regs(a["logits"], dl, K, a["ldl"], a["lddl"]):
        name, cap = "ce_kernel (scalar)", None
    elif K8 > 256 * 8 * 5:
        name, cap = "ce_row_kernel<4,1024>", 1024
    elif K8 > 256 * 8 * 2:
        name, cap = "ce_row_kernel<5,256>", 2048
    else:
        name, cap = "ce_row_kernel<2,256>", 2048
    return name + (" row loop" if (cap is not None and M > cap) else "") + f" dlogits {_tn(dl)}"


def _k_sumsq(a):
    n = a["n"]
    n4 = n >> 2
    grid = min(max(_cdiv(n4, 256), 1), 512)
    stride = grid * 256
    unrolled = n4 > 3 * stride                                  # thread 0 enters the 4x unrolled loop
    rounds = _cdiv(n4 - 3 * stride, 4 * stride) if unrolled else 0
    single = n4 > 4 * stride * rounds                           # ... and is left with i < n4 behind it
    return f"sumsq_kernel grid={grid}" + (" unrolled" if unrolled else "") + (" single" if single else "") + (" tail" if n & 3 else "")


def _k_adamw(a):
    n4 = a["n"] >> 2
    mb = _env_int("XL_ADAMW_BLOCKS", 256)
    grid = min(mb if mb > 0 else 256, _cdiv(n4, 1024))
    return (f"adamw_kernel passes={_cdiv(n4, grid * 1024)} compute copy {_tn(a['p_compute'])}"
            + (" flags" if a["decay_flags"] is not None else "") + (" chunk_steps" if a["chunk_steps"] is not None else "")
            + (" clip" if (a["max_norm"] > 0 and a["sumsq"] is not None) else "") + (" zero_grad" if a["zero_grad"] else ""))


def _k_schedule(a):
    done = int(a["step"][0])
    if done < a["warmup_steps"]:
        return "schedule_step_kernel warm-up"
    return "schedule_step_kernel decay" + (" clamped" if done >= a["total_steps"] else "")


SCORE_MAX_BLOCKS = 1024       # csrc/rowops.hip: the grid cap of rowscore_combine_kernel (64 rows a block) and score_rows_kernel (4 rows)
_ROWOP = {
    "layernorm_fwd": lambda a: f"ln_fwd_kernel<{_tn(a['x'])}> NIT={_nit(a['N'], 64 * _vec(a['x']))}",
    "layernorm_bwd": _k_layernorm_bwd,
    "layernorm_fwd_res": lambda a: f"ln_fwd_res_kernel NIT={_nit(a['N'], 256, (1, 2, 3, 4, 8))}",
    "layernorm_bwd_res": lambda a: (f"ln_bwd_res_kernel NIT={_nit(a['N'], 256, (1, 2, 3, 4, 8))}"
                                    + (" grid-capped" if _cdiv(a["M"], 8) > 512 else "") + _ws(a)),
    "visn_ln_fwd": _k_visn("fwd"), "visn_ln_bwd": _k_visn("bwd"),
    "embed_ln_fwd": lambda a: f"embed_ln_fwd_kernel<{_tn(a['word'])}> NIT={_nit(a['N'], 64 * _vec(a['word']))}",
    "embed_bwd": _k_embed_bwd,
    "colsum": _k_colsum(False), "masked_colsum": _k_colsum(True),
    "ce_fwd_bwd": _k_ce,
    "sumsq": _k_sumsq, "adamw": _k_adamw, "schedule_step": _k_schedule,
    "codebook_gather": lambda a: f"codebook_gather_kernel<{_tn(a['feats'])}>" + (" masked" if a["vis_mask"] is not None else ""),
    "dropout": lambda a: f"dropout_kernel<{_tn(a['x'])}>",
    "gelu_bwd": lambda a: f"gelu_bwd_kernel<{_tn(a['dx'])}> (A-S erf)",
    "tanh_bwd": lambda a: f"tanh_bwd_kernel<{_tn(a['dx'])}>",
    "bce_logits_fwd_bwd": lambda a: "bce_logits_kernel" + (f" dlogits {_tn(a['dlogits'])}" if a["dlogits"] is not None else " (no gradient)"),
    "gather_rows": lambda a: f"move_rows_kernel<{_tn(a['src'])}> gather",
    "scatter_rows": lambda a: f"move_rows_kernel<{_tn(a['src'])}> scatter",
    "gather_labels": lambda a: "gather_labels_kernel",
    "mask_counts": lambda a: "mask_counts_kernel",
    "featloss_fwd_bwd": lambda a: (f"featloss_kernel<{_tn(a['pred'])}>" + (" rows" if a["rows"] is not None else "")
                                   + (" targets" if a["targets"] is not None else " centroids")),
    "cast_from_f32": lambda a: f"cast_from_f32_kernel<{_tn(a['dst'])}>",
    "cast_to_f32": lambda a: f"cast_to_f32_kernel<{_tn(a['src'])}>",
    "take_f32": lambda a: "take_f32_kernel", "put_f32": lambda a: "put_f32_kernel",
    "rowsample_combine": lambda a: "rowsample_combine_kernel",
    "rowscore_combine": lambda a: ("rowscore_combine_kernel" + (" second pass" if _cdiv(a["M"], 64) > SCORE_MAX_BLOCKS else "")
                                   + (" + totals" if a["totals"] is not None else "")),
    "sample_rows": lambda a: "sample_rows_kernel",
    "score_rows": lambda a: ("score_rows_kernel" + (" second pass" if _cdiv(a["M"], 4) > SCORE_MAX_BLOCKS else "")
                             + (" + totals" if a["totals"] is not None else "") + ("" if a["labels"] is not None else " no labels")),
    "rowmax_combine": lambda a: "rowmax_combine_kernel", "remask_lowest": lambda a: "remask_lowest_kernel",
    "sampler_update": lambda a: "sampler_update_kernel",
    "sampler_ar_update": lambda a: "sampler_ar_update_kernel " + ("(fixed position)" if a["fixed_pos"] >= 0 else "(most confident)"),
}


def rowop_kernel(name, a):
    """the kernel(s) an entry point of csrc/rowops.hip / csrc/optim.hip launches for the arguments `a` (the call's tensors and
    scalars by parameter name), as gemm_kernel restates csrc/gemm.hip: the kernel's name and template arguments and what the launcher
    branches on --
      NIT=k          DISPATCH_NIT / DISPATCH_NIT2 / DISPATCH_NIT_RES: 64-lane passes over a row (None: the launcher rejects N)
      grid-capped    the grid is capped (LayerNorm backward 512 blocks of 8 rows, feature-encoder backward 256 blocks), blocks loop
      workspace / atomics   the column sums leave through partial slabs and reduce_partials_kernel, or through atomics
      ln_bwd_dma_kernel<1|2>   bf16, N <= 512 | 1024, N % 8 == 0, M >= 8192 rows, < 2e9 bytes, dy and x on 16 bytes
      visn_ln_*_lds_kernel      P <= 4 and N <= 128 VEC
      embed_bwd_[sorted_]kernel passes=1|2|4 [+ type kernel] + pos kernel
      colsum_kernel rows_per_block=R slabs=G   (R doubles until G <= 128 with a workspace)
      ce_row_kernel<4,1024> / <5,256> / <2,256> [row loop]  or  ce_kernel (scalar)
      sumsq_kernel grid=G [unrolled] [single] [tail];  adamw_kernel passes=k ...;  schedule_step_kernel warm-up / decay [clamped]
      rowscore_combine_kernel / score_rows_kernel [second pass] [+ totals] [no labels]   second pass: more than 1024 blocks of 64 / 4
                     rows, the blocks walk on by the grid
    An entry point without a branch is labelled by its kernel and element type."""
    f = _ROWOP.get(name)
    return f(a) if f is not None else name


def _t(t, *shape):
    """(tensor, shape, contiguous strides) of an output view, None for an absent tensor"""
    if t is None:
        return None
    st, acc = [], 1
    for n in reversed(shape):
        st.append(acc)
        acc *= n
    return (t, tuple(shape), tuple(reversed(st)))


def _t2(t, rows, cols, ld):
    return None if t is None else (t, (rows, cols), (ld, 1))


def _whole(t):
    return None if t is None else (t, tuple(t.shape), tuple(t.stride()))


def _o_ce(a):
    K = a["K"]
    Kw = (K + 7) // 8 * 8 if ce_in_regs(a["logits"], a["dlogits"], K, a["ldl"], a["lddl"]) else K      # the register kernels zero K..K8
    M = a["M"]
    return [_t2(a["dlogits"], M, Kw, a["lddl"]), _t(a["loss_out"], 1), _t(a["row_lse"], M), _t(a["row_argmax"], M), _t(a["row_maxprob"], M)]


def _o_ln_bwd(a):
    M, N = a["M"], a["N"]
    dropped = a["dx_dropped"] is not None and a["p_drop"] > 0            # (p_drop == 0: the launcher drops the pointer -- not written)
    return [_t(a["dx"], M, N), _t(a["dgamma"], N), _t(a["dbeta"], N), _t(a["dbias_prev"], N), _whole(a["ws"]),
            _t(a["dx_dropped"], M if dropped else 0, N)]


def _o_visn_bwd(a):
    M, N, P = a["M"], a["N"], a["P"]
    return [_t(a["dxv"], M, N)] + [_t(a[k], N) for k in ("dgv", "dbv", "dgb", "dbb", "dbbox", "dbias_visn")] + [_t(a["dwbox"], N * P), _whole(a["ws"])]


def _o_adamw(a):
    n = a["n"]
    pc = a["p_compute"] if (a["p_compute"] is not None and a["p_compute"].data_ptr() != a["p"].data_ptr()) else None
    return [_t(a["p"], n), _t(a["m"], n), _t(a["v"], n), _t(a["g"], n if a["zero_grad"] else 0), _t(pc, n)]


def _o_featloss(a):
    n = a["B"] * a["V"] if a["rows"] is None else a["n_rows"]
    return [_t(a["dpred"], n, a["F"]), _t(a["loss_out"], 1)]


def _at(t, k):
    """a one-element view of t's storage k elements behind its base: the anchor of a logical view that starts there"""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + k)


def _held(*ts):
    """tensors a call only reads: an empty view each, so that their whole storage is held to its earlier bits"""
    return [(t, (0,), (1,)) for t in ts if t is not None]


def _o_rows(t, B, n, HD, ld, off, pad):
    """what an attention call writes of a q- or k-side buffer: all H heads of the [len_b, dh] row blocks (dense: B n rows; packed:
    min(n, off[b+1] - off[b]) rows from row off[b] -- rows of an example beyond the capacity stay), and the pad rows [off[B], pad)"""
    if t is None:
        return []
    if off is None:
        return [(t, (B * n, HD), (ld, 1))]
    o = [int(x) for x in off.reshape(-1)[:B + 1]]
    v = [(_at(t, o[b] * ld), (min(n, o[b + 1] - o[b]), HD), (ld, 1)) for b in range(B) if o[b + 1] > o[b]]
    if pad > o[B]:
        v.append((_at(t, o[B] * ld), (pad - o[B], HD), (ld, 1)))
    return v


def _o_lse(lse, B, H, nq, off):
    """the lse entries of the queries that exist ([B, H, nq capacity] indexing)"""
    if off is None:
        return [(lse, (B * H * nq,), (1,))]
    o = [int(x) for x in off.reshape(-1)[:B + 1]]
    return [(_at(lse, b * H * nq), (H, min(nq, o[b + 1] - o[b])), (nq, 1)) for b in range(B) if o[b + 1] > o[b]]


def keep_bits_words(B, H, nq, nk):
    """dwords of the keep_bits buffer (KeepBits::word0 of csrc/sdpa.hip): per problem and 32-query fragment, 32 per key fragment"""
    return B * H * ((nq + 31) // 32) * ((nk + 31) // 32) * 32


def _o_sdpa_fwd(a):
    B, H, nq, nk = a["B"], a["H"], a["nq"], a["nk"]
    written = a["keep_bits"] is not None and a["p_drop"] > 0             # (DROP && keep_bits != nullptr: no store without dropout)
    return (_o_rows(a["o"], B, nq, H * a["dh"], a["ldo"], a["q_off"], a["q_pad"]) + _o_lse(a["lse"], B, H, nq, a["q_off"])
            + ([(a["keep_bits"], (keep_bits_words(B, H, nq, nk),), (1,))] if written else _held(a["keep_bits"]))
            + _held(a["q"], a["k"], a["v"], a["key_mask"]))


def _o_sdpa_bwd(a):
    B, H, nq, nk, HD = a["B"], a["H"], a["nq"], a["nk"], a["H"] * a["dh"]
    return (_o_rows(a["dq"], B, nq, HD, a["lddq"], a["q_off"], a["q_pad"]) + _o_rows(a["dk"], B, nk, HD, a["lddk"], a["k_off"], a["k_pad"])
            + _o_rows(a["dv"], B, nk, HD, a["lddv"], a["k_off"], a["k_pad"])
            + [x for x in (_whole(a["ws"]), _t(a["bias_grad"], 3 * HD)) if x is not None]
            + _held(a["q"], a["k"], a["v"], a["key_mask"], a["dout"], a["lse"], a["keep_bits"]))


def _o_attn_probs(a):
    """attn_probs_kernel writes the whole dense [B, H, nq, nk] block: zeros for missing queries, missing and masked keys"""
    return [_t(a["probs"], a["B"] * a["H"] * a["nq"] * a["nk"])] + _held(a["q"], a["k"], a["key_mask"], a["lse"])


# name -> the logical views a call may write (everything else of the outputs' storages stays bit-identical: "outside view")
ROW_OUTS = {
    "layernorm_fwd": lambda a: [_t(a["y"], a["M"], a["N"]), _t(a["mean"], a["M"]), _t(a["rstd"], a["M"])],
    "layernorm_bwd": _o_ln_bwd,
    "visn_ln_fwd": lambda a: [_t(a["y"], a["M"], a["N"])] + [_t(a[k], a["M"]) for k in ("mean_v", "rstd_v", "mean_b", "rstd_b")],
    "visn_ln_bwd": _o_visn_bwd,
    "embed_ln_fwd": lambda a: [_t(a["y"], a["B"] * a["L"], a["N"]), _t(a["pre"], a["B"] * a["L"], a["N"]),
                               _t(a["mean"], a["B"] * a["L"]), _t(a["rstd"], a["B"] * a["L"])],
    "embed_bwd": lambda a: [_whole(a["dword"]), _whole(a["dpos"]), _whole(a["dtype_tab"])],
    "codebook_gather": lambda a: [_t(a["feats"], a["M"], a["F"])],
    "dropout": lambda a: [_t2(a["y"], a["M"], a["N"], a["ldy"])],
    "gelu_bwd": lambda a: [_t(a["dx"], a["n"])], "tanh_bwd": lambda a: [_t(a["dx"], a["n"])],
    "colsum": lambda a: [_t(a["out"], a["N"]), _whole(a["ws"])],
    "masked_colsum": lambda a: [_t(a["out"], a["N"]), _whole(a["ws"])],
    "cast_from_f32": lambda a: [_t(a["dst"], a["n"])], "cast_to_f32": lambda a: [_t(a["dst"], a["n"])],
    "take_f32": lambda a: [_t(a["dst"], a["idx"].numel())], "put_f32": lambda a: [_whole(a["dst"])],
    "gather_rows": lambda a: [_t2(a["dst"], a["n_rows"], a["N"], a["ld_dst"])],
    "scatter_rows": lambda a: [_t2(a["dst"], int(a["rows"].reshape(-1)[:a["n_rows"]].max()) + 1, a["N"], a["ld_dst"])],
    "gather_labels": lambda a: [_t(a["out"], a["n_rows"])],
    "mask_counts": lambda a: [_t(a["counts"], 1), _t(a["nmask"], a["B"])],
    "ce_fwd_bwd": _o_ce,
    "featloss_fwd_bwd": _o_featloss,
    "bce_logits_fwd_bwd": lambda a: [_t2(a["dlogits"], a["M"], a["ld_dlogits"], a["ld_dlogits"]), _t(a["loss"], 1)],
    "sumsq": lambda a: [_t(a["out"], 1), _whole(a.get("scratch"))],
    "schedule_step": lambda a: [_t(a["step"], 1), _t(a["lr_and_steps"], 4)],
    "adamw": _o_adamw,
    "rowmax_combine": lambda a: [_t(a["row_maxprob"], a["M"]), _t(a["row_argmax"], a["M"]), _t(a["row_lse"], a["M"])],
    "rowsample_combine": lambda a: [_t(a["row_prob"], a["M"]), _t(a["row_id"], a["M"]), _t(a["row_lse"], a["M"])] + _held(a["ws"]),
    "sample_rows": lambda a: [_t(a["row_prob"], a["M"]), _t(a["row_id"], a["M"]), _t(a["row_lse"], a["M"])] + _held(a["logits"]),
    "rowscore_combine": lambda a: [_t(a["row_nll"], a["M"]), _t(a["row_pred"], a["M"]), _t(a["row_max"], a["M"]), _t(a["totals"], 3)]
    + _held(a["ws"], a["labels"]),
    "score_rows": lambda a: [_t(a["row_nll"], a["M"]), _t(a["row_pred"], a["M"]), _t(a["row_max"], a["M"]), _t(a["totals"], 3)]
    + _held(a["logits"], a["labels"]),
    "remask_lowest": lambda a: [_t(a["vis_mask"], a["B"] * a["V"])],
    "sampler_update": lambda a: [_t(a["code_ids"], a["n"])],
    "sampler_ar_update": lambda a: [_t(a[k], a["B"] * a["V"]) for k in ("code_ids", "vis_mask", "visited")],
    "sdpa_fwd": _o_sdpa_fwd, "sdpa_bwd": _o_sdpa_bwd, "attn_probs": _o_attn_probs,
}


class Recorder:
    """stands in for the step's HipOps: forwards every attribute, checks the first call of each signature"""

    def __init__(self, ops, every_call=False):
        object.__setattr__(self, "_ops", ops)
        object.__setattr__(self, "_every", bool(every_call))      # check every call, whether or not its signature was seen before
        object.__setattr__(self, "_rowrec", {})         # aux pointer -> (epilogue, float64 logits, error, noise / labels) of a checked
        #                                                 XL_EPI_ROWSAMPLE / ROWSCORE launch, for the composed check at its combine
        object.__setattr__(self, "_ref", FakeOps(ops.dtype, compute=torch.float64))
        object.__setattr__(self, "_seen", set())
        object.__setattr__(self, "rows", [])
        object.__setattr__(self, "called", set())
        object.__setattr__(self, "unchecked", set())
        object.__setattr__(self, "failures", [])
        object.__setattr__(self, "_tag", None)          # step index of a sampler loop (part of the signature of its ops)
        object.__setattr__(self, "_deferred", False)
        object.__setattr__(self, "_pending", {})        # producing stream -> entries whose second stage has not run yet
        object.__setattr__(self, "_dirty", {})          # producing stream -> [(lo, hi, recorded)] destinations written since its flush
        object.__setattr__(self, "uncheckable", [])     # pending sums whose destination also holds an unrecorded contribution
        object.__setattr__(self, "_force", set())       # signatures recorded at every call from now on (see retry())
        object.__setattr__(self, "flushes_checked", 0)
        object.__setattr__(self, "sharp", [])           # (tag, share of rows with > 1 admissible column, most in a row)
        object.__setattr__(self, "_rowmax", None)
        object.__setattr__(self, "_cur", None)
        object.__setattr__(self, "ncalls", {})          # (step tag, method) -> number of calls
        object.__setattr__(self, "checked", [])         # (method, {argument: scalar value / None / "T" for a tensor}) of every checked call
        object.__setattr__(self, "_tr_read", True)      # xl_set_lds_transpose_read (library default 1): part of the attention dispatch
        object.__setattr__(self, "_sw", gemm_switches())   # the xl_gemm switches forwarded so far: part of the GEMM dispatch
        object.__setattr__(self, "_ws_slabs", {})       # stream -> slabs of the workspace registered on it (gemm_workspace)
        object.__setattr__(self, "_kern", None)         # rowop_kernel(...) of the call being checked (taken BEFORE the call runs)
        object.__setattr__(self, "lse_excluded", [])    # (method, shape, number of lse entries left out: queries without a valid key)

    def mark(self, tag):
        object.__setattr__(self, "_tag", tag)

    @staticmethod
    def _rowops():
        return _ROWOP

    @staticmethod
    def _row_outs():
        return ROW_OUTS

    def retry(self):
        """A destination may receive two contributions between flushes (the shared cross-attention's q / k / v bias: one sdpa_bwd
        per direction), and the first may be a call whose signature had been checked before, which the recorder lets pass
        unrecorded.  Such a destination cannot be checked in that step (it is listed in `uncheckable`); the signature of the
        unrecorded call is now recorded at EVERY call, and its partner follows by the overlap rule.  Returns True when the step
        has to be run once more for that; the list starts empty again."""
        again = bool(self.uncheckable)
        del self.uncheckable[:]
        return again

    def leftover(self):
        """pending column sums that no flush has covered, and destinations that could not be checked"""
        return [f"{e['row'][0]} {e['row'][1]} {e['row'][2]}" for v in self._pending.values() for e in v] + list(self.uncheckable)

    def __setattr__(self, k, v):
        setattr(self._ops, k, v)

    def __getattr__(self, name):
        attr = getattr(self._ops, name)
        if not callable(attr) or name.startswith("_"):
            return attr
        if name == "set_step_seed_ptr":
            def fwd(step_seed):
                self._ref.set_step_seed_ptr(step_seed)
                return attr(step_seed)
            return fwd
        if name == "set_deferred_reduce":
            def fwd_defer(on):
                object.__setattr__(self, "_deferred", bool(on))
                return attr(on)
            return fwd_defer
        if name == "set_lds_transpose_read":
            def fwd_tr(enable):
                object.__setattr__(self, "_tr_read", bool(enable))
                self._sw["tr_read"] = bool(enable)
                return attr(enable)
            return fwd_tr
        if name in ("set_gemm_pingpong", "set_gemm_duo", "set_gemm_wgrad_slabs"):
            def fwd_sw(v):
                self._sw[{"set_gemm_pingpong": "pingpong", "set_gemm_duo": "duo", "set_gemm_wgrad_slabs": "slabs"}[name]] = int(v)
                return attr(v)
            return fwd_sw
        if name == "set_gemm_tail_split":
            def fwd_tail(max_tail_tiles, min_k):
                self._sw["tail_max"], self._sw["tail_min_k"] = int(max_tail_tiles), int(min_k)
                return attr(max_tail_tiles, min_k)
            return fwd_tail
        if name == "gemm_workspace":
            def fwd_ws(slabs=256, stream=None):
                self._ws_slabs[stream.cuda_stream if stream is not None else self._stream_key()] = int(slabs)
                return attr(slabs, stream)
            return fwd_ws
        if name in ("flush_reductions", "flush_reductions_on"):
            return lambda *args: self._flush(name, attr, args)
        if name in NON_NUMERIC or _is_setter(name):
            return attr
        if name == "gemm_pair":
            def pair(c0, c1):
                self.gemm(*c0.a, **c0.kw)
                self.gemm(*c1.a, **c1.kw)
            return pair
        chk = getattr(self, "chk_" + name, None)

        def call(*args, **kw):
            self.called.add(name)
            self.ncalls[(self._tag, name)] = self.ncalls.get((self._tag, name), 0) + 1
            if chk is None:
                self.unchecked.add(name)
                return attr(*args, **kw)
            sig = inspect.signature(attr)
            ba = sig.bind(*args, **kw)
            ba.apply_defaults()
            a = dict(ba.arguments)
            key = self._signature(name, a)
            if name in ("sdpa_fwd", "sdpa_bwd"):      # a call that changes kernel (a switch, an alignment) is checked again
                key += (("kernel", self._sdpa_kernel(name[5:], a)[0]),)
            elif name == "attn_probs":
                key += (("kernel", "attn_probs_kernel"), ("n_kblk", (a["nk"] + 63) // 64))
            elif name == "gemm":                    # (the same for the GEMM switches and leading dimensions)
                key += (("kernel", self._gemm_kernel(a)),)
            elif name == "gemm_wgrad_group":
                key += (("kernel", tuple(wgrad_group_kernel(a["problems"], a["overwrite_mask"], self._switches())[1])),)
            elif name in self._rowops():            # (the same for the launchers of csrc/rowops.hip and csrc/optim.hip)
                object.__setattr__(self, "_kern", rowop_kernel(name, a))
                key += (("kernel", self._kern),)
            if name in STEP_KEYED or (name == "gemm" and a["epilogue"] in (BD.EPI_ROWMAX, EPI_ROWSAMPLE)):
                key += (("step", self._tag),)
            dests = self._dests(name, a) if self._deferred else []
            force = self._overlaps_recorded(dests) or key in self._force or self._every
            if key in self._seen and not force:
                self._note_dests(dests, False, key)
                return attr(*args, **kw)
            self._seen.add(key)
            object.__setattr__(self, "_cur", (name, self._short(a)))
            _sync()
            cache = {}
            s = {k: self._snap(v, cache) for k, v in a.items()}

            ran = []

            def run():
                ran.append(1)
                r = attr(*args, **kw)
                _sync()
                return r
            try:
                outs = self._row_outs().get(name)
                guard = self._guard([o for o in outs(a) if o is not None], "outside view") if outs is not None else None
                res = chk(a, s, run)
                if guard is not None:
                    res.append(guard(res[0][2] if res else self._kern))
            except Exception as e:          # (a checker that fails still leaves the call done: the step goes on)
                if not ran:
                    run()
                self.failures.append(f"{name} {self._short(a)}: {type(e).__name__}: {e}")
                print(f"FAILED {self.failures[-1]}", flush=True)
                return None
            self._note_dests(dests, True, key)
            self.checked.append((name, dict({k: ("T" if isinstance(v, (torch.Tensor, list, tuple)) else v) for k, v in a.items()},
                                            _kernel=res[0][2] if res else None)))
            for what, ratio, kernel in res:
                self.rows.append((name, what, self._short(a), kernel, ratio))
            print(f"checked {name} {self._short(a)}" + (f" step={self._tag}" if key[-1][0] == "step" else ""), flush=True)
            return None
        return call

    # -- deferred second stages of the column reductions
    @staticmethod
    def _stream_key():
        return torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0

    @staticmethod
    def _range(t):
        span = sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1 if t.numel() else 0
        return t.data_ptr(), t.data_ptr() + span * t.element_size()

    def _dests(self, name, a):
        return [self._range(a[k]) for k in REDUCE_OUTS.get(name, ()) if a.get(k) is not None]

    def _overlaps_recorded(self, dests):
        """does a destination already hold a RECORDED pending contribution?  (then this call is recorded too, whatever its
        signature: the flush is checked against the sum of all contributions)"""
        dirty = self._dirty.get(self._stream_key(), ())
        return any(lo < dhi and dlo < hi and recd for lo, hi in dests for dlo, dhi, recd, _ in dirty)

    def _note_dests(self, dests, recorded, key):
        if dests:
            self._dirty.setdefault(self._stream_key(), []).extend((lo, hi, recorded, key) for lo, hi in dests)

    def _sum_out(self, res, what, got, ref, prev, bound, kern):
        """a column-sum output of a producer: checked at once when its call completed it, else (deferred mode, destination
        untouched by the call) entered into the pending list of the producing stream with its float64 contribution ref - prev"""
        if self._deferred and torch.equal(got.double(), prev.double()):
            lo, hi = self._range(got)
            dirty = self._dirty.get(self._stream_key(), ())
            blind = [k for dlo, dhi, recd, k in dirty if lo < dhi and dlo < hi and not recd]
            if blind:
                self._force.update(blind)
                self.uncheckable.append(f"{self._cur[0]} {what} {self._cur[1]}: destination shared with an unrecorded call")
                return
            bound = torch.as_tensor(bound, dtype=torch.float64, device=ref.device).expand_as(ref)
            self._pending.setdefault(self._stream_key(), []).append(
                dict(got=got, delta=(ref.double() - prev.double()).clone(), bound=bound.clone(), row=(self._cur[0], what, self._cur[1], kern)))
            return
        res.append((what, BD.check(got, ref, bound, f"{self._cur[0]} {what}"), kern))

    def _flush(self, name, attr, args):
        """flush_reductions (the current stream's pending sums) / flush_reductions_on(producer): every pending destination of
        that stream := its content before the flush + the float64 contributions recorded for it, within the sum of their bounds"""
        self.called.add(name)
        key = self._stream_key() if name == "flush_reductions" else args[0].cuda_stream
        pend = self._pending.pop(key, [])
        self._dirty.pop(key, None)
        if not pend:
            return attr(*args)
        _sync()
        groups = {}
        for e in pend:
            g = e["got"]
            groups.setdefault((g.data_ptr(), tuple(g.shape), tuple(g.stride())), []).append(e)
        before = {k: v[0]["got"].double().clone() for k, v in groups.items()}
        r = attr(*args)
        _sync()
        n = 0
        for k, es in groups.items():
            ref = before[k] + sum(e["delta"] for e in es)
            bound = sum(e["bound"] for e in es) + BD.U32 * (before[k].abs() + ref.abs())
            nm, what, short, kern = es[-1]["row"]
            try:
                ratio = BD.check(es[0]["got"], ref, bound, f"{nm} {what} at {name}")
                self.rows.append((nm, what + (f" x{len(es)}" if len(es) > 1 else "") + " @flush", short, kern, ratio))
                n += 1
            except AssertionError as e:
                self.failures.append(f"{name}: {e}")
                print(f"FAILED {self.failures[-1]}", flush=True)
                n += 1
        if n == 0:
            self.failures.append(f"{name}: {len(pend)} pending entries, none checked")
        object.__setattr__(self, "flushes_checked", self.flushes_checked + 1)
        print(f"checked {name}: {n} destinations of {len(pend)} pending entries", flush=True)
        return r

    # -- snapshots: every tensor operand's whole storage, float64 for floating types (aliasing between operands is kept)
    def _snap(self, v, cache):
        if isinstance(v, torch.Tensor):
            st = v.untyped_storage()
            key = (st.data_ptr(), v.dtype)
            if key not in cache:
                n = st.nbytes() // v.element_size()
                base = torch.tensor([], dtype=v.dtype, device=v.device).set_(st, 0, (n,), (1,))
                cache[key] = base.double() if v.is_floating_point() else base.clone()
            return torch.as_strided(cache[key], v.shape, v.stride(), v.storage_offset())
        if isinstance(v, (list, tuple)):
            return type(v)(self._snap(x, cache) for x in v)
        return v

    @staticmethod
    def _signature(name, a):
        def one(v):
            if isinstance(v, torch.Tensor):
                return ("T", v.dtype, _al16(v))
            if isinstance(v, float):
                return v > 0
            if isinstance(v, (list, tuple)):
                return tuple(one(x) for x in v)
            if v is None:
                return None
            return v
        skip = {"seed", "alpha", "scale", "base_lr", "eps", "grad_scale", "beta1", "beta2", "weight_decay", "max_norm"}
        return (name,) + tuple((k, one(v)) for k, v in a.items() if k not in skip)

    @staticmethod
    def _short(a):
        keys = ("M", "N", "K", "B", "H", "nq", "nk", "n", "V", "L", "n_rows", "epilogue", "accumulate", "n_seg", "n_mask", "fixed_pos")
        return " ".join(f"{k}={a[k]}" for k in keys if k in a and not isinstance(a[k], torch.Tensor))

    # ------------------------------------------------------------------------------------------------ contractions
    def _gemm_pre(self, s, M, N, K, parts=False):
        """float64 alpha A B^T + bias and |alpha| |A| |B|^T + |bias| (alpha as the kernel receives it: fp32); parts: also the
        contraction's share |alpha| |A| |B|^T alone and |bias| [1, N] (zeros without a bias), what bounds.rowmax_logit_error takes"""
        A = (_v2(s["A"], M, K, s["lda"]) if s["a_kmajor"] else _v2(s["A"], K, M, s["lda"]).t())
        B = (_v2(s["B"], N, K, s["ldb"]) if s["b_kmajor"] else _v2(s["B"], K, N, s["ldb"]).t())
        al = float(torch.tensor(float(s["alpha"]), dtype=torch.float32))
        pre = al * (A @ B.t())
        absdot = abs(al) * (A.abs() @ B.abs().t())
        b_abs = torch.zeros(1, N, dtype=torch.float64, device=pre.device)
        absprod = absdot
        if s["bias"] is not None:
            b = torch.as_strided(s["bias"], (N,), (1,))
            b_abs = b.abs()[None, :]
            pre, absprod = pre + b[None, :], absdot + b_abs
        return (pre, absprod, absdot, b_abs) if parts else (pre, absprod)

    def _switches(self):
        """the forwarded switches with the slab workspace of the CURRENT stream (where the next call is queued)"""
        return dict(self._sw, ws_slabs=self._ws_slabs.get(self._stream_key(), 0))

    def _gemm_kernel(self, a):
        epi = a["epilogue"]
        res32 = epi == BD.EPI_RESIDUAL and a["residual"] is not None and a["residual"].dtype == torch.float32 \
            and a["A"].dtype == torch.bfloat16
        return gemm_kernel(a["M"], a["N"], a["K"], a["lda"], a["ldb"], a["A"], a["B"], a["out_f32"], epi, a["a_kmajor"], a["b_kmajor"],
                           a["accumulate"], gemm_vec_epi(a["C"], a["ldc"], a["out_f32"], epi, a["residual"], a["ldr"], a["aux"], a["ldx"]),
                           a["bias"] is None or bool(_al16(a["bias"])), a["colsum"] is not None, res32, self._switches())

    # -- stray stores: everything an output's storage holds OUTSIDE the logical views the call may write stays bit-identical
    @staticmethod
    def _raw(t):
        """the whole storage of t as integers of its element size (a view: bit patterns, so that NaN sentinels compare)"""
        st = t.untyped_storage()
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
        return torch.tensor([], dtype=it, device=t.device).set_(st, 0, (st.nbytes() // t.element_size(),), (1,))

    def _guard(self, outs, what="C outside view"):
        """outs: [(tensor, shape, stride)] -- the logical views this call may write (strides in elements of the tensor's type, from
        its storage offset).  Snapshots the bit patterns of every storage involved; the returned function, called after the run,
        holds every element outside all the views to its earlier bits and returns the result row."""
        groups = {}
        for t, shape, stride in outs:
            groups.setdefault((t.untyped_storage().data_ptr(), t.element_size()), []).append((t, shape, stride))
        before = {k: self._raw(v[0][0]).clone() for k, v in groups.items()}

        def after(kern):
            for k, views in groups.items():
                now, was = self._raw(views[0][0]), before[k]
                for t, shape, stride in views:          # inside the views: whatever the call wrote
                    torch.as_strided(was, shape, stride, t.storage_offset()).copy_(torch.as_strided(now, shape, stride, t.storage_offset()))
                BD.check_exact(now, was, f"{self._cur[0]} stores outside the [M, N] views of its outputs (storage of {len(now)} elements)")
            return (what, 0.0, kern)
        return after

    def chk_gemm(self, a, s, run):
        M, N, K, epi = a["M"], a["N"], a["K"], a["epilogue"]
        if epi in ROW_EPILOGUES:
            return self._chk_gemm_rows(a, s, run)
        outs = [(a["C"], (M, N), (a["ldc"], 1))]
        if epi in (BD.EPI_GELU, BD.EPI_GELU_DG):
            outs.append((a["aux"], (M, N), (a["ldx"], 1)))
        if a["colsum"] is not None:                     # (the column-sum workspace is scratch: all of it may change)
            outs.append((a["colsum"], (N,), (1,)))
            if a["ws"] is not None:
                outs.append((a["ws"], tuple(a["ws"].shape), tuple(a["ws"].stride())))
        guard = self._guard(outs)
        pre, absprod = self._gemm_pre(s, M, N, K)
        prev = _v2(s["C"], M, N, a["ldc"]).clone() if a["accumulate"] else None
        aux_in = _v2(s["aux"], M, N, a["ldx"]).clone() if epi in (BD.EPI_DGELU, BD.EPI_MULAUX) else None
        cs_prev = torch.as_strided(s["colsum"], (N,), (1,)).clone() if a["colsum"] is not None else None
        keep = None
        if epi == BD.EPI_RESIDUAL and a["p_drop"] > 0:
            keep = keep_scale(self._ref._seed(a["seed"]), torch.arange(M, device=pre.device)[:, None],
                              torch.arange(N, device=pre.device)[None, :], a["p_drop"]).double()
        run()
        self._ref.gemm(**{k: v for k, v in s.items()})
        out_dt = torch.float32 if a["out_f32"] else a["C"].dtype
        ref_c = _v2(s["C"], M, N, a["ldc"])
        ref_aux = _v2(s["aux"], M, N, a["ldx"]) if epi in (BD.EPI_GELU, BD.EPI_GELU_DG) else None
        bc, ba = BD.gemm_bounds(pre, absprod, K, epi, out_dt, ref_c, aux_in=aux_in, ref_aux=ref_aux, keep=keep,
                                aux_dtype=a["C"].dtype)
        if prev is not None:
            bc = bc + BD.SLACK * BD.U32 * (prev.abs() + ref_c.abs())
        kern = self._gemm_kernel(a)
        res = [("C", BD.check(_v2(a["C"], M, N, a["ldc"]), ref_c, bc, "gemm C"), kern), guard(kern)]
        if ba is not None:
            res.append(("aux", BD.check(_v2(a["aux"], M, N, a["ldx"]), ref_aux, ba, "gemm aux"), kern))
        if a["colsum"] is not None:
            ref_cs = torch.as_strided(s["colsum"], (N,), (1,))
            bcs = BD.colsum_bound(bc, ref_c, cs_prev)
            self._sum_out(res, "colsum", torch.as_strided(a["colsum"], (N,), (1,)), ref_cs, cs_prev, bcs, kern)
        return res

    def _chk_gemm_rows(self, a, s, run):
        """XL_EPI_ROWMAX / ROWSAMPLE / ROWSCORE: no C; the segment records in aux against the float64 logits x = alpha A B^T + bias
        (bounds.check_rowmax_records, bounds_sampling.check_records, bounds_eval.check_rowscore_records), and the storage of aux
        outside its (N / 64) M records of four floats held to its earlier bits.
        alpha and a NULL bias need no term of their own: bounds.rowmax_logit_error is K U32 (|alpha| |A| |B|^T + |bias|) + 2 U32 |x|
        as bounds.gemm_bounds has it, so _gemm_pre's |alpha|-scaled contraction share and a bias share of zero go in as they are
        (alpha scales the fp32 accumulator once: one rounding, inside the 2 U32 |x|; without a bias no addition follows).
        The logits and their error stay with the recorder for the composed check at the combine that reads these records."""
        M, N, K, epi = a["M"], a["N"], a["K"], a["epilogue"]
        assert a["a_kmajor"] and a["b_kmajor"] and a["C"] is None and N % 64 == 0
        n_seg = N // 64
        guard = self._guard([(a["aux"], (n_seg * M * 4,), (1,))], "aux outside view")
        pre, _, absdot, b_abs = self._gemm_pre(s, M, N, K, parts=True)
        e = BD.rowmax_logit_error(pre, absdot, b_abs, K)
        run()
        kern = self._gemm_kernel(a)
        what = f"gemm {ROW_EPILOGUES[epi]}"
        if epi == BD.EPI_ROWMAX:
            res, n_adm = BD.check_rowmax_records(a["aux"], pre, e, what)
        elif epi == EPI_ROWSAMPLE:
            g = gumbel_noise(a["seed"], torch.arange(M, device=pre.device)[:, None], torch.arange(N, device=pre.device)[None, :])
            res, n_adm = BS.check_records(a["aux"], pre, g, e, what)
        else:
            lab = s["residual"].reshape(-1)[:M]
            res = BE.check_rowscore_records(a["aux"], pre, e, lab, what)
        out = [(w, r, kern) for w, r in res] + [guard(kern)]
        if epi == BD.EPI_ROWMAX:
            object.__setattr__(self, "_rowmax", (a["aux"].data_ptr(), pre, e))
        else:
            self._rowrec[a["aux"].data_ptr()] = (epi, pre, e, g if epi == EPI_ROWSAMPLE else lab)
        return out

    def chk_rowmax_combine(self, a, s, run):
        n_seg, M = a["n_seg"], a["M"]
        ws_in = a["ws"].reshape(-1)[:n_seg * M * 4].clone()          # the records the kernel reads (fp32: the argmax is a bit pattern)
        run()
        kern = self._kern
        res = [(w, r, kern) for w, r in BD.check_rowmax_combine(self._ref, ws_in, n_seg, M, a["row_maxprob"], a["row_argmax"],
                                                                 a["row_lse"])]
        if self._rowmax is not None and self._rowmax[0] == a["ws"].data_ptr():
            _, pre, e = self._rowmax
            object.__setattr__(self, "_rowmax", None)
            rows, n_adm = BD.check_rowmax_rows(pre, e, n_seg, a["row_maxprob"][:M] if a["row_maxprob"] is not None else None,
                                               a["row_argmax"][:M], a["row_lse"][:M] if a["row_lse"] is not None else None)
            res += [("composed " + w, r, "ROWMAX epilogue + combine") for w, r in rows]
            share, most = BD.sharpness(n_adm)
            self.sharp.append((self._tag, share, most))
            print(f"sharpness step={self._tag}: {100 * share:.1f} % of {n_adm.numel()} rows with more than one admissible column, "
                  f"at most {most} in a row", flush=True)
        return res

    def _sharp(self, n_adm, what):
        share, most = BD.sharpness(n_adm)
        self.sharp.append((self._tag, share, most))
        print(f"sharpness {what} step={self._tag}: {100 * share:.1f} % of {n_adm.numel()} rows with more than one admissible column, "
              f"at most {most} in a row", flush=True)

    def chk_rowsample_combine(self, a, s, run):
        """on the records it read (bounds_sampling.check_combine), and -- the records came from a checked XL_EPI_ROWSAMPLE launch with
        this seed -- composed with it against the float64 logits of the whole row (bounds_sampling.check_rows)"""
        n_seg, M = a["n_seg"], a["M"]
        ws_in = a["ws"].reshape(-1)[:n_seg * M * 4].clone()
        run()
        kern = self._kern
        res = [(w, r, kern) for w, r in BS.check_combine(ws_in, n_seg, M, a["seed"], a["row_prob"], a["row_id"], a["row_lse"])]
        rec = self._rowrec.pop(a["ws"].data_ptr(), None)
        if rec is not None and rec[0] == EPI_ROWSAMPLE and a["row_id"] is not None:
            _, y, e, g = rec
            rows, n_adm = BS.check_rows(y, g, e, n_seg, a["row_prob"][:M] if a["row_prob"] is not None else None, a["row_id"][:M],
                                        a["row_lse"][:M] if a["row_lse"] is not None else None, "ROWSAMPLE + combine")
            res += [("composed " + w, r, "ROWSAMPLE epilogue + combine") for w, r in rows]
            self._sharp(n_adm, "ROWSAMPLE")
        return res

    def chk_sample_rows(self, a, s, run):
        M, K = a["M"], a["K"]
        y, g, e = BS.logits_reference(_v2(s["logits"], M, K, a["ldl"]), K, a["inv_T"], a["seed"])
        run()
        assert a["row_id"] is not None, "sample_rows without a row_id: nothing to hold the draw to"
        rows, n_adm = BS.check_rows(y, g, e, (K + 63) // 64 + 6, a["row_prob"][:M] if a["row_prob"] is not None else None,
                                    a["row_id"][:M], a["row_lse"][:M] if a["row_lse"] is not None else None, "sample_rows")
        self._sharp(n_adm, "sample_rows")
        return [(w, r, self._kern) for w, r in rows]

    def _chk_totals(self, a, M, before, labels, n_cols, nll, b_nll, pred):
        """totals[0:3] of a scores launch: bounds_eval.check_totals on the outputs returned, or -- without a row_nll / row_pred --
        check_totals_ref on the float64 ones"""
        if a["totals"] is None:
            return []
        lab = labels if labels is not None else torch.full((M,), -100, dtype=torch.int64, device=a["totals"].device)
        if a["row_nll"] is not None and a["row_pred"] is not None:
            return BE.check_totals(before, a["totals"], lab, n_cols, a["row_nll"][:M], a["row_pred"][:M])
        valid = BE.valid_labels(lab, n_cols)
        pr = a["row_pred"][:M].long() if a["row_pred"] is not None else pred
        return BE.check_totals_ref(before, a["totals"], valid, valid & (pr == lab), nll, b_nll)

    def chk_rowscore_combine(self, a, s, run):
        """on the records it read (bounds_eval.check_rowscore_combine), the totals, and -- the records came from a checked
        XL_EPI_ROWSCORE launch with these labels -- composed with it against the float64 logits (bounds_eval.check_rowscore_rows)"""
        n_seg, M, n_cols = a["n_seg"], a["M"], a["n_cols"]
        ws_in = a["ws"].reshape(-1)[:n_seg * M * 4].clone()
        lab = s["labels"].reshape(-1)[:M] if a["labels"] is not None else None
        before = a["totals"].clone() if a["totals"] is not None else None
        run()
        kern = self._kern
        res = [(w, r, kern) for w, r in BE.check_rowscore_combine(ws_in, n_seg, M, lab, n_cols, a["row_nll"], a["row_pred"], a["row_max"])]
        nll, b_nll, pred, _, _ = BE.rowscore_combine_bounds(ws_in, n_seg, M, lab, n_cols)
        res += [(w, r, kern) for w, r in self._chk_totals(a, M, before, lab, n_cols, nll, b_nll, pred)]
        rec = self._rowrec.pop(a["ws"].data_ptr(), None)
        if rec is not None and rec[0] == EPI_ROWSCORE and lab is not None and torch.equal(rec[3], lab):
            _, pre, e, _ = rec
            rows = BE.check_rowscore_rows(pre, e, n_seg, lab, n_cols, a["row_nll"][:M] if a["row_nll"] is not None else None,
                                          a["row_pred"][:M].long() if a["row_pred"] is not None else None,
                                          a["row_max"][:M] if a["row_max"] is not None else None)
            res += [("composed " + w, r, "ROWSCORE epilogue + combine") for w, r in rows]
        return res

    def chk_score_rows(self, a, s, run):
        M, K = a["M"], a["K"]
        x = _v2(s["logits"], M, K, a["ldl"])
        lab = s["labels"].reshape(-1)[:M] if a["labels"] is not None else None
        before = a["totals"].clone() if a["totals"] is not None else None
        run()
        kern = self._kern
        res = [(w, r, kern) for w, r in BE.check_score_rows(x, lab, a["row_nll"][:M] if a["row_nll"] is not None else None,
                                                            a["row_pred"][:M] if a["row_pred"] is not None else None,
                                                            a["row_max"][:M] if a["row_max"] is not None else None)]
        nll, b_nll, first, _, _ = BE.score_rows_bounds(x, lab)
        return res + [(w, r, kern) for w, r in self._chk_totals(a, M, before, lab, K, nll, b_nll, first)]

    # ------------------------------------------------------------------------------------------------ sampler index kernels
    def chk_remask_lowest(self, a, s, run):
        B, V, n_mask = a["B"], a["V"], a["n_mask"]
        run()
        self._ref.remask_lowest(s["prob"], s["vis_mask"], B, V, n_mask)
        got = a["vis_mask"].reshape(-1)[:B * V].view(B, V)
        cnt = torch.full((B,), n_mask, device=got.device)
        return [("vis_mask", BD.check_exact(got.long(), s["vis_mask"].reshape(-1)[:B * V].view(B, V).long(), "remask_lowest"), self._kern),
                ("per-row count", BD.check_exact((got != 0).sum(1), cnt, "remask_lowest count"), self._kern)]

    def chk_sampler_update(self, a, s, run):
        n = a["n"]
        run()
        self._ref.sampler_update(s["pred_ids"], s["vis_mask"], s["code_ids"], n)
        return [("code_ids", BD.check_exact(a["code_ids"].reshape(-1)[:n], s["code_ids"].reshape(-1)[:n], "sampler_update"), self._kern)]

    def chk_sampler_ar_update(self, a, s, run):
        B, V = a["B"], a["V"]
        run()
        self._ref.sampler_ar_update(s["prob"], s["pred_ids"], s["visited"], s["vis_mask"], s["code_ids"], B, V, a["fixed_pos"])
        kern = self._kern
        res = [(k, BD.check_exact(a[k].reshape(-1)[:B * V].long(), s[k].reshape(-1)[:B * V].long(), f"sampler_ar_update {k}"), kern)
               for k in ("code_ids", "vis_mask", "visited") if a[k] is not None]
        if a["fixed_pos"] < 0:
            res.append(("one new visit per row", BD.check_exact((a["visited"].view(B, V) != 0).sum(1) - (s["visited"].view(B, V) != 0).sum(1),
                                                                torch.zeros(B, dtype=torch.long, device=a["visited"].device),
                                                                "sampler_ar_update visits"), kern))
        return res

    def chk_take_f32(self, a, s, run):
        n = a["idx"].numel()
        run()
        self._ref.take_f32(s["src"], s["idx"], a["own_lo"], a["own_hi"], s["dst"])
        return [("dst", BD.check_exact(a["dst"][:n].double(), s["dst"][:n], "take_f32"), self._kern)]

    def chk_put_f32(self, a, s, run):
        run()
        self._ref.put_f32(s["dst"], s["idx"], s["src"])
        return [("dst", BD.check_exact(a["dst"].double(), s["dst"], "put_f32"), self._kern)]

    def chk_bce_logits_fwd_bwd(self, a, s, run):
        M, N, ld = a["M"], a["N"], a["ld_dlogits"]
        x, t = _v2(s["logits"], M, N, a["ld_logits"]).clone(), _v2(s["targets"], M, N, a["ld_targets"]).clone()
        prev = float(s["loss"][0])
        run()
        self._ref.bce_logits_fwd_bwd(**s)
        kern = self._kern
        dl = _v2(s["dlogits"], M, ld, ld) if a["dlogits"] is not None else torch.zeros(M, N, dtype=torch.float64, device=x.device)
        b_dl, b_loss = BD.bce_bounds(x, t, M, N, dl[:, :N], float(s["loss"][0]), prev,
                                     a["dlogits"].dtype if a["dlogits"] is not None else torch.float32)
        res = [("loss", BD.check(a["loss"][:1], s["loss"][:1], b_loss, "bce loss"), kern)]
        if a["dlogits"] is not None:
            bound = torch.full_like(dl, BD.TINY)
            bound[:, :N] = b_dl
            res.append(("dlogits (pad columns 0)", BD.check(_v2(a["dlogits"], M, ld, ld), dl, bound, "bce dlogits"), kern))
        return res

    def chk_attn_probs(self, a, s, run):
        B, H, nq, nk, dh = a["B"], a["H"], a["nq"], a["nk"], a["dh"]
        Q, K, _, valid, keep = BD.attention_inputs(self._ref, s["q"], s["k"], s["k"], s["key_mask"], B, H, nq, nk, dh, a["ldq"], a["ldk"],
                                                   a["ldk"], a["p_drop"], a["seed"], s["q_off"], s["k_off"])
        lse = s["lse"].reshape(-1)[:B * H * nq].view(B, H, nq).clone()
        run()
        self._ref.attn_probs(**s)
        ref = s["probs"].reshape(-1)[:B * H * nq * nk].view(B, H, nq, nk)
        n_kblk = (nk + 63) // 64
        bound = BD.attn_probs_bound(Q, K, None, valid.expand(B, H, nq, nk), keep, a["scale"], lse, ref, n_kblk=n_kblk)
        kern = f"attn_probs_kernel{' + dropout' if a['p_drop'] > 0 else ''}{' packed' if a['q_off'] is not None or a['k_off'] is not None else ''}"
        return [("probs", BD.check(a["probs"].reshape(-1)[:B * H * nq * nk].view(B, H, nq, nk), ref, bound, "attn_probs"), kern)]

    def chk_gemm_wgrad_group(self, a, s, run):
        probs, mask = s["problems"], a["overwrite_mask"]
        pre = []
        for i, (A, B, C, M, N, K, lda, ldb, ldc) in enumerate(probs):
            p, ab = self._gemm_pre(dict(A=A, B=B, lda=lda, ldb=ldb, a_kmajor=0, b_kmajor=0, alpha=1.0, bias=None), M, N, K)
            prev = None if (mask >> i) & 1 else _v2(C, M, N, ldc).clone()
            pre.append((p, ab, prev))
        launch, kerns = wgrad_group_kernel(a["problems"], mask, self._switches())
        guard = self._guard([(pr[2], (pr[3], pr[4]), (pr[8], 1)) for pr in a["problems"]])
        run()
        self._ref.gemm_wgrad_group(probs, mask)
        res = []
        for i, ((A, B, C, M, N, K, lda, ldb, ldc), (p, ab, prev)) in enumerate(zip(probs, pre)):
            ref_c = _v2(C, M, N, ldc)
            bc, _ = BD.gemm_bounds(p, ab, K, BD.EPI_NONE, torch.float32, ref_c)
            if prev is not None:
                bc = bc + BD.SLACK * BD.U32 * (prev.abs() + ref_c.abs())
            res.append((f"dW[{i}] {M}x{N}x{K}" + (" overwrite" if prev is None else ""),
                        BD.check(_v2(a["problems"][i][2], M, N, ldc), ref_c, bc, f"wgrad problem {i}"), kerns[i]))
        res.append(guard(launch))
        return res

    # ------------------------------------------------------------------------------------------------ attention
    def _att(self, s, a):
        return BD.attention_inputs(self._ref, s["q"], s["k"], s["v"], s["key_mask"], a["B"], a["H"], a["nq"], a["nk"], a["dh"],
                                   a["ldq"], a["ldk"], a["ldv"], a["p_drop"], a["seed"], s["q_off"], s["k_off"])

    def _sdpa_kernel(self, direction, a):
        """sdpa_kernel(...) of a call's arguments: (label with the dropout / keep_bits / packed suffixes, n_kblk, n_qblk)"""
        lds = [a[k] for k in ("ldq", "ldk", "ldv", "ldo")]
        ptrs = [a[k] for k in ("q", "k", "v")]
        if direction == "fwd":
            ptrs.append(a["o"])
        else:
            lds += [a[k] for k in ("lddq", "lddk", "lddv")]
            ptrs += [a[k] for k in ("dout", "dq", "dk", "dv")]
        name, n_kblk, n_qblk = sdpa_kernel(direction, a["nq"], a["nk"], a["dh"], lds, [_al16(t) for t in ptrs], self._tr_read,
                                           a["q"].dtype)
        name += f"{' + dropout' if a['p_drop'] > 0 else ''}{' keep_bits' if a.get('keep_bits') is not None else ''}" \
                f"{' packed' if a['q_off'] is not None or a['k_off'] is not None else ''}"
        if direction == "bwd" and a["bias_grad"] is not None:
            # xl_sdpa_bwd: per-example partials in the workspace and one reduce (the on-chip MFMA kernel, a workspace, and B slabs
            # of 3 H dh floats inside xl_workspace_floats(H dh)), otherwise three xl_colsum calls over the STORED dq / dk / dv
            HD = a["H"] * a["dh"]
            fused = (name.startswith("sdpa_bwd_mfma") and a["ws"] is not None
                     and a["B"] * 3 * HD <= self._ops.workspace_floats(HD))
            name += " fused bias" if fused else " separate colsum" if a["ws"] is not None else " separate colsum no workspace"
        return name, n_kblk, n_qblk

    @staticmethod
    def _arith(kern, t):
        """(storage type of the outputs, arithmetic) for the attention bounds: the on-chip generic kernels compute in fp32
        throughout and are held to the storage type they write; every other kernel keeps the bounds it has always been held to
        (bf16 outputs, P and dS rounded to bf16 between the MFMA contractions)"""
        return (t.dtype, "fp32") if "_generic" in kern else (torch.bfloat16, "mfma")

    def _keep_bits_ref(self, a, dev):
        """the keep_bits buffer as the comment at struct KeepBits (csrc/sdpa.hip) lays it out: for problem bh and query fragment j,
        dword (i*16 + r)*2 + h holds at bit t the keep decision of query j*32 + t and key i*32 + (r&3) + 8*(r>>2) + 4*h, hashed
        with row counter bh * nq + query (capacity indexing; also for the queries and keys a fragment carries beyond nq / nk)"""
        B, H, nq, nk = a["B"], a["H"], a["nq"], a["nk"]
        nqf, nkf = (nq + 31) // 32, (nk + 31) // 32
        ar = lambda n: torch.arange(n, device=dev)                                   # noqa: E731
        bh, j, i, r, h, t = (x.view(*sh) for x, sh in zip((ar(B * H), ar(nqf), ar(nkf), ar(16), ar(2), ar(32)),
                                                           ((-1, 1, 1, 1, 1, 1), (1, -1, 1, 1, 1, 1), (1, 1, -1, 1, 1, 1),
                                                            (1, 1, 1, -1, 1, 1), (1, 1, 1, 1, -1, 1), (1, 1, 1, 1, 1, -1))))
        row = bh * nq + j * 32 + t
        col = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h
        row, col = torch.broadcast_tensors(row, col)
        keep = (keep_scale(self._ref._seed(a["seed"]), row, col, a["p_drop"]) > 0).to(torch.int64)
        words = (keep << t.to(torch.int64)).sum(-1)                                  # [BH, nqf, nkf, 16, 2] -> dword order
        return words.reshape(-1)

    def chk_sdpa_fwd(self, a, s, run):
        B, H, nq, nk, dh = a["B"], a["H"], a["nq"], a["nk"], a["dh"]
        Q, K, V, valid, keep = self._att(s, a)
        run()
        self._ref.sdpa_fwd(**s)
        # an example whose keys are all masked: a softmax over no key (NaN in the restatement); the kernels' convention is a zero
        # row (and lse = -inf), which the bound below (P' = 0 there) holds to within TINY
        BD.attention_rows(self._ref, s["o"], B, nq, H, dh, a["ldo"], s["q_off"], a["q_pad"]).nan_to_num_(0.0)
        O_, _ = self._ref._load(s["o"], B, nq, H, dh, a["ldo"], s["q_off"])
        lse = s["lse"].reshape(-1)[:B * H * nq].view(B, H, nq)
        kern, n_kblk, _ = self._sdpa_kernel("fwd", a)
        out_dt, arith = self._arith(kern, a["o"])
        bO, bl = BD.sdpa_fwd_bounds(Q, K, V, valid, keep, a["scale"], O_, lse, n_kblk=n_kblk, out_dtype=out_dt, arith=arith)
        rows = lambda t: BD.attention_rows(self._ref, t, B, nq, H, dh, a["ldo"], a["q_off"], a["q_pad"])   # noqa: E731
        ref_rows = BD.attention_rows(self._ref, s["o"], B, nq, H, dh, a["ldo"], s["q_off"], a["q_pad"])
        bO = BD.attention_scatter(self._ref, bO, B, nq, H, dh, a["ldo"], s["q_off"], a["q_pad"])[:ref_rows.shape[0]]
        exist = valid.any(-1).expand(B, H, nq)       # (the only elements left out of a comparison: the lse of a query without a key)
        self.lse_excluded.append(("sdpa_fwd", self._short(a), int((~exist).sum())))
        # ... and their number follows from the inputs: per head, the queries an example does not have (packed q side) and the
        # queries of an example none of whose keys attends (key mask, packed k side)
        lens = lambda off, n: ([n] * B if off is None else                            # noqa: E731
                               [min(n, int(off.reshape(-1)[b + 1]) - int(off.reshape(-1)[b])) for b in range(B)])
        lq, lk = lens(s["q_off"], nq), lens(s["k_off"], nk)
        on = [lk[b] if s["key_mask"] is None else int((s["key_mask"].reshape(-1)[b * nk:b * nk + lk[b]] != 0).sum()) for b in range(B)]
        want = H * sum((nq - lq[b]) + (lq[b] if on[b] == 0 else 0) for b in range(B))
        assert int((~exist).sum()) == want, f"sdpa_fwd: {int((~exist).sum())} lse entries left out of the comparison, the inputs give {want}"
        got_l = a["lse"].reshape(-1)[:B * H * nq].view(B, H, nq)
        res = [("O", BD.check(rows(a["o"]), ref_rows, bO, "sdpa_fwd O"), kern),
               ("lse", BD.check(got_l[exist], lse[exist], bl[exist], "sdpa_fwd lse"), kern)]
        if a["keep_bits"] is not None and a["p_drop"] > 0:
            n = keep_bits_words(B, H, nq, nk)
            got_w = a["keep_bits"].reshape(-1)[:n].to(torch.int64) & 0xFFFFFFFF
            res.append(("keep_bits", BD.check_exact(got_w, self._keep_bits_ref(a, got_w.device), "sdpa_fwd keep_bits"), kern))
        return res

    def chk_sdpa_bwd(self, a, s, run):
        B, H, nq, nk, dh = a["B"], a["H"], a["nq"], a["nk"], a["dh"]
        Q, K, V, valid, keep = self._att(s, a)
        dO, _ = self._ref._load(s["dout"], B, nq, H, dh, a["ldo"], s["q_off"])
        lse = s["lse"].reshape(-1)[:B * H * nq].view(B, H, nq).clone()
        bias_prev = s["bias_grad"].clone() if a["bias_grad"] is not None else None
        run()
        self._ref.sdpa_bwd(**s)
        sides = (("dq", nq, "lddq", "q_off", "q_pad"), ("dk", nk, "lddk", "k_off", "k_pad"), ("dv", nk, "lddv", "k_off", "k_pad"))
        dense = [self._ref._load(s[nm], B, n, H, dh, a[ld], s[off])[0] for nm, n, ld, off, _ in sides]
        kern, n_kblk, n_qblk = self._sdpa_kernel("bwd", a)
        out_dt, arith = self._arith(kern, a["dq"])
        bounds, terms = BD.sdpa_bwd_bounds(Q, K, V, dO, valid, keep, a["scale"], lse, *dense, n_kblk=n_kblk, n_qblk=n_qblk,
                                           out_dtype=out_dt, arith=arith)
        # the long and the generic kernels have no fused partials: their bias gradients are xl_colsum of the STORED dq / dk / dv
        # (bf16-rounded), so each element enters the sum with its whole bound: bounds.colsum_bound.  The on-chip MFMA kernel keeps
        # the bound it has always been held to (fused fp32 partials: no rounding of the summands).
        # So does the on-chip MFMA kernel when it has no workspace, or more examples than the workspace has slabs for.
        stored_sums = "fused bias" not in kern
        res = []
        HD = H * dh
        for (nm, n, ld, off, pad), b, t in zip(sides, bounds, terms):
            ref_rows = BD.attention_rows(self._ref, s[nm], B, n, H, dh, a[ld], s[off], a[pad])
            got_rows = BD.attention_rows(self._ref, a[nm], B, n, H, dh, a[ld], a[off], a[pad])
            bb = BD.attention_scatter(self._ref, b, B, n, H, dh, a[ld], s[off], a[pad])[:ref_rows.shape[0]]
            res.append((nm, BD.check(got_rows, ref_rows, bb, f"sdpa_bwd {nm}"), kern))
            if bias_prev is not None:
                i = "dq dk dv".split().index(nm)
                tt = BD.attention_scatter(self._ref, t, B, n, H, dh, a[ld], s[off], a[pad])[:ref_rows.shape[0]]
                ref_b = s["bias_grad"][i * HD:(i + 1) * HD]
                if stored_sums:
                    bnd = BD.colsum_bound(bb, ref_rows, bias_prev[i * HD:(i + 1) * HD]) + BD.U32 * ref_b.abs()
                    self._sum_out(res, f"bias {nm}", a["bias_grad"][i * HD:(i + 1) * HD], ref_b, bias_prev[i * HD:(i + 1) * HD], bnd, kern)
                    continue
                bnd = BD.SLACK * tt.sum(0) + BD.SLACK * (ref_rows.shape[0] + 1) * BD.U32 * (ref_rows.abs().sum(0)
                                                                                        + bias_prev[i * HD:(i + 1) * HD].abs()) \
                    + BD.U32 * ref_b.abs() + BD.TINY
                self._sum_out(res, f"bias {nm}", a["bias_grad"][i * HD:(i + 1) * HD], ref_b, bias_prev[i * HD:(i + 1) * HD], bnd, kern)
        return res

    # ------------------------------------------------------------------------------------------------ LayerNorm family
    def chk_layernorm_fwd(self, a, s, run):
        M, N = a["M"], a["N"]
        run()
        self._ref.layernorm_fwd(**s)
        x, y = _v2(s["x"], M, N, N).clone(), _v2(s["y"], M, N, N)
        by, bm, br = BD.ln_fwd_bounds(x, s["gamma"].double(), y, s["mean"][:M], s["rstd"][:M], a["y"].dtype)
        kern = self._kern
        return [("y", BD.check(_v2(a["y"], M, N, N), y, by, "layernorm_fwd y"), kern),
                ("mean", BD.check(a["mean"][:M], s["mean"][:M], bm, "layernorm_fwd mean"), kern),
                ("rstd", BD.check(a["rstd"][:M], s["rstd"][:M], br, "layernorm_fwd rstd"), kern)]

    def chk_layernorm_bwd(self, a, s, run):
        M, N = a["M"], a["N"]
        dy, x = _v2(s["dy"], M, N, N).clone(), _v2(s["x"], M, N, N).clone()
        mean, rstd = s["mean"][:M].clone(), s["rstd"][:M].clone()
        prev = {k: s[k].clone() for k in ("dgamma", "dbeta", "dbias_prev") if s[k] is not None}
        assert "dgamma" in prev and "dbeta" in prev
        keep = None
        if a["dx_dropped"] is not None and a["p_drop"] > 0:
            keep = keep_scale(self._ref._seed(a["seed"]), torch.arange(M, device=dy.device)[:, None],
                              torch.arange(N, device=dy.device)[None, :], a["p_drop"]).double()
        run()
        self._ref.layernorm_bwd(**s)
        dx = _v2(s["dx"], M, N, N)
        bdx, t, bdg, bdb = BD.ln_bwd_bounds(dy, x, s["gamma"].double(), mean, rstd, dx, a["dx"].dtype)
        kern = self._kern
        res = [("dx", BD.check(_v2(a["dx"], M, N, N), dx, bdx, "layernorm_bwd dx"), kern)]
        self._sum_out(res, "dgamma", a["dgamma"], s["dgamma"], prev["dgamma"], bdg + BD.U32 * (s["dgamma"].abs() + prev["dgamma"].abs()), kern)
        self._sum_out(res, "dbeta", a["dbeta"], s["dbeta"], prev["dbeta"], bdb + BD.U32 * (s["dbeta"].abs() + prev["dbeta"].abs()), kern)
        if keep is not None:
            dd = _v2(s["dx_dropped"], M, N, N)
            bdd = BD.U16 * dd.abs() + BD.SLACK * keep * t + BD.TINY
            res.append(("dx_dropped", BD.check(_v2(a["dx_dropped"], M, N, N), dd, bdd, "layernorm_bwd dx_dropped"), kern))
            if a["dbias_prev"] is not None:
                ref = s["dbias_prev"]
                # (the kernel adds the fp32 dropped value BEFORE its store: a summand carries the fp32 term and the rounding of
                #  the multiply by the keep scale, no output rounding)
                bb = BD.ln_bwd_bias_bound(keep * t + BD.U32 * dd.abs(), dd, prev["dbias_prev"], ref)
                self._sum_out(res, "dbias_prev", a["dbias_prev"], ref, prev["dbias_prev"], bb, kern)
        elif a["dbias_prev"] is not None:
            # without dropout (the eval-mode path, or no dropped copy asked for) the kernel still writes it: the column sums of
            # the fp32 dx BEFORE its store (no rounding of the summands)
            ref = s["dbias_prev"]
            self._sum_out(res, "dbias_prev", a["dbias_prev"], ref, prev["dbias_prev"],
                          BD.ln_bwd_bias_bound(t, dx, prev["dbias_prev"], ref), kern)
        return res

    def _box(self, s, M, N, P):
        pos, w, b = s["pos"].reshape(-1)[:M * P].view(M, P), s["wbox"].reshape(-1)[:N * P].view(N, P), s["bbox"].reshape(-1)[:N]
        box = pos @ w.t() + b
        err = (P + 1) * BD.U32 * (pos.abs() @ w.abs().t() + b.abs())
        return box, err, pos

    def chk_visn_ln_fwd(self, a, s, run):
        M, N, P = a["M"], a["N"], a["P"]
        xv = _v2(s["xv"], M, N, N).clone()
        box, berr, _ = self._box(s, M, N, P)
        run()
        self._ref.visn_ln_fwd(**s)
        ya, mv, rv = FakeOps._ln(xv, s["gv"].double(), s["bv"].double(), a["eps"])
        yb, mb, rb = FakeOps._ln(box, s["gb"].double(), s["bb"].double(), a["eps"])
        y = _v2(s["y"], M, N, N)
        b1, bmv, brv = BD.ln_fwd_bounds(xv, s["gv"].double(), ya, mv, rv, torch.float64)
        b2, bmb, brb = BD.ln_fwd_bounds(box, s["gb"].double(), yb, mb, rb, torch.float64, x_err=berr)
        by = BD.unit(a["y"].dtype) * y.abs() + 0.5 * (b1 + b2) + BD.SLACK * BD.U32 * y.abs()
        kern = self._kern
        return [("y", BD.check(_v2(a["y"], M, N, N), y, by, "visn_ln_fwd y"), kern),
                ("mean_v", BD.check(a["mean_v"][:M], s["mean_v"][:M], bmv, "visn mean_v"), kern),
                ("rstd_v", BD.check(a["rstd_v"][:M], s["rstd_v"][:M], brv, "visn rstd_v"), kern),
                ("mean_b", BD.check(a["mean_b"][:M], s["mean_b"][:M], bmb + BD.SLACK * berr.amax(-1), "visn mean_b"), kern),
                ("rstd_b", BD.check(a["rstd_b"][:M], s["rstd_b"][:M],
                                    brb + BD.SLACK * 2 * rb.abs() ** 3 * berr.amax(-1) * (box - mb[:, None]).abs().amax(-1),
                                    "visn rstd_b"), kern)]

    def chk_visn_ln_bwd(self, a, s, run):
        M, N, P = a["M"], a["N"], a["P"]
        dh = _v2(s["dy"], M, N, N).clone() * 0.5
        xv = _v2(s["xv"], M, N, N).clone()
        box, berr, pos = self._box(s, M, N, P)
        pos = pos.clone()
        mean_v, rstd_v, mean_b, rstd_b = (s[k][:M].clone() for k in ("mean_v", "rstd_v", "mean_b", "rstd_b"))
        names = ("dgv", "dbv", "dgb", "dbb", "dwbox", "dbbox", "dbias_visn")
        prev = {k: s[k].clone() for k in names if s[k] is not None}
        run()
        self._ref.visn_ln_bwd(**s)
        d1, _, _ = FakeOps._ln_bwd(dh, xv, s["gv"].double(), mean_v, rstd_v)
        d2, _, _ = FakeOps._ln_bwd(dh, box, s["gb"].double(), mean_b, rstd_b)
        b1, t1, bg1, bb1 = BD.ln_bwd_bounds(dh, xv, s["gv"].double(), mean_v, rstd_v, d1, a["dxv"].dtype)
        _, t2, bg2, bb2 = BD.ln_bwd_bounds(dh, box, s["gb"].double(), mean_b, rstd_b, d2, torch.float64, x_err=berr)
        t2 = BD.SLACK * t2
        kern = self._kern

        res = [("dxv", BD.check(_v2(a["dxv"], M, N, N), _v2(s["dxv"], M, N, N), b1, "visn_ln_bwd dxv"), kern)]

        def acc(k, bnd):
            ref, pv = s[k].reshape(-1), prev[k].reshape(-1)
            self._sum_out(res, k, a[k].reshape(-1), ref, pv, bnd.reshape(-1) + BD.U32 * (ref.abs() + pv.abs()), kern)
        dw_terms = (d2.abs().t() @ pos.abs())
        acc("dgv", bg1), acc("dbv", bb1), acc("dgb", bg2), acc("dbb", bb2)
        acc("dwbox", t2.t() @ pos.abs() + BD.SLACK * (M + 1) * BD.U32 * dw_terms)
        acc("dbbox", t2.sum(0) + BD.SLACK * (M + 1) * BD.U32 * d2.abs().sum(0))
        if a["dbias_visn"] is not None:
            acc("dbias_visn", (BD.U16 * d1.abs() + BD.SLACK * t1).sum(0) + BD.SLACK * (M + 1) * BD.U32 * d1.abs().sum(0))
        return res

    def chk_embed_ln_fwd(self, a, s, run):
        B, L, N = a["B"], a["L"], a["N"]
        M = B * L
        run()
        self._ref.embed_ln_fwd(**s)
        pre = _v2(s["pre"], M, N, N)
        wsum = (s["word"][s["ids"].reshape(-1).long()].abs() + s["pos"][torch.arange(L, device=pre.device).repeat(B)].abs()
                + s["type_"][s["tt"].reshape(-1).long()].abs())
        bpre = BD.unit(a["pre"].dtype) * pre.abs() + BD.SLACK * 2 * BD.U32 * wsum + BD.TINY
        kern = self._kern
        res = [("pre", BD.check(_v2(a["pre"], M, N, N), pre, bpre, "embed pre"), kern)]
        gpre = _v2(a["pre"], M, N, N).double()              # the kernel normalises the STORED sum (csrc/rowops.hip)
        y, m, r = FakeOps._ln(gpre, s["gamma"].double(), s["beta"].double(), a["eps"])
        by, bm, br = BD.ln_fwd_bounds(gpre, s["gamma"].double(), y, m, r, a["y"].dtype)
        res += [("y", BD.check(_v2(a["y"], M, N, N), y, by, "embed y"), kern),
                ("mean", BD.check(a["mean"][:M], m, bm, "embed mean"), kern),
                ("rstd", BD.check(a["rstd"][:M], r, br, "embed rstd"), kern)]
        return res

    def chk_embed_bwd(self, a, s, run):
        B, L, N = a["B"], a["L"], a["N"]
        M = B * L
        tabs = ("dword", "dpos", "dtype_tab")
        absd = {k: s[k].abs() for k in tabs}                 # |prev| + sum of |terms| (the same scatter on absolute values)
        sa = dict(s, dpre=_v2(s["dpre"], M, N, N).abs().contiguous(), **absd)
        rows0 = torch.cat([s[k][0].reshape(-1).clone() for k in tabs])
        run()
        self._ref.embed_bwd(**sa)
        self._ref.embed_bwd(**s)
        res = [(k, BD.check(a[k], s[k], BD.U32 * s[k].abs() + BD.SLACK * (M + 1) * BD.U32 * sa[k] + BD.TINY, f"embed_bwd {k}"),
                self._kern) for k in tabs]
        # padding_idx = 0: row 0 of the word, the position and the token-type table is frozen
        res.append(("rows 0 frozen", BD.check_exact(torch.cat([a[k][0].reshape(-1).double() for k in tabs]), rows0,
                                                    "embed_bwd rows 0 of the three tables"), self._kern))
        return res

    # ------------------------------------------------------------------------------------------------ elementwise / copies
    def chk_codebook_gather(self, a, s, run):
        M, F = a["M"], a["F"]
        run()
        self._ref.codebook_gather(**s)
        ref = _v2(s["feats"], M, F, F)
        return [("feats", BD.check(_v2(a["feats"], M, F, F), ref, BD.unit(a["feats"].dtype) * ref.abs() + BD.TINY, "codebook"),
                 self._kern)]

    def chk_dropout(self, a, s, run):
        M, N = a["M"], a["N"]
        run()
        self._ref.dropout(**s)
        ref = _v2(s["y"], M, N, a["ldy"])
        return [("y", BD.check(_v2(a["y"], M, N, a["ldy"]), ref, BD.scaled_copy_bound(ref, a["y"].dtype), "dropout"), self._kern)]

    def chk_gelu_bwd(self, a, s, run):
        n = a["n"]
        dy, pre = s["dy"].reshape(-1)[:n].clone(), s["pre"].reshape(-1)[:n].clone()
        run()
        self._ref.gelu_bwd(**s)
        ref = s["dx"].reshape(-1)[:n]
        return [("dx", BD.check(a["dx"].reshape(-1)[:n], ref, BD.gelu_bwd_bound(dy, pre, ref, a["dx"].dtype), "gelu_bwd"),
                 self._kern)]

    def chk_tanh_bwd(self, a, s, run):
        n = a["n"]
        dy, y = s["dy"].reshape(-1)[:n].clone(), s["y"].reshape(-1)[:n].clone()
        run()
        self._ref.tanh_bwd(**s)
        ref = s["dx"].reshape(-1)[:n]
        return [("dx", BD.check(a["dx"].reshape(-1)[:n], ref, BD.tanh_bwd_bound(dy, y, ref, a["dx"].dtype), "tanh_bwd"), self._kern)]

    def _colsum_like(self, name, a, s, run):
        M, N = a["M"], a["N"]
        sa = dict(s, x=_v2(s["x"], M, N, a["ldx"]).abs().contiguous(), ldx=N, out=s["out"].abs())
        prev = s["out"][:N].clone()
        run()
        getattr(self._ref, name)(**sa)
        getattr(self._ref, name)(**s)
        ref = s["out"][:N]
        bnd = BD.U32 * ref.abs() + BD.SLACK * (M + 1) * BD.U32 * sa["out"][:N] + BD.TINY
        res = []
        self._sum_out(res, "out", a["out"][:N], ref, prev, bnd, self._kern)
        return res

    def chk_colsum(self, a, s, run):
        return self._colsum_like("colsum", a, s, run)

    def chk_masked_colsum(self, a, s, run):
        return self._colsum_like("masked_colsum", a, s, run)

    def _cast(self, name, a, s, run):
        n = a["n"]
        run()
        getattr(self._ref, name)(**s)
        ref = s["dst"].reshape(-1)[:n]
        return [("dst", BD.check(a["dst"].reshape(-1)[:n], ref, BD.unit(a["dst"].dtype) * ref.abs() + BD.TINY, name), self._kern)]

    def chk_cast_from_f32(self, a, s, run):
        return self._cast("cast_from_f32", a, s, run)

    def chk_cast_to_f32(self, a, s, run):
        return self._cast("cast_to_f32", a, s, run)

    def chk_gather_rows(self, a, s, run):
        n, N = a["n_rows"], a["N"]
        run()
        self._ref.gather_rows(**s)
        return [("dst", BD.check_exact(_v2(a["dst"], n, N, a["ld_dst"]).double(), _v2(s["dst"], n, N, a["ld_dst"]), "gather_rows"),
                 self._kern)]

    def chk_scatter_rows(self, a, s, run):
        n, N = a["n_rows"], a["N"]
        rows = int(a["rows"].reshape(-1)[:n].max()) + 1
        run()
        self._ref.scatter_rows(**s)
        return [("dst", BD.check_exact(_v2(a["dst"], rows, N, a["ld_dst"]).double(), _v2(s["dst"], rows, N, a["ld_dst"]),
                                       "scatter_rows"), self._kern)]

    def chk_gather_labels(self, a, s, run):
        n = a["n_rows"]
        run()
        self._ref.gather_labels(**s)
        return [("out", BD.check_exact(a["out"].reshape(-1)[:n], s["out"].reshape(-1)[:n], "gather_labels"), self._kern)]

    def chk_mask_counts(self, a, s, run):
        B, V = a["B"], a["V"]
        run()
        self._ref.mask_counts(**s)
        return [("counts", BD.check_exact(a["counts"][:1].double(), s["counts"][:1], "mask_counts"), self._kern),
                ("nmask", BD.check_exact(a["nmask"][:B].double(), s["nmask"][:B], "mask_counts nmask"), self._kern)]

    # ------------------------------------------------------------------------------------------------ losses
    def chk_ce_fwd_bwd(self, a, s, run):
        M, K = a["M"], a["K"]
        lg = _v2(s["logits"], M, K, a["ldl"]).clone()
        loss_prev = s["loss_out"].clone() if a["loss_out"] is not None else None
        run()
        self._ref.ce_fwd_bwd(**s)
        lab = s["labels"].reshape(-1)[:M].long() if a["labels"] is not None else None
        valid = (lab != -100).double() if lab is not None else torch.zeros(M, dtype=torch.float64, device=lg.device)
        cnt = float(s["counts"][0].clamp(min=1)) if a["counts"] is not None else 1.0
        lse = torch.logsumexp(lg, 1)
        dl = _v2(s["dlogits"], M, K, a["lddl"]) if a["dlogits"] is not None else torch.zeros_like(lg)
        blse, bdl = BD.ce_bounds(lg, valid, a["grad_scale"] / cnt, lse, dl, a["dlogits"].dtype if a["dlogits"] is not None
                                 else torch.float32)
        kern = self._kern
        res = []
        if a["dlogits"] is not None:
            # the register kernels also write the slots K .. K8 of a row, with zeros: inside the view, exactly zero
            Kw = (K + 7) // 8 * 8 if ce_in_regs(a["logits"], a["dlogits"], K, a["ldl"], a["lddl"]) else K
            ref_w, b_w = torch.zeros(M, Kw, dtype=torch.float64, device=lg.device), torch.zeros(M, Kw, dtype=torch.float64, device=lg.device)
            ref_w[:, :K], b_w[:, :K] = dl, bdl
            res.append(("dlogits" + (" (slots K..K8 zero)" if Kw > K else ""),
                        BD.check(_v2(a["dlogits"], M, Kw, a["lddl"]), ref_w, b_w, "ce dlogits"), kern))
        if a["row_lse"] is not None:
            res.append(("row_lse", BD.check(a["row_lse"][:M], s["row_lse"][:M], blse, "ce row_lse"), kern))
        if a["row_argmax"] is not None:
            got = a["row_argmax"][:M].long()
            BD.check_exact((got >= 0) & (got < K), torch.ones(M, dtype=torch.bool, device=got.device), "ce row_argmax (an index of the row)")
            mx = lg.amax(1)
            res.append(("row_argmax", BD.check_exact(lg.gather(1, got[:, None])[:, 0], mx, "ce row_argmax (value at the index)"), kern))
            unique = (lg == mx[:, None]).sum(1) == 1
            res.append(("row_argmax idx", BD.check_exact(got[unique], s["row_argmax"][:M].long()[unique], "ce row_argmax"), kern))
            # the admissibility rule (bounds.argmax_admissible) on exact inputs, E = 0: the LOWEST index of the maximum, ties included
            n_adm = BD.check_admissible(lg, got, torch.zeros(M, dtype=torch.float64, device=lg.device), "ce row_argmax (lowest index of the maximum)")
            res.append(("row_argmax admissible", 0.0, kern))
            self.sharp.append((self._tag,) + BD.sharpness(n_adm))
        if a["row_maxprob"] is not None:
            ref = s["row_maxprob"][:M]
            res.append(("row_maxprob", BD.check(a["row_maxprob"][:M], ref, BD.SLACK * ref.abs() * (blse + 2 * BD.U32) + BD.U32 * ref.abs()
                                                + BD.TINY, "ce row_maxprob"), kern))
        if a["loss_out"] is not None and lab is not None:
            ref = s["loss_out"][0]
            bl = BD.ce_loss_bound(lg, lab, valid, cnt, blse, float(ref)) + BD.U32 * float(loss_prev[0].abs())
            res.append(("loss", BD.check(a["loss_out"][:1], s["loss_out"][:1], bl, "ce loss"), kern))
        elif a["loss_out"] is not None:         # no labels: no loss term
            res.append(("loss untouched", BD.check_exact(a["loss_out"][:1].double(), loss_prev[:1], "ce loss without labels"), kern))
        return res

    def chk_featloss_fwd_bwd(self, a, s, run):
        B, V, F = a["B"], a["V"], a["F"]
        n = B * V if a["rows"] is None else a["n_rows"]
        run()
        self._ref.featloss_fwd_bwd(**s)
        g = torch.arange(B * V, device=s["pred"].device) if a["rows"] is None else s["rows"].reshape(-1)[:n].long()
        pad = g < 0
        g = g.clamp(min=0)
        pred = _v2(s["pred"], n, F, F)
        tgt = (s["centroids"][s["cluster_ids"].reshape(-1)[g].long()] if a["targets"] is None else s["targets"].view(B * V, F)[g])
        w = ((s["vis_mask"].reshape(-1) != 0).double() / (s["nmask"].clamp(min=1).repeat_interleave(V) * B))[g]
        w = torch.where(pad, torch.zeros_like(w), w)
        dref = _v2(s["dpred"], n, F, F) if a["dpred"] is not None else torch.zeros_like(pred)
        lb, bd = BD.featloss_bounds(pred, tgt, w, F, dref, float(s["loss_out"][0]) if a["loss_out"] is not None else 0.0,
                                    a["dpred"].dtype if a["dpred"] is not None else torch.float32)
        res = []
        if a["dpred"] is not None:
            res.append(("dpred", BD.check(_v2(a["dpred"], n, F, F), dref, bd, "featloss dpred"), self._kern))
        if a["loss_out"] is not None:
            res.append(("loss", BD.check(a["loss_out"][:1], s["loss_out"][:1], lb, "featloss loss"), self._kern))
        return res

    # ------------------------------------------------------------------------------------------------ optimizer
    def chk_sumsq(self, a, s, run):
        n = a["n"]
        prev = float(s["out"][0])
        run()
        self._ref.sumsq(**s)
        ref = s["out"][:1]
        bnd = BD.sumsq_bound(s["g"][:n], float(ref)) + BD.U32 * abs(prev)
        return [("out", BD.check(a["out"][:1], ref, bnd, "sumsq"), self._kern)]

    def chk_schedule_step(self, a, s, run):
        run()
        self._ref.schedule_step(**s)
        ref = s["lr_and_steps"][:4]
        t = float(ref[3])
        scale = torch.tensor([abs(float(ref[0])), a["beta1"] ** t, a["beta2"] ** t, 0.0], dtype=torch.float64, device=ref.device)
        bnd = BD.SLACK * 4 * BD.U32 * scale + BD.U32 * ref.abs() + BD.TINY
        return [("step", BD.check_exact(a["step"][:1], s["step"][:1], "schedule step"), self._kern),
                ("lr_and_steps", BD.check(a["lr_and_steps"][:4], ref, bnd, "schedule lr_and_steps"), self._kern)]

    def chk_adamw(self, a, s, run):
        n = a["n"]
        dev = s["p"].device
        before = {k: s[k][:n].clone() for k in ("p", "g", "m", "v")}
        g0, m0, v0 = before["g"], before["m"], before["v"]
        separate = a["p_compute"] is not None and a["p_compute"].data_ptr() != a["p"].data_ptr()
        if separate:
            before["p_compute"] = s["p_compute"][:n].clone()
        lrs = [float(x) for x in s["lr_and_steps"][:3]]
        clip = a["grad_scale"]
        if a["max_norm"] > 0 and a["sumsq"] is not None:
            norm = float(s["sumsq"][0]) ** 0.5 * a["grad_scale"]
            clip *= min(1.0, a["max_norm"] / (norm + 1e-6))
        fl = (s["decay_flags"].repeat_interleave(256)[:n] if a["decay_flags"] is not None
              else torch.zeros(n, dtype=torch.uint8, device=dev))
        skip, keep_g = (fl & 2) != 0, (fl & 4) != 0
        if a["chunk_steps"] is not None:        # per-chunk update counts: the kernel derives the step size in fp32 (bounds.adamw_chunk_step)
            t = s["chunk_steps"].repeat_interleave(256)[:n].double().clamp(min=1)
            step, step_rel = BD.adamw_chunk_step(lrs[0], a["beta1"], a["beta2"], t)
        else:
            step, step_rel = lrs[0] * lrs[2] ** 0.5 / lrs[1], 0.0
        kern = self._kern
        run()
        self._ref.adamw(**s)
        bp, bm, bv = BD.adamw_bounds(s["p"][:n], s["m"][:n], s["v"][:n], g0, m0, v0, step, clip, a["beta1"], a["beta2"], a["eps"],
                                     lrs[0], a["weight_decay"], step_rel=step_rel)
        res = [("p", BD.check(a["p"][:n], s["p"][:n], bp, "adamw p"), kern),
               ("m", BD.check(a["m"][:n], s["m"][:n], bm, "adamw m"), kern),
               ("v", BD.check(a["v"][:n], s["v"][:n], bv, "adamw v"), kern)]
        if separate:
            ref = s["p_compute"][:n]
            res.append(("p_compute", BD.check(a["p_compute"][:n], ref, BD.unit(a["p_compute"].dtype) * ref.abs() + bp, "adamw p_compute"),
                        kern))
        if a["zero_grad"]:
            ref = s["g"][:n]
            kept = torch.isnan(ref)                  # the restatement poisons the chunks the kernel leaves alone
            res.append(("g cleared", BD.check_exact(a["g"][:n][~kept].double(), ref[~kept], "adamw zero_grad"), kern))
            if bool((keep_g & ~skip).any()):         # bit 2: the next backward overwrites this chunk -- the gradient stays as it is
                res.append(("g kept (bit 2)", BD.check_exact(a["g"][:n][keep_g & ~skip].double(), g0[keep_g & ~skip],
                                                              "adamw gradient of a chunk flagged keep"), kern))
        if bool(skip.any()):                         # bit 1: a tensor without a gradient this step is not touched at all
            for k, was in before.items():
                res.append((f"{k} skipped (bit 1)", BD.check_exact(a[k][:n][skip].double(), was[skip].double(),
                                                                    f"adamw {k} of a chunk flagged skip"), kern))
        return res


def _table(rows, seconds):
    print(f"\n{'op':<22} {'output':<22} {'shape':<52} {'kernel':<44} {'headroom':>9}")
    for name, what, shape, kern, ratio in rows:
        head = "exact" if ratio == 0 else f"{1.0 / ratio:9.1f}x"
        print(f"{name:<22} {what[:22]:<22} {shape[:52]:<52} {kern[:44]:<44} {head:>9}")
    print(f"{len(rows)} outputs checked in {seconds:.1f} s")


def test_every_numeric_call_of_a_bf16_training_step_is_within_its_bound(monkeypatch):
    """one training step (forward, backward, clip + AdamW) of the benchmarked geometry with dropout on; every numeric method the
    step calls is checked at the first call of each signature (method, shapes, leading dimensions, layouts, epilogue, output type,
    accumulate, dropout on / off, column sums / workspace present, 16-byte alignment)"""
    t0 = time.time()
    monkeypatch.setenv("XL_DEFER_REDUCE", "0")             # column sums complete at their own call
    from xlxmert_amd.config import XLxmertConfig
    from xlxmert_amd.ops import HipOps
    from xlxmert_amd.params import ParamStore
    from xlxmert_amd.trainer import PretrainStep, synthetic_batch
    cfg = XLxmertConfig()
    oc = O.OracleConfig(**{k: getattr(cfg, k) for k in CFG_KEYS})
    sd = O.make_state_dict(oc, 2718)
    B = 256
    store = ParamStore(cfg, "cuda", torch.bfloat16)
    store.load_named(sd)
    rec = Recorder(HipOps(torch.bfloat16))
    tr = PretrainStep(cfg, B, 20, 64, dtype=torch.bfloat16, device="cuda", store=store, lr=1e-4, total_steps=1000, warmup_ratio=0.0,
                      plan=False,
                      drop_grads=False, overlap_optimizer=False, train_dropout=True, ops=rec)
    batch = synthetic_batch(cfg, B, 20, 8, seed=31)
    dev = {k: v.cuda() for k, v in batch.items()}
    losses = tr.step(dev)
    tr.sync()
    _sync()
    assert tr.engine.packed, "the language rows ran dense: the packed attention paths were not exercised"
    assert all(torch.isfinite(torch.as_tensor(x)).all() for x in losses if x is not None)
    _table(rec.rows, time.time() - t0)
    assert not rec.unchecked, f"numeric methods without a checker: {sorted(rec.unchecked)}"
    assert not rec.failures, "\n".join(rec.failures)
    assert not rec.leftover(), rec.leftover()
    for must in ("gemm", "gemm_wgrad_group", "sdpa_fwd", "sdpa_bwd", "layernorm_fwd", "layernorm_bwd", "ce_fwd_bwd", "sumsq", "adamw"):
        assert must in rec.called, must
    print(f"methods called: {sorted(rec.called)}; run time {time.time() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------------------------- edge cases
# The same checkers on random bf16 data at what the step does not reach.  Every call below is a new signature, so every one is
# checked; the test fails on any bound exceeded.
def _rec():
    from xlxmert_amd.ops import HipOps
    return Recorder(HipOps(torch.bfloat16))


def _done(rec, t0, n_min):
    _table(rec.rows, time.time() - t0)
    assert not rec.unchecked, sorted(rec.unchecked)
    assert not rec.failures, "\n".join(rec.failures)
    assert len(rec.rows) >= n_min, len(rec.rows)


def _rn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(torch.bfloat16)


@pytest.mark.parametrize("pingpong", [1, 2], ids=["default_dispatch", "pingpong_forced"])
def test_gemm_ragged_tiles_padded_ld_and_short_k_within_bounds(pingpong):
    """M, N off the tile grid, leading dimensions padded by 8 elements, K not a multiple of 64, every fast epilogue (the ragged
    edge tiles take the scalar erff epilogue, the interior the A-S one: both inside one output), pre-activations spread to |x| ~ 10"""
    t0 = time.time()
    rec = _rec()
    rec.set_gemm_pingpong(pingpong)
    g = torch.Generator(device="cuda").manual_seed(5)
    for M, N, K in ((300, 264, 200), (520, 776, 840)):
        lda = ldb = K + 8
        ldc = N + 8
        A, W = _rn(g, M, lda, scale=3.0), _rn(g, N, ldb, scale=1.0 / K ** 0.5)
        bias = torch.randn(N, generator=g, device="cuda") * 0.5
        res, aux_in = _rn(g, M, ldc), _rn(g, M, ldc, scale=3.0)
        for epi, p in ((BD.EPI_NONE, 0.0), (BD.EPI_GELU, 0.0), (BD.EPI_RESIDUAL, 0.1), (BD.EPI_DGELU, 0.0), (BD.EPI_GELU_DG, 0.0),
                       (BD.EPI_TANH, 0.0), (BD.EPI_MULAUX, 0.0)):
            C = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
            aux = aux_in.clone()
            rec.gemm(A, W, C, bias, res, aux, M, N, K, lda, ldb, ldc, ldr=ldc, ldx=ldc, epilogue=epi, p_drop=p, seed=11)
        C = torch.randn(M, ldc, generator=g, device="cuda")
        rec.gemm(A, W, C, None, None, None, M, N, K, lda, ldb, ldc, out_f32=True, accumulate=1)
        C = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
        cs, ws = torch.zeros(N, device="cuda"), torch.zeros(rec.workspace_floats(N), device="cuda")
        rec.gemm(A, W, C, bias, None, None, M, N, K, lda, ldb, ldc, colsum=cs, ws=ws)
    _done(rec, t0, 24)


@pytest.mark.parametrize("pingpong", [1, 2], ids=["default_dispatch", "pingpong_forced"])
def test_gemm_m_major_operands_with_an_odd_extent_within_bounds(pingpong):
    """dW = dY^T X as the 3 129-answer head issues it: A [K, M] and B [K, N] row-major (a_kmajor = b_kmajor = 0), fp32 out, with M
    -- then N -- odd (3129 inside a leading dimension of 3136, the pad columns holding other data).  Row M-1 of the product lost
    its last K term on the ping-pong kernel before its buffer range was rounded to whole 16-byte pieces (csrc/gemm_pp_kernel.h)."""
    t0 = time.time()
    rec = _rec()
    rec.set_gemm_pingpong(pingpong)
    g = torch.Generator(device="cuda").manual_seed(12)
    K, M, N, ld = 128, 3129, 1536, 3136
    dY, X = _rn(g, K, ld, scale=0.01), _rn(g, K, N)
    C = torch.zeros(M, N, device="cuda")
    rec.gemm(dY, X, C, None, None, None, M, N, K, ld, N, N, a_kmajor=0, b_kmajor=0, out_f32=True)
    C = torch.zeros(N, ld, device="cuda")
    rec.gemm(X, dY, C, None, None, None, N, M, K, N, ld, ld, a_kmajor=0, b_kmajor=0, out_f32=True)
    rec.gemm_wgrad_group([(dY, X, torch.zeros(M, N, device="cuda"), M, N, K, ld, N, N)], overwrite_mask=1)
    _done(rec, t0, 3)


def test_gelu_bwd_tails_within_bound():
    t0 = time.time()
    rec = _rec()
    g = torch.Generator(device="cuda").manual_seed(6)
    n = 10008                               # (a multiple of the kernel's 8-element vector; not of its block)
    pre = (torch.linspace(-10, 10, n, device="cuda") + torch.randn(n, generator=g, device="cuda") * 0.1).to(torch.bfloat16)
    dy = _rn(g, n)
    rec.gelu_bwd(dy, pre, torch.zeros(n, dtype=torch.bfloat16, device="cuda"), n)
    _done(rec, t0, 1)


@pytest.mark.parametrize("nq,nk", [(1, 33), (33, 1), (33, 33), (1, 1), (64, 33)])
def test_attention_short_sides_and_an_all_masked_example_within_bounds(nq, nk):
    """dense attention with nq or nk of 1 and 33, dropout on, example 1's keys all masked (kernel convention: zero output rows,
    zero gradients), forward and backward (saved keep bits where the geometry has them)"""
    t0 = time.time()
    rec = _rec()
    g = torch.Generator(device="cuda").manual_seed(7)
    B, H, dh = 4, 12, 64
    ld = 3 * H * dh
    qkv = _rn(g, B * max(nq, nk), ld)
    q, k, v = qkv, qkv[:, H * dh:], qkv[:, 2 * H * dh:]
    km = (torch.rand(B, nk, generator=g, device="cuda") > 0.3).to(torch.uint8)
    km[:, 0] = 1
    km[1] = 0
    o = torch.zeros(B * nq, H * dh, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(B * H * nq, device="cuda")
    kbn = rec.sdpa_keep_bits_bytes(B, H, nq, nk, dh)
    kb = torch.zeros(max(kbn, 4) // 4, dtype=torch.int32, device="cuda") if kbn else None
    rec.sdpa_fwd(q, k, v, km, o, lse, B, H, nq, nk, dh, ld, ld, ld, H * dh, 0.125, p_drop=0.1, seed=3, keep_bits=kb)
    dout = _rn(g, B * nq, H * dh)
    dq, dk, dv = (torch.zeros(B * n, H * dh, dtype=torch.bfloat16, device="cuda") for n in (nq, nk, nk))
    bg = torch.zeros(3 * H * dh, device="cuda")
    rec.sdpa_bwd(q, k, v, km, dout, lse, dq, dk, dv, B, H, nq, nk, dh, ld, ld, ld, H * dh, H * dh, H * dh, H * dh, 0.125,
                 p_drop=0.1, seed=3, bias_grad=bg, keep_bits=kb)
    _done(rec, t0, 5)


def test_attention_packed_with_one_token_examples_within_bounds():
    t0 = time.time()
    rec = _rec()
    g = torch.Generator(device="cuda").manual_seed(8)
    B, H, dh, n = 5, 12, 64, 20
    lens = torch.tensor([1, 20, 7, 1, 13])
    off = torch.zeros(B + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lens, 0)
    off = off.cuda()
    rows, pad = int(off[-1]), 64
    ld = 3 * H * dh
    qkv = torch.zeros(pad, ld, dtype=torch.bfloat16, device="cuda")
    qkv[:rows] = _rn(g, rows, ld)
    q, k, v = qkv, qkv[:, H * dh:], qkv[:, 2 * H * dh:]
    o = torch.zeros(pad, H * dh, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(B * H * n, device="cuda")
    kbn = rec.sdpa_keep_bits_bytes(B, H, n, n, dh)
    kb = torch.zeros(max(kbn, 4) // 4, dtype=torch.int32, device="cuda") if kbn else None
    rec.sdpa_fwd(q, k, v, None, o, lse, B, H, n, n, dh, ld, ld, ld, H * dh, 0.125, p_drop=0.1, seed=4, q_off=off, k_off=off,
                 q_pad=pad, k_pad=pad, keep_bits=kb)
    dout = torch.zeros(pad, H * dh, dtype=torch.bfloat16, device="cuda")
    dout[:rows] = _rn(g, rows, H * dh)
    dq, dk, dv = (torch.zeros(pad, H * dh, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    rec.sdpa_bwd(q, k, v, None, dout, lse, dq, dk, dv, B, H, n, n, dh, ld, ld, ld, H * dh, H * dh, H * dh, H * dh, 0.125,
                 p_drop=0.1, seed=4, q_off=off, k_off=off, q_pad=pad, k_pad=pad, keep_bits=kb)
    _done(rec, t0, 5)


@pytest.mark.parametrize("M", [300, 16384], ids=["ragged_rows", "dma_variant"])
def test_layernorm_rows_with_mean_100x_std_within_bounds(M):
    """pins the two-pass statistics: E[x^2] - E[x]^2 in fp32 loses every digit of the variance on these rows"""
    t0 = time.time()
    rec = _rec()
    g = torch.Generator(device="cuda").manual_seed(9)
    N = 768
    x = (100.0 + torch.randn(M, N, generator=g, device="cuda")).to(torch.bfloat16)
    gamma = 1 + 0.1 * torch.randn(N, generator=g, device="cuda")
    beta = 0.1 * torch.randn(N, generator=g, device="cuda")
    y = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    mean, rstd = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
    rec.layernorm_fwd(x, gamma, beta, y, mean, rstd, M, N, 1e-12)
    dy = _rn(g, M, N)
    dx, dxd = (torch.zeros(M, N, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    dg, db, dbp = (torch.zeros(N, device="cuda") for _ in range(3))
    ws = torch.zeros(rec.workspace_floats(N), device="cuda")
    rec.layernorm_bwd(dy, x, gamma, mean, rstd, dx, dg, db, dbp, M, N, ws=ws, dx_dropped=dxd, p_drop=0.1, seed=5)
    _done(rec, t0, 8)


def test_cross_entropy_10k_classes_padded_stride_logits_to_80_within_bounds():
    t0 = time.time()
    rec = _rec()
    g = torch.Generator(device="cuda").manual_seed(10)
    M, K, ld = 300, 10000, 10016
    logits = (torch.rand(M, ld, generator=g, device="cuda") * 160 - 80).to(torch.bfloat16).float()
    labels = torch.randint(0, K, (M,), generator=g, device="cuda")
    labels[::7] = -100
    counts = torch.tensor([float((labels != -100).sum())], device="cuda")
    dl = torch.zeros(M, ld, dtype=torch.bfloat16, device="cuda")
    loss, lse, mp = torch.zeros(1, device="cuda"), torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
    am = torch.zeros(M, dtype=torch.int32, device="cuda")
    rec.ce_fwd_bwd(logits, labels, counts, dl, loss, lse, am, mp, M, K, ld, ld)
    _done(rec, t0, 5)


def test_featloss_not_in_the_canonical_recipe_within_bounds():
    t0 = time.time()
    rec = _rec()
    g = torch.Generator(device="cuda").manual_seed(11)
    B, V, F, K = 8, 64, 2048, 500
    pred = _rn(g, B * V, F)
    cent = _rn(g, K, F)
    cid = torch.randint(0, K, (B, V), generator=g, device="cuda")
    vm = (torch.rand(B, V, generator=g, device="cuda") < 0.15).to(torch.uint8)
    nm = vm.sum(1).float()
    dpred = torch.zeros(B * V, F, dtype=torch.bfloat16, device="cuda")
    loss = torch.zeros(1, device="cuda")
    rec.featloss_fwd_bwd(pred, cent, cid, vm, nm, dpred, loss, B, V, F)
    _done(rec, t0, 2)
