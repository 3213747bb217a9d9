"""TEST INFRASTRUCTURE: records the launch schedule of the engine / trainer as a stream_audit.Trace.

Three sources, all forwarding unchanged (nothing is synchronised, reordered or skipped):
  - every call of the ops object (HipOps on the device, the fake ops on the CPU): the stream is torch's current stream at call time
    (what HipOps._stream() passes), the accesses come from ACCESS below; stream_fork / event_record / stream_wait become ordering events;
  - torch-side work between those calls (TorchOps, a TorchDispatchMode): every aten op that touches a CUDA tensor is a launch on the
    current stream -- mutated arguments and outputs written, the other tensors read; blocking device-to-host reads are host_sync;
  - torch's own ordering calls (patch_torch_ordering): synchronize / wait_stream / wait_event / record_event / Event.record / .wait.
A replayed launch plan runs no Python: LaunchPlan.run is wrapped and the C-ABI events of the recorded step are spliced in.

State that is not in an argument list:
  - while set_step_seed_ptr is set, every call with p_drop > 0 reads the seed tensor;
  - gemm_workspace(slabs, stream) registers a region that every gemm / gemm_wgrad_group on that stream accesses rw;
  - with set_deferred_reduce(1) a producer with a workspace does not touch its column-sum destinations (REDUCE_OUTS): it writes partials
    into `ws`; flush_reductions / flush_reductions_on(producer) reads those workspaces and adds into the destinations on ITS stream.
Memory reuse is not modelled: an address is an address.
"""
import inspect
import os
import sys

import torch

import stream_audit as SA

EPI_GELU, EPI_RESIDUAL, EPI_DGELU, EPI_ROWMAX, EPI_GELU_DG, EPI_MULAUX, EPI_ROWSAMPLE, EPI_ROWSCORE = 1, 2, 3, 5, 6, 7, 9, 10
_ROW_EPI = (EPI_ROWMAX, EPI_ROWSAMPLE, EPI_ROWSCORE)


def _aux_mode(a):
    """xl_gemm's aux: written by the epilogues that save something for later, read by the backward epilogues"""
    return "r" if a["epilogue"] in (EPI_DGELU, EPI_MULAUX) else "w"


def _c_mode(a):
    return "rw" if a["accumulate"] else "w"


def _drop_mode(a):
    return "w" if a["p_drop"] > 0 else "-"          # xl_layernorm_bwd drops the pointer when p_drop == 0


# method -> {tensor argument: mode}.  r / w / rw as include/xlxmert_hip.h states them ("-": registered or ignored, not accessed by the
# call itself); a callable takes the bound arguments.  The column-sum destinations of REDUCE_OUTS are "rw" here and move to the flush
# while reductions are deferred.  No entry is "acc": the library's fp32 atomics (K-split weight gradients, column sums without a
# workspace) are modelled as rw -- a pair of them on two streams must be ordered like any other pair of writers.
ACCESS = {
    "zero": {"t": "w"},
    "gemm_trace": {"buffer": "-"},
    "set_step_seed_ptr": {"step_seed": "-"},
    "gemm": {"A": "r", "B": "r", "C": _c_mode, "bias": "r", "residual": "r", "aux": _aux_mode, "colsum": "rw", "ws": "w"},
    "gemm_pair": {"c0": "-", "c1": "-"},                        # two gemm argument lists: expanded by the tracer
    "gemm_wgrad_group": {"problems": "-"},                      # [(dY r, X r, dW rw, ...)]: expanded by the tracer
    "wgrad_group_one_writer": {"problems": "-"},                # host query over the integer extents
    "layernorm_fwd": {"x": "r", "gamma": "r", "beta": "r", "y": "w", "mean": "w", "rstd": "w"},
    "layernorm_fwd_res": {"x": "r", "gamma": "r", "beta": "r", "y32": "w", "y16": "w", "mean": "w", "rstd": "w"},
    "layernorm_bwd": {"dy": "r", "x": "r", "gamma": "r", "mean": "r", "rstd": "r", "dx": "w", "dgamma": "rw", "dbeta": "rw",
                      "dbias_prev": "rw", "ws": "w", "dx_dropped": _drop_mode},
    "layernorm_bwd_res": {"dy": "r", "x": "r", "gamma": "r", "mean": "r", "rstd": "r", "dx": "w", "dgamma": "rw", "dbeta": "rw",
                          "dbias_prev": "rw", "ws": "w", "dx_dropped": "w"},
    "visn_ln_fwd": {"xv": "r", "pos": "r", "wbox": "r", "bbox": "r", "gv": "r", "bv": "r", "gb": "r", "bb": "r", "y": "w",
                    "mean_v": "w", "rstd_v": "w", "mean_b": "w", "rstd_b": "w"},
    "visn_ln_bwd": {"dy": "r", "xv": "r", "pos": "r", "wbox": "r", "bbox": "r", "gv": "r", "gb": "r", "mean_v": "r", "rstd_v": "r",
                    "mean_b": "r", "rstd_b": "r", "dxv": "w", "dgv": "rw", "dbv": "rw", "dgb": "rw", "dbb": "rw", "dwbox": "rw",
                    "dbbox": "rw", "dbias_visn": "rw", "ws": "w"},
    "embed_ln_fwd": {"ids": "r", "tt": "r", "word": "r", "pos": "r", "type_": "r", "gamma": "r", "beta": "r", "y": "w", "pre": "w",
                     "mean": "w", "rstd": "w"},
    "embed_bwd": {"dpre": "r", "ids": "r", "tt": "r", "dword": "rw", "dpos": "rw", "dtype_tab": "rw", "order": "r"},
    "codebook_gather": {"cluster_ids": "r", "vis_mask": "r", "centroids": "r", "mask_feat": "r", "feats": "w"},
    "masked_colsum": {"x": "r", "mask": "r", "out": "rw", "ws": "w"},
    "colsum": {"x": "r", "out": "rw", "ws": "w"},
    "dropout": {"x": "r", "y": "w"},
    "gelu_bwd": {"dy": "r", "pre": "r", "dx": "w"},
    "tanh_bwd": {"dy": "r", "y": "r", "dx": "w"},
    "bce_logits_fwd_bwd": {"logits": "r", "targets": "r", "dlogits": "w", "loss": "rw"},
    "remask_lowest": {"prob": "r", "vis_mask": "w"},
    "sampler_update": {"pred_ids": "r", "vis_mask": "r", "code_ids": "rw"},
    "sampler_ar_update": {"prob": "r", "pred_ids": "r", "visited": "rw", "vis_mask": "rw", "code_ids": "rw"},
    "caption_step": {"row_prob": "r", "row_id": "r", "lang_off": "r", "lengths": "r", "tokens": "rw", "fed_ids": "w",
                     "word_mask": "rw", "conf": "w", "score": "w"},
    "grid_step": {"row_prob": "r", "row_id": "r", "free_mask": "r", "order": "r", "code_ids": "rw", "vis_mask": "rw", "conf": "rw",
                  "score": "w"},
    "pair_expand": {"vis": "r", "lang": "r", "lang_off": "r", "x0": "w", "chunk_off": "w", "chunk_rows": "w", "chunk_kmask": "w",
                    "vis2": "r", "lang2": "r", "x0_2": "w", "lang_len": "r"},
    "match_rank": {"rel": "r", "margin": "rw", "prob": "w", "topk_images": "w", "topk_captions": "w", "image_of_caption": "r",
                   "caption_of_image": "r", "rank_t2i": "w", "rank_i2t": "w"},
    "conv2d_nhwc": {"x": "r", "w": "r", "bias": "r", "y": "w", "aux": "r", "mean": "r", "rstd": "r", "noise": "r"},
    "instnorm_stats": {"x": "r", "mean": "w", "rstd": "w", "ws": "w"},
    "resize_bilinear_nhwc": {"x": "r", "y": "w"},
    "torgb_accum": {"rgb": "r", "acc": "rw", "out": "w"},
    "normal_planes": {"out": "w"},
    "normal_from_bits": {"h0": "r", "h1": "r", "z": "w"},
    "sdpa_fwd": {"q": "r", "k": "r", "v": "r", "key_mask": "r", "o": "w", "lse": "w", "q_off": "r", "k_off": "r",
                 "keep_bits": lambda a: "w" if a["p_drop"] > 0 else "-"},
    "sdpa_bwd": {"q": "r", "k": "r", "v": "r", "key_mask": "r", "dout": "r", "lse": "r", "dq": "w", "dk": "w", "dv": "w",
                 "bias_grad": "rw", "ws": "w", "q_off": "r", "k_off": "r", "keep_bits": lambda a: "r" if a["p_drop"] > 0 else "-"},
    "attn_probs": {"q": "r", "k": "r", "key_mask": "r", "lse": "r", "probs": "w", "q_off": "r", "k_off": "r"},
    "mask_counts": {"labels": "r", "vis_mask": "r", "counts": "w", "nmask": "w"},
    "ce_fwd_bwd": {"logits": "r", "labels": "r", "counts": "r", "dlogits": "w", "loss_out": "rw", "row_lse": "w", "row_argmax": "w",
                   "row_maxprob": "w"},
    "featloss_fwd_bwd": {"pred": "r", "centroids": "r", "cluster_ids": "r", "vis_mask": "r", "nmask": "r", "dpred": "w",
                         "loss_out": "rw", "rows": "r", "targets": "r"},
    "gather_rows": {"src": "r", "rows": "r", "dst": "w"},
    "scatter_rows": {"src": "r", "rows": "r", "dst": "w"},
    "rowmax_combine": {"ws": "r", "row_maxprob": "w", "row_argmax": "w", "row_lse": "w"},
    "rowsample_combine": {"ws": "r", "row_prob": "w", "row_id": "w", "row_lse": "w"},
    "rowscore_combine": {"ws": "r", "labels": "r", "row_nll": "w", "row_pred": "w", "row_max": "w", "totals": "rw"},
    "score_rows": {"logits": "r", "labels": "r", "row_nll": "w", "row_pred": "w", "row_max": "w", "totals": "rw"},
    "sample_rows": {"logits": "r", "row_prob": "w", "row_id": "w", "row_lse": "w"},
    "sample_rows_trunc": {"logits": "r", "row_prob": "w", "row_id": "w", "row_lse": "w", "row_kept": "w"},
    "gumbel_from_bits": {"h": "r", "g": "w"},
    "gather_labels": {"labels": "r", "rows": "r", "out": "w"},
    "sumsq": {"g": "r", "out": "rw", "scratch": "rw"},
    "schedule_step": {"step": "rw", "lr_and_steps": "w"},
    "adamw": {"p": "rw", "g": "rw", "m": "rw", "v": "rw", "p_compute": "w", "decay_flags": "r", "sumsq": "r", "lr_and_steps": "r",
              "chunk_steps": "r"},
    # the collectives run on the communicator's stream, which is out of this audit's scope: the tracer refuses them
    "comm_allreduce": {"buf": "rw"},
    "comm_reduce_scatter": {"buf": "rw"},
    "comm_allgather": {"buf": "rw"},
    "take_f32": {"src": "r", "idx": "r", "dst": "w"},
    "put_f32": {"dst": "rw", "idx": "r", "src": "r"},
    "cast_from_f32": {"src": "r", "dst": "w"},
    "cast_to_f32": {"src": "r", "dst": "w"},
}
COMM = ("comm_allreduce", "comm_reduce_scatter", "comm_allgather", "comm_wait")
ORDERING = ("stream_fork", "event_record", "stream_wait", "new_event")
REDUCE_OUTS = {"gemm": ("colsum",), "layernorm_bwd": ("dgamma", "dbeta", "dbias_prev"),
               "layernorm_bwd_res": ("dgamma", "dbeta", "dbias_prev"), "sdpa_bwd": ("bias_grad",),
               "visn_ln_bwd": ("dgv", "dbv", "dgb", "dbb", "dwbox", "dbbox", "dbias_visn"), "colsum": ("out",), "masked_colsum": ("out",)}


def _es(t):
    return t.element_size()


def view_region(t):
    """the bytes of a tensor view: a rectangle for a row-strided 2-d view, else the range between its first and last element"""
    if t.numel() == 0:
        return SA.rng(t.data_ptr(), t.data_ptr())
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) > t.shape[1]:
        return SA.rect(t.data_ptr(), t.shape[0], t.shape[1] * _es(t), t.stride(0) * _es(t))
    lo = sum((n - 1) * st for n, st in zip(t.shape, t.stride()) if st < 0)
    hi = sum((n - 1) * st for n, st in zip(t.shape, t.stride()) if st > 0)
    return SA.rng(t.data_ptr() + lo * _es(t), t.data_ptr() + (hi + 1) * _es(t))


def _r2(t, rows, cols, ld):
    return SA.rect(t.data_ptr(), rows, cols * _es(t), ld * _es(t))


def _vec(t, n):
    return SA.rng(t.data_ptr(), t.data_ptr() + int(n) * _es(t))


def _packed_rows(t, a, off, n, ld):
    """rows of an attention operand: B * n dense rows, or -- packed, the count lives on the device -- the rows of the view"""
    HD = a["H"] * a["dh"]
    if a[off] is None:
        return _r2(t, a["B"] * n, HD, ld)
    rows = t.shape[0] if t.dim() == 2 else max(1, t.numel() // max(HD, 1))
    pad = a.get("q_pad" if off == "q_off" else "k_pad", 0)
    return _r2(t, max(rows, pad), HD, ld)


def _gemm_extents(a):
    M, N, K = a["M"], a["N"], a["K"]
    out = {"A": lambda t: _r2(t, M, K, a["lda"]) if a["a_kmajor"] else _r2(t, K, M, a["lda"]),
           "B": lambda t: _r2(t, N, K, a["ldb"]) if a["b_kmajor"] else _r2(t, K, N, a["ldb"]),
           "C": lambda t: _r2(t, M, N, a["ldc"]), "bias": lambda t: _vec(t, N), "colsum": lambda t: _vec(t, N)}
    if a["epilogue"] in _ROW_EPI:
        out["aux"] = lambda t: SA.rng(t.data_ptr(), t.data_ptr() + (N // 64) * M * 16)
        out["residual"] = lambda t: _vec(t, M)             # (XL_EPI_ROWSCORE: int64 labels; ignored by the other two)
    else:
        out["aux"] = lambda t: _r2(t, M, N, a["ldx"])
        out["residual"] = lambda t: _r2(t, M, N, a["ldr"])
    return out


def _sdpa_extents(a):
    out = {"q": lambda t: _packed_rows(t, a, "q_off", a["nq"], a["ldq"]), "k": lambda t: _packed_rows(t, a, "k_off", a["nk"], a["ldk"])}
    if "ldv" in a:
        out["v"] = lambda t: _packed_rows(t, a, "k_off", a["nk"], a["ldv"])
    if "o" in a:
        out["o"] = lambda t: _packed_rows(t, a, "q_off", a["nq"], a["ldo"])
    if "dout" in a:
        out.update(dout=lambda t: _packed_rows(t, a, "q_off", a["nq"], a["ldo"]), dq=lambda t: _packed_rows(t, a, "q_off", a["nq"], a["lddq"]),
                   dk=lambda t: _packed_rows(t, a, "k_off", a["nk"], a["lddk"]), dv=lambda t: _packed_rows(t, a, "k_off", a["nk"], a["lddv"]))
    return out


# method -> f(bound arguments) -> {argument: f(tensor) -> region}: the calls that carry (rows, columns, leading dimension).
# Every other tensor argument is taken by its view (view_region).
EXTENTS = {
    "gemm": _gemm_extents,
    "sdpa_fwd": _sdpa_extents, "sdpa_bwd": _sdpa_extents, "attn_probs": _sdpa_extents,
    "dropout": lambda a: {"x": lambda t: _r2(t, a["M"], a["N"], a["ldx"]), "y": lambda t: _r2(t, a["M"], a["N"], a["ldy"])},
    "colsum": lambda a: {"x": lambda t: _r2(t, a["M"], a["N"], a["ldx"]), "out": lambda t: _vec(t, a["N"])},
    "masked_colsum": lambda a: {"x": lambda t: _r2(t, a["M"], a["N"], a["ldx"]), "out": lambda t: _vec(t, a["N"])},
    "gather_rows": lambda a: {"dst": lambda t: _r2(t, a["n_rows"], a["N"], a["ld_dst"])},
    "scatter_rows": lambda a: {"src": lambda t: _r2(t, a["n_rows"], a["N"], a["ld_src"])},
    "ce_fwd_bwd": lambda a: {"logits": lambda t: _r2(t, a["M"], a["K"], a["ldl"]),
                             "dlogits": lambda t: _r2(t, a["M"], min(a["lddl"], (a["K"] + 7) // 8 * 8), a["lddl"])},
    "bce_logits_fwd_bwd": lambda a: {"logits": lambda t: _r2(t, a["M"], a["N"], a["ld_logits"]),
                                     "targets": lambda t: _r2(t, a["M"], a["N"], a["ld_targets"]),
                                     "dlogits": lambda t: _r2(t, a["M"], a["ld_dlogits"], a["ld_dlogits"])},
    "score_rows": lambda a: {"logits": lambda t: _r2(t, a["M"], a["K"], a["ldl"])},
    "sample_rows": lambda a: {"logits": lambda t: _r2(t, a["M"], a["K"], a["ldl"])},
    "sample_rows_trunc": lambda a: {"logits": lambda t: _r2(t, a["M"], a["K"], a["ldl"])},
}

_PKG = os.sep + "xlxmert_amd" + os.sep
_SKIP_FILES = ("ops.py", "_lib.py")


def call_site():
    """file:line of the innermost engine / trainer frame of the current call (the package's ops.py and _lib.py are plumbing)"""
    f = sys._getframe(1)
    fallback = ""
    while f is not None:
        fn = f.f_code.co_filename
        base = os.path.basename(fn)
        if _PKG in fn and base not in _SKIP_FILES:
            return f"{base}:{f.f_lineno}"
        if not fallback and base.startswith("test_"):
            fallback = f"{base}:{f.f_lineno}"
        f = f.f_back
    return fallback or "?"


def _cur_stream():
    return torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0


class Tracer:
    def __init__(self, stream_of=_cur_stream):
        self.trace = SA.Trace()
        self.stream_of = stream_of
        self.deferred = False
        self.pending = {}            # producing stream -> [(workspace region, [(destination region, argument)], producer name, site)]
        self.seed = None             # the tensor xl_set_step_seed_ptr registered
        self.slabs = {}              # stream -> region of its slab workspace
        self.n_abi = self.n_torch = 0
        self._depth = 0
        self._rec = None             # C-ABI events of the launch plan being recorded
        self._keep = []              # torch events seen (kept alive: their id() is their name)
        self._sigs = {}

    # ---- emitting
    def _emit(self, ev, abi=True):
        self.trace.events.append(ev)
        if abi and self._rec is not None:
            self._rec.append(ev)

    def launch(self, stream, accesses, name, site, abi=True):
        acc = [(r, m, n) for r, m, n in accesses if SA.bounds(r)[1] > SA.bounds(r)[0]]
        self._emit(SA.Launch(stream, acc, name, site), abi)

    # ---- the ops object's calls
    def bind(self, name, fn, args, kw):
        """the call's arguments by the names of HipOps.<name> (the engine's calls are calls of that signature, whatever object stands in)"""
        sig = self._sigs.get(name)
        if sig is None:
            from xlxmert_amd.ops import HipOps
            base = inspect.getattr_static(HipOps, name, None)
            if base is not None and not isinstance(base, staticmethod):
                sig = inspect.signature(base)
                sig = sig.replace(parameters=list(sig.parameters.values())[1:])
            else:
                sig = inspect.signature(fn)
            self._sigs[name] = sig
        ba = sig.bind(*args, **kw)
        ba.apply_defaults()
        return dict(ba.arguments)

    def accesses_of(self, name, a):
        """[(region, mode, argument)] of one call with bound arguments `a`, and the deferred destinations [(region, argument)]"""
        if name == "gemm_pair":
            out, dests = [], []
            for c in (a["c0"], a["c1"]):
                g = self._bind_gemm(c)
                o, d = self.accesses_of("gemm", g)
                out += o
                dests += d
            return out, dests
        if name == "gemm_wgrad_group":
            out = []
            for i, (dY, X, dW, M, N, K, lda, ldb, ldc) in enumerate(a["problems"]):
                over = (a["overwrite_mask"] >> i) & 1
                out += [(_r2(dY, K, M, lda), "r", f"dY{i}"), (_r2(X, K, N, ldb), "r", f"X{i}"), (_r2(dW, M, N, ldc), "w" if over else "rw", f"dW{i}")]
            return out, []
        table = ACCESS[name]
        if name == "gemm" and a.get("colsum") is None:
            a = dict(a, ws=None)                    # (HipOps.gemm drops the workspace of a call without column sums)
        ext = EXTENTS[name](a) if name in EXTENTS else {}
        # (without a workspace the column sums are fp32 atomics on the destination, issued by the producer itself)
        defer = set(REDUCE_OUTS.get(name, ())) if (self.deferred and a.get("ws") is not None) else set()
        out, dests = [], []
        for arg, mode in table.items():
            t = a.get(arg)
            if t is None or not isinstance(t, torch.Tensor):
                continue
            if callable(mode):
                mode = mode(a)
            if mode == "-":
                continue
            region = ext[arg](t) if arg in ext else view_region(t)
            if arg in defer:
                dests.append((region, arg))
            else:
                out.append((region, mode, arg))
        return out, dests

    def call(self, name, fn, args, kw):
        if self._depth:                              # a call the ops object makes of itself (gemm_pair -> gemm): part of the outer one
            return fn(*args, **kw)
        self._depth += 1
        try:
            return self._call(name, fn, args, kw)
        finally:
            self._depth -= 1

    def _call(self, name, fn, args, kw):
        site = call_site()
        if name in COMM:
            raise NotImplementedError(f"{name}: the collectives' stream is outside the stream audit")
        if name == "stream_fork":
            a = self.bind(name, fn, args, kw)
            self._emit(SA.Fork(a["from_stream"].cuda_stream, a["to_stream"].cuda_stream, site))
            return fn(*args, **kw)
        if name == "event_record":
            a = self.bind(name, fn, args, kw)
            self._emit(SA.Record(("xl", a["ev"]), a["stream"].cuda_stream, site))
            return fn(*args, **kw)
        if name == "stream_wait":
            a = self.bind(name, fn, args, kw)
            self._emit(SA.Wait(("xl", a["ev"]), a["stream"].cuda_stream, site))
            return fn(*args, **kw)
        if name == "set_deferred_reduce":
            self.deferred = bool(args[0] if args else kw["on"])
            return fn(*args, **kw)
        if name == "set_step_seed_ptr":
            self.seed = args[0] if args else kw["step_seed"]
            return fn(*args, **kw)
        if name == "gemm_workspace":
            ws = fn(*args, **kw)
            a = self.bind(name, fn, args, kw)
            st = a["stream"].cuda_stream if a["stream"] is not None else self.stream_of()
            if ws is not None:
                self.slabs[st] = view_region(ws)
            return ws
        if name in ("flush_reductions", "flush_reductions_on"):
            return self._flush(name, fn, args, kw, site)
        if name not in ACCESS:
            return fn(*args, **kw)                   # switches, size queries, new_event ...
        a = self.bind(name, fn, args, kw)
        stream = self.stream_of()
        acc, dests = self.accesses_of(name, a)
        p_drop = a.get("p_drop", 0.0)
        if name == "gemm_pair":
            p_drop = max(self._bind_gemm(c)["p_drop"] for c in (a["c0"], a["c1"]))
        if self.seed is not None and p_drop and p_drop > 0:
            acc.append((view_region(self.seed), "r", "step_seed"))
        if name in ("gemm", "gemm_pair", "gemm_wgrad_group") and stream in self.slabs:
            acc.append((self.slabs[stream], "rw", "slab_workspace"))
        if dests:
            ws = [r for r, m, n in acc if n == "ws"]
            self.pending.setdefault(stream, []).append((ws[0] if ws else None, dests, name, site))
        if acc:
            self.n_abi += 1
            self.launch(stream, acc, name, site)
        return self.invoke(name, a, acc, dests, lambda: fn(*args, **kw))

    def _bind_gemm(self, c):
        """bound arguments of a held-back gemm call (ops.GemmCall)"""
        return self.bind("gemm", None, tuple(c.a), c.kw)

    def invoke(self, name, a, accesses, dests, run):
        """run the call (the CPU honesty test overrides this to look at the arguments before and after)"""
        return run()

    def _flush(self, name, fn, args, kw, site):
        stream = self.stream_of()
        producer = stream if name == "flush_reductions" else (args[0] if args else kw["producer_stream"]).cuda_stream
        pend = self.pending.pop(producer, [])
        acc = []
        for ws, dests, pname, psite in pend:
            if ws is not None:
                acc.append((ws, "r", f"ws<-{pname}@{psite}"))
            acc += [(r, "rw", f"{arg}<-{pname}@{psite}") for r, arg in dests]
        if acc:
            self.n_abi += 1
            self.launch(stream, acc, name, site)
        return self.invoke(name, {"_pending": pend}, acc, [], lambda: fn(*args, **kw))

    # ---- launch plans
    def patch_plans(self, monkeypatch):
        """record(): collect the C-ABI events of the recorded step; make_plan(): attach them to the plan; LaunchPlan.run: splice them"""
        from xlxmert_amd import _lib
        tr = self
        orig_record, orig_make, orig_run = _lib.Lib.record, _lib.Lib.make_plan, _lib.LaunchPlan.run

        def record(lib):
            inner = orig_record(lib)

            class _Rec:
                def __enter__(self_):
                    tr._rec = []
                    return inner.__enter__()

                def __exit__(self_, *exc):
                    tr._last_rec, tr._rec = tr._rec, None
                    return inner.__exit__(*exc)
            return _Rec()

        def make_plan(lib, calls):
            plan = orig_make(lib, calls)
            assert isinstance(plan, _lib.LaunchPlan), "multi-segment plans are outside the stream audit"
            plan._audit_events = list(tr._last_rec)
            return plan

        def run(plan):
            tr.trace.mark("plan replay")
            tr.trace.events.extend(plan._audit_events)
            tr.n_replayed = getattr(tr, "n_replayed", 0) + 1
            return orig_run(plan)
        monkeypatch.setattr(_lib.Lib, "record", record)
        monkeypatch.setattr(_lib.Lib, "make_plan", make_plan)
        monkeypatch.setattr(_lib.LaunchPlan, "run", run)

    # ---- torch's own ordering calls
    def patch_torch_ordering(self, monkeypatch):
        tr = self
        S, E = torch.cuda.Stream, torch.cuda.Event

        def ev_key(e):
            tr._keep.append(e)
            return ("torch", id(e))

        def outer(emit, orig):
            def f(*args, **kw):
                if tr._depth:
                    return orig(*args, **kw)
                tr._depth += 1
                try:
                    emit(call_site(), *args, **kw)
                    return orig(*args, **kw)
                finally:
                    tr._depth -= 1
            return f

        def cur():
            return torch.cuda.current_stream().cuda_stream

        def on(stream):
            return stream.cuda_stream if stream is not None else cur()

        patches = [          # (the emitters take torch's own parameter names: a caller may pass them by keyword)
            (torch.cuda, "synchronize", lambda site, device=None: tr._emit(SA.HostSync(SA.ALL, site), False)),
            (S, "synchronize", lambda site, self: tr._emit(SA.HostSync(self.cuda_stream, site), False)),
            (E, "synchronize", lambda site, self: tr._emit(SA.HostSync(SA.EventRef(ev_key(self)), site), False)),
            (S, "wait_stream", lambda site, self, stream: tr._emit(SA.Fork(stream.cuda_stream, self.cuda_stream, site), False)),
            (S, "wait_event", lambda site, self, event: tr._emit(SA.Wait(ev_key(event), self.cuda_stream, site), False)),
            (E, "record", lambda site, self, stream=None: tr._emit(SA.Record(ev_key(self), on(stream), site), False)),
            (E, "wait", lambda site, self, stream=None: tr._emit(SA.Wait(ev_key(self), on(stream), site), False)),
        ]
        for owner, name, emit in patches:
            monkeypatch.setattr(owner, name, outer(emit, getattr(owner, name)))
        orig_re = S.record_event

        def record_event(s, event=None):
            if tr._depth:
                return orig_re(s, event)
            tr._depth += 1
            try:
                e = orig_re(s, event)
                tr._emit(SA.Record(ev_key(e), s.cuda_stream, call_site()), False)
                return e
            finally:
                tr._depth -= 1
        monkeypatch.setattr(S, "record_event", record_event)


class TracingProxy:
    """stands in for any ops object (the fake ops on the CPU): every attribute forwarded, every call through the tracer"""

    def __init__(self, inner, tracer):
        object.__setattr__(self, "_inner", inner)
        object.__setattr__(self, "_tracer", tracer)

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr) or name.startswith("_"):
            return attr
        return lambda *args, **kw: self._tracer.call(name, attr, args, kw)

    def __setattr__(self, name, value):
        setattr(self._inner, name, value)


def public_methods(cls):
    return sorted(n for n, f in inspect.getmembers(cls, predicate=inspect.isfunction) if not n.startswith("_"))


def tracing_hipops(dtype, tracer):
    """a HipOps (the trainer asks isinstance) whose public methods all pass through the tracer"""
    from xlxmert_amd.ops import HipOps

    class TracingHipOps(HipOps):
        pass

    def make(name):
        base = getattr(HipOps, name)

        def method(self, *args, **kw):
            return tracer.call(name, base.__get__(self, TracingHipOps), args, kw)
        method.__name__ = name
        return method
    for name in public_methods(HipOps):
        if isinstance(inspect.getattr_static(HipOps, name), staticmethod):
            continue
        setattr(TracingHipOps, name, make(name))
    return TracingHipOps(dtype)


# ---------------------------------------------------------------- torch-side work
_SYNC_OPS = ("_local_scalar_dense", "nonzero", "masked_select", "_unique2", "equal", "is_nonzero")
_NO_KERNEL = ("empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided", "detach", "alias", "lift_fresh",
              "_unsafe_view", "_reshape_alias", "resize_", "set_", "is_pinned", "_pin_memory")


class TorchOps(torch.utils._python_dispatch.TorchDispatchMode):
    """every aten op that touches a CUDA tensor, as a launch on the current stream"""

    def __init__(self, tracer):
        super().__init__()
        self.tracer = tracer

    @staticmethod
    def _tensors(v, out):
        if isinstance(v, torch.Tensor):
            out.append(v)
        elif isinstance(v, (list, tuple)):
            for x in v:
                TorchOps._tensors(x, out)
        return out

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        res = func(*args, **kwargs)
        name = func._schema.name.split("::")[-1]
        if name in _NO_KERNEL:
            return res
        reads, writes = [], []
        for i, sa in enumerate(func._schema.arguments):
            v = args[i] if i < len(args) else kwargs.get(sa.name)
            ts = self._tensors(v, [])
            if ts:
                (writes if (sa.alias_info is not None and sa.alias_info.is_write) else reads).extend((t, sa.name) for t in ts)
        outs = self._tensors(res, [])
        rets = func._schema.returns
        is_view = bool(outs) and not writes and all(r.alias_info is not None and not r.alias_info.is_write for r in rets)
        if is_view:
            return res
        taken = {t.data_ptr() for t, _ in reads + writes if t.numel()}          # (an op that hands back an argument wrote nothing new)
        writes += [(t, f"out{i}") for i, t in enumerate(outs) if t.data_ptr() not in taken]
        cuda = [t for t, _ in reads + writes if t.is_cuda]
        if not cuda:
            return res
        tr = self.tracer
        site = call_site()
        acc = [(view_region(t), "r", n) for t, n in reads if t.is_cuda] + [(view_region(t), "w", n) for t, n in writes if t.is_cuda]
        stream = torch.cuda.current_stream().cuda_stream
        tr.n_torch += 1
        tr.launch(stream, acc, "aten." + name, site, abi=False)
        to_host = any(t.is_cuda for t, _ in reads) and any(not t.is_cuda for t, _ in writes)
        non_blocking = bool(kwargs.get("non_blocking", False)) or (name == "copy_" and len(args) > 2 and bool(args[2]))
        if name in _SYNC_OPS or (to_host and not non_blocking):
            tr._emit(SA.HostSync(stream, site), False)
        return res
