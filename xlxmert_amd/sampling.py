"""The classifier tail both sampler heads and the validation pass share, and the sampler loops of the engine.

RowPredictor: "softmax over x W^T + bias per row" for a tied classifier that is frozen for the call -- the codebook head (W = the
centroids) and the MLM decoder (W = the word embeddings).  Engine (SamplerMixin) and LangHeads hold one each; only the final
contraction is here, each head's transform stays with the head.  SamplerMixin: the four on-device loops over them.
"""
import math
import os

import torch

from .ops import EPI_ROWMAX, EPI_ROWSAMPLE, EPI_ROWSCORE

# Temperature sampling: each position DRAWS its code from softmax(logits / T) instead of taking the mode -- Gumbel-max, the
# noise a pure function of (launch seed, global row b*V+v, code), so the fused and the unfused path draw identically.  The
# draw fills the buffers of the greedy step (the id row = the drawn code, the prob row = its tempered probability: the
# confidence of the re-masking and of the `confidence` position policy), so everything behind RowPredictor.run is unchanged.
TEMPERATURE_MIN, TEMPERATURE_MAX = 1e-3, 1e3     # the range of the pad-column guarantee (include/xlxmert_hip.h XL_EPI_ROWSAMPLE)
# Truncated sampling: top-k, top-p (nucleus) and min-p next to the temperature (include/xlxmert_hip.h xl_sample_rows_trunc states
# the semantics).  Any of the three given: the step materialises the fp32 logits and draws with xl_sample_rows_trunc, for fp32 and
# bf16 alike -- also where the fused predict path is available: truncation needs a row's logits ranked, which the fused epilogue
# never has in memory.  Same noise function and launch seed as the temperature path: a truncated draw equals the untruncated one
# whenever that lies in the kept set.  The prob row stays the probability under the FULL tempered softmax (a confidence for the
# re-masking and the `confidence` policy); row_kept holds the kept-set sizes.  top-p and min-p act within at most
# TRUNC_MAX_CAND = 256 candidates (row_kept == 256 reveals the cap).
TRUNC_MAX_CAND = 256
GRID_MODES = {"nar": 0, "confidence": 1, "tlbr": 2, "order": 2}     # XL_GRID_NAR / XL_GRID_AR_CONF / XL_GRID_AR_ORDER
CAPTION_MAX_L = 64              # xl_caption_step: one lane per token position


def check_temperature(temperature):
    if temperature is None:
        return None
    t = float(temperature)
    if not math.isfinite(t) or not (TEMPERATURE_MIN <= t <= TEMPERATURE_MAX):
        raise ValueError(f"temperature {temperature!r}: a finite value in [{TEMPERATURE_MIN}, {TEMPERATURE_MAX}] (None = greedy)")
    return t


def check_truncation(top_k, top_p, min_p):
    """None (no truncation argument given), or (top_k, top_p, log_min_p) as xl_sample_rows_trunc takes them"""
    if top_k is None and top_p is None and min_p is None:
        return None
    if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or not (1 <= top_k <= TRUNC_MAX_CAND)):
        raise ValueError(f"top_k {top_k!r}: an int in [1, {TRUNC_MAX_CAND}] (None = {TRUNC_MAX_CAND} candidates)")
    for name, v in (("top_p", top_p), ("min_p", min_p)):
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not (0.0 < v <= 1.0):
            raise ValueError(f"{name} {v!r}: a finite float in (0, 1] (None = off)")
    return (TRUNC_MAX_CAND if top_k is None else top_k, 1.0 if top_p is None else float(top_p),
            -math.inf if min_p is None else math.log(float(min_p)))


def sample_launch_seed(seed, step):
    """noise seed of sampler step `step`: seed * 0x9E3779B97F4A7C15 + step (mod 2^64) -- distinct per step, and for the seeds
    a caller picks (small integers, 63-bit draws) distinct across (seed, step) pairs"""
    return (int(seed) * 0x9E3779B97F4A7C15 + int(step)) & 0xFFFFFFFFFFFFFFFF


class RowPredictor:
    """Rows x [M, k] through the classifier W [n, k] + bias: per row the predicted / drawn column, its probability and the
    log-sum-exp (run), or loss and accuracy totals against labels (score).

    Sampling and scoring never need the logits themselves, only per row (max, sum exp, argmax / the draw / the label's logit): on
    the bf16 path the contraction ends in the XL_EPI_ROWMAX / ROWSAMPLE / ROWSCORE epilogue (a record per row and 64-column
    segment) and xl_row*_combine finishes the rows -- for the 10k codebook at bs 256, 42 MB of segment records instead of writing
    and re-reading the 655 MB fp32 logits.  W is padded to a multiple of 256 rows for it (zero rows with bias -1e30: never the
    maximum, exp() = 0); columns a head bans sit at -1e30 in its bias the same way, so every path below excludes them without a
    line of kernel code.  Otherwise (fp32, rows off the 256 grid, XL_FUSED_PREDICT=0, truncation) the fp32 logits go to memory.

    weight() / bias(): the head's current W (compute dtype) and fp32 bias, read again at every prepare() and logits contraction
    (the centroids may have been replaced, the banned ids changed).  logits, ldl, ldd: the fp32 logits buffer, its row stride and
    the row stride of the CE kernel's gradient operand (image K, Kp; words Vp, Vp).  out: the (prob, id, lse) rows.  `logits` and
    `out` may be attached later (the MLM head allocates them with its first caption loop).  The padded operand, the padded bias,
    its copy divided by T, the segment workspace of (n_pad / 64) * rows * 4 floats and row_kept are allocated when first needed."""

    def __init__(self, eng, n, k, rows, weight, bias, ldl, ldd, logits=None, out=None):
        self.e, self.n, self.k, self.rows = eng, n, k, rows
        self.weight, self.bias, self.ldl, self.ldd, self.logits, self.out = weight, bias, ldl, ldd, logits, out
        self.n_pad = (n + 255) // 256 * 256
        self.w_pad = self.bias_pad = self.bias_pad_T = self.seg_ws = self.row_kept = None

    def available(self, M, entry="rowmax_combine"):
        """the one gate of the fused paths; `entry`: the combine entry point the caller needs (asked of the ops object, not of
        its type: a proxy forwards it)"""
        e = self.e
        return (e.cdtype == torch.bfloat16 and M % 256 == 0 and self.k % 8 == 0 and hasattr(e.ops, entry)
                and os.environ.get("XL_FUSED_PREDICT", "1") != "0")

    def prepare(self, bias=None):
        """the fused paths' operands: W padded with zero rows, the bias (the head's own, or `bias`) padded with -1e30"""
        e = self.e
        if self.w_pad is None:
            self.w_pad = torch.zeros(self.n_pad, self.k, dtype=e.cdtype, device=e.dev)
            self.bias_pad = torch.full((self.n_pad,), -1e30, dtype=torch.float32, device=e.dev)
            self.seg_ws = torch.zeros((self.n_pad // 64) * self.rows * 4, dtype=torch.float32, device=e.dev)
        self.w_pad[:self.n].copy_(self.weight())
        self.bias_pad[:self.n].copy_((self.bias() if bias is None else bias)[:self.n])

    def prepare_temperature(self, temperature):
        """after prepare(), once per loop: the padded bias divided by T; banned and pad columns keep -1e30, NOT divided.
        where(bias > -1e29, bias * (1 / T), bias) for both heads: for a finite bias and T in [TEMPERATURE_MIN, TEMPERATURE_MAX]
        this is the fp32 product bias * (1 / T) on the real columns and -1e30 on the rest, bit for bit what multiplying the
        slice [:n] in place gives."""
        if self.bias_pad_T is None:
            self.bias_pad_T = torch.empty_like(self.bias_pad)
        self.bias_pad_T.copy_(torch.where(self.bias_pad > -1e29, self.bias_pad * (1.0 / temperature), self.bias_pad))

    def begin_loop(self, M, temperature, trunc):
        """what a sampler loop decides and stages once, before its steps: returns `fused`"""
        fused = trunc is None and self.available(M)
        if fused:
            self.prepare()
            if temperature is not None:
                self.prepare_temperature(temperature)
        return fused

    def run(self, x, M, fused, temperature=None, launch_seed=0, trunc=None):
        """x [M, k] -> out[:M]: greedy (softmax-max / argmax), a draw from softmax(logits / temperature), or a truncated draw
        (always through the logits).  fused: begin_loop's answer."""
        ops, n, k = self.e.ops, self.n, self.k
        if fused and trunc is None:
            nq = self.n_pad
            prob, idx, lse = self.out
            if temperature is None:
                ops.gemm(x, self.w_pad, None, self.bias_pad, None, self.seg_ws, M, nq, k, k, k, nq, epilogue=EPI_ROWMAX)
                ops.rowmax_combine(self.seg_ws, nq // 64, M, prob, idx, lse)
            else:
                ops.gemm(x, self.w_pad, None, self.bias_pad_T, None, self.seg_ws, M, nq, k, k, k, nq, epilogue=EPI_ROWSAMPLE,
                         alpha=1.0 / temperature, seed=launch_seed)
                ops.rowsample_combine(self.seg_ws, nq // 64, M, launch_seed, prob, idx, lse)
            return
        ops.gemm(x, self.weight(), self.logits, self.bias(), None, None, M, n, k, k, k, self.ldl, out_f32=True)
        self.from_logits(M, temperature, launch_seed, trunc)

    def from_logits(self, M, temperature=None, launch_seed=0, trunc=None):
        """the logits exits of run(): self.logits[:M] hold x W^T + bias"""
        ops, n = self.e.ops, self.n
        prob, idx, lse = self.out
        if trunc is not None:
            if self.row_kept is None:
                self.row_kept = torch.zeros(self.rows, dtype=torch.int32, device=self.e.dev)
            top_k, top_p, log_min_p = trunc
            ops.sample_rows_trunc(self.logits, M, n, self.ldl, 1.0 / (1.0 if temperature is None else temperature), launch_seed,
                                  top_k, top_p, log_min_p, prob, idx, lse, self.row_kept)
        elif temperature is not None:
            ops.sample_rows(self.logits, M, n, self.ldl, 1.0 / temperature, launch_seed, prob, idx, lse)
        else:
            ops.ce_fwd_bwd(self.logits, None, None, None, None, lse, idx, prob, M, n, self.ldl, self.ldd, 1.0)

    def score(self, x, M, labels, pred, totals, bias=None, logits=None):
        """validation: totals += {sum nll, labelled rows, rows predicted right}, pred[:M] = the argmax.  bias / logits: the
        MLM head's un-banned bias and its training logits buffer (default: the predictor's own).  The fused path leaves `bias`
        in the padded copy; every sampler loop's prepare() writes its own back."""
        ops, n, k = self.e.ops, self.n, self.k
        if self.available(M, "rowscore_combine"):
            self.prepare(bias)
            nq = self.n_pad
            ops.gemm(x, self.w_pad, None, self.bias_pad, labels, self.seg_ws, M, nq, k, k, k, nq, epilogue=EPI_ROWSCORE)
            ops.rowscore_combine(self.seg_ws, nq // 64, M, labels, n, None, pred, None, totals)
        else:
            logits = self.logits if logits is None else logits
            ops.gemm(x, self.weight(), logits, self.bias() if bias is None else bias, None, None, M, n, k, k, k, self.ldl, out_f32=True)
            ops.score_rows(logits, M, n, self.ldl, labels, None, pred, None, totals)


class SamplerMixin:
    """The on-device sampler loops of Engine: Mask-Predict and autoregressive image codes, in-painting, Mask-Predict captions.
    State (cid, vmask, feats, row_maxprob / row_argmax / row_lse, ...) and the forward are the engine's."""
    TEMPERATURE_MIN, TEMPERATURE_MAX, TRUNC_MAX_CAND = TEMPERATURE_MIN, TEMPERATURE_MAX, TRUNC_MAX_CAND
    GRID_MODES, CAPTION_MAX_L = GRID_MODES, CAPTION_MAX_L
    check_temperature, check_truncation = staticmethod(check_temperature), staticmethod(check_truncation)
    sample_launch_seed = staticmethod(sample_launch_seed)
    reuse_vis_stack = True          # False: every step recomputes the visual stack (A/B of the saving, tools/task_bench.py)

    @property
    def row_kept(self):
        """kept-set sizes of the last truncated image step (None before the first)"""
        return self.code_pred.row_kept

    def fused_predict_available(self):
        return self.code_pred.available(self.MV)

    def predict_codes(self):
        """head -> softmax -> max over the codebook (ref tasks/imggen_model.py:229-235): (max prob, argmax) per row."""
        self.code_pred.from_logits(self.MV)
        return self.row_maxprob, self.row_argmax

    def _predict_step(self, fused, temperature=None, seed=0, trunc=None):
        self.head_forward(want_logits=False)
        self.code_pred.run(self.feat, self.MV, fused, temperature, seed, trunc)

    def _forward_reusing(self, flag, reuse):
        """encoder forward of a loop step; `reuse`: the stack named by `flag` (_reuse_lang_stack / _reuse_vis_stack) saw the same
        input in step 0 and is skipped"""
        setattr(self, flag, reuse)
        try:
            self.encoder_forward(want_pooled=False)
        finally:
            setattr(self, flag, False)

    def sample_codes_nar(self, n_steps=4, on_step=None, *, temperature=None, seed=0, top_k=None, top_p=None, min_p=None):
        """Iterative Mask-Predict sampling (ref tasks/imggen_model.py:169-243) without a host round trip between steps:
        re-mask the lowest-confidence positions -> encoder -> codebook head -> softmax-max / argmax -> keep the predictions
        of the masked positions.  Text inputs come from set_inputs (cluster_ids / vis_mask there are placeholders).
        Returns (code_ids [B,V] int64, code features [B*V, F] in the compute dtype, pred_prob [B*V] fp32); the caller
        hands `code.view(B,V,F).permute(0,2,1).view(B,F,g,g)` to the frozen GAN generator (stock PyTorch, ref :254).
        on_step(i): called after step i's update (return_intermediate of the reference, :245-248: materialise_codes() gives the
        code tensor of that moment).
        temperature (None = greedy, exactly the calls above): every position draws its code from softmax(logits / temperature),
        reproducibly for one `seed`; the confidence of the re-masking is the tempered probability of the drawn code.
        top_k / top_p / min_p (any given: truncated sampling, temperature None meaning 1): the draw is restricted to the kept set
        of check_truncation's comment; self.row_kept holds its sizes."""
        temperature, trunc = check_temperature(temperature), check_truncation(top_k, top_p, min_p)
        ops, B, V = self.ops, self.B, self.V
        st = self.store
        self.use_codebook, self.has_vmask = True, True
        self.cid.zero_()
        fused = self.code_pred.begin_loop(self.MV, temperature, trunc)
        for i in range(n_steps):
            n_mask = int((n_steps - i) / n_steps * V)                      # ref :201-202 (host arithmetic on the step index)
            if i == 0:
                self.vmask.fill_(1)                                        # ref :204-206
            else:
                ops.remask_lowest(self.row_maxprob, self.vmask, B, V, n_mask)
            self._forward_reusing("_reuse_lang_stack", i > 0)              # the text is the same in every refinement step;
            #                                                                codebook_gather == where(mask, mask_feat, vis_emb(ids))
            self._predict_step(fused, temperature, sample_launch_seed(seed, i), trunc)
            ops.sampler_update(self.row_argmax, self.vmask, self.cid, B * V)
            if on_step is not None:
                on_step(i)
        ops.codebook_gather(self.cid, None, st.centroids_c, st.view("mask_feat"), self.feats, self.MV, self.F)
        return self.cid, self.feats, self.row_maxprob

    def materialise_codes(self, masked=False):
        """the sampler's code tensor [B*V, F] (compute dtype) of this moment: centroid rows of the current code ids; masked=True
        (autoregressive loop): `mask_feat` rows where vis_mask is still set, as the reference's `code` holds them (ref :99-102)."""
        st = self.store
        self.ops.codebook_gather(self.cid, self.vmask if masked else None, st.centroids_c, st.view("mask_feat"), self.feats,
                                 self.MV, self.F)
        return self.feats

    def sample_codes_ar(self, n_steps=None, mode="confidence", positions=None, trace=None, on_step=None, *, temperature=None, seed=0,
                        top_k=None, top_p=None, min_p=None):
        """Autoregressive sampling (ref tasks/imggen_model.py:49-153): one grid position per image is filled per step --
        the most confident not-yet-visited one ("confidence", the reference's default), position i ("tlbr"), or the host's
        shuffled order popped from the end ("random", positions = that list).  Same device-resident state as
        sample_codes_nar; `trace` (a list) receives a copy of vis_mask after every step.  temperature / seed: as in sample_codes_nar
        (the `confidence` policy ranks positions by the tempered probability of their drawn code); top_k / top_p / min_p likewise."""
        temperature, trunc = check_temperature(temperature), check_truncation(top_k, top_p, min_p)
        ops, B, V = self.ops, self.B, self.V
        st = self.store
        n_steps = V if n_steps is None else n_steps
        self.use_codebook, self.has_vmask = True, True
        self.cid.zero_()
        self.vmask.fill_(1)
        if not hasattr(self, "visited"):
            self.visited = torch.zeros(B, V, dtype=torch.uint8, device=self.dev)
        self.visited.zero_()
        positions = list(positions) if positions is not None else None
        fused = self.code_pred.begin_loop(self.MV, temperature, trunc)
        for i in range(n_steps):
            cur = -1
            if mode == "random":
                cur = positions.pop() % V
                self.vmask[:, cur] = 1                                     # ref :104-108 (re-visits beyond V steps)
            elif mode == "tlbr":
                cur = i
            self._forward_reusing("_reuse_lang_stack", i > 0)
            self._predict_step(fused, temperature, sample_launch_seed(seed, i), trunc)
            ops.sampler_ar_update(self.row_maxprob, self.row_argmax, self.visited, self.vmask, self.cid, B, V, cur)
            if trace is not None:
                trace.append(self.vmask.clone())
            if on_step is not None:
                on_step(i)
        ops.codebook_gather(self.cid, self.vmask, st.centroids_c, st.view("mask_feat"), self.feats, self.MV, self.F)
        return self.cid, self.feats, self.row_maxprob

    # ------------------------------------------------------------ in-painting (the image loops with part of the grid given)
    def inpaint_codes(self, init_codes, free_mask, n_steps=4, mode="nar", order=None, on_step=None, *, temperature=None, seed=0,
                      top_k=None, top_p=None, min_p=None):
        """Sample the FREE cells of the grid around given codes (include/xlxmert_hip.h xl_grid_step states the rules; DESIGN.md "N2
        notes"), without a host round trip between steps.  set_inputs has staged the text as for sample_codes_nar.
        init_codes [B, V] int: the codes of the given cells (whatever the free cells hold is ignored); a host tensor / sequence is
        range-checked against [0, K) at the given cells, a device tensor is clamped into it.  free_mask [B, V]: non-zero = sampled;
        rows may have any number of free cells, none included (such a row comes back untouched, score 0).
        mode "nar": Mask-Predict over the free cells, n_steps refinement steps with the per-row integer schedule.  "confidence" /
        "tlbr" / "order": one free cell per image per step -- the most confident one, raster order, or ascending `order` [B, V] (int,
        e.g. a permutation per image); n_steps=None = the largest free count of the batch (one host read before the loop), fewer
        leave cells masked (mask_feat in the returned features, as in sample_codes_ar).
        temperature / seed / top_k / top_p / min_p: as in sample_codes_nar -- the same predict paths, launch seeds and noise rows
        b*V + v, so with every cell free the loop reproduces sample_codes_nar / sample_codes_ar bit for bit.
        Returns (code_ids [B, V] int64, code features [B*V, F], score [B] fp32: mean log-probability of the sampled cells, conf [B, V]
        fp32: the probability each sampled cell was last predicted / filled with); on_step(i) is called after step i's update."""
        temperature, trunc = check_temperature(temperature), check_truncation(top_k, top_p, min_p)
        ops, B, V = self.ops, self.B, self.V
        st = self.store
        if mode not in GRID_MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(GRID_MODES)}")
        gmode = GRID_MODES[mode]
        if V > 64:
            raise ValueError(f"inpaint_codes: {V} grid cells > 64 (xl_grid_step: one lane per cell)")
        host_codes = not (isinstance(init_codes, torch.Tensor) and init_codes.device.type != "cpu")
        init_codes, free_mask = torch.as_tensor(init_codes), torch.as_tensor(free_mask)
        if tuple(init_codes.shape) != (B, V) or init_codes.is_floating_point() or init_codes.dtype == torch.bool:
            raise ValueError(f"init_codes: int codes of shape [B = {B}, V = {V}] (got {init_codes.dtype} {tuple(init_codes.shape)})")
        if tuple(free_mask.shape) != (B, V):
            raise ValueError(f"free_mask: shape [B = {B}, V = {V}] (got {tuple(free_mask.shape)})")
        if (order is not None) != (mode == "order"):
            raise ValueError(f"order: needed by mode 'order' and by no other (mode {mode!r})")
        if order is not None:
            order = torch.as_tensor(order)
            if tuple(order.shape) != (B, V) or order.is_floating_point() or order.dtype == torch.bool:
                raise ValueError(f"order: ints of shape [B = {B}, V = {V}] (got {order.dtype} {tuple(order.shape)})")
        free = free_mask != 0
        if host_codes and bool((~free.cpu() & ((init_codes < 0) | (init_codes >= self.K))).any()):
            raise ValueError(f"init_codes: a given cell holds a code outside [0, {self.K})")
        if n_steps is None:
            n_steps = int(free.sum(1).max())                               # the one host read, before the loop
        T = int(n_steps)
        if T < (1 if gmode == 0 else 0):
            raise ValueError(f"n_steps {n_steps!r}: at least 1")
        if getattr(self, "grid_free", None) is None:
            self.grid_free = torch.zeros(B, V, dtype=torch.uint8, device=self.dev)
            self.grid_conf, self.grid_score = self.f32(B, V), self.f32(B)
            self.grid_order = torch.zeros(B, V, dtype=torch.int32, device=self.dev)
        self.use_codebook, self.has_vmask = True, True
        self.grid_free.copy_(free)
        self.cid.copy_(init_codes)
        self.cid.clamp_(0, self.K - 1).masked_fill_(self.grid_free != 0, 0)   # free cells start from code 0, as sample_codes_nar's do
        self.vmask.copy_(self.grid_free)                                    # step 0: every free cell masked
        self.grid_conf.zero_()
        self.grid_score.zero_()
        if order is not None:
            self.grid_order.copy_(order)
        fused = self.code_pred.begin_loop(self.MV, temperature, trunc)
        for i in range(T):
            self._forward_reusing("_reuse_lang_stack", i > 0)              # the text is the same in every step
            self._predict_step(fused, temperature, sample_launch_seed(seed, i), trunc)
            ops.grid_step(self.row_maxprob, self.row_argmax, self.grid_free, self.grid_order if order is not None else None, self.cid,
                          self.vmask, self.grid_conf, self.grid_score, B, V, gmode, i, T)
            if on_step is not None:
                on_step(i)
        ops.codebook_gather(self.cid, None if gmode == 0 else self.vmask, st.centroids_c, st.view("mask_feat"), self.feats, self.MV,
                            self.F)
        return self.cid, self.feats, self.grid_score, self.grid_conf

    # ------------------------------------------------------------ caption sampler (Mask-Predict over the MLM head)
    def sample_words_nar(self, lengths, n_steps=10, prefix_len=0, on_step=None, *, temperature=None, seed=0, top_k=None, top_p=None,
                         min_p=None, suppress_repeats=False, mask_token_id=103, banned_ids=None):
        """Mask-Predict caption decoding, the word-side twin of sample_codes_nar (include/xlxmert_hip.h xl_caption_step states the
        rules; DESIGN.md "N2 notes"), without a host round trip between steps.  set_inputs has staged the visual side (real grid
        features or un-masked cluster ids) and the token layout: row b = [CLS], prefix_len prefix ids, lengths[b] free positions
        (whatever they hold: the loop feeds mask_token_id there), [SEP], [PAD]; attention_mask = l < prefix_len + lengths[b] + 2.
        lengths: an int, or ints [B] (a host sequence / CPU tensor is range-checked here: 1 <= n <= L - 2 - prefix_len; a device
        tensor cannot be without a round trip and is clamped by the kernel).  banned_ids: token ids that are never predicted
        (default: every id below 999, the specials of bert-base-uncased).  temperature / seed / top_k / top_p / min_p: as in
        sample_codes_nar; the noise row of position (b, l) is its row in the head's input matrix, b*L + l dense and loff[b] + l packed,
        so one seed reproduces a run bit for bit for one batch and packing.  Steps after the first reuse the visual stack.
        Returns (tokens [B, L] int64, score [B] fp32: mean log-probability of the free tokens under the last forward, conf [B, L] fp32:
        the last forward's confidences); on_step(i) is called after step i's update."""
        temperature, trunc = check_temperature(temperature), check_truncation(top_k, top_p, min_p)
        ops, B, L = self.ops, self.B, self.L
        lh = self.lang_heads
        if lh is None or not lh.has_mlm or not self.need_lang:
            raise RuntimeError("sample_words_nar needs the MLM head: a store with task 'word_mask' or 'all' (cls.predictions.*) and an "
                               "engine built with need_lang=True")
        if self.embeds_mode:
            raise ValueError("sample_words_nar feeds token ids: set_inputs(input_ids=...), not inputs_embeds")
        P, T = int(prefix_len), int(n_steps)
        if L > CAPTION_MAX_L:
            raise ValueError(f"caption sampler: text length {L} > {CAPTION_MAX_L}")
        if P < 0 or L - 2 - P < 1:
            raise ValueError(f"prefix_len {prefix_len!r}: need 0 <= prefix_len <= L - 3 = {L - 3}")
        if T < 1:
            raise ValueError(f"n_steps {n_steps!r}: at least 1")
        if not (isinstance(lengths, torch.Tensor) and lengths.device.type != "cpu"):
            lens = torch.as_tensor(lengths).reshape(-1)
            if lens.is_floating_point() or lens.dtype == torch.bool:
                raise ValueError(f"lengths {lengths!r}: an int or ints [B]")
            lens = lens.to(torch.int64)
            if lens.numel() == 1:
                lens = lens.expand(B)
            if lens.numel() != B or int(lens.min()) < 1 or int(lens.max()) > L - 2 - P:
                raise ValueError(f"lengths {lengths!r}: an int or ints [B = {B}] with 1 <= n <= L - 2 - prefix_len = {L - 2 - P}")
        else:
            lens = lengths.reshape(-1)
            if lens.numel() != B:
                raise ValueError(f"lengths: {lens.numel()} entries for a batch of {B}")
        if getattr(self, "cap_len", None) is None:
            self.cap_len = torch.zeros(B, dtype=torch.int32, device=self.dev)
            self.cap_tokens = torch.zeros(B, L, dtype=torch.int64, device=self.dev)
            self.word_mask = torch.zeros(B, L, dtype=torch.uint8, device=self.dev)
            self.cap_conf, self.cap_score = self.f32(B, L), self.f32(B)
            self._cap_pos = torch.arange(L, dtype=torch.int32, device=self.dev).view(1, L)
        self.cap_len.copy_(lens, non_blocking=True)
        if banned_ids is None:
            banned_ids = torch.arange(min(999, self.cfg.vocab_size - 1))
        lh._prepare_predict(banned_ids)
        packed = self.packed
        # step 0's state, by the host (sample_codes_nar: vmask.fill_(1)): every free position masked, tokens = the layout with [MASK] there
        free = (self._cap_pos > P) & (self._cap_pos < P + 1 + self.cap_len.view(B, 1))
        self.word_mask.copy_(free)
        self.ids.masked_fill_(free, int(mask_token_id))
        self.cap_tokens.copy_(self.ids)
        self.cap_conf.zero_()
        self._packed_head = packed
        try:
            fused = lh.word_pred.begin_loop(self.ML, temperature, trunc)
            for i in range(T):
                self._forward_reusing("_reuse_vis_stack", i > 0 and self.reuse_vis_stack)   # the picture is the same in every step
                lh.predict(self.lang_final, self.ML, fused, temperature, sample_launch_seed(seed, i), trunc)
                ops.caption_step(lh.row_prob, lh.row_id, self.loff if packed else None, self.cap_len, self.cap_tokens, self.ids,
                                 self.word_mask, self.cap_conf, self.cap_score, B, L, P, i, T, int(mask_token_id), suppress_repeats)
                if on_step is not None:
                    on_step(i)
        finally:
            self._packed_head = False
        return self.cap_tokens, self.cap_score, self.cap_conf
