"""The prediction heads on top of the encoder, forward and hand-derived backward: the codebook head of the masked-visual-token task
(ref lxrt/modeling.py:38-53, 237-290), the answer head (HF:602-614) and the language pretraining heads (HF:589-657).

What they share is said once here: HeadTransform -- Linear -> GELU -> LayerNorm, the first stage of all three -- and RowSubset --
a head that runs on a row list only.  The tails that turn logits into ids and scores are sampling.RowPredictor."""
import torch

from .blocks import _h
from .ops import EPI_GELU, EPI_RESIDUAL
from .sampling import RowPredictor


class HeadTransform:
    """Linear(K, N) -> GELU -> LayerNorm(N), parameters `dense` / `ln` of the store, on up to `rows` rows: the parameters, their
    gradients and what the forward saves for the backward (x; bufs = pre-activation, GELU output, LayerNorm output, mean, rstd)."""

    def __init__(self, eng, dense, ln, N, K, eps, rows):
        st = eng.store
        self.e, self.N, self.K, self.eps, self.x = eng, N, K, eps, None
        self.w, self.gw, self.b, self.gb = st.cview(dense + ".weight"), st.gview(dense + ".weight"), st.view(dense + ".bias"), st.gview(dense + ".bias")
        self.g, self.gg, self.beta, self.gbeta = st.view(ln + ".weight"), st.gview(ln + ".weight"), st.view(ln + ".bias"), st.gview(ln + ".bias")
        self.bufs = (eng.act(rows, N), eng.act(rows, N), eng.act(rows, N), eng.f32(rows), eng.f32(rows))

    def fwd(self, x, M, bufs=None):
        """x [M, K] -> LayerNorm output.  bufs: a forward-only caller's own buffers (the predict path, validation on row slices);
        a forward into the transform's own buffers is the one a backward may follow, and keeps x for the weight gradient"""
        ops, N, K = self.e.ops, self.N, self.K
        if bufs is None:
            bufs, self.x = self.bufs, x
        pre, h, hn, mean, rstd = bufs
        ops.gemm(x, self.w, h, self.b, None, pre, M, N, K, K, K, N, ldx=N, epilogue=EPI_GELU)
        ops.layernorm_fwd(h, self.g, self.beta, hn, mean, rstd, M, N, self.eps)
        return hn

    def bwd(self, dhn, M, dh, dpre, dx, Mk=None, flush=True, **kw):
        """dhn = d(LayerNorm output) [M, N]; dh / dpre: the caller's scratch.  Accumulates the parameter gradients (flush: launch the
        engine's weight-gradient group now) and writes d(x) into dx -- a buffer, or a callable that names it once the flush has advanced
        the scratch generation.  Mk > M: the weight gradient contracts over Mk rows, gradient rows [M, Mk) zeroed.  kw: of the d(x) GEMM"""
        e, N, K = self.e, self.N, self.K
        ops = e.ops
        pre, h, _, mean, rstd = self.bufs
        ops.layernorm_bwd(dhn, h, self.g, mean, rstd, dh, self.gg, self.gbeta, None, M, N, ws=e.ws)
        ops.gelu_bwd(dh, pre, dpre, M * N)
        ops.colsum(dpre, self.gb, M, N, N, ws=e.ws)
        if Mk is not None and Mk > M:
            ops.zero(dpre[M:Mk])
        e.wgrad_defer(dpre, self.x, self.gw, N, K, M if Mk is None else Mk, N, K, K)
        if flush:
            e.wgrad_flush()
        if callable(dx):
            dx = dx()
        ops.gemm(dpre, self.w, dx, None, None, None, M, K, N, N, K, K, a_kmajor=1, b_kmajor=0, **kw)
        return dx


class RowSubset:
    """The row list of a head that runs on some rows only (exact where the loss reads nothing else): int32 row ids padded with -1
    to the row tile (Engine.pad_rows), the padded count `n` (0: no list) and the labels of those rows, compact."""

    def __init__(self, eng, cap):
        self.e, self.cap, self.n = eng, cap, 0
        self.idx = torch.zeros(cap, dtype=torch.int32, device=eng.dev)
        self.labels_c = torch.zeros(cap, dtype=torch.int64, device=eng.dev)

    def set(self, idx):
        self.n = self.e.pad_rows(self.idx, idx, int(idx.numel()), self.cap)

    def gather(self, src, dst, N):
        self.e.ops.gather_rows(src, self.idx, dst, self.n, N, N, N)

    def gather_labels(self, labels):
        out = self.labels_c[:self.n]
        self.e.ops.gather_labels(labels, self.idx, out, self.n)
        return out

    def scatter(self, src, dst, N):
        self.e.ops.scatter_rows(src, self.idx, dst, self.n, N, N, N)


# ---------------------------------------------------------------- codebook head (LxmertVisualObjHead; buffers: Engine attributes)
# The head runs either on all B*V visual rows (inference, sampler, the nn.Module API) or, inside the training step and the validation
# pass, on the masked rows only: both losses read nothing else (ref lxrt/modeling.py:253-256: labels -100 elsewhere; :273-287: the
# SmoothL1 term is multiplied by vis_mask).  `rows` = None (all rows) or the RowSubset of the masked rows.
def codebook_forward(eng, rows=None, want_logits=True, scratch=None):
    """LxmertVisualObjHead.forward (ref lxrt/modeling.py:38-53): returns (feat, logits).  The rows of a list are handed over compact
    by the last visual feed-forward block (encoder_forward ffn_rows) or gathered into scratch(name, M, N) (default: Engine.tmp)."""
    ops, d, F, K, hd = eng.ops, eng.d, eng.F, eng.K, eng.hd
    ops.block = "head"
    M, x = eng.MV, eng.vis_final
    if rows is not None and eng._ffn_rows_run is not None:
        assert eng._ffn_rows_run[1] == rows.n
        M, x = rows.n, _h(eng._vis_c)
    elif rows is not None:          # x: the whole buffer (the backward's weight gradient contracts over a rounded-up row count), kept by
        M, x = rows.n, (scratch or eng.tmp)("vis_c", eng.MV, d)     # the transform: tmp() in the backward may hand out another scratch set
        rows.gather(eng.vis_final, x[:M], d)
    t_y = eng.head_tr.fwd(x, M)
    ops.gemm(t_y, hd["wf"][0], eng.feat, hd["bf"][0], None, None, M, F, d, d, d, F)
    if want_logits:
        ops.gemm(eng.feat, eng.store.centroids_c, eng.logits, hd["bc"][0], None, None, M, K, F, F, F, K, out_f32=True)
    return eng.feat, eng.logits


def codebook_losses(eng, rows=None, want_grad=True, feat_loss=True):
    """ref lxrt/modeling.py:237-290.  Leaves d(logits) / d(feat) for codebook_backward; returns [obj_loss, feat_loss] (device)."""
    ops, F, K = eng.ops, eng.F, eng.K
    M = eng.MV if rows is None else rows.n
    ops.zero(eng.losses)
    ops.mask_counts(eng.labels, eng.vmask, eng.counts, eng.nmask, eng.B, eng.V)
    labels = eng.labels if rows is None else rows.gather_labels(eng.labels)
    ops.ce_fwd_bwd(eng.logits, labels, eng.counts, eng.dlogits if want_grad else None, eng.losses[0:],
                   None, None, None, M, K, K, eng.Kp, 1.0)
    eng.with_feat_loss = feat_loss
    if feat_loss:
        ops.featloss_fwd_bwd(eng.feat, eng.store.centroids_c, eng.cid, eng.vmask, eng.nmask, eng.dfeat if want_grad else None,
                             eng.losses[1:], eng.B, eng.V, F, 1.0, rows=rows.idx if rows is not None else None,
                             n_rows=M if rows is not None else 0, targets=eng.feat_tgt)
    return eng.losses


def codebook_backward(eng, d_vis, rows=None, report=True):
    """consumes dlogits / dfeat; writes d(vision_output) into d_vis.  report=False: the QA branch's backward still follows."""
    ops, d, MV, F, K, hd = eng.ops, eng.d, eng.MV, eng.F, eng.K, eng.hd
    ops.block = "head"
    M = MV if rows is None else rows.n
    ops.colsum(eng.dlogits, hd["bc"][1], M, eng.Kp, eng.Kp, ws=eng.ws_wide("codebook", eng.Kp))      # pad columns are zero; the bias unit is padded
    dfeat = eng.tmp("dfeat", MV, F)
    if eng.with_feat_loss:
        ops.gemm(eng.dlogits, eng.store.centroids_c, dfeat, None, eng.dfeat, None, M, F, K, eng.Kp, F, F, ldr=F,
                 a_kmajor=1, b_kmajor=0, epilogue=EPI_RESIDUAL)
    else:
        ops.gemm(eng.dlogits, eng.store.centroids_c, dfeat, None, None, None, M, F, K, eng.Kp, F, F, a_kmajor=1, b_kmajor=0)
    ops.colsum(dfeat, hd["bf"][1], M, F, F, ws=eng.ws)
    # weight gradients contract over the rows: round a compacted row count up to the K tile with zero gradient rows
    Mk = min(MV, (M + 63) // 64 * 64)
    if Mk > M:
        ops.zero(dfeat[M:Mk])
    eng.wgrad_defer(dfeat, eng.t_y, hd["wf"][1], F, d, Mk, F, d, d)
    dty = eng.tmp("dz", MV, d)
    ops.gemm(dfeat, hd["wf"][0], dty, None, None, None, M, d, F, F, d, d, a_kmajor=1, b_kmajor=0)
    # into d_vis, or -- a row list -- into scratch (fp32 stream: the head's gradient enters it in fp32)
    dvc = eng.head_tr.bwd(dty, M, eng.tmp("dctx", MV, d), eng.tmp("dzm", MV, d),
                          d_vis if rows is None else (lambda: eng.tmp("dvis_c", MV, d, res=True)), Mk=Mk, **eng.rkw)
    if rows is not None:        # gradient of the masked rows, scattered into an otherwise zero d(vision_output)
        if eng._ffn_rows_run is not None:           # ... or handed over compact: the last visual feed-forward block's
            eng._dvis_c = dvc[:M]                   # backward runs on these rows too (_encoder_backward); d_vis is not written
        else:
            ops.zero(d_vis)
            rows.scatter(dvc, d_vis, d)
    if report:
        eng._ready_heads()


class AnswerHead:
    """LxmertVisualAnswerHead on pooled_output (HF:602-614: Linear(d,2d) -> GeLU -> LayerNorm(2d) -> Linear(2d,A)) with
    BCEWithLogitsLoss on soft targets -- the VQA/GQA fine-tune step (ref tasks/vqa_model.py:22-72, vqa.py:166-187)."""

    def __init__(self, eng, num_answers, pair=False):
        self.e, self.A, self.pair = eng, num_answers, pair
        st, d = eng.store, eng.d
        # pair head (NLVR2, ref tasks/nlvr2_model.py:80-86): pooled_output [2P, d] of the flattened (statement, image) rows is
        # read as [P, 2d] -- a view of the same contiguous buffer -- by a head whose first Linear is (2d, 2d)
        assert not pair or eng.B % 2 == 0, "the pair head needs an even number of encoder rows (two images per statement)"
        B = self.Bh = eng.B // 2 if pair else eng.B
        self.din = 2 * d if pair else d
        p = "answer_head.logit_fc"
        self.w3, self.gw3 = st.cview(p + ".3.weight"), st.gview(p + ".3.weight")
        self.b3, self.gb3 = st.view(p + ".3.bias"), st.gview(p + ".3.bias")
        self.Ap = (num_answers + 7) // 8 * 8
        self.tr = HeadTransform(eng, p + ".0", p + ".2", 2 * d, self.din, 1e-12, B)
        self.logit = torch.zeros(B, num_answers, dtype=torch.float32, device=eng.dev)
        self.targets = torch.zeros(B, num_answers, dtype=torch.float32, device=eng.dev)
        self.dlogit = eng.act(B, self.Ap)
        self.dhn, self.dh, self.dpre = eng.act(B, 2 * d), eng.act(B, 2 * d), eng.act(B, 2 * d)
        self.dpooled, self.dz = eng.act(eng.B, d), eng.act(eng.B, d)
        self.loss = eng.f32(1)
        # pretraining QA branch (ref lxrt/modeling.py:292-304): CrossEntropyLoss over one answer id per example (-100 = none)
        self.labels = torch.full((B,), -100, dtype=torch.int64, device=eng.dev)
        self.counts, self._ones, self._nm = eng.f32(4), torch.ones(B, dtype=torch.uint8, device=eng.dev), eng.f32(B)
        self.row_argmax = torch.zeros(B, dtype=torch.int32, device=eng.dev)
        self.row_lse, self.row_maxprob = eng.f32(B), eng.f32(B)

    def fwd(self, pooled):
        e, d, B, A = self.e, self.e.d, self.Bh, self.A
        hn = self.tr.fwd(pooled.view(B, self.din), B)
        e.ops.gemm(hn, self.w3, self.logit, self.b3, None, None, B, A, 2 * d, 2 * d, 2 * d, A, out_f32=True)
        return self.logit

    def loss_fwd_bwd(self, want_grad=True):
        B, A = self.Bh, self.A
        self.e.ops.zero(self.loss)
        self.e.ops.bce_logits_fwd_bwd(self.logit, self.targets, self.dlogit if want_grad else None, self.loss, B, A, A, A, self.Ap)
        return self.loss

    def ce_loss_fwd_bwd(self, want_grad=True):
        """qa_loss = CrossEntropyLoss()(answer_score, qa_labels) (ref lxrt/modeling.py:295-298; ignore_index -100) and its
        d(logit); also records qa_pred = argmax (ref :300)."""
        B, A = self.Bh, self.A
        ops = self.e.ops
        ops.zero(self.loss)
        ops.mask_counts(self.labels, self._ones, self.counts, self._nm, B, 1)          # counts[0] = #labels != -100
        if want_grad and self.Ap > A:
            ops.zero(self.dlogit)                                                      # pad columns
        ops.ce_fwd_bwd(self.logit, self.labels, self.counts, self.dlogit if want_grad else None, self.loss, self.row_lse,
                       self.row_argmax, self.row_maxprob, B, A, A, self.Ap, 1.0)
        return self.loss

    def bwd(self, cls_rows, d_cls, accumulate=False):
        """consumes dlogit; accumulates the head's and the pooler's parameter gradients; writes (or, accumulate=True, adds)
        d(lang_output[:, 0]) into d_cls (a [B, d] view with row stride L*d)."""
        self.bwd_to_pooled()
        self.e.pooler_backward(self.dpooled, self.dz, cls_rows, d_cls, accumulate=accumulate)

    def bwd_to_pooled(self):
        """consumes dlogit; accumulates the head's parameter gradients; leaves d(pooled_output) in self.dpooled."""
        e, d, B, A, Ap = self.e, self.e.d, self.Bh, self.A, self.Ap
        ops = e.ops
        ops.colsum(self.dlogit, self.gb3_pad(), B, Ap, Ap, ws=e.ws_wide("answer", Ap))      # pad columns of dlogit are zero
        e.wgrad_defer(self.dlogit, self.tr.bufs[2], self.gw3, A, 2 * d, B, Ap, 2 * d, 2 * d)
        ops.gemm(self.dlogit, self.w3, self.dhn, None, None, None, B, 2 * d, A, Ap, 2 * d, 2 * d, a_kmajor=1, b_kmajor=0)
        # (own scratch, no flush: the pooler's backward launches the group)
        self.tr.bwd(self.dhn, B, self.dh, self.dpre, self.dpooled.view(B, self.din), flush=False)

    def gb3_pad(self):
        """bias-gradient view padded to the 8-column granule of dlogit (the bias unit is padded in the flat buffer)."""
        m = self.e.store.index["answer_head.logit_fc.3.bias"]
        return self.e.store.grad[m.offset:m.offset + self.Ap]


class LangHeads:
    """LxmertPreTrainingHeads (HF:589-657) for the `word_mask` and `matched` pretraining branches (ref lxrt/modeling.py:
    211-235): MLM = decoder(LN(gelu(dense(lang)))) + bias with the decoder TIED to the word-embedding matrix, vocab-way CE
    over the masked tokens; matched = seq_relationship(pooled_output), 2-way CE."""

    def __init__(self, eng):
        self.e = eng
        st, d, ML, B = eng.store, eng.d, eng.MLd, eng.B
        self.has_mlm = "cls.predictions.bias" in st.index and eng.task in ("word_mask", "all")
        self.has_rel = "cls.seq_relationship.weight" in st.index and eng.task in ("matched", "all")
        self.loss = eng.f32(2)                  # [lm_loss, matched_loss]
        self.counts, self.dummy, self.rel_counts = eng.f32(4), eng.f32(B), eng.f32(4)
        if self.has_mlm:
            t = "cls.predictions.transform"
            self.vb = st.view("cls.predictions.bias")
            self.Vn = eng.cfg.vocab_size
            self.Vp = (self.Vn + 7) // 8 * 8
            self.tr = HeadTransform(eng, t + ".dense", t + ".LayerNorm", d, d, 1e-12, ML)
            self.pre, self.h, self.hn, self.mean, self.rstd = self.tr.bufs
            self.scores = torch.zeros(ML, self.Vp, dtype=torch.float32, device=eng.dev)       # row stride padded to 8
            self.dscores = eng.act(ML, self.Vp)
            self.word_labels = torch.full((B, eng.L), -100, dtype=torch.int64, device=eng.dev)
            # masked-row mode (row list from the data loader): decoder, loss and backward on the labelled rows only (exact)
            self.sub = RowSubset(eng, ML)
            self.rows = self.sub.idx
            # the tied decoder's tail for the caption sampler and the validation pass (the padded word-embedding operand is one)
            self.word_pred = RowPredictor(eng, self.Vn, d, eng.MLc, lambda: st.cview("bert.embeddings.word_embeddings.weight"),
                                          lambda: self.vb_ban, self.Vp, self.Vp)
            self.p_hn = None                    # buffers of the predict paths: made by the first _prepare_predict
        if self.has_rel:
            self.wr, self.gwr = st.cview("cls.seq_relationship.weight"), st.gview("cls.seq_relationship.weight")
            self.br, self.gbr = st.view("cls.seq_relationship.bias"), st.gview("cls.seq_relationship.bias")
            self.rel = torch.zeros(B, 8, dtype=torch.float32, device=eng.dev)                # 2 columns used
            self.drel = eng.act(B, 8)
            self.matched_labels = torch.zeros(B, dtype=torch.int64, device=eng.dev)
            self.dpooled, self.dz = eng.act(B, d), eng.act(B, d)
            self._g8, self._gb8 = eng.f32(8, d), eng.f32(8)                # rel_bwd: the two output rows padded to 8
            self._w8 = torch.zeros(8, d, dtype=eng.cdtype, device=eng.dev)

    @property
    def n_rows(self):
        return self.sub.n

    def _gvb_pad(self):
        m = self.e.store.index["cls.predictions.bias"]
        return self.e.store.grad[m.offset:m.offset + self.Vp]

    # ---- word_mask
    def set_rows(self, word_rows):
        """word_rows: flat indices b*L+l of the labelled positions (host tensor / list: its length is the launch size), or None."""
        self.sub.n = 0
        if word_rows is not None and 0 < len(word_rows) < self.e.MLd:
            self.sub.set(torch.as_tensor(word_rows, dtype=torch.int64))

    def stage_labels(self, word_labels, word_rows):
        """the step's MLM labels (any negative = not masked: the reference writes -1, its loss ignores -100) and the labelled rows"""
        wl = word_labels.clone()
        wl[wl < 0] = -100
        self.word_labels.copy_(wl, non_blocking=True)
        self.set_rows(word_rows)

    def _rows_of(self, lang, scratch):
        """(row count, head input): all rows of `lang`, or the labelled rows gathered into scratch("mlm_x", M, N)"""
        e, n = self.e, self.n_rows
        if not n:
            return e.MLd, lang
        x = scratch("mlm_x", e.MLd, e.d)[:n]
        self.sub.gather(lang, x, e.d)
        return n, x

    def mlm_fwd(self, lang):
        e, d = self.e, self.e.d
        M, x = self._rows_of(lang, e.tmp)
        hn = self.tr.fwd(x, M)
        e.ops.gemm(hn, e.store.cview("bert.embeddings.word_embeddings.weight"), self.scores, self.vb, None, None,
                   M, self.Vn, d, d, d, self.Vp, out_f32=True)
        return self.scores

    def mlm_loss(self):
        """lm_loss (CE over the masked tokens, labels -100 ignored) and d(scores); nothing of the parameter gradients is touched"""
        e, Vn, Vp = self.e, self.Vn, self.Vp
        ops = e.ops
        M = self.n_rows or e.MLd
        ops.zero(self.loss[0:1])
        ops.mask_counts(self.word_labels, e.kmask, self.counts, self.dummy, e.B, e.L)
        labels = self.sub.gather_labels(self.word_labels) if self.n_rows else self.word_labels
        ops.ce_fwd_bwd(self.scores, labels, self.counts, self.dscores, self.loss[0:], None, None, None,
                       M, Vn, Vp, Vp, 1.0)
        return self.loss

    def mlm_bwd(self, d_lang):
        """backward down to d(language_output), written to d_lang (which the caller has zeroed)"""
        e, d, Vn, Vp = self.e, self.e.d, self.Vn, self.Vp
        ops, st = e.ops, e.store
        M = self.n_rows or e.MLd
        emb = "bert.embeddings.word_embeddings.weight"
        ops.colsum(self.dscores, self._gvb_pad(), M, Vp, Vp, ws=e.ws_wide("mlm", Vp))
        e.wgrad_defer(self.dscores, self.hn, st.gview(emb), Vn, d, M, Vp, d, d, once=False)  # tied decoder: d(word embeddings) also
                                                                                            # receives the embedding scatter-add
        dhn = e.tmp("dctx", e.MLd, d)
        ops.gemm(self.dscores, st.cview(emb), dhn, None, None, None, M, d, Vn, Vp, d, d, a_kmajor=1, b_kmajor=0)
        # into d_lang, or -- a row list -- into scratch (fp32 stream: the heads' gradients enter it in fp32) and scattered from there
        dx = self.tr.bwd(dhn, M, e.tmp("dz", e.MLd, d), e.tmp("dzm", e.MLd, d),
                         (lambda: e.tmp("mlm_dx", e.MLd, d, res=True)[:M]) if self.n_rows else d_lang, **e.rkw)
        if self.n_rows:
            self.sub.scatter(dx, d_lang, d)
        return self.loss

    # ---- prediction over the vocabulary (caption sampler, SamplerMixin.sample_words_nar): the word-side twin of the codebook head's
    # step.  The head runs on the rows of the last cross layer's language output AS THEY LIE -- packed rows lang_off[b] + l (rounded up
    # to the row tile with zero rows) or dense rows b*L + l -- and leaves per row the predicted / drawn token id, its probability and
    # the log-sum-exp.  Banned ids are -1e30 in the decoder bias, the mechanism of the codebook's pad columns (sampling.RowPredictor).
    def fused_predict_available(self):
        return self.word_pred.available(self.e.ML)

    def _prepare_predict(self, banned_ids):
        """buffers of the predict paths (row capacity MLc: a packed row count is rounded up to the row tile, which may exceed B*L)
        and the decoder bias with the banned ids at -1e30"""
        e, d = self.e, self.e.d
        Mc = e.MLc
        if self.p_hn is None:
            own = Mc > e.MLd
            self.p_pre, self.p_h, self.p_hn = (e.act(Mc, d) for _ in range(3)) if own else (self.pre, self.h, self.hn)
            self.p_mean, self.p_rstd = (e.f32(Mc), e.f32(Mc)) if own else (self.mean, self.rstd)
            self.p_scores = torch.zeros(Mc, self.Vp, dtype=torch.float32, device=e.dev) if own else self.scores
            self.row_prob, self.row_lse = e.f32(Mc), e.f32(Mc)
            self.row_id = torch.zeros(Mc, dtype=torch.int32, device=e.dev)
            self.vb_ban = torch.zeros(self.Vp, dtype=torch.float32, device=e.dev)
            self.word_pred.logits, self.word_pred.out = self.p_scores, (self.row_prob, self.row_id, self.row_lse)
        self.vb_ban[:self.Vn].copy_(self.vb)
        if self.Vp > self.Vn:
            self.vb_ban[self.Vn:].fill_(-1e30)
        ban = torch.as_tensor(banned_ids, dtype=torch.int64).reshape(-1)
        if ban.numel() and (int(ban.min()) < 0 or int(ban.max()) >= self.Vn):
            raise ValueError(f"banned_ids outside the vocabulary [0, {self.Vn})")
        if ban.numel() >= self.Vn or ban.unique().numel() >= self.Vn:
            raise ValueError("banned_ids leaves no token to predict")
        self.vb_ban[ban.to(e.dev)] = -1e30

    def predict(self, lang, M, fused, temperature=None, launch_seed=0, trunc=None):
        """lang: the head's input rows [M, d].  Fills row_id / row_prob / row_lse[:M]: greedy (softmax-max / argmax), a draw from
        softmax(logits / temperature), or a truncated draw (always through the logits, as on the image side)."""
        self.e.ops.block = "head"
        hn = self.tr.fwd(lang, M, (self.p_pre[:M], self.p_h[:M], self.p_hn[:M], self.p_mean, self.p_rstd))
        self.word_pred.run(hn, M, fused, temperature, launch_seed, trunc)

    # ---- validation (TaskMixin.evaluate_task): the head forward-only, loss and accuracy from xl_rowscore_combine / xl_score_rows
    def mlm_evaluate(self, lang, totals, row_pred):
        """MLM head on the labelled rows (set_rows) or on all rows: totals += {sum nll, labelled rows, rows predicted right}"""
        e = self.e
        e.ops.block = "head"
        M, x = self._rows_of(lang, e.eval_buf)              # (not the backward scratch of mlm_fwd)
        labels = self.sub.gather_labels(self.word_labels) if self.n_rows else self.word_labels
        hn = self.tr.fwd(x, M, (self.pre[:M], self.h[:M], self.hn[:M], self.mean, self.rstd))
        self.word_pred.score(hn, M, labels, row_pred, totals, bias=self.vb, logits=self.scores)    # (nothing is banned here)
        return M

    # ---- matched
    def rel_fwd(self, pooled):
        e, d, B = self.e, self.e.d, self.e.B
        e.ops.gemm(pooled, self.wr, self.rel, self.br, None, None, B, 2, d, d, d, 8, out_f32=True)
        return self.rel

    def rel_loss(self):
        e, B = self.e, self.e.B
        e.ops.zero(self.loss[1:2])
        self.rel_counts.fill_(float(B))                                 # every example carries a matched label
        e.ops.ce_fwd_bwd(self.rel, self.matched_labels, self.rel_counts, self.drel, self.loss[1:], None, None, None, B, 2, 8, 8, 1.0)
        return self.loss

    def rel_bwd(self, pooled, cls_rows, d_cls, extra_dpooled=None):
        e, d, B = self.e, self.e.d, self.e.B
        ops = e.ops
        # the two output rows of seq_relationship: tiny contractions, done on the 8-column padded gradient
        g8, gb8, w8 = self._g8, self._gb8, self._w8
        g8.zero_()
        ops.gemm(self.drel, pooled, g8, None, None, None, 8, d, B, 8, d, d, a_kmajor=0, b_kmajor=0, out_f32=True)
        self.gwr.add_(g8[:2])
        gb8.zero_()
        ops.colsum(self.drel, gb8, B, 8, 8, ws=e.ws)
        e.flush_reductions()                     # consumed right away
        self.gbr.add_(gb8[:2])
        w8[:2].copy_(self.wr)
        ops.gemm(self.drel, w8, self.dpooled, None, None, None, B, d, 8, 8, d, d, a_kmajor=1, b_kmajor=0)
        if extra_dpooled is not None:            # task_qa model: the answer head's d(pooled_output) joins here
            self.dpooled.add_(extra_dpooled)
        e.pooler_backward(self.dpooled, self.dz, cls_rows, d_cls)
        return self.loss
