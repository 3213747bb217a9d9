"""Task programs of the engine (TaskMixin, mixed into xlxmert_amd.engine.Engine): every branch of XLxmertForPretraining.forward
(ref lxrt/modeling.py:154-308) and the VQA / NLVR2 fine-tune steps as forward + backward over the encoder and the heads
(xlxmert_amd.heads), the forward-only validation pass, and the backward of the nn.Module surface from output gradients."""
import torch

from . import heads
from .ops import EPI_RESIDUAL


class TaskMixin:
    # ---- codebook head: heads.codebook_* on this engine's buffers (rows: the heads.RowSubset the head runs on; None = all rows)
    def head_forward(self, want_logits=True, rows=None):
        return heads.codebook_forward(self, rows, want_logits)

    def losses_forward_backward(self, want_grad=True, feat_loss=True, rows=None):
        return heads.codebook_losses(self, rows, want_grad, feat_loss)

    def head_backward(self, d_vis, report=True, rows=None):
        heads.codebook_backward(self, d_vis, rows, report)

    def _step_rows(self):
        """the masked rows as the row list of the codebook head and of the last visual feed-forward block, or None (all rows)"""
        use_rows = self.compact_head and self.has_vmask and 0 < self.n_mrows < self.MV
        return self.mask_rows if use_rows else None

    def pooler_backward(self, dpooled, dz, cls_rows, d_cls, accumulate=False):
        """LxmertPooler backward (HF:566-572): pooled = tanh(W_p cls + b_p).  cls_rows / d_cls are [B, d] views of the
        language output / its gradient with row stride L*d (the [CLS] rows); accumulate: d_cls += instead of =."""
        ops, st, d, B, L = self.ops, self.store, self.d, self.B, self.L
        ops.tanh_bwd(dpooled, self.pooled, dz, B * d)
        ops.colsum(dz, st.gview("bert.pooler.dense.bias"), B, d, d, ws=self.ws)
        self.wgrad_defer(dz, cls_rows, st.gview("bert.pooler.dense.weight"), d, d, B, d, L * d, d)
        self.wgrad_flush()
        if accumulate:              # in-place: every output element is read (residual) and written by the same lane
            ops.gemm(dz, st.cview("bert.pooler.dense.weight"), d_cls, None, d_cls, None, B, d, d, d, d, L * d, ldr=L * d,
                     a_kmajor=1, b_kmajor=0, epilogue=EPI_RESIDUAL, **self.rkw)
        else:
            ops.gemm(dz, st.cview("bert.pooler.dense.weight"), d_cls, None, None, None, B, d, d, d, d, L * d,
                     a_kmajor=1, b_kmajor=0, **self.rkw)

    def _stage_qa_labels(self, qa_labels):
        """QA branch of a task_qa pretraining model (ref lxrt/modeling.py:292-304; it rides on every task): True when it is active"""
        if not self.task_qa:
            assert qa_labels is None, "qa_labels given but the model has no QA head (build the store with num_answers > 0)"
            return False
        assert qa_labels is not None, "a task_qa model adds qa_loss in every branch: label_dict['qa_labels'] is required"
        self.answer.labels.copy_(qa_labels.reshape(-1), non_blocking=True)
        return True

    def _task_encoder_forward(self, task, rows, word_labels, word_rows, matched_labels):
        """stage the task's labels, then the encoder forward the task needs (rows: the masked rows of a vis_mask step, or None)"""
        if task == "word_mask":
            self.lang_heads.stage_labels(word_labels, word_rows)
        elif task == "matched":
            self.lang_heads.matched_labels.copy_(matched_labels, non_blocking=True)
        assert task != "qa" or self.task_qa, "task 'qa' needs a model built with the QA head (num_answers > 0)"
        self.encoder_forward(want_pooled=self.task_qa or task in ("matched", "qa"),
                             ffn_rows=(rows.idx, rows.n) if rows is not None else None)

    def backward_from_outputs(self, d_lang=None, d_vis=None, d_pooled=None):
        """backward of LxmertModel.forward from gradients of its three outputs (any may be None): ACCUMULATES into store.grad
        (HF:691-822; the pooler's gradient joins the [CLS] rows of d(language_output))."""
        assert self.need_lang, "needs the language side of the last cross layer (engine built with need_lang=True)"
        d = self.d
        if self._ffn_rows_run is not None:          # the last forward was a masked-visual-token step's: the vision output exists
            if d_vis is not None:                   # at the masked rows only, in compact form (encoder_forward ffn_rows)
                raise RuntimeError("backward_from_outputs(d_vis=): the last forward computed the vision output at the masked rows "
                                   "only; run encoder_forward() for a backward from a vision-output gradient")
            self._dvis_c = self._NO_VIS_GRAD
        self.begin_backward()
        GA = self.GA
        if d_lang is None or d_vis is None:
            self.zero_out_grads(GA)
        if d_lang is not None:
            self.glang(GA).copy_(d_lang.reshape(self.MLd, d))
        if d_vis is not None:
            self.vr(GA).copy_(d_vis.reshape(self.MV, d))
        if d_pooled is not None:
            if self._dpooled is None:
                self._dpooled, self._dpool_z = self.act(self.B, d), self.act(self.B, d)
            self._dpooled.copy_(d_pooled.reshape(self.B, d))
            cls_rows, d_cls = self._cls_views(GA)
            self.pooler_backward(self._dpooled, self._dpool_z, cls_rows, d_cls, accumulate=True)
        self.encoder_backward(have_lang_grad=True)

    def glang(self, G):
        """where the heads leave d(language_output) in the reference's dense [B*L, d] layout: the language rows of the gradient
        buffer G themselves, or -- packed language rows -- a dense side buffer that encoder_backward gathers into them."""
        return self.glang_pad if self.packed else self.lr(G)

    def zero_out_grads(self, G):
        """d(language_output) = d(vision_output) = 0 (the caller then writes what its loss produces)"""
        self.ops.zero(G[:self.MX])
        if self.packed:
            self.ops.zero(self.glang_pad)

    def _cls_views(self, G):
        """[B, d] views with row stride L*d of the [CLS] rows of language_output and of its gradient"""
        B, L, d = self.B, self.L, self.d
        return self.lang_final.view(B, L * d)[:, :d], self.glang(G).view(B, L * d)[:, :d]

    # Every branch of XLxmertForPretraining.forward (ref lxrt/modeling.py:154-308) as two phases: task_forward = encoder + heads
    # + losses (and the loss gradients w.r.t. the head outputs: no parameter gradient is touched), task_backward = everything
    # that accumulates into store.grad.  The trainer runs them back to back around one clear of the gradient buffer
    # (*_forward_backward below); the nn.Module surface runs them from autograd's forward / backward.
    def task_forward(self, task, word_labels=None, word_rows=None, matched_labels=None, qa_labels=None, feat_loss=True,
                     want_grad=True):
        """returns {name: 0-d/1-element device tensor} with the reference's out_dict keys (lm_loss / matched_loss / obj_loss,
        feat_loss / qa_loss)."""
        assert task in ("vis_mask", "word_mask", "matched", "qa"), task
        lh = self.lang_heads
        self._task_run = task
        rows = self._step_rows_run = self._step_rows() if task == "vis_mask" and want_grad else None
        self._task_encoder_forward(task, rows, word_labels, word_rows if want_grad else None, matched_labels)
        out = {}
        if task == "vis_mask":
            self.head_forward(rows=rows)
            losses = self.losses_forward_backward(want_grad, feat_loss, rows=rows)
            out["obj_loss"] = losses[0:1]
            if feat_loss:
                out["feat_loss"] = losses[1:2]
        elif task == "word_mask":
            lh.mlm_fwd(self.lang_final)
            out["lm_loss"] = lh.mlm_loss()[0:1]
        elif task == "matched":
            lh.rel_fwd(self.pooled)
            out["matched_loss"] = lh.rel_loss()[1:2]
        if self._stage_qa_labels(qa_labels):
            self.answer.fwd(self.pooled)
            self.answer.ce_loss_fwd_bwd(True)
            out["qa_loss"] = self.answer.loss[0:1]
        self._qa_run = "qa_loss" in out
        return out

    # ---- validation pass (ref pretrain/lxmert_pretrain.py:553-673 evaluate_epoch; tasks/vqa.py:259-311 predict / evaluate): one task
    # per batch, forward only, model.eval() semantics.  The losses need of the logits only (max, sum exp, the label's logit) per row
    # and the accuracy the argmax: on the bf16 path the big heads' contractions end in XL_EPI_ROWSCORE and the logits never reach
    # memory; the small heads (and fp32 engines, rows off the 256 grid, XL_FUSED_PREDICT=0) go through xl_score_rows over fp32 logits.
    def eval_buf(self, name, M, N, dtype=None):
        """scratch of the validation pass: its own (the backward scratch generations -- tmp() -- are not touched)"""
        dt = self.cdtype if dtype is None else dtype
        key = (name, M, N, dt)
        if key not in self._eval_bufs:
            self._eval_bufs[key] = torch.zeros(M, N, dtype=dt, device=self.dev)
        return self._eval_bufs[key]

    def _eval_totals(self, key):
        """fp32[4] of xl_rowscore_combine / xl_score_rows {sum nll, valid rows, rows predicted right, -}, zeroed for this call"""
        t = self.eval_buf("tot_" + key, 1, 4, torch.float32).view(4)
        self.ops.zero(t)
        return t

    @staticmethod
    def _eval_out(out, key, tot):
        """the mean loss (what task_forward(want_grad=False) calls `key`: sum / max(count, 1)) and the additive totals"""
        out[key] = tot[0:1] / tot[1:2].clamp(min=1.0)
        out[key + "_sum"], out[key + "_count"], out[key + "_correct"] = tot[0:1].clone(), tot[1:2].clone(), tot[2:3].clone()

    def evaluate_task(self, task, word_labels=None, word_rows=None, matched_labels=None, qa_labels=None, targets=None, labels=None,
                      feat_loss=True):
        """Forward-only losses and accuracies of one task on the batch set_inputs staged: `vis_mask`, `word_mask`, `matched`, `qa`
        (arguments as task_forward) and the fine-tune tasks `vqa` (targets [B, A] soft scores) and `nlvr2` (labels [P]).
        Dropout is off for the call whatever the engine was built with; the step seed, store.grad, the parameters, the optimizer
        state, the accumulation flags and the backward scratch are not touched.  Returns {name: device tensor}, no host
        synchronisation: the reference's loss keys (obj_loss, feat_loss, lm_loss, matched_loss, qa_loss; `loss` for vqa / nlvr2) --
        each mean is what task_forward(want_grad=False) returns for the same inputs -- and per classification loss <key>_sum,
        <key>_count, <key>_correct (additive over batches: EvalMeter), qa_pred (ref lxrt/modeling.py:300), and for vqa / nlvr2
        `score`, `pred` = logit.max(1).  The tensors are valid until the next evaluate_task."""
        assert task in ("vis_mask", "word_mask", "matched", "qa", "vqa", "nlvr2"), task
        p_saved = (self.p_hid, self.p_attn)
        self.p_hid = self.p_attn = 0.0
        try:
            if task in ("vqa", "nlvr2"):
                return self._evaluate_finetune(task, targets, labels)
            return self._evaluate_task(task, word_labels, word_rows, matched_labels, qa_labels, feat_loss)
        finally:
            self.p_hid, self.p_attn = p_saved

    def _eval_pred(self, key, n):
        return self.eval_buf("pred_" + key, 1, n, torch.int32).view(n)

    def _evaluate_finetune(self, task, targets, labels):
        ops, ans = self.ops, self.answer
        out = {}
        assert ans is not None and not self.task_qa, "vqa / nlvr2 need a fine-tune model (ParamStore task='vqa' / 'nlvr2')"
        B, A = ans.Bh, ans.A
        pred, score = self._eval_pred("ans", B), self.eval_buf("score_ans", 1, B, torch.float32).view(B)
        if task == "vqa":
            ans.targets.copy_(targets, non_blocking=True)
            self.vqa_forward()
            out["loss"] = ans.loss_fwd_bwd(False)                                   # BCEWithLogitsLoss, no d(logit)
            ops.score_rows(ans.logit, B, A, A, None, None, pred, score, None)
            out["loss_sum"], out["loss_count"] = out["loss"] * float(B), torch.full_like(out["loss"], float(B))
            # the reference's VQA accuracy (tasks/vqa.py:288-297 evaluate): the soft score of the predicted answer
            out["loss_correct"] = ans.targets.gather(1, pred.long()[:, None]).sum().reshape(1)
        else:
            assert ans.pair, "build the store with task='nlvr2'"
            ans.labels.copy_(labels.reshape(-1), non_blocking=True)
            self.vqa_forward()
            tot = self._eval_totals("ans")
            ops.score_rows(ans.logit, B, A, A, ans.labels, None, pred, score, tot)
            self._eval_out(out, "loss", tot)
        out["pred"], out["score"] = pred, score
        return out

    def _evaluate_task(self, task, word_labels, word_rows, matched_labels, qa_labels, feat_loss):
        ops, lh, ans = self.ops, self.lang_heads, self.answer
        out = {}
        if task == "vis_mask":
            assert self.task in ("vis_mask", "all"), "the codebook head belongs to a model built for task 'vis_mask' / 'all'"
        rows = self._step_rows() if task == "vis_mask" else None
        self._task_encoder_forward(task, rows, word_labels, word_rows, matched_labels)
        if task == "vis_mask":
            self._eval_vis_head(out, rows, feat_loss)
        elif task == "word_mask":
            tot = self._eval_totals("lm")
            lh.mlm_evaluate(self.lang_final, tot, self._eval_pred("lm", self.MLd))
            self._eval_out(out, "lm_loss", tot)
        elif task == "matched":
            lh.rel_fwd(self.pooled)
            tot = self._eval_totals("matched")
            ops.score_rows(lh.rel, self.B, 2, 8, lh.matched_labels, None, None, None, tot)
            self._eval_out(out, "matched_loss", tot)
        if self._stage_qa_labels(qa_labels):
            ans.fwd(self.pooled)
            tot, pred = self._eval_totals("qa"), self._eval_pred("qa", ans.Bh)
            ops.score_rows(ans.logit, ans.Bh, ans.A, ans.A, ans.labels, None, pred, None, tot)
            self._eval_out(out, "qa_loss", tot)
            out["qa_pred"] = pred
        return out

    def _eval_vis_head(self, out, rows, feat_loss):
        """LxmertVisualObjHead and both of its losses on the masked rows only (exact; pad entries of the row list are zero rows with
        label -100) or on all rows: the training step's head forward without the logits, on the validation scratch, then the scores"""
        ops = self.ops
        ops.block = "head"
        M = rows.n if rows is not None else self.MV
        labels = rows.gather_labels(self.labels) if rows is not None else self.labels
        feat, _ = heads.codebook_forward(self, rows, want_logits=False, scratch=self.eval_buf)
        tot, pred = self._eval_totals("obj"), self._eval_pred("obj", self.MV)[:M]        # (pred: the head's rows, in row-list order)
        self.code_pred.score(feat, M, labels, pred, tot)
        self._eval_out(out, "obj_loss", tot)
        if feat_loss:
            ops.zero(self.losses[1:2])
            ops.mask_counts(self.labels, self.vmask, self.counts, self.nmask, self.B, self.V)
            ops.featloss_fwd_bwd(feat, self.store.centroids_c, self.cid, self.vmask, self.nmask, None, self.losses[1:], self.B, self.V,
                                 self.F, 1.0, rows=rows.idx if rows is not None else None, n_rows=M if rows is not None else 0,
                                 targets=self.feat_tgt)
            out["feat_loss"] = self.losses[1:2]

    def task_backward(self):
        """backward of the branch task_forward ran last; ACCUMULATES into store.grad."""
        task, qa, lh, ans = self._task_run, self._qa_run, self.lang_heads, self.answer
        self.begin_backward()
        GA = self.GA
        if task == "vis_mask":
            self.head_backward(self.vr(GA), report=not qa, rows=self._step_rows_run)
            if self.need_lang:          # the language side of the last cross layer exists: zero gradient ...
                self.ops.zero(self.glang(GA))
            if qa:                      # ... unless the QA branch reads pooled_output
                cls_rows, d_cls = self._cls_views(GA)
                ans.bwd(cls_rows, d_cls)
                self._ready_heads()
            self.encoder_backward(self.need_lang)
            return
        self.zero_out_grads(GA)
        cls_rows, d_cls = self._cls_views(GA)
        if task == "word_mask":
            lh.mlm_bwd(self.glang(GA))
            if qa:
                ans.bwd(cls_rows, d_cls, accumulate=True)     # the MLM gradient of the [CLS] rows is there
        elif task == "matched":
            extra = None
            if qa:
                ans.bwd_to_pooled()
                extra = ans.dpooled
            lh.rel_bwd(self.pooled, cls_rows, d_cls, extra_dpooled=extra)
        else:
            ans.bwd(cls_rows, d_cls)
        self._ready_heads()
        self.encoder_backward(True)

    def _task_step(self, task, **kw):
        out = self.task_forward(task, **kw)
        self.clear_grads()
        self.task_backward()
        return out

    def vis_mask_forward_backward(self, feat_loss=True, qa_labels=None):
        """XLxmertForPretraining.forward(task='vis_mask') + loss.backward() (ref lxrt/modeling.py:154-308,
        lxmert_pretrain.py:338).  Gradients land in store.grad; returns the device loss buffer [obj_loss, feat_loss]
        (a task_qa model's qa_loss is in self.answer.loss)."""
        self._task_step("vis_mask", feat_loss=feat_loss, qa_labels=qa_labels)
        return self.losses

    def qa_forward_backward(self, qa_labels):
        """XLxmertForPretraining.forward(task='qa') + backward on a task_qa model (ref lxrt/modeling.py:154-210, 292-306):
        un-masked codebook features in, total_loss = qa_loss.  Returns the device loss buffer [1]."""
        return self._task_step("qa", qa_labels=qa_labels)["qa_loss"]

    def word_mask_forward_backward(self, word_labels, word_rows=None, qa_labels=None):
        """XLxmertForPretraining.forward(task='word_mask') + backward (ref lxrt/modeling.py:211-219): un-masked codebook
        features in (set_inputs(cluster_ids=..., vis_mask=None)), MLM loss over `word_labels` (negative = ignored)."""
        return self._task_step("word_mask", word_labels=word_labels, word_rows=word_rows, qa_labels=qa_labels)["lm_loss"]

    def matched_forward_backward(self, matched_labels, qa_labels=None):
        """XLxmertForPretraining.forward(task='matched') + backward (ref lxrt/modeling.py:221-229)."""
        return self._task_step("matched", matched_labels=matched_labels, qa_labels=qa_labels)["matched_loss"]

    # ------------------------------------------------------------ fine-tune steps
    def vqa_forward(self):
        """VQAModel.forward (ref tasks/vqa_model.py:22-72): real grid features -> encoder -> pooled_output -> answer head."""
        self.encoder_forward(want_pooled=True)
        return self.answer.fwd(self.pooled)

    def _finetune_step(self, loss_fwd_bwd):
        """forward, the answer head's loss (and d(logit)), backward through the head, the pooler and the whole encoder: only the
        [CLS] rows of the language output carry gradient"""
        self.vqa_forward()
        self.zero_accumulated_grads()
        loss = loss_fwd_bwd(True)
        GA = self.GA
        self.zero_out_grads(GA)
        cls_rows, d_cls = self._cls_views(GA)
        self.answer.bwd(cls_rows, d_cls)
        self._ready_heads()
        self.encoder_backward(True)
        return loss

    def vqa_forward_backward(self, targets):
        """one VQA/GQA fine-tune forward + backward (ref tasks/vqa.py:166-189): BCEWithLogitsLoss(logit, target).backward().
        Gradients land in store.grad; returns the device loss buffer [1]."""
        self.answer.targets.copy_(targets, non_blocking=True)
        return self._finetune_step(self.answer.loss_fwd_bwd)

    def nlvr2_forward_backward(self, labels):
        """one NLVR2 fine-tune forward + backward (ref tasks/nlvr2.py:72 CrossEntropyLoss over the 2-way logit of each
        statement; tasks/nlvr2_model.py:50-86: encoder over the flattened [2P] (statement, image) rows, pooled outputs of a
        statement's two images concatenated).  `labels` [P] int64.  Returns the device loss buffer [1]."""
        ans = self.answer
        assert ans is not None and ans.pair, "build the store with task='nlvr2'"
        ans.labels.copy_(labels.reshape(-1), non_blocking=True)
        return self._finetune_step(ans.ce_loss_fwd_bwd)
