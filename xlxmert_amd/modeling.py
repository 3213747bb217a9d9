"""Drop-in model classes for the X-LXMERT hot path, keeping the reference's API surface:

  * `LxmertModel.forward(input_ids, visual_feats, visual_pos, attention_mask, visual_attention_mask, token_type_ids,
    inputs_embeds, output_attentions, output_hidden_states, return_dict)` -> index-able
    `(language_output, vision_output, pooled_output)`                                   (HF:691-822)
  * `LxmertVisualObjHead.forward(hidden_states, out_keys=[]) -> {'feat', 'obj'}`        (ref lxrt/modeling.py:38-53)
  * `XLxmertForPretraining` with `.bert`, `.obj_predict_head`, `.mask_feat`, `.vis_emb`, `set_visual_embedding()`,
    `forward(..., cluster_ids, vis_mask, label_dict, task='vis_mask') -> dict of losses` (ref lxrt/modeling.py:56-308)
  * `state_dict()` / `load_state_dict()` with the reference's key layout, incl. the DDP
    `module.` prefix convention of the published checkpoints (ref utils.py:42-49)
  * legacy aliases `LXRTEncoder`, `LXRTModel` for the original LXMERT names used by BASELINE.json

All parameters are views into one flat buffer (params.ParamStore); compute runs through engine.Engine on the HIP kernels.
Autograd integration: each forward is ONE torch.autograd.Function whose backward runs the engine's hand-derived backward
and deposits parameter gradients directly into `param.grad` (views of the flat gradient buffer).
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from .config import XLxmertConfig
from .engine import Engine, _h
from .ops import HipOps
from .params import ParamStore


class LxmertModelOutput(tuple):
    """Index-able (language_output, vision_output, pooled_output) with the HF field names."""

    def __new__(cls, lang, vis, pooled):
        obj = super().__new__(cls, (lang, vis, pooled))
        obj.language_output, obj.vision_output, obj.pooled_output = lang, vis, pooled
        obj.language_hidden_states, obj.vision_hidden_states = None, None        # filled when output_hidden_states is asked for
        obj.language_attentions, obj.vision_attentions, obj.cross_encoder_attentions = None, None, None      # output_attentions
        return obj


class _Named(nn.Module):
    """A module whose parameters are views of the ParamStore (registered under the reference's attribute names)."""

    def _bind(self, store, prefix, names):
        for full in names:
            assert full.startswith(prefix)
            rel = full[len(prefix):].lstrip(".")
            mod = self
            parts = rel.split(".")
            for p in parts[:-1]:
                if p not in mod._modules:
                    mod.add_module(p, nn.Module())
                mod = mod._modules[p]
            param = nn.Parameter(store.view(full), requires_grad=True)
            param.grad = store.gview(full)
            mod.register_parameter(parts[-1], param)


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, anchor, inputs_embeds=None):
        eng = model._engine
        lang, vis, pooled = eng.encoder_forward(want_pooled=True)
        ctx.model = model
        ctx.emb_dtype = inputs_embeds.dtype if inputs_embeds is not None and inputs_embeds.requires_grad else None
        ctx.set_materialize_grads(False)            # outputs the loss does not read arrive as None in backward
        B, L, V, d = eng.B, eng.L, eng.V, eng.d
        return lang.view(B, L, d).clone(), vis.view(B, V, d).clone(), pooled.view(B, d).clone()

    @staticmethod
    def backward(ctx, d_lang, d_vis, d_pooled):
        # vec-type gradients accumulate into param.grad (views of the flat buffer): call model.zero_grad() per step
        eng = ctx.model._engine
        eng.backward_from_outputs(d_lang, d_vis, d_pooled)
        return None, None, (eng.d_inputs_embeds().to(ctx.emb_dtype) if ctx.emb_dtype is not None else None)


class LxmertModel(_Named):
    """Embeddings + LxmertEncoder (9 language / 5 visual / 5 cross layers) + pooler (HF:675-822)."""

    def __init__(self, config: XLxmertConfig, store=None, device=None, dtype=torch.bfloat16, task="all", residual_dtype=None):
        """residual_dtype ("bf16" | "fp32"; None: env XL_RESIDUAL, default "bf16"; meaningful with dtype=torch.bfloat16): storage type
        of the residual stream, passed on to engine.Engine -- "fp32" keeps the pre-LayerNorm sums, the LayerNorm outputs and their
        gradients in fp32 beside bf16 operands; output_hidden_states then returns the fp32 values."""
        super().__init__()
        self.config = config
        self._residual_dtype = residual_dtype
        dev = torch.device(device if device is not None else "cuda")
        self._owns_store = store is None
        self._store = store if store is not None else ParamStore(config, dev, dtype, task=task)
        self._ops = HipOps(self._store.compute_dtype)
        self._engine = None
        self._geom = None
        names = [n for n in self._store.names() if n.startswith("bert.")]
        self._bind(self._store, "bert", names)
        self.dtype = self._store.compute_dtype
        self._anchor = torch.zeros(1, device=dev, requires_grad=True)

    def _engine_for(self, B, L, V):
        if self._geom != (B, L, V, self.training):
            self._engine = Engine(self.config, self._store, self._ops, B, L, V, need_lang=True,
                                  train_dropout=self.training, residual_dtype=self._residual_dtype)
            self._geom = (B, L, V, self.training)
        self._engine.sync_compute_weights()
        self._advance_seed(self._engine)
        return self._engine

    _train_calls = 0

    def _advance_seed(self, eng):
        """training mode: every forward draws fresh dropout masks -- the step part of the seeds (device memory, read by the
        kernels of this forward AND of its backward) advances once per call, as torch's generator state does in the reference."""
        if eng.p_hid > 0 or eng.p_attn > 0:
            self._train_calls += 1
            eng.set_step_seed(self._train_calls)

    def forward(self, input_ids=None, visual_feats=None, visual_pos=None, attention_mask=None,
                visual_attention_mask=None, token_type_ids=None, inputs_embeds=None, output_attentions=None,
                output_hidden_states=None, return_dict=None, **kwargs):
        # argument validation mirrors HF:731-744
        if input_ids is not None and inputs_embeds is not None:
            raise ValueError("You cannot specify both input_ids and inputs_embeds at the same time")
        if input_ids is None and inputs_embeds is None:
            raise ValueError("You have to specify either input_ids or inputs_embeds")
        if visual_feats is None:
            raise ValueError("`visual_feats` cannot be `None`")
        if visual_pos is None:
            raise ValueError("`visual_pos` cannot be `None`")
        B, L = input_ids.shape if input_ids is not None else inputs_embeds.shape[:-1]          # HF:735-741
        V = visual_feats.shape[1]
        eng = self._engine_for(B, L, V)
        eng.set_inputs(input_ids, attention_mask, token_type_ids, visual_pos, visual_feats=visual_feats,
                       visual_attention_mask=visual_attention_mask, inputs_embeds=inputs_embeds)
        eng.use_codebook = False
        if torch.is_grad_enabled():
            lang, vis, pooled = _EncoderFn.apply(self, self._anchor, inputs_embeds)
        else:
            l_, v_, p_ = eng.encoder_forward(want_pooled=True)
            lang, vis, pooled = l_.view(B, L, -1).clone(), v_.view(B, V, -1).clone(), p_.view(B, -1).clone()
        out = LxmertModelOutput(lang, vis, pooled)
        if output_hidden_states:        # HF:806-822: (language_hidden_states, vision_hidden_states); copies without a gradient path
            lh, vh = eng.hidden_states()
            out.language_hidden_states = tuple(h.view(B, L, -1).detach().clone() for h in lh)
            out.vision_hidden_states = tuple(h.view(B, V, -1).detach().clone() for h in vh)
        if output_attentions:           # HF:806-822; fp32 [B, H, nq, nk] copies without a gradient path, recomputed on demand
            la, va, xa = eng.attention_probs()
            out.language_attentions, out.vision_attentions, out.cross_encoder_attentions = tuple(la), tuple(va), tuple(xa)
        if return_dict in (None, True):
            return out
        t = tuple(out)
        if output_hidden_states:
            t = t + (out.language_hidden_states, out.vision_hidden_states)
        if output_attentions:
            t = t + (out.language_attentions, out.vision_attentions, out.cross_encoder_attentions)
        return t


LXRTModel = LxmertModel          # legacy names (original LXMERT code base / BASELINE.json wording)
LXRTEncoder = LxmertModel


class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, head, vis, want_obj):
        eng = head._bert._engine
        eng.vis_final = _h(eng.vr(eng.X[-1]))               # (the head reads the bf16 copy of an fp32 residual stream)
        eng.vis_final.copy_(vis.reshape(eng.MV, eng.d))
        feat, logits = eng.head_forward(want_logits=want_obj)
        ctx.head = head
        B, V = eng.B, eng.V
        return feat.view(B, V, -1).float().clone(), logits.view(B, V, -1).clone()

    @staticmethod
    def backward(ctx, d_feat, d_obj):
        eng = ctx.head._bert._engine
        MV = eng.MV
        eng.dlogits.zero_()
        if d_obj is not None:
            eng.dlogits[:, :eng.K].copy_(d_obj.reshape(MV, eng.K))
        eng.with_feat_loss = d_feat is not None
        if d_feat is not None:
            eng.dfeat.copy_(d_feat.reshape(MV, eng.F))
        d_vis = torch.empty(MV, eng.d, dtype=torch.float32 if eng.res32 else eng.cdtype, device=eng.dev)
        eng.head_backward(d_vis)
        return None, d_vis.view(eng.B, eng.V, eng.d), None


class LxmertVisualObjHead(_Named):
    """Cluster-codebook head (ref lxrt/modeling.py:8-53): transform -> linear_feat -> out_cluster (frozen centroids)."""

    def __init__(self, config, bert):
        super().__init__()
        self.config = config
        object.__setattr__(self, "_bert", bert)
        store = bert._store
        names = [n for n in store.names() if n.startswith("obj_predict_head.")]
        self._bind(store, "obj_predict_head", names)
        self.visual_losses = {"obj": {"shape": (-1,), "num": config.num_clusters},
                              "feat": {"shape": (-1, config.visual_feat_dim), "num": config.visual_feat_dim}}
        self.cluster_out = config.num_clusters > 0

    def forward(self, hidden_states, out_keys=()):
        eng = self._bert._engine
        assert eng is not None, "run .bert first: the head shares the engine's batch geometry"
        if torch.is_grad_enabled() and hidden_states.requires_grad:
            feat, obj = _HeadFn.apply(self, hidden_states, True)
        else:
            eng.vis_final = _h(eng.vr(eng.X[-1]))
            eng.vis_final.copy_(hidden_states.reshape(eng.MV, eng.d))
            f, o = eng.head_forward(True)
            feat, obj = f.view(eng.B, eng.V, -1).float().clone(), o.view(eng.B, eng.V, -1).clone()
        output = {}
        if "feat" in self.visual_losses or "feat" in out_keys:
            output["feat"] = feat
        if "obj" in self.visual_losses or "obj" in out_keys:
            output["obj"] = obj
        return output


class _TaskStepFn(torch.autograd.Function):
    """One branch of XLxmertForPretraining.forward as engine.task_forward (encoder, heads, losses) with engine.task_backward
    as its backward; `losses` come back as one tensor in the order of `keys`."""

    @staticmethod
    def forward(ctx, model, anchor, task, kw, keys):
        eng = model.bert._engine
        out = eng.task_forward(task, **kw)
        keys.extend(out.keys())
        ctx.model = model
        return torch.cat([out[k].reshape(1) for k in keys]).clone()

    @staticmethod
    def backward(ctx, d_losses):
        eng = ctx.model.bert._engine
        s = d_losses.tolist()
        if max(s) - min(s) > 1e-12 * max(1.0, abs(s[0])):
            raise NotImplementedError("the branch's losses must be weighted equally (total_loss is their plain sum)")
        # gradients ACCUMULATE into the flat buffer (several forward/backward calls per update, --update > 1): clearing is
        # zero_grad()'s job, as with autograd; the deferred column reductions are switched on and off inside this backward
        st = ctx.model._store
        if s[0] != 1.0:             # a scaled loss (gradient accumulation / loss scaling): scale what this call adds
            keep = st.grad[:st.n_used].clone()
            st.grad[:st.n_used].zero_()
            eng.task_backward()
            st.grad[:st.n_used].mul_(s[0]).add_(keep)
        else:
            eng.task_backward()
        return None, None, None, None, None


class LxmertPreTrainingHeads(_Named):
    """HF:648-657 `cls`: predictions (LxmertLMPredictionHead, decoder tied to the word embeddings) + seq_relationship;
    parameters are views of the flat buffer, compute runs in engine.LangHeads."""

    def __init__(self, store):
        super().__init__()
        self._bind(store, "cls", [n for n in store.names() if n.startswith("cls.")])


def _sample_seed(seed):
    """the samplers' noise seed: the caller's, or one drawn from torch's default CPU generator (torch.manual_seed governs)"""
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)


def _truncation_kw(top_k, top_p, min_p):
    """the truncation keywords that were given, validated (Engine.check_truncation); {} = none: the call lists of before"""
    Engine.check_truncation(top_k, top_p, min_p)
    return {k: v for k, v in (("top_k", top_k), ("top_p", top_p), ("min_p", min_p)) if v is not None}


def _sampling_kw(temperature, sample_seed, top_k, top_p, min_p):
    """keywords of Engine.sample_codes_nar / _ar for the ImggenModel surface; {} = the greedy loop"""
    trunc = _truncation_kw(top_k, top_p, min_p)
    if temperature is None and not trunc:
        return {}
    return {"temperature": temperature, "seed": _sample_seed(sample_seed), **trunc}


class XLxmertForPretraining(nn.Module):
    """ref lxrt/modeling.py:56-308: `.bert`, `.cls` (task_mask_lm or task_matched), `.obj_predict_head` (task_obj_predict),
    `.answer_head` (task_qa), `.mask_feat`, `.vis_emb`; forward(task = 'vis_mask' | 'word_mask' | 'matched' | 'qa')."""

    def __init__(self, config: XLxmertConfig, num_clusters=None, device=None, dtype=torch.bfloat16, residual_dtype=None):
        """residual_dtype: see LxmertModel (storage type of the residual stream: "bf16" default, "fp32")."""
        super().__init__()
        if num_clusters is not None:
            config.num_clusters = num_clusters
        self.config = config
        self.task_mask_lm, self.task_matched = config.task_mask_lm, config.task_matched
        self.task_obj_predict, self.task_qa = config.task_obj_predict, config.task_qa
        self.num_qa_labels = config.num_qa_labels
        dev = torch.device(device if device is not None else "cuda")
        multi = self.task_mask_lm or self.task_matched or self.task_qa
        # one parameter set for every branch the model was built for; a model with only the codebook head keeps the
        # dead-branch-free layout of the masked-visual-token step
        self._store = ParamStore(config, dev, dtype, task="all" if multi else "vis_mask",
                                 num_answers=self.num_qa_labels if self.task_qa else 0)
        self.bert = LxmertModel(config, store=self._store, device=dev, residual_dtype=residual_dtype)
        if self.task_mask_lm or self.task_matched:
            self.cls = LxmertPreTrainingHeads(self._store)
        self.obj_predict_head = LxmertVisualObjHead(config, self.bert)
        if self.task_qa:
            self.answer_head = LxmertVisualAnswerHead(self._store)
        self.mask_feat = nn.Parameter(self._store.view("mask_feat"))
        self.mask_feat.grad = self._store.gview("mask_feat")
        self.vis_emb = None
        self._match_key, self._match_runner = None, None        # caption-image matching: the runner of the last geometry asked for
        self._anchor = torch.zeros(1, device=dev, requires_grad=True)
        from .trainer import init_reference_weights
        init_reference_weights(self._store, seed=0)

    # ---- reference API
    def set_visual_embedding(self, centroids):
        """ref lxrt/modeling.py:140-151: frozen nn.Embedding over the k-means centroids, tied to out_cluster.weight."""
        import numpy as np
        if isinstance(centroids, np.ndarray):
            centroids = torch.from_numpy(centroids)
        self._store.set_centroids(centroids)
        self.vis_emb = nn.Embedding.from_pretrained(self._store.centroids, freeze=True)
        self.obj_predict_head.out_cluster.weight = self.vis_emb.weight        # tied, frozen (ref :150-151)

    def zero_grad(self, set_to_none=False):
        """Gradients live in the flat buffer that every `param.grad` views: clear it in place (never detach the views)."""
        self._store.grad.zero_()
        for name, p_ in self.named_parameters():
            if p_.grad is None and name in self._store.index:
                p_.grad = self._store.gview(name)

    def state_dict(self, *args, prefix="", **kwargs):
        sd = OrderedDict((prefix + k, v.detach()) for k, v in self._store.named_state().items())
        return sd

    def load_state_dict(self, state_dict, strict=False):
        """Accepts the reference layout, with or without the DDP `module.` prefix (ref utils.py:42-49)."""
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        missing = self._store.load_named(sd, strict=strict)
        if self.vis_emb is None and self._store.centroids is not None:
            self.set_visual_embedding(self._store.centroids)
        # aliases of tensors stored once: the frozen codebook (vis_emb == out_cluster.weight) and the MLM decoder, tied to the
        # word embeddings (transformers 4.1.1 LxmertPreTrainingHeads(config, embedding_weight), ref lxrt/modeling.py:86)
        alias = ("vis_emb.weight", "obj_predict_head.out_cluster.weight", "cls.predictions.decoder.weight")
        unexpected = [k for k in sd if k not in self._store.index and k not in alias]
        return missing, unexpected

    def forward(self, input_ids=None, visual_feats=None, visual_pos=None, attention_mask=None,
                visual_attention_mask=None, cluster_ids=None, vis_mask=None, token_type_ids=None, inputs_embeds=None,
                output_attentions=None, output_hidden_states=None, return_dict=None, label_dict=None,
                task="vis_mask", **kwargs):
        if task not in ("vis_mask", "word_mask", "matched", "qa"):
            raise ValueError(f"task must be one of 'word_mask', 'vis_mask', 'matched', 'qa' (got {task!r})")
        if self.vis_emb is None:
            raise RuntimeError("call set_visual_embedding(centroids) first (ref lxrt/modeling.py:185-186)")
        if inputs_embeds is not None or visual_attention_mask is not None or output_attentions or output_hidden_states:
            raise NotImplementedError("inputs_embeds / visual_attention_mask / attention maps / hidden states: None in every "
                                      "reference caller of this model (ref lxmert_pretrain.py:201-223)")
        label_dict = label_dict or {}
        B, L = input_ids.shape
        V = cluster_ids.shape[1]
        eng = self._step_engine(B, L, V)
        kw = {}
        if task == "vis_mask":
            # feature regression iff the caller supplies its targets: the reference trainer adds label_dict['feat_labels']
            # (the real grid features) exactly when 'feat' is in --visualLosses (lxmert_pretrain.py:177-179); the canonical
            # recipe (scripts/pretrain.bash:15, --visualLosses obj) has no feature loss.  (The published model code keys the
            # branch on visual_obj_loss and then fails on the missing label: SURVEY App. A item 10.)
            feat_labels = label_dict.get("feat_labels")
            eng.set_inputs(input_ids, attention_mask, token_type_ids, visual_pos, cluster_ids=cluster_ids, vis_mask=vis_mask,
                           obj_labels=label_dict["obj_labels"], feat_labels=feat_labels)
            kw["feat_loss"] = feat_labels is not None
        else:
            if task == "word_mask":
                if not self.task_mask_lm:
                    raise RuntimeError("task 'word_mask' on a model built without task_mask_lm (no `cls` head)")
                kw["word_labels"] = label_dict["word_labels"]
            elif task == "matched":
                if not self.task_matched:
                    raise RuntimeError("task 'matched' on a model built without task_matched (no `cls` head)")
                kw["matched_labels"] = label_dict["matched_labels"]
            # the [MASK]-feature substitution belongs to task == 'vis_mask' only (ref lxrt/modeling.py:190-193)
            eng.set_inputs(input_ids, attention_mask, token_type_ids, visual_pos, cluster_ids=cluster_ids)
        if self.task_qa:                    # `if self.task_qa:` -- on the MODEL, not the task argument (ref :292)
            kw["qa_labels"] = label_dict["qa_labels"]
        elif task == "qa":
            return {"total_loss": torch.zeros((), device=input_ids.device)}         # the reference adds nothing either
        keys = []
        if torch.is_grad_enabled():
            losses = _TaskStepFn.apply(self, self._anchor, task, kw, keys)
        else:
            out = eng.task_forward(task, want_grad=False, **kw)
            keys = list(out.keys())
            losses = torch.cat([out[k].reshape(1) for k in keys]).clone()
        out_dict = {k: losses[i].detach() for i, k in enumerate(keys)}
        if task == "vis_mask":
            out_dict["vis_loss"] = sum(losses[i] for i, k in enumerate(keys) if k in ("obj_loss", "feat_loss")).detach()
        if self.task_qa:
            out_dict["qa_pred"] = eng.answer.row_argmax.long().clone()          # ref :300
        out_dict["total_loss"] = losses.sum()
        return out_dict

    @torch.no_grad()
    def evaluate(self, input_ids=None, visual_feats=None, visual_pos=None, attention_mask=None,
                 visual_attention_mask=None, cluster_ids=None, vis_mask=None, token_type_ids=None, inputs_embeds=None,
                 output_attentions=None, output_hidden_states=None, return_dict=None, label_dict=None,
                 task="vis_mask", **kwargs):
        """One batch of the reference's validation pass (ref lxmert_pretrain.py:553-673 evaluate_epoch: model.eval(), no_grad, one
        task per batch): forward's arguments, Engine.evaluate_task's dict -- the task's loss keys, <key>_sum / _count / _correct
        (additive: trainer.EvalMeter) and qa_pred -- as device tensors without a host synchronisation.  eval() semantics for the
        call (no dropout); the training flag is restored afterwards, as the samplers do."""
        if task not in ("vis_mask", "word_mask", "matched", "qa"):
            raise ValueError(f"task must be one of 'word_mask', 'vis_mask', 'matched', 'qa' (got {task!r})")
        if self.vis_emb is None:
            raise RuntimeError("call set_visual_embedding(centroids) first (ref lxrt/modeling.py:185-186)")
        if inputs_embeds is not None or visual_attention_mask is not None or output_attentions or output_hidden_states:
            raise NotImplementedError("inputs_embeds / visual_attention_mask / attention maps / hidden states: None in every "
                                      "reference caller of this model (ref lxmert_pretrain.py:201-223)")
        label_dict = label_dict or {}
        was_training = self.training
        self.eval()
        try:
            B, L = input_ids.shape
            eng = self._step_engine(B, L, cluster_ids.shape[1])
            kw = {}
            if task == "vis_mask":
                feat_labels = label_dict.get("feat_labels")
                eng.set_inputs(input_ids, attention_mask, token_type_ids, visual_pos, cluster_ids=cluster_ids, vis_mask=vis_mask,
                               obj_labels=label_dict["obj_labels"], feat_labels=feat_labels)
                kw["feat_loss"] = feat_labels is not None
            else:
                if task == "word_mask":
                    if not self.task_mask_lm:
                        raise RuntimeError("task 'word_mask' on a model built without task_mask_lm (no `cls` head)")
                    kw["word_labels"] = label_dict["word_labels"]
                elif task == "matched":
                    if not self.task_matched:
                        raise RuntimeError("task 'matched' on a model built without task_matched (no `cls` head)")
                    kw["matched_labels"] = label_dict["matched_labels"]
                eng.set_inputs(input_ids, attention_mask, token_type_ids, visual_pos, cluster_ids=cluster_ids)
            if self.task_qa:
                kw["qa_labels"] = label_dict["qa_labels"]
            elif task == "qa":
                return {}                                                           # the reference adds nothing either
            return {k: v.clone() for k, v in eng.evaluate_task(task, **kw).items()}
        finally:
            self.train(was_training)

    @torch.no_grad()
    def match_scores(self, input_ids, attention_mask=None, token_type_ids=None, visual_feats=None, cluster_ids=None, visual_pos=None, *,
                     top_k=None, chunk_pairs=None, image_of_caption=None, caption_of_image=None):
        """Score every one of N captions (`input_ids` [N, L]; `attention_mask` prefix masks, None = full length) against every one of
        M images (`visual_feats` [M, V, F] or `cluster_ids` [M, V], un-masked; `visual_pos` [M, V, 4], default: the boxes of a square
        grid) with the `matched` head -- image retrieval, caption retrieval, re-ranking of samples, recall@k -- match.MatchRunner:
        the language stack runs once at batch N, the visual stack once at batch M, only the cross layers, the pooler and the 2-way
        head run per pair, in chunks of `chunk_pairs` pairs (default min(N*M, 256)); N, M <= 4096.  eval() semantics for the call.
        Returns a dict of device tensors: `margin` [N, M] = logit(matched) - logit(not matched) and `prob` [N, M] = its sigmoid, the
        softmax's matched probability; with top_k (<= min(32, N, M)) `topk_images` [N, k] / `topk_captions` [M, k] int32, ordered by
        margin, ties to the lower index; with targets `image_of_caption` [N] / `caption_of_image` [M] (ints, -1 = none) `rank_t2i` /
        `rank_i2t` (the number of candidates that rank before the target, -1 without one) and `recall` = {"t2i" | "i2t": {1, 5, 10:
        fraction of the queries with a target whose rank is < k}}, computed on the device and read by the host once (with it
        `recall_hits` fp32 [2, 4], the additive counts {rank < 1, < 5, < 10, queries with a target} per direction)."""
        from .match import RECALL_AT, MatchRunner
        if not self.task_matched:
            raise RuntimeError("match_scores on a model built without task_matched (no `cls` matched head)")
        if (visual_feats is None) == (cluster_ids is None):
            raise ValueError("give the pictures either as visual_feats or as cluster_ids")
        if cluster_ids is not None and self.vis_emb is None:
            raise RuntimeError("cluster_ids given but the model has no codebook: call set_visual_embedding(centroids) first")
        vis = visual_feats if cluster_ids is None else cluster_ids
        (N, L), M, V = input_ids.shape, vis.shape[0], vis.shape[1]
        if visual_pos is None:
            g = int(round(V ** 0.5))
            if g * g != V:
                raise ValueError(f"visual_pos is needed for {V} visual tokens (not a square grid)")
            visual_pos = self._grid_pos(g, M, vis.device)
        key = (N, M, L, V, chunk_pairs)
        if self._match_key != key:
            self._match_runner = MatchRunner(self.config, self._store, self.bert._ops, N, M, L, V, chunk_pairs=chunk_pairs,
                                             residual_dtype=self.bert._residual_dtype)
            self._match_key = key
        runner = self._match_runner
        runner.sync_compute_weights()
        out = runner.run(input_ids, attention_mask, token_type_ids, visual_feats=visual_feats, cluster_ids=cluster_ids,
                         visual_pos=visual_pos, top_k=top_k, image_of_caption=image_of_caption, caption_of_image=caption_of_image)
        out = {k: v.clone() for k, v in out.items()}
        if "recall_hits" in out:
            hits = out["recall_hits"].tolist()                                  # the one host read
            names = [n for n, r in (("t2i", "rank_t2i"), ("i2t", "rank_i2t")) if r in out]
            out["recall"] = {n: {k: hits[i][j] / max(hits[i][3], 1.0) for j, k in enumerate(RECALL_AT)}
                             for i, n in enumerate(("t2i", "i2t")) if n in names}
        return out

    @torch.no_grad()
    def sample_codes(self, input_ids, n_steps=4, grid_size=8, *, temperature=None, seed=None, top_k=None, top_p=None, min_p=None):
        """The device part of ImggenModel.sample_image_NAR (ref tasks/imggen_model.py:169-254): Mask-Predict sampling of
        the grid codes, returned as the generator's input `[B, feat_dim, grid, grid]` (fp32) plus the chosen code ids.
        Tokenisation (before) and the frozen GAN `G(code)` + denorm (after) stay with the caller, as in the reference.
        temperature (None = the reference's greedy choice): draw every code from softmax(logits / temperature); seed=None takes
        one from torch's default CPU generator (torch.manual_seed governs).  top_k / top_p / min_p (any given; temperature None
        then means 1): the draw is truncated as Engine.check_truncation describes."""
        import numpy as np
        temperature = Engine.check_temperature(temperature)
        trunc = _truncation_kw(top_k, top_p, min_p)
        if self.vis_emb is None:
            raise RuntimeError("call set_visual_embedding(centroids) first")
        was_training = self.training
        self.eval()
        B, L = input_ids.shape
        V = grid_size * grid_size
        eng = self._step_engine(B, L, V)
        pos = np.zeros((V, 4), np.float32)                      # ref utils.box_position
        for i in range(grid_size):
            for j in range(grid_size):
                pos[i * grid_size + j] = [j / grid_size, i / grid_size, (j + 1) / grid_size, (i + 1) / grid_size]
        dev = input_ids.device
        eng.set_inputs(input_ids, input_ids > 0, None, torch.from_numpy(pos).to(dev).unsqueeze(0).expand(B, -1, -1),
                       cluster_ids=torch.zeros(B, V, dtype=torch.long, device=dev),
                       vis_mask=torch.ones(B, V, dtype=torch.bool, device=dev))
        if temperature is None and not trunc:
            cid, code, _ = eng.sample_codes_nar(n_steps)
        else:
            cid, code, _ = eng.sample_codes_nar(n_steps, temperature=temperature, seed=_sample_seed(seed), **trunc)
        out = code.view(B, V, -1).permute(0, 2, 1).reshape(B, -1, grid_size, grid_size).float()
        self.train(was_training)
        return out, cid.clone()

    @torch.no_grad()
    def sample_caption_ids(self, visual_feats=None, visual_pos=None, *, cluster_ids=None, lengths, prefix_ids=None, n_steps=10,
                           max_text_length=20, temperature=None, seed=None, top_k=None, top_p=None, min_p=None, suppress_repeats=False,
                           banned_ids=None, return_intermediate=False, mask_token_id=103, cls_token_id=101, sep_token_id=102,
                           first_word_id=999):
        """Caption an image by Mask-Predict decoding over the MLM head (Engine.sample_words_nar; the reference trains the head for
        it, pretrain/lxmert_data.py --word_mask_predict, and has the loop on the visual side only).  The picture is given as real
        grid features `visual_feats` [B, V, F] or as `cluster_ids` [B, V] (e.g. what sample_codes just produced), both un-masked;
        visual_pos [B, V, 4] defaults to the boxes of a square grid.  Row b of the result is [CLS], prefix_ids (the same for every
        row, e.g. the ids of "a picture of"), lengths[b] predicted tokens, [SEP], [PAD] up to max_text_length (<= 64; [PAD] = id 0).
        lengths: an int (every row), an int tensor [B] (one per row), or a python list of C CANDIDATE lengths: every image is then
        decoded once per candidate (a batch of B*C rows) and the candidate with the highest score is returned -- Mask-Predict's
        length-candidate rule.  Each must satisfy 1 <= n <= max_text_length - 2 - len(prefix_ids).
        banned_ids (default: every id below first_word_id, the specials of bert-base-uncased) are never predicted.
        temperature / seed / top_k / top_p / min_p: as in sample_codes.  suppress_repeats: re-mask a token equal to its left neighbour
        first.  Tokenising a prefix and decoding ids to text stay with the caller.
        Returns (token_ids [B, L] int64, score [B] fp32 = mean log-probability of the predicted tokens under the last forward); with
        candidate lengths also the chosen length per image [B]; with return_intermediate also the list of token matrices after
        every step (all candidates: [B*C, L], image-major)."""
        temperature = Engine.check_temperature(temperature)
        trunc = _truncation_kw(top_k, top_p, min_p)
        if not self.task_mask_lm:
            raise RuntimeError("sample_caption_ids on a model built without task_mask_lm (no `cls` MLM head)")
        if (visual_feats is None) == (cluster_ids is None):
            raise ValueError("give the picture either as visual_feats or as cluster_ids")
        if cluster_ids is not None and self.vis_emb is None:
            raise RuntimeError("cluster_ids given but the model has no codebook: call set_visual_embedding(centroids) first")
        vis = visual_feats if cluster_ids is None else cluster_ids
        B, V = vis.shape[0], vis.shape[1]
        dev = vis.device
        L = int(max_text_length)
        prefix = [int(t) for t in (prefix_ids.tolist() if isinstance(prefix_ids, torch.Tensor) else (prefix_ids or ()))]
        P = len(prefix)
        cand = isinstance(lengths, (list, tuple))
        C = len(lengths) if cand else 1
        if cand:
            lens = torch.as_tensor(lengths, dtype=torch.int64).reshape(1, C).expand(B, C).reshape(-1)
        else:
            lens = torch.as_tensor(lengths, dtype=torch.int64).cpu().reshape(-1)
            lens = lens.expand(B) if lens.numel() == 1 else lens
        if L > Engine.CAPTION_MAX_L or L - 2 - P < 1:
            raise ValueError(f"max_text_length {max_text_length}: at most {Engine.CAPTION_MAX_L} and at least len(prefix_ids) + 3")
        if lens.numel() != B * C or int(lens.min()) < 1 or int(lens.max()) > L - 2 - P:
            raise ValueError(f"lengths {lengths!r}: ints with 1 <= n <= max_text_length - 2 - len(prefix_ids) = {L - 2 - P} "
                             "(an int, a tensor [B], or a list of candidate lengths)")
        if visual_pos is None:
            g = int(round(V ** 0.5))
            if g * g != V:
                raise ValueError(f"visual_pos is needed for {V} visual tokens (not a square grid)")
            idx = torch.arange(V)
            i, j = (idx // g).float(), (idx % g).float()                   # ref utils.box_position
            visual_pos = torch.stack([j / g, i / g, (j + 1) / g, (i + 1) / g], 1).unsqueeze(0).expand(B, -1, -1)
        if C > 1:
            vis = vis.repeat_interleave(C, 0)
            visual_pos = visual_pos.repeat_interleave(C, 0)
        # the token layout, on the host: [CLS] prefix [MASK] x n [SEP] [PAD] ...; packed-row list and offsets next to it (no round trip)
        pos = torch.arange(L).view(1, L)
        n = lens.view(-1, 1)
        ids = torch.zeros(B * C, L, dtype=torch.int64)
        ids[:, 0] = cls_token_id
        if P:
            ids[:, 1:P + 1] = torch.tensor(prefix, dtype=torch.int64)
        ids[(pos > P) & (pos < P + 1 + n)] = mask_token_id
        ids[pos.expand(B * C, L) == P + 1 + n] = sep_token_id
        att = pos < P + n + 2
        was_training = self.training
        self.eval()
        eng = self._step_engine(B * C, L, V)
        rows = att.reshape(-1).nonzero().reshape(-1)
        off = torch.cat([lens.new_zeros(1), (lens + P + 2).cumsum(0)])
        eng.set_inputs(ids.to(dev), att.to(dev), None, visual_pos.to(dev), cluster_ids=vis if cluster_ids is not None else None,
                       visual_feats=vis if cluster_ids is None else None, lang_rows=rows.to(dev), lang_off=off.to(dev))
        if banned_ids is None:
            banned_ids = torch.arange(min(int(first_word_id), self.config.vocab_size))
        steps = []
        kw = {} if temperature is None and not trunc else {"temperature": temperature, "seed": _sample_seed(seed), **trunc}
        tok, score, _ = eng.sample_words_nar(lens, n_steps, P, (lambda i: steps.append(eng.cap_tokens.clone())) if return_intermediate else None,
                                             suppress_repeats=suppress_repeats, mask_token_id=mask_token_id, banned_ids=banned_ids, **kw)
        self.train(was_training)
        tok, score = tok.clone(), score.clone()
        out = (tok, score)
        if cand:                                # the length-candidate rule: per image the candidate with the highest score (host arithmetic)
            best = score.view(B, C).argmax(1)
            pick = torch.arange(B, device=score.device) * C + best
            out = (tok[pick], score[pick], lens.to(score.device).view(B, C)[torch.arange(B, device=score.device), best])
        return out + (steps,) if return_intermediate else out

    @staticmethod
    def _grid_pos(grid_size, B, dev):
        """ref utils.box_position as [B, V, 4] on `dev`"""
        idx = torch.arange(grid_size * grid_size)
        i, j, g = (idx // grid_size).float(), (idx % grid_size).float(), float(grid_size)
        return torch.stack([j / g, i / g, (j + 1) / g, (i + 1) / g], 1).to(dev).unsqueeze(0).expand(B, -1, -1)

    def _inpaint(self, input_ids, init_codes, free_mask, n_steps, grid_size, mode, order, temperature, seed, top_k, top_p, min_p,
                 n_candidates, on_step=None):
        """the loop behind inpaint_codes / ImggenModel.inpaint_image: (code ids [B, V], code features [B, V, F], score [B], conf [B, V])
        of the best replica per image.  on_step(eng, i) sees all B * n_candidates rows (image-major)."""
        temperature = Engine.check_temperature(temperature)
        trunc = _truncation_kw(top_k, top_p, min_p)
        if self.vis_emb is None:
            raise RuntimeError("call set_visual_embedding(centroids) first")
        C = int(n_candidates)
        if C < 1:
            raise ValueError(f"n_candidates {n_candidates!r}: at least 1")
        if C > 1 and temperature is None and not trunc:
            raise ValueError("n_candidates > 1 needs a temperature or a truncation argument: greedy replicas would be identical")
        B, L = input_ids.shape
        V = grid_size * grid_size
        dev = input_ids.device
        init_codes, free_mask = torch.as_tensor(init_codes), torch.as_tensor(free_mask)
        for name, t in (("init_codes", init_codes), ("free_mask", free_mask)) + ((("order", torch.as_tensor(order)),) if order is not None else ()):
            if tuple(t.shape) != (B, V):
                raise ValueError(f"{name}: shape [B = {B}, V = {V}] (got {tuple(t.shape)})")
        if order is not None:
            order = torch.as_tensor(order)
        if C > 1:                                               # replicas: other rows b*V + v of the noise function, so other draws
            input_ids = input_ids.repeat_interleave(C, 0)
            init_codes, free_mask = init_codes.repeat_interleave(C, 0), free_mask.repeat_interleave(C, 0)
            order = None if order is None else order.repeat_interleave(C, 0)
        was_training = self.training
        self.eval()
        eng = self._step_engine(B * C, L, V)
        eng.set_inputs(input_ids, input_ids > 0, None, self._grid_pos(grid_size, B * C, dev),
                       cluster_ids=torch.zeros(B * C, V, dtype=torch.long, device=dev),
                       vis_mask=torch.ones(B * C, V, dtype=torch.bool, device=dev))
        kw = {} if temperature is None and not trunc else {"temperature": temperature, "seed": _sample_seed(seed), **trunc}
        hook = None if on_step is None else (lambda i: on_step(eng, i))
        cid, code, score, conf = eng.inpaint_codes(init_codes, free_mask, n_steps, mode, order, hook, **kw)
        self.train(was_training)
        cid, code, score, conf = cid.clone(), code.view(B * C, V, -1), score.clone(), conf.clone()
        if C > 1:                                               # per image the replica with the highest score (host arithmetic)
            pick = torch.arange(B, device=score.device) * C + score.view(B, C).argmax(1)
            cid, code, score, conf = cid[pick], code[pick], score[pick], conf[pick]
        return cid, code, score, conf

    @torch.no_grad()
    def inpaint_codes(self, input_ids, init_codes, free_mask, n_steps=4, grid_size=8, *, mode="nar", order=None, temperature=None,
                      seed=None, top_k=None, top_p=None, min_p=None, n_candidates=1):
        """In-painting: sample the grid cells that `free_mask` [B, V] marks (non-zero) around the given codes `init_codes` [B, V] (e.g.
        the cluster ids of a real image, xlxmert_amd.io) under the caption `input_ids` -- Engine.inpaint_codes.  mode "nar" (Mask-Predict,
        n_steps refinements), "confidence" / "tlbr" / "order" (one cell per image per step; n_steps=None = as many as the fullest
        mask needs; `order` [B, V] ints for "order").  temperature / seed / top_k / top_p / min_p: as in sample_codes.
        n_candidates = C > 1: every image is sampled C times (a batch of B*C rows, each with its own noise) and the replica with the
        highest score is returned; it needs a temperature or a truncation argument.
        Returns (code ids [B, V] int64, score [B] fp32: mean log-probability of the sampled cells, conf [B, V] fp32)."""
        cid, _, score, conf = self._inpaint(input_ids, init_codes, free_mask, n_steps, grid_size, mode, order, temperature, seed, top_k,
                                            top_p, min_p, n_candidates)
        return cid, score, conf

    def _step_engine(self, B, L, V):
        key = (B, L, V, self.training, "step")
        if self.bert._geom != key:
            self.bert._engine = Engine(self.config, self._store, self.bert._ops, B, L, V,
                                       need_lang=self._store.task != "vis_mask", train_dropout=self.training,
                                       residual_dtype=self.bert._residual_dtype)
            self.bert._geom = key
        self.bert._engine.sync_compute_weights()
        self.bert._advance_seed(self.bert._engine)
        return self.bert._engine


# ---------------------------------------------------------------------------------------------- VQA / GQA
class _VqaFn(torch.autograd.Function):
    """VQAModel.forward as one engine forward; backward takes d(logit) from whatever loss the caller applied
    (BCEWithLogitsLoss in the reference, tasks/vqa.py:187) and runs answer head + pooler + encoder backward."""

    @staticmethod
    def forward(ctx, model, anchor):
        eng = model.bert._engine
        logit = eng.vqa_forward()
        ctx.model = model
        return logit.clone()

    @staticmethod
    def backward(ctx, d_logit):
        eng = ctx.model.bert._engine
        ans = eng.answer
        ans.dlogit.zero_()
        ans.dlogit[:, :ans.A].copy_(d_logit)
        eng.zero_out_grads(eng.GA)
        cls_rows, d_cls = eng._cls_views(eng.GA)
        ans.bwd(cls_rows, d_cls)
        eng.encoder_backward(True)            # gradients accumulate into the flat buffer: call model.zero_grad() per step
        return None, None


class LxmertVisualAnswerHead(_Named):
    """HF:602-614; parameters `logit_fc.{0,2,3}.{weight,bias}` are views of the flat parameter buffer."""

    def __init__(self, store):
        super().__init__()
        self._bind(store, "answer_head", [n for n in store.names() if n.startswith("answer_head.")])


class VQAModel(nn.Module):
    """ref tasks/vqa_model.py:7-72 (also the GQA model, tasks/gqa_model.py): `.bert` + `.answer_head`, forward returns
    {'logit': [B, num_answers] fp32}.  Unlike the published class this one can be constructed (its ctor reads
    `config.num_answers` before setting it and calls `_init_weights` on a non-existent attribute)."""

    _task = "vqa"

    def __init__(self, config: XLxmertConfig, num_answers, num_clusters=-1, device=None, dtype=torch.bfloat16, residual_dtype=None):
        """residual_dtype: see LxmertModel (storage type of the residual stream: "bf16" default, "fp32")."""
        super().__init__()
        self.config, self.num_answers = config, num_answers
        dev = torch.device(device if device is not None else "cuda")
        self._store = ParamStore(config, dev, dtype, task=self._task, num_answers=num_answers)
        self.bert = LxmertModel(config, store=self._store, device=dev, residual_dtype=residual_dtype)
        self.answer_head = LxmertVisualAnswerHead(self._store)
        self._anchor = torch.zeros(1, device=dev, requires_grad=True)
        from .trainer import init_reference_weights
        init_reference_weights(self._store, seed=0)

    def zero_grad(self, set_to_none=False):
        self._store.grad.zero_()
        for name, p_ in self.named_parameters():
            if p_.grad is None and name in self._store.index:
                p_.grad = self._store.gview(name)

    def state_dict(self, *args, prefix="", **kwargs):
        keep = ("bert.", "answer_head.")
        return OrderedDict((prefix + k, v.detach()) for k, v in self._store.named_state().items() if k.startswith(keep))

    def load_state_dict(self, state_dict, strict=False):
        """reference layout, with or without the DDP `module.` prefix; a pretraining checkpoint (no answer head: the
        reference's load_lxmert_qa path, tasks/vqa.py:55-62) loads the encoder and leaves the head at its init."""
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        missing = self._store.load_named(sd, strict=False)
        missing = [k for k in missing if k.startswith(("bert.", "answer_head."))]
        if strict and missing:
            raise KeyError(f"missing keys: {missing[:8]}...")
        return missing, [k for k in sd if k not in self._store.index]

    def forward(self, input_ids=None, visual_feats=None, visual_pos=None, attention_mask=None, visual_attention_mask=None,
                token_type_ids=None, inputs_embeds=None, return_dict=True):
        if inputs_embeds is not None and inputs_embeds.requires_grad:
            raise NotImplementedError("d(inputs_embeds) through the task wrappers: use .bert directly (no reference caller does)")
        B, L = input_ids.shape if input_ids is not None else inputs_embeds.shape[:-1]
        V = visual_feats.shape[1]
        key = (B, L, V, self.training, self._task)
        if self.bert._geom != key:
            self.bert._engine = Engine(self.config, self._store, self.bert._ops, B, L, V, need_lang=True,
                                       train_dropout=self.training, residual_dtype=self.bert._residual_dtype)
            self.bert._geom = key
        eng = self.bert._engine
        eng.sync_compute_weights()
        self.bert._advance_seed(eng)
        eng.set_inputs(input_ids, attention_mask, token_type_ids, visual_pos, visual_feats=visual_feats,
                       visual_attention_mask=visual_attention_mask, inputs_embeds=inputs_embeds)
        logit = _VqaFn.apply(self, self._anchor) if torch.is_grad_enabled() else eng.vqa_forward().clone()
        return {"logit": logit}


    @torch.no_grad()
    def predict(self, input_ids=None, visual_feats=None, visual_pos=None, attention_mask=None, visual_attention_mask=None,
                token_type_ids=None, inputs_embeds=None):
        """The fine-tune drivers' predict / evaluate step (ref tasks/vqa.py:259-311, tasks/gqa.py, tasks/nlvr2.py): forward's
        arguments (NLVR2: the [P, 2, V, F] pairs), eval() semantics, returns (score, pred) = logit.max(1) as device tensors -- the
        answer head's logits go through xl_score_rows, no host synchronisation.  The training flag is restored afterwards."""
        if visual_feats.dim() == 4:                     # NLVR2 pairs (ref tasks/nlvr2_model.py:64-66)
            visual_feats, visual_pos = visual_feats.reshape(-1, *visual_feats.shape[2:]), visual_pos.reshape(-1, *visual_pos.shape[2:])
        was_training = self.training
        self.eval()
        try:
            B, L = input_ids.shape if input_ids is not None else inputs_embeds.shape[:-1]
            key = (B, L, visual_feats.shape[1], self.training, self._task)
            if self.bert._geom != key:
                self.bert._engine = Engine(self.config, self._store, self.bert._ops, B, L, visual_feats.shape[1], need_lang=True,
                                           train_dropout=False, residual_dtype=self.bert._residual_dtype)
                self.bert._geom = key
            eng = self.bert._engine
            eng.sync_compute_weights()
            eng.set_inputs(input_ids, attention_mask, token_type_ids, visual_pos, visual_feats=visual_feats,
                           visual_attention_mask=visual_attention_mask, inputs_embeds=inputs_embeds)
            ans = eng.answer
            p_saved = (eng.p_hid, eng.p_attn)
            eng.p_hid = eng.p_attn = 0.0
            try:
                eng.vqa_forward()
            finally:
                eng.p_hid, eng.p_attn = p_saved
            pred = torch.zeros(ans.Bh, dtype=torch.int32, device=ans.logit.device)
            score = torch.zeros(ans.Bh, dtype=torch.float32, device=ans.logit.device)
            self.bert._ops.score_rows(ans.logit, ans.Bh, ans.A, ans.A, None, None, pred, score, None)
            return score, pred.long()
        finally:
            self.train(was_training)


class GQAModel(VQAModel):
    """ref tasks/gqa_model.py:7-72: the same module as VQAModel under the name the GQA driver imports (tasks/gqa.py:70,150:
    `.bert` + `.answer_head`, BCEWithLogitsLoss on the soft targets, forward returns {'logit': [B, num_answers]})."""


class NLVR2Model(VQAModel):
    """ref tasks/nlvr2_model.py:7-93: `.bert` + `.answer_head`; forward takes visual_feats [P, 2, V, F], visual_pos
    [P, 2, V, 4] and input_ids [2P, L] (every statement repeated for its two images), flattens the pairs, and feeds
    pooled_output viewed as [P, 2d] to the head; returns {'logit': [P, 2] fp32}.  The published class cannot run (its ctor
    builds `logit_fc` with a d-wide input, its forward calls an undefined `answer_head` on the 2d-wide vector); this one has
    the head that forward needs -- Linear(2d, 2d) -> GeLU -> LayerNorm(2d) -> Linear(2d, 2) -- under `.answer_head`."""
    _task = "nlvr2"

    def __init__(self, config: XLxmertConfig, num_answers=2, num_clusters=-1, device=None, dtype=torch.bfloat16, residual_dtype=None):
        super().__init__(config, num_answers, num_clusters, device, dtype, residual_dtype=residual_dtype)

    def forward(self, input_ids=None, visual_feats=None, visual_pos=None, attention_mask=None, visual_attention_mask=None,
                token_type_ids=None, inputs_embeds=None, return_dict=True):
        P, n_images, V, Fd = visual_feats.shape
        assert n_images == 2                                                             # ref :64
        return super().forward(input_ids, visual_feats.reshape(P * 2, V, Fd), visual_pos.reshape(P * 2, V, -1), attention_mask,
                               visual_attention_mask, token_type_ids, inputs_embeds, return_dict)


# ---------------------------------------------------------------------------------------------- image generation
class ImggenModel(XLxmertForPretraining):
    """ref tasks/imggen_model.py:11-257: `.bert`, `.obj_predict_head`, `.mask_feat`, `.vis_emb`, `set_visual_embedding`,
    `set_image_generator(G)`, `sample_image_NAR` (Mask-Predict, :169-257) and `sample_image_AR` (one grid position per step:
    position_random / position_TLBR / position_confidence, :49-167).  The loops run on the device without a host round trip
    (Engine.sample_codes_nar / sample_codes_ar); tokenisation in front and the frozen GAN generator `G` + denorm behind stay
    stock PyTorch, as in the reference.

    `sentences`: a list of strings (needs `tokenizer`: any callable with LxmertTokenizer's call signature -- the reference
    downloads 'unc-nlp/lxmert-base-uncased' in its constructor, :26, which an offline machine cannot) or, beyond the reference, an
    int64 tensor of input ids [B, L] (0 = [PAD]).  grid_size / the code width follow the config (the reference hardcodes 8 / 2048)."""

    def __init__(self, config: XLxmertConfig, args=None, num_clusters=10000, device=None, dtype=torch.bfloat16, tokenizer=None,
                 grid_size=8):
        import copy
        config = copy.copy(config)
        config.task_mask_lm = config.task_matched = config.task_qa = False          # the published class has the codebook head only
        config.task_obj_predict = True
        super().__init__(config, num_clusters=num_clusters, device=device, dtype=dtype)
        self.args, self.tokenizer, self.grid_size = args, tokenizer, grid_size
        self.G = None

    def set_image_generator(self, generator):
        """ref :41-42: any callable [B, code_dim, g, g] fp32 -> image batch (image_generator.src.layers.Generator in the reference)"""
        self.G = generator

    @staticmethod
    def denorm(x):
        """(-1, 1) => (0, 1)   (ref :44-47)"""
        return ((x + 1) / 2).clamp(0, 1)

    def _input_ids(self, sentences, max_text_length):
        if torch.is_tensor(sentences):
            return sentences.to(self._store.device)
        if self.tokenizer is None:
            raise RuntimeError("ImggenModel got sentences but no tokenizer: pass tokenizer=LxmertTokenizer.from_pretrained(...) "
                               "(the reference downloads one in its constructor) or hand over input ids")
        ids = self.tokenizer(sentences, max_length=max_text_length, truncation=True, return_tensors="pt").input_ids      # ref :56-58
        return ids.to(self._store.device)

    def _prepare(self, input_ids):
        import numpy as np
        if self.vis_emb is None:
            raise RuntimeError("call set_visual_embedding(centroids) first")
        self.eval()                                                 # ref :54, :180
        g = self.grid_size
        B, L = input_ids.shape
        V = g * g
        eng = self._step_engine(B, L, V)
        pos = np.zeros((V, 4), np.float32)                          # ref utils.box_position
        for i in range(g):
            for j in range(g):
                pos[i * g + j] = [j / g, i / g, (j + 1) / g, (i + 1) / g]
        dev = input_ids.device
        eng.set_inputs(input_ids, input_ids > 0, None, torch.from_numpy(pos).to(dev).unsqueeze(0).expand(B, -1, -1),
                       cluster_ids=torch.zeros(B, V, dtype=torch.long, device=dev), vis_mask=torch.ones(B, V, dtype=torch.bool, device=dev))
        return eng, B, V

    def _image(self, code, B):
        """code [B*V, F] -> G(code as [B, F, g, g]) -> denorm -> host (ref :160-165, :250-256)"""
        if self.G is None:
            raise RuntimeError("call set_image_generator(G) first (ref tasks/imggen_model.py:41)")
        from .generator import Generator
        if isinstance(self.G, Generator):           # the native generator takes the code rows as they are (channels last, engine dtype)
            return self.denorm(self.G.render_codes(code, B)).cpu()
        g = self.grid_size
        x = code.view(B, g * g, -1).permute(0, 2, 1).reshape(B, -1, g, g).float()
        return self.denorm(self.G(x)).cpu()

    @torch.no_grad()
    def rank_images(self, sentences, cluster_ids, max_text_length=20, *, top_k=None, chunk_pairs=None):
        """Rank M images, given as grid codes `cluster_ids` [M, V] (e.g. what the samplers return), for every one of the N sentences by
        the model's own matching score: XLxmertForPretraining.match_scores with the tokenisation of the samplers (attention mask =
        input ids > 0).  Returns its dict (margin, prob, and with top_k the lists)."""
        ids = self._input_ids(sentences, max_text_length)
        return self.match_scores(ids, ids > 0, None, cluster_ids=cluster_ids, top_k=top_k, chunk_pairs=chunk_pairs)

    @torch.no_grad()
    def sample_image_NAR(self, sentences, max_text_length=20, n_steps=None, return_intermediate=False, *, temperature=None,
                         sample_seed=None, top_k=None, top_p=None, min_p=None):
        """ref :169-257.  n_steps=None -> grid_size ** 2 (ref :191-192).  temperature (beyond the reference; None = its greedy
        choice): every position draws its code from softmax(logits / temperature) -- different, reproducible images per caption;
        sample_seed=None takes a seed from torch's default CPU generator.  top_k / top_p / min_p (any given; temperature None then
        means 1): the draw keeps to the top_k most probable codes, the shortest prefix of mass top_p, the codes of at least min_p
        times the mode's probability (Engine.check_truncation)."""
        temperature = Engine.check_temperature(temperature)
        kw = _sampling_kw(temperature, sample_seed, top_k, top_p, min_p)
        eng, B, V = self._prepare(self._input_ids(sentences, max_text_length))
        n_steps = V if n_steps is None else n_steps
        imgs = []
        hook = (lambda i: imgs.append(self._image(eng.materialise_codes(), B))) if return_intermediate else None
        _, code, _ = eng.sample_codes_nar(n_steps, on_step=hook, **kw)
        self.code_ids = eng.cid.clone()                             # the chosen codebook ids [B, V] (beyond the reference: handy)
        return imgs if return_intermediate else self._image(code, B)

    @torch.no_grad()
    def sample_image_AR(self, sentences, max_text_length=20, position_random=False, position_TLBR=False, position_confidence=True,
                        n_steps=None, seed=None, return_intermediate=False, *, temperature=None, sample_seed=None, top_k=None,
                        top_p=None, min_p=None):
        """ref :49-167: the three position policies with the reference's precedence (random, else TLBR, else confidence) and its
        host-side order for `position_random` (random.Random(seed).shuffle, extended for n_steps > grid ** 2, :77-89).
        temperature / sample_seed / top_k / top_p / min_p: as in sample_image_NAR (`seed` keeps meaning the position order)."""
        import random
        temperature = Engine.check_temperature(temperature)
        kw = _sampling_kw(temperature, sample_seed, top_k, top_p, min_p)
        eng, B, V = self._prepare(self._input_ids(sentences, max_text_length))
        n_steps = V if n_steps is None else n_steps
        positions = None
        if position_random:
            mode = "random"
            positions = list(range(V))
            (random.Random(seed) if seed is not None else random).shuffle(positions)
            if n_steps > V:
                extra = list(range(n_steps - V))
                (random.Random(seed) if seed is not None else random).shuffle(extra)
                positions = extra + positions
        elif position_TLBR:
            mode = "tlbr"
        elif position_confidence:
            mode = "confidence"
        else:
            raise ValueError("sample_image_AR: one of position_random / position_TLBR / position_confidence must be set")
        imgs = []
        hook = (lambda i: imgs.append(self._image(eng.materialise_codes(masked=True), B))) if return_intermediate else None
        _, code, _ = eng.sample_codes_ar(n_steps, mode, positions=positions, on_step=hook, **kw)
        self.code_ids = eng.cid.clone()
        return imgs if return_intermediate else self._image(code, B)

    @torch.no_grad()
    def inpaint_image(self, sentences, init_codes, free_mask, max_text_length=20, n_steps=None, mode="nar", return_intermediate=False,
                      *, order=None, temperature=None, sample_seed=None, top_k=None, top_p=None, min_p=None, n_candidates=1):
        """In-paint an image (beyond the reference): the cells that free_mask [B, V] marks are sampled around the given codes init_codes
        [B, V] under the caption (XLxmertForPretraining.inpaint_codes; n_steps=None = the largest free count), and the generator set
        by set_image_generator renders the result.  return_intermediate: the list of image batches after every step (all
        B * n_candidates rows, image-major; cells still masked hold mask_feat) -- the last entry of the list is NOT reduced to the
        best replica, the plain return value is.  self.code_ids / inpaint_score / inpaint_conf keep the chosen ids, scores and
        confidences."""
        ids = self._input_ids(sentences, max_text_length)
        if self.G is None:
            raise RuntimeError("call set_image_generator(G) first (ref tasks/imggen_model.py:41)")
        imgs = []
        hook = (lambda eng, i: imgs.append(self._image(eng.materialise_codes(masked=mode != "nar"), eng.B))) if return_intermediate else None
        cid, code, score, conf = self._inpaint(ids, init_codes, free_mask, n_steps, self.grid_size, mode, order, temperature, sample_seed,
                                               top_k, top_p, min_p, n_candidates, hook)
        self.code_ids, self.inpaint_score, self.inpaint_conf = cid, score, conf
        return imgs if return_intermediate else self._image(code.reshape(-1, code.shape[-1]), cid.shape[0])
