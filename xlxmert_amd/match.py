"""Caption-image matching: every one of N captions scored against every one of M images by the `matched` head (seq_relationship on
pooled_output, label 1 = caption and image belong together, ref pretrain/lxmert_data.py:345-361), and ranked, on the device.

The encoder's structure does the saving.  The 9 language layers never see the picture, the feature encoder and the 5 visual layers
never see the text -- the exactness argument of Engine._reuse_lang_stack / _reuse_vis_stack -- so the language stack runs ONCE at
batch N and the visual stack ONCE at batch M; only the 5 cross layers, the pooler and the 2-way head depend on the pair.  They run
on a chunk engine of B_c pair slots whose X[0] xl_pair_expand fills from the two stacks' outputs (pair p = n*M + m, caption-major),
chunk after chunk without a host synchronisation; xl_match_rank scatters each chunk's logits into margin / prob [N, M] and, after
the last chunk, ranks both directions (include/xlxmert_hip.h states both kernels' rules; DESIGN.md "N3 notes").

All engines share one ParamStore and one HipOps: no parameter is copied.  Gradients, parameters, optimizer state, step seeds, an
open accumulation window and recorded launch plans are not touched (forward only, engines of the runner's own)."""
import torch

from .engine import Engine, _f, _h

RECALL_AT = (1, 5, 10)
MAX_SIDE, MAX_K = 4096, 32          # xl_match_rank's limits


class MatchRunner:
    def __init__(self, cfg, store, ops, N, M, L, V, chunk_pairs=None, train_dropout=False, pack_lang=None, residual_dtype=None):
        lh_ok = getattr(store, "task", "vis_mask") in ("matched", "all") and "cls.seq_relationship.weight" in store.index
        assert lh_ok, "match_scores needs the matched head: a store with task 'matched' or 'all' (cls.seq_relationship.*)"
        if not (1 <= N <= MAX_SIDE and 1 <= M <= MAX_SIDE):
            raise ValueError(f"N = {N} captions, M = {M} images: 1..{MAX_SIDE} each")
        B_c = min(N * M, 256) if chunk_pairs is None else int(chunk_pairs)
        if not 1 <= B_c <= N * M:
            raise ValueError(f"chunk_pairs {chunk_pairs!r}: 1..N*M = {N * M}")
        self.cfg, self.store, self.ops = cfg, store, ops
        self.N, self.M, self.L, self.V, self.B_c = N, M, L, V, B_c
        kw = dict(need_lang=True, train_dropout=train_dropout, pack_lang=pack_lang, residual_dtype=residual_dtype)
        self.lang_eng = Engine(cfg, store, ops, N, L, V, **kw)
        self.vis_eng = self.lang_eng if M == N else Engine(cfg, store, ops, M, L, V, **kw)
        self.chunk_eng = Engine(cfg, store, ops, B_c, L, V, **kw)
        assert self.chunk_eng.lang_heads is not None and self.chunk_eng.lang_heads.has_rel
        dev = store.device
        self.dev = dev
        self.margin = torch.zeros(N, M, dtype=torch.float32, device=dev)
        self.prob = torch.zeros(N, M, dtype=torch.float32, device=dev)
        self.dense_off = torch.arange(N + 1, dtype=torch.int32, device=dev) * L       # offsets of a dense [N*L, d] language source
        self.dense_len = torch.zeros(N, dtype=torch.int32, device=dev)                # ... and its captions' lengths
        self._bufs = {}

    def sync_compute_weights(self):
        """Engine.sync_compute_weights (the store's compute copy from its fp32 master): the caller's business, as for an engine"""
        self.lang_eng.sync_compute_weights()

    def _buf(self, name, shape, dtype):
        key = (name, tuple(shape), dtype)
        if key not in self._bufs:
            self._bufs[key] = torch.zeros(*shape, dtype=dtype, device=self.dev)
        return self._bufs[key]

    def _lengths(self, attention_mask):
        """per-caption token counts on the host (the one round trip of a call: they size every chunk's launches).  The packed
        chunk layout addresses a caption's rows by position, so the mask must be a prefix mask, as every tokenizer produces."""
        N, L = self.N, self.L
        if attention_mask is None:
            return [L] * N
        m = (attention_mask.reshape(N, L) != 0).cpu()
        lens = m.sum(1)
        if int(lens.min()) < 1:
            raise ValueError("attention_mask: a caption without a single real token")
        if not bool((m == (torch.arange(L)[None, :] < lens[:, None])).all()):
            raise ValueError("attention_mask: match_scores needs prefix masks (real tokens first, [PAD] after)")
        return [int(x) for x in lens.tolist()]

    def _stage(self, input_ids, attention_mask, token_type_ids, visual_feats, cluster_ids, visual_pos, lens):
        """set_inputs of the two stack engines: the captions on one, the pictures on the other (one engine when N == M); the side
        an engine does not run gets placeholders that nothing reads"""
        N, M, L, V = self.N, self.M, self.L, self.V
        le, ve = self.lang_eng, self.vis_eng
        lang_kw = {}
        if attention_mask is not None and le.pack_lang:             # row list and offsets from the host lengths: no second round trip
            off = [0]
            for n in lens:
                off.append(off[-1] + n)
            rows = [n * L + l for n in range(N) for l in range(lens[n])]
            lang_kw = dict(lang_rows=torch.tensor(rows, dtype=torch.int32, device=self.dev),
                           lang_off=torch.tensor(off, dtype=torch.int32, device=self.dev))
        vis_kw = dict(cluster_ids=cluster_ids) if cluster_ids is not None else dict(visual_feats=visual_feats)
        if le is ve:
            le.set_inputs(input_ids, attention_mask, token_type_ids, visual_pos, **vis_kw, **lang_kw)
            return
        le.set_inputs(input_ids, attention_mask, token_type_ids, self._buf("pos0", (N, V, le.P), torch.float32),
                      visual_feats=self._buf("feat0", (N, V, le.F), le.cdtype), **lang_kw)
        ve.set_inputs(self._buf("ids0", (M, L), torch.int64), None, None, visual_pos, **vis_kw)

    def _chunk_rows(self, lens, start, count):
        """packed language rows of the chunk [start, start+count): the closed form of xl_pair_expand on the host's lengths"""
        M, B_c = self.M, self.B_c
        off = [0]
        for n in lens:
            off.append(off[-1] + n)

        def first(p):
            return M * off[p // M] + (p % M) * lens[p // M]
        last = start + count - 1
        return first(last) + lens[last // M] * (B_c - (count - 1)) - first(start)

    def run(self, input_ids, attention_mask=None, token_type_ids=None, visual_feats=None, cluster_ids=None, visual_pos=None, *,
            top_k=None, image_of_caption=None, caption_of_image=None):
        """-> {margin, prob [N, M] fp32; topk_images [N, k], topk_captions [M, k] int32 (top_k); rank_t2i [N], rank_i2t [M] int32 and
        recall_hits fp32 [2, 4] = per direction (captions -> images, images -> captions) the queries with rank < 1, 5, 10 and the
        queries that have a target (targets)}: device tensors, valid until the next call; no host synchronisation after staging."""
        N, M, L, V, B_c = self.N, self.M, self.L, self.V, self.B_c
        ops, le, ve, ce = self.ops, self.lang_eng, self.vis_eng, self.chunk_eng
        assert tuple(input_ids.shape) == (N, L), (input_ids.shape, (N, L))
        if (visual_feats is None) == (cluster_ids is None):
            raise ValueError("give the pictures either as visual_feats or as cluster_ids")
        vis_in = visual_feats if cluster_ids is None else cluster_ids
        assert vis_in.shape[0] == M and vis_in.shape[1] == V, (vis_in.shape, (M, V))
        k = 0
        if top_k is not None:
            k = int(top_k)
            if not 1 <= k <= min(MAX_K, N, M):
                raise ValueError(f"top_k {top_k!r}: 1..min({MAX_K}, N, M) = {min(MAX_K, N, M)}")
        out = {"margin": self.margin, "prob": self.prob}
        rank_kw = {}
        if k:
            out["topk_images"] = rank_kw["topk_images"] = self._buf("topk_i", (N, k), torch.int32)
            out["topk_captions"] = rank_kw["topk_captions"] = self._buf("topk_c", (M, k), torch.int32)
        for name, tgt, n, rname in (("image_of_caption", image_of_caption, N, "rank_t2i"), ("caption_of_image", caption_of_image, M, "rank_i2t")):
            if tgt is not None:
                assert tgt.numel() == n, (name, tgt.shape, n)
                t = self._buf(name, (n,), torch.int32)
                t.copy_(tgt.reshape(-1), non_blocking=True)
                rank_kw[name] = t
                out[rname] = rank_kw[rname] = self._buf(rname, (n,), torch.int32)
        lens = self._lengths(attention_mask)
        engines = {id(e): e for e in (le, ve, ce)}.values()
        saved = [(e, e.p_hid, e.p_attn) for e in engines]
        for e in engines:               # dropout is off for the call whatever the engines were built with (Engine.evaluate_task)
            e.p_hid = e.p_attn = 0.0
        try:
            self._stage(input_ids, attention_mask, token_type_ids, visual_feats, cluster_ids, visual_pos, lens)
            with Engine._Seeded(le):
                le.fork()
                with le.lang_stream():
                    le._language_stack_forward()
                ve._visual_stack_forward(self.cfg.r_layers)
                le.join()
            self._pairs(lens, k, rank_kw)
        finally:
            for e, ph, pa in saved:
                e.p_hid, e.p_attn = ph, pa
        if "rank_t2i" in out or "rank_i2t" in out:
            hits = self._buf("recall_hits", (2, 4), torch.float32)
            hits.zero_()
            for i, rname in enumerate(("rank_t2i", "rank_i2t")):
                if rname in out:
                    r = out[rname]
                    has = r >= 0
                    hits[i] = torch.stack([(has & (r < kk)).sum() for kk in RECALL_AT] + [has.sum()]).float()
            out["recall_hits"] = hits
        return out

    def _pairs(self, lens, k, rank_kw):
        """the chunk loop: expand, cross layers + pooler, 2-way head, scatter; the rank stage rides on the last chunk's call"""
        N, M, L, V, B_c = self.N, self.M, self.L, self.V, self.B_c
        ops, le, ve, ce = self.ops, self.lang_eng, self.vis_eng, self.chunk_eng
        d = ce.d
        packed = le.packed
        lang_off = le.loff if packed else self.dense_off
        if not packed:
            self.dense_len.copy_(torch.tensor(lens, dtype=torch.int32), non_blocking=True)
        src_v, src_l = ve.vr(ve.X[0]), le.lr(le.X[0])
        X0 = ce.X[0]
        two = ce.res32                          # fp32 stream: the cross layers read the fp32 value AND its bf16 rounding
        lh = ce.lang_heads
        want_rank = bool(k) or bool(rank_kw)
        ce._x0_given = True
        try:
            for start in range(0, N * M, B_c):
                count = min(B_c, N * M - start)
                rows = self._chunk_rows(lens, start, count) if packed else B_c * L
                rows_pad = min(ce.MLc, (rows + ce.ROW_PAD - 1) // ce.ROW_PAD * ce.ROW_PAD) if packed else rows
                ce.packed, ce.ML = packed, rows_pad
                ops.pair_expand(_f(src_v), _f(src_l), lang_off, _f(X0), ce.loff, ce.lrows, ce.kmask, N, M, V, L, d, start, count, B_c,
                                packed, le.ML, rows, rows_pad, vis2=_h(src_v) if two else None, lang2=_h(src_l) if two else None,
                                x0_2=_h(X0) if two else None, lang_len=None if packed else self.dense_len)
                ce.encoder_forward(want_pooled=True)
                lh.rel_fwd(ce.pooled)
                final = start + count == N * M
                ops.match_rank(lh.rel, start, count, self.margin, self.prob, N, M, rank_stage=final and want_rank, k=k,
                               **(rank_kw if final else {}))
        finally:
            ce._x0_given = False
