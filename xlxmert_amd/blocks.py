"""The encoder's sub-blocks (self-attention, feed-forward and cross-attention layers of LxmertEncoder, HF:304-449), forward and hand-derived
backward, and the residual-stream value pair of the fp32-stream mode.  Streams, scratch and the weight-gradient schedule are Engine's."""
import torch

from .ops import EPI_GELU_DG, EPI_MULAUX, EPI_RESIDUAL, GemmCall


class _Res:
    """A residual-stream value of the fp32-stream mode (Engine residual_dtype="fp32"): `f` the fp32 value that travels along
    the residual path, `h` its bf16 rounding, which the contractions read as their operand.  Row slices keep the pair."""
    __slots__ = ("f", "h")

    def __init__(self, f, h):
        self.f, self.h = f, h

    def __getitem__(self, s):
        return _Res(self.f[s], self.h[s])


def _h(x):
    """what a contraction reads of a stream value (the tensor itself in the bf16-stream mode)"""
    return x.h if isinstance(x, _Res) else x


def _f(x):
    """what the residual path reads of a stream value"""
    return x.f if isinstance(x, _Res) else x


class _Att:
    """LxmertAttention + LxmertAttentionOutput parameters (fused q/k/v views)."""

    def __init__(self, eng, prefix, self_name):
        st = eng.store
        qkv_w = [f"{prefix}.{self_name}.{n}.weight" for n in ("query", "key", "value")]
        qkv_b = [f"{prefix}.{self_name}.{n}.bias" for n in ("query", "key", "value")]
        self.wqkv, self.gwqkv = st.fused(qkv_w, st.compute), st.fused(qkv_w, st.grad)
        self.bqkv, self.gbqkv = st.fused(qkv_b, st.master), st.fused(qkv_b, st.grad)
        o = f"{prefix}.output"
        self.wo, self.gwo = st.cview(o + ".dense.weight"), st.gview(o + ".dense.weight")
        self.bo, self.gbo = st.view(o + ".dense.bias"), st.gview(o + ".dense.bias")
        self.g, self.gg = st.view(o + ".LayerNorm.weight"), st.gview(o + ".LayerNorm.weight")
        self.b, self.gb = st.view(o + ".LayerNorm.bias"), st.gview(o + ".LayerNorm.bias")


class SelfAttBlock:
    """LxmertSelfAttentionLayer (HF:304-316): y = LN(dense(attn(x,x,mask)) + x).  `masked` = language rows (key padding mask, or
    -- packed language rows -- per-example row offsets instead: engine.Engine pack_lang)."""

    def __init__(self, eng, prefix, n_tok, masked, tag):
        self.e, self.n, self.masked, self.tag = eng, n_tok, masked, tag
        self.p = _Att(eng, prefix, "self")
        Mc = eng.MLc if masked else eng.MV          # row capacity (the active row count of a packed language side varies per batch)
        d = eng.d
        self.qkv = eng.act(Mc, 3 * d)
        self.ctx = eng.act(Mc, d)
        self.z = eng.zact(Mc, d)
        self.lse = eng.f32(eng.B * eng.H * n_tok)
        self.keep = eng.keep_bits(n_tok, n_tok)
        self.mean, self.rstd = eng.f32(Mc), eng.f32(Mc)
        self.site = eng.new_site(2)

    @property
    def M(self):
        return self.e.ML if self.masked else self.e.MV

    def _att_args(self):
        """(key mask, packed-row keyword arguments) of this block's attention core"""
        e = self.e
        if not self.masked:
            return e.vkmask, {}
        if e.packed:
            return None, dict(q_off=e.loff, k_off=e.loff, q_pad=e.ML, k_pad=e.ML)
        return e.kmask, {}

    def fwd(self, x, y):
        self.e.run_steps(self.fwd_steps(x, y))

    def fwd_steps(self, x, y):
        """the forward as a generator: every dense contraction is YIELDED (ops.GemmCall) instead of launched, everything else is
        issued as the generator advances -- Engine.run_steps launches each yielded call, Engine.run_pair advances a visual and a
        language block of this class in lock step and launches their contractions two at a time (xl_gemm_pair)."""
        e, p, d, M = self.e, self.p, self.e.d, self.M
        ops, tag = e.ops, self.tag
        qkv, ctx, z = self.qkv[:M], self.ctx[:M], self.z[:M]
        yield GemmCall(_h(x), p.wqkv, qkv, p.bqkv, None, None, M, 3 * d, d, d, d, 3 * d, tag=tag)
        km, vl = self._att_args()
        ops.block = tag
        ops.sdpa_fwd(qkv, qkv[:, d:], qkv[:, 2 * d:], km, ctx, self.lse, e.B, e.H, self.n, self.n,
                     e.dh, 3 * d, 3 * d, 3 * d, d, e.scale, e.p_attn, e.seed(self.site), keep_bits=e.kb(self.keep), **vl)
        yield GemmCall(ctx, p.wo, z, p.bo, _f(x), None, M, d, d, d, d, d, ldr=d, epilogue=EPI_RESIDUAL,
                       p_drop=e.p_hid, seed=e.seed(self.site + 1), tag=tag, **e.rkw)
        ops.block = tag
        e.ln_fwd(z, p.g, p.b, y, self.mean, self.rstd, M, d)
        self.x = x

    def probs(self):
        """attention probabilities [B, H, n, n] fp32 of the last forward (after dropout, as HF returns them)"""
        e, d, M = self.e, self.e.d, self.M
        qkv = self.qkv[:M]
        out = torch.zeros(e.B, e.H, self.n, self.n, dtype=torch.float32, device=e.dev)
        km, vl = self._att_args()
        vl = {k: v for k, v in vl.items() if k in ("q_off", "k_off")}
        e.ops.attn_probs(qkv, qkv[:, d:], km, self.lse, out, e.B, e.H, self.n, self.n, e.dh, 3 * d, 3 * d, e.scale, e.p_attn,
                         e.seed(self.site), **vl)
        return out

    def bwd(self, dy, dx):
        self.e.run_steps(self.bwd_steps(dy, dx))

    def bwd_steps(self, dy, dx):
        e, p, d, M = self.e, self.p, self.e.d, self.M
        ops, tag = e.ops, self.tag
        ops.block = tag
        e.wgrad_sync()                  # the previous block's weight-gradient GEMMs still read the shared scratch
        qkv, ctx, z = self.qkv[:M], self.ctx[:M], self.z[:M]
        dz = e.tmp("dz", M, d, res=True)
        dzm = e.ln_bwd_dense(dy, z, p.g, self.mean, self.rstd, dz, p.gg, p.gb, p.gbo, M, d, self.site + 1)
        e.wgrad_defer(dzm, ctx, p.gwo, d, d, M, d, d, d)
        dctx = e.tmp("dctx", M, d)
        yield GemmCall(dzm, p.wo, dctx, None, None, None, M, d, d, d, d, d, a_kmajor=1, b_kmajor=0, tag=tag)
        dqkv = e.tmp("dqkv", M, 3 * d)
        km, vl = self._att_args()
        ops.block = tag
        ops.sdpa_bwd(qkv, qkv[:, d:], qkv[:, 2 * d:], km, dctx, self.lse, dqkv, dqkv[:, d:],
                     dqkv[:, 2 * d:], e.B, e.H, self.n, self.n, e.dh, 3 * d, 3 * d, 3 * d, d, 3 * d, 3 * d, 3 * d,
                     e.scale, e.p_attn, e.seed(self.site), bias_grad=p.gbqkv, ws=e.ws, keep_bits=e.kb(self.keep), **vl)      # + d(b_q | b_k | b_v)
        e.wgrad_defer(dqkv, _h(self.x), p.gwqkv, 3 * d, d, M, 3 * d, d, d)
        e.wgrad_flush(pair=True)        # this layer's four weight gradients: launched together with the next layer's
        yield GemmCall(dqkv, p.wqkv, dx, None, dz, None, M, d, 3 * d, 3 * d, d, d, ldr=d, a_kmajor=1, b_kmajor=0,
                       epilogue=EPI_RESIDUAL, tag=tag, **e.rkw)


class FFNBlock:
    """LxmertIntermediate + LxmertOutput (HF:325-342): y = LN(W2 gelu(W1 x + b1) + b2 + x).  `lang`: language rows (their
    active count follows the batch when the language rows are packed)."""

    def __init__(self, eng, p_inter, p_out, lang, tag):
        self.e, self.lang, self.tag = eng, lang, tag
        st = eng.store
        self.w1, self.gw1 = st.cview(p_inter + ".dense.weight"), st.gview(p_inter + ".dense.weight")
        self.b1, self.gb1 = st.view(p_inter + ".dense.bias"), st.gview(p_inter + ".dense.bias")
        self.w2, self.gw2 = st.cview(p_out + ".dense.weight"), st.gview(p_out + ".dense.weight")
        self.b2, self.gb2 = st.view(p_out + ".dense.bias"), st.gview(p_out + ".dense.bias")
        self.g, self.gg = st.view(p_out + ".LayerNorm.weight"), st.gview(p_out + ".LayerNorm.weight")
        self.b, self.gb = st.view(p_out + ".LayerNorm.bias"), st.gview(p_out + ".LayerNorm.bias")
        d, dff = eng.d, eng.dff
        Mc = eng.MLc if lang else eng.MV
        self.pre = eng.act(Mc, dff)
        self.h = eng.act(Mc, dff)
        self.z = eng.zact(Mc, d)
        self.mean, self.rstd = eng.f32(Mc), eng.f32(Mc)
        self.site = eng.new_site(1)
        self.rows = None                # row count of a forward on a row SUBSET (Engine: the last cross layer's visual side
                                        # on the masked rows only); None = all rows of the side

    @property
    def M(self):
        if self.rows is not None:
            return self.rows
        return self.e.ML if self.lang else self.e.MV

    def fwd(self, x, y):
        self.e.run_steps(self.fwd_steps(x, y))

    def fwd_steps(self, x, y):
        """(a generator of the block's dense contractions: see SelfAttBlock.fwd_steps)"""
        e, d, dff, M = self.e, self.e.d, self.e.dff, self.M
        ops, tag = e.ops, self.tag
        pre, h, z = self.pre[:M], self.h[:M], self.z[:M]
        # self.pre holds gelu'(pre-activation): erf and exp(-x^2/2) are in registers in the forward epilogue anyway, and the
        # backward epilogue becomes a multiply (no second erf + exp per element of the [M, dff] gradient)
        yield GemmCall(_h(x), self.w1, h, self.b1, None, pre, M, dff, d, d, d, dff, ldx=dff, epilogue=EPI_GELU_DG, tag=tag)
        yield GemmCall(h, self.w2, z, self.b2, _f(x), None, M, d, dff, dff, dff, d, ldr=d, epilogue=EPI_RESIDUAL,
                       p_drop=e.p_hid, seed=e.seed(self.site), tag=tag, **e.rkw)
        ops.block = tag
        e.ln_fwd(z, self.g, self.b, y, self.mean, self.rstd, M, d)
        self.x = x

    def bwd(self, dy, dx):
        self.e.run_steps(self.bwd_steps(dy, dx))

    def bwd_steps(self, dy, dx):
        e, d, dff, M = self.e, self.e.d, self.e.dff, self.M
        ops, tag = e.ops, self.tag
        ops.block = tag
        e.wgrad_sync()
        pre, h, z = self.pre[:M], self.h[:M], self.z[:M]
        # own scratch names: the two weight gradients registered here are launched together with the attention block's
        # (which runs next on this stream and flushes), so dz / dzm / dpre must outlive that block's scratch use
        dz = e.tmp("f_dz", M, d, res=True)
        dzm = e.ln_bwd_dense(dy, z, self.g, self.mean, self.rstd, dz, self.gg, self.gb, self.gb2, M, d, self.site,
                             tmp_name="f_dzm")
        e.wgrad_defer(dzm, h, self.gw2, d, dff, M, d, dff, dff)
        dpre = e.tmp("dpre", M, dff)
        yield GemmCall(dzm, self.w2, dpre, None, None, pre, M, dff, d, d, dff, dff, ldx=dff, a_kmajor=1, b_kmajor=0,
                       epilogue=EPI_MULAUX, colsum=self.gb1, ws=e.ws_gemm, tag=tag)      # d(b1) = column sums of dpre, in the same epilogue
        e.wgrad_defer(dpre, _h(self.x), self.gw1, dff, d, M, dff, d, d)
        yield GemmCall(dpre, self.w1, dx, None, dz, None, M, d, dff, dff, d, d, ldr=d, a_kmajor=1, b_kmajor=0,
                       epilogue=EPI_RESIDUAL, tag=tag, **e.rkw)


class CrossAttBlock:
    """LxmertXLayer.cross_att (HF:377-398): ONE LxmertCrossAttentionLayer applied in both directions on the
    pre-update inputs.  Rows = [visual (B*V) ; language (ML)] -- the visual rows first, so that the language rows, whose count
    follows the batch when they are packed (Engine pack_lang), are the tail of every buffer."""

    def __init__(self, eng, prefix, need_lang, tag, need_vis=True):
        """need_lang / need_vis: whether the language / visual rows of the OUTPUT are consumed.  The last cross layer of a
        masked-visual-token step needs only the visual side, the one of the pooled-output / language tasks (VQA, word_mask,
        matched) only the language side: the other direction of the attention, its output projection and LayerNorm are
        skipped (their parameters get no gradient in the reference either)."""
        assert need_lang or need_vis
        self.e, self.need_lang, self.need_vis, self.tag = eng, need_lang, need_vis, tag
        self.p = _Att(eng, prefix, "att")
        d = eng.d
        self.qkv = eng.act(eng.MXc, 3 * d)
        self.ctx = eng.act(eng.MXc, d)
        self.z = eng.zact(eng.MXc, d)
        self.lse_l = eng.f32(eng.B * eng.H * eng.L)
        self.lse_v = eng.f32(eng.B * eng.H * eng.V)
        self.keep_l, self.keep_v = eng.keep_bits(eng.L, eng.V), eng.keep_bits(eng.V, eng.L)
        self.mean, self.rstd = eng.f32(eng.MXc), eng.f32(eng.MXc)
        self.site = eng.new_site(3)

    def _lq(self):
        """packed-row arguments of the attention with LANGUAGE queries over visual keys"""
        e = self.e
        return dict(q_off=e.loff, q_pad=e.ML) if e.packed else {}

    def _lk(self):
        """(key mask, packed-row arguments) of the attention with visual queries over LANGUAGE keys"""
        e = self.e
        return (None, dict(k_off=e.loff, k_pad=e.ML)) if e.packed else (e.kmask, {})

    def fwd(self, X, Y):
        e, p, d = self.e, self.p, self.e.d
        ops, ML, MV, MX = e.ops, e.ML, e.MV, e.MX
        ops.block = self.tag
        L_, V_ = e.lr, e.vr
        qkv_l, qkv_v = L_(self.qkv), V_(self.qkv)
        Xh, Xf = _h(X), _f(X)           # (fp32 stream: the contractions read the bf16 copy, the residual epilogue the fp32 value)
        if not self.need_vis:
            ops.gemm(L_(Xh), p.wqkv, qkv_l, p.bqkv, None, None, ML, d, d, d, d, 3 * d)                    # Q of language rows
            ops.gemm(V_(Xh), p.wqkv[d:], qkv_v[:, d:], p.bqkv[d:], None, None, MV, 2 * d, d, d, d, 3 * d)  # K,V of visual rows
            ops.sdpa_fwd(qkv_l, qkv_v[:, d:], qkv_v[:, 2 * d:], e.vkmask, L_(self.ctx), self.lse_l, e.B, e.H, e.L, e.V, e.dh,
                         3 * d, 3 * d, 3 * d, d, e.scale, e.p_attn, e.seed(self.site), keep_bits=e.kb(self.keep_l), **self._lq())
            ops.gemm(L_(self.ctx), p.wo, L_(self.z), p.bo, L_(Xf), None, ML, d, d, d, d, d, ldr=d, epilogue=EPI_RESIDUAL,
                     p_drop=e.p_hid, seed=e.seed(self.site + 2), **e.rkw)
            e.ln_fwd(L_(self.z), p.g, p.b, L_(Y), L_(self.mean), L_(self.rstd), ML, d)
            self.X = X
            return
        if self.need_lang:
            ops.gemm(Xh[:MX], p.wqkv, self.qkv[:MX], p.bqkv, None, None, MX, 3 * d, d, d, d, 3 * d)
            # language queries over visual keys/values (no mask: visual_attention_mask is None in every caller)
            ops.sdpa_fwd(qkv_l, qkv_v[:, d:], qkv_v[:, 2 * d:], e.vkmask, L_(self.ctx), self.lse_l, e.B, e.H, e.L, e.V, e.dh,
                         3 * d, 3 * d, 3 * d, d, e.scale, e.p_attn, e.seed(self.site), keep_bits=e.kb(self.keep_l), **self._lq())
        else:
            ops.gemm(V_(Xh), p.wqkv, qkv_v, p.bqkv, None, None, MV, d, d, d, d, 3 * d)                    # Q of visual rows
            ops.gemm(L_(Xh), p.wqkv[d:], qkv_l[:, d:], p.bqkv[d:], None, None, ML, 2 * d, d, d, d, 3 * d)  # K,V of language rows
        # visual queries over language keys/values, padded language keys excluded
        km, vl = self._lk()
        ops.sdpa_fwd(qkv_v, qkv_l[:, d:], qkv_l[:, 2 * d:], km, V_(self.ctx), self.lse_v, e.B, e.H, e.V, e.L, e.dh,
                     3 * d, 3 * d, 3 * d, d, e.scale, e.p_attn, e.seed(self.site + 1), keep_bits=e.kb(self.keep_v), **vl)
        M = MX if self.need_lang else MV           # rows [0, M): visual rows, then (both directions) the language rows
        ops.gemm(self.ctx[:M], p.wo, self.z[:M], p.bo, Xf[:M], None, M, d, d, d, d, d, ldr=d, epilogue=EPI_RESIDUAL,
                 p_drop=e.p_hid, seed=e.seed(self.site + 2), **e.rkw)
        e.ln_fwd(self.z[:M], p.g, p.b, Y[:M], self.mean[:M], self.rstd[:M], M, d)
        self.X = X

    def probs(self):
        """cross-attention probabilities of the LANGUAGE queries over the visual keys, [B, H, L, V] fp32 -- what
        LxmertXLayer.forward hands out as its attention output (HF:417-449: `attention_probs = lang_att_output[1:]`)"""
        e, d = self.e, self.e.d
        assert self.need_lang, "this cross layer skipped its language direction (dead-branch elimination)"
        qkv_l, qkv_v = e.lr(self.qkv), e.vr(self.qkv)
        out = torch.zeros(e.B, e.H, e.L, e.V, dtype=torch.float32, device=e.dev)
        vl = {k: v for k, v in self._lq().items() if k == "q_off"}
        e.ops.attn_probs(qkv_l, qkv_v[:, d:], e.vkmask, self.lse_l, out, e.B, e.H, e.L, e.V, e.dh, 3 * d, 3 * d, e.scale, e.p_attn,
                         e.seed(self.site), **vl)
        return out

    def bwd(self, dY, dX):
        e, p, d = self.e, self.p, self.e.d
        ops, ML, MV, MX = e.ops, e.ML, e.MV, e.MX
        ops.block = self.tag
        e.wgrad_sync()
        if not self.need_vis:
            return self._bwd_lang_only(dY, dX)
        L_, V_ = e.lr, e.vr
        M = MX if self.need_lang else MV
        dz_full = e.tmp("dz", MX, d, res=True)
        dz = dz_full[:M]
        dzm = e.ln_bwd_dense(dY[:M], self.z[:M], p.g, self.mean[:M], self.rstd[:M], dz, p.gg, p.gb, p.gbo, M, d,
                             self.site + 2)
        e.wgrad_defer(dzm, self.ctx[:M], p.gwo, d, d, M, d, d, d)
        dctx_full = e.tmp("dctx", MX, d)
        dctx = dctx_full[:M]
        ops.gemm(dzm, p.wo, dctx, None, None, None, M, d, d, d, d, d, a_kmajor=1, b_kmajor=0)
        dqkv = e.tmp("dqkv", MX, 3 * d)
        dqkv_l, dqkv_v = L_(dqkv), V_(dqkv)
        qkv_l, qkv_v = L_(self.qkv), V_(self.qkv)
        km, vl = self._lk()
        ops.sdpa_bwd(qkv_v, qkv_l[:, d:], qkv_l[:, 2 * d:], km, V_(dctx_full), self.lse_v, dqkv_v, dqkv_l[:, d:],
                     dqkv_l[:, 2 * d:], e.B, e.H, e.V, e.L, e.dh, 3 * d, 3 * d, 3 * d, d, 3 * d, 3 * d, 3 * d, e.scale,
                     e.p_attn, e.seed(self.site + 1), bias_grad=p.gbqkv, ws=e.ws, keep_bits=e.kb(self.keep_v), **vl)
        X = _h(self.X)
        if self.need_lang:
            ops.sdpa_bwd(qkv_l, qkv_v[:, d:], qkv_v[:, 2 * d:], e.vkmask, L_(dctx_full), self.lse_l, dqkv_l, dqkv_v[:, d:],
                         dqkv_v[:, 2 * d:], e.B, e.H, e.L, e.V, e.dh, 3 * d, 3 * d, 3 * d, d, 3 * d, 3 * d, 3 * d, e.scale,
                         e.p_attn, e.seed(self.site), bias_grad=p.gbqkv, ws=e.ws, keep_bits=e.kb(self.keep_l), **self._lq())      # both directions share the projections
            e.wgrad_defer(dqkv, X[:MX], p.gwqkv, 3 * d, d, MX, 3 * d, d, d)
            e.wgrad_flush()
            ops.gemm(dqkv, p.wqkv, dX[:MX], None, dz_full, None, MX, d, 3 * d, 3 * d, d, d, ldr=d, a_kmajor=1, b_kmajor=0,
                     epilogue=EPI_RESIDUAL, **e.rkw)
        else:
            e.wgrad_defer(dqkv_v, V_(X), p.gwqkv, d, d, MV, 3 * d, d, d)
            e.wgrad_defer(dqkv_l[:, d:], L_(X), p.gwqkv[d:], 2 * d, d, ML, 3 * d, d, d)
            e.wgrad_flush()
            ops.gemm(dqkv_v, p.wqkv, V_(dX), None, dz, None, MV, d, d, 3 * d, d, d, ldr=d, a_kmajor=1, b_kmajor=0,
                     epilogue=EPI_RESIDUAL, **e.rkw)
            e.gemm_dx_plain(dqkv_l[:, d:], p.wqkv[d:], L_(dX), ML, d, 2 * d, 3 * d, d)

    def _bwd_lang_only(self, dY, dX):
        e, p, d = self.e, self.p, self.e.d
        ops, ML, MV, MX = e.ops, e.ML, e.MV, e.MX
        L_, V_ = e.lr, e.vr
        X = _h(self.X)
        dz = L_(e.tmp("dz", MX, d, res=True))
        dzm = e.ln_bwd_dense(L_(dY), L_(self.z), p.g, L_(self.mean), L_(self.rstd), dz, p.gg, p.gb, p.gbo, ML, d, self.site + 2)
        e.wgrad_defer(dzm, L_(self.ctx), p.gwo, d, d, ML, d, d, d)
        dctx = L_(e.tmp("dctx", MX, d))
        ops.gemm(dzm, p.wo, dctx, None, None, None, ML, d, d, d, d, d, a_kmajor=1, b_kmajor=0)
        dqkv = e.tmp("dqkv", MX, 3 * d)
        dqkv_l, dqkv_v = L_(dqkv), V_(dqkv)
        qkv_l, qkv_v = L_(self.qkv), V_(self.qkv)
        ops.sdpa_bwd(qkv_l, qkv_v[:, d:], qkv_v[:, 2 * d:], e.vkmask, dctx, self.lse_l, dqkv_l, dqkv_v[:, d:], dqkv_v[:, 2 * d:],
                     e.B, e.H, e.L, e.V, e.dh, 3 * d, 3 * d, 3 * d, d, 3 * d, 3 * d, 3 * d, e.scale, e.p_attn, e.seed(self.site),
                     bias_grad=p.gbqkv, ws=e.ws, keep_bits=e.kb(self.keep_l), **self._lq())
        e.wgrad_defer(dqkv_l, L_(X), p.gwqkv, d, d, ML, 3 * d, d, d)
        e.wgrad_defer(dqkv_v[:, d:], V_(X), p.gwqkv[d:], 2 * d, d, MV, 3 * d, d, d)
        e.wgrad_flush()
        ops.gemm(dqkv_l, p.wqkv, L_(dX), None, dz, None, ML, d, d, 3 * d, d, d, ldr=d, a_kmajor=1, b_kmajor=0, epilogue=EPI_RESIDUAL,
                 **e.rkw)
        e.gemm_dx_plain(dqkv_v[:, d:], p.wqkv[d:], V_(dX), MV, d, 2 * d, 3 * d, d)
