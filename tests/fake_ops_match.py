"""TEST INFRASTRUCTURE: the host restatement of caption-image matching (include/xlxmert_hip.h xl_pair_expand, xl_match_rank) on top of
tests/fake_ops_eval.EvalFakeOps -- the rules of the header restated one by one, a slot / a query at a time, in plain loops.

xl_pair_expand   slot j of a chunk holds pair p_j = pair_start + min(j, pair_count - 1), caption n = p_j // M, image m = p_j % M
  visual rows      x0[j*V + v] = vis[m*V + v]
  packed           slot j's language rows start at chunk_off[j] = F(p_j) + len * (j - min(j, pair_count-1)) - F(pair_start),
                   F(p) = M*lang_off[n] + m*len_n; row chunk_off[j] + l = lang[lang_off[n] + l]; chunk_rows there = j*L + l;
                   chunk_off[B_c] = the chunk's rows; rows up to lang_rows_pad are zero rows with chunk_rows = -1
  dense            row j*L + l = lang[lang_off[n] + l] for l < len_n, a zero row beyond
  chunk_kmask      [B_c, L] = (l < len_n)
  lang_len         (dense layout only) len_n itself, for a dense source whose offsets n*L are not the prefix sums of its lengths
xl_match_rank    scatter: margin[p] = rel[i,1] - rel[i,0], prob[p] = 1 / (1 + exp(-margin)) for the pair_count REAL pairs of the chunk;
                 rank: order by (margin descending, index ascending); top-k lists and the number of candidates before the target

MatchFakeOps(dtype, compute, fault=...) selects ONE deliberately wrong rule for the injected-fault tests:
  "transposed"   the pair index read image-major: n = p % N, m = p // N
  "no_m_term"    chunk offsets without the m * len_n term
  "tail_dirty"   the tail rows that pad the packed rows to the row tile are not zeroed
  "pad_scores"   the scores of a ragged last chunk's padding slots are written too (into the pairs that follow)
  "ties_high"    equal margins go to the HIGHER index
  "by_prob"      the ranking orders by prob (which saturates at 1.0 in fp32) instead of margin
  "rank_ge"      the target's rank counts the candidates with margin >= the target's instead of those that rank before it
"""
import torch

from fake_ops import v2
from fake_ops_eval import EvalFakeOps

FAULTS = ("transposed", "no_m_term", "tail_dirty", "pad_scores", "ties_high", "by_prob", "rank_ge")


class MatchFakeOps(EvalFakeOps):
    def __init__(self, dtype, compute=torch.float32, fault=None):
        assert fault is None or fault in FAULTS, fault
        super().__init__(dtype, compute, None)
        self.match_fault = fault

    def pair_expand(self, vis, lang, lang_off, x0, chunk_off, chunk_rows, chunk_kmask, N, M, V, L, d, pair_start, pair_count, B_c, packed,
                    lang_src_rows, lang_rows, lang_rows_pad, vis2=None, lang2=None, x0_2=None, lang_len=None):
        f = self.match_fault
        assert lang_len is None or not packed
        given = [int(x) for x in lang_len.view(-1)[:N].tolist()] if lang_len is not None else None
        assert d % 8 == 0 and 1 <= pair_count <= B_c and pair_start >= 0 and pair_start + pair_count <= N * M
        assert (lang_rows <= lang_rows_pad) if packed else (lang_rows == lang_rows_pad == B_c * L)
        self.calls.append(("pair_expand", N, M, pair_start, pair_count, B_c, bool(packed)))
        off = [int(x) for x in lang_off.view(-1)[:N + 1].tolist()]

        def pair(p):
            n, m = (p % N, p // N) if f == "transposed" else (p // M, p % M)
            ln = min(max(given[n] if given is not None else off[n + 1] - off[n], 0), L)
            return n, m, ln, M * off[n] + (0 if f == "no_m_term" else m * ln)
        base = pair(pair_start)[3]
        copies = [(vis, lang, x0)] + ([(vis2, lang2, x0_2)] if vis2 is not None else [])
        km = chunk_kmask.view(B_c, L)
        for j in range(B_c):
            jr = min(j, pair_count - 1)
            n, m, ln, first = pair(pair_start + jr)
            start = first + ln * (j - jr) - base
            for sv, sl, dst in copies:
                dv, dl = v2(dst, B_c * V, d, d), v2(dst[B_c * V:], lang_rows_pad, d, d)
                dv[j * V:(j + 1) * V].copy_(v2(sv, M * V, d, d)[m * V:(m + 1) * V])
                src = v2(sl, lang_src_rows, d, d)[off[n]:off[n] + ln]
                if packed:
                    dl[start:start + ln].copy_(src)
                else:
                    dl[j * L:j * L + ln].copy_(src)
                    dl[j * L + ln:(j + 1) * L].zero_()
            for l in range(L):
                km[j, l] = 1 if l < ln else 0
            if packed:
                chunk_off[j] = start
                for l in range(ln):
                    chunk_rows[start + l] = j * L + l
                if j == B_c - 1:
                    chunk_off[B_c] = start + ln
        if packed:
            total = int(chunk_off[B_c])
            chunk_rows[total:lang_rows_pad] = -1
            if f != "tail_dirty":
                for _, _, dst in copies:
                    v2(dst[B_c * V:], lang_rows_pad, d, d)[total:].zero_()

    def match_rank(self, rel, pair_start, pair_count, margin, prob, N, M, rank_stage=False, k=0, topk_images=None, topk_captions=None,
                   image_of_caption=None, caption_of_image=None, rank_t2i=None, rank_i2t=None):
        f = self.match_fault
        self.calls.append(("match_rank", pair_start, pair_count, bool(rank_stage), k))
        mg, pb = margin.view(-1), prob.view(-1) if prob is not None else None
        if rel is not None:
            n_slots = rel.shape[0] if f == "pad_scores" else pair_count
            for i in range(n_slots):
                p = pair_start + i
                if p >= N * M:
                    break
                m_ = rel[i, 1] - rel[i, 0]
                mg[p] = m_
                if pb is not None:
                    pb[p] = (1.0 / (1.0 + torch.exp(-m_.to(self.compute)))).to(pb.dtype)
        if not rank_stage:
            return
        assert (topk_images is None or 1 <= k <= min(32, M)) and (topk_captions is None or 1 <= k <= min(32, N))
        key = (prob if f == "by_prob" else margin).view(N, M)

        def order(vals):
            return sorted(range(len(vals)), key=lambda c: (-vals[c], -c if f == "ties_high" else c))

        def rank_of(vals, t):
            if f == "rank_ge":
                return sum(1 for c in range(len(vals)) if c != t and vals[c] >= vals[t])
            return order(vals).index(t)
        for q_n, cand, topk, target, rank in ((N, lambda q: key[q, :], topk_images, image_of_caption, rank_t2i),
                                              (M, lambda q: key[:, q], topk_captions, caption_of_image, rank_i2t)):
            for q in range(q_n):
                vals = [float(x) for x in cand(q).tolist()]
                if topk is not None:
                    topk.view(q_n, k)[q] = torch.tensor(order(vals)[:k], dtype=topk.dtype)
                if rank is not None:
                    t = int(target[q])
                    rank[q] = rank_of(vals, t) if 0 <= t < len(vals) else -1
