"""TEST INFRASTRUCTURE shared by the caption-image matching tests (CPU over tests/fake_ops_match.MatchFakeOps, GPU over HipOps): the
cases, the expected outputs of xl_pair_expand / xl_match_rank built with torch.index_select and a stable torch.sort, the bound of
`prob`, and the tiny model with its oracle margins.

Bound of prob (the way tests/bounds_eval.py derives its own; U32 = 2^-24, the fp32 unit roundoff, 1 ulp = 2 U32):
  the kernel computes  e = expf(-margin),  s = 1 + e,  p = 1 / s  on the margin it returned (the negation is exact).
  e  carries the exponential's error: EXP_ULP = 2 ulp (tests/bounds.py: the constant every exp of this suite is held to), relative;
     the accurate expf, not the fast form, so there is no argument-scaling term;
  s  one fp32 add: relative U32;     p  one IEEE division (RCP_ULP = 1 ulp would be the reciprocal instruction; a division rounds
     once): this is the output's FINAL rounding, U32 |p|, never scaled by SLACK.
  d p / p = -(e / (1 + e)) d e / e = -(1 - p) d e / e, so to first order
     |p_hat - p| <= U32 p  +  SLACK * (2 EXP_ULP U32 (1 - p) + U32) p  +  TINY
  (margins of +-60 keep e, s and p normal numbers: e^-60 = 8.8e-27 > 2^-126.)
"""
import torch

import lxmert_oracle as O
from _util import golden_cfg, load_golden
from bounds import EXP_ULP, SLACK, TINY, U32, check
from xlxmert_amd.config import XLxmertConfig

CFG_KEYS = ("vocab_size", "hidden_size", "num_attention_heads", "intermediate_size", "max_position_embeddings", "type_vocab_size",
            "l_layers", "x_layers", "r_layers", "visual_feat_dim", "visual_pos_dim", "num_clusters")


def same_bits(a, b):
    """bit-for-bit equality of two tensors of one dtype and shape"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---------------------------------------------------------------------------------------------- xl_pair_expand
def chunk_rows(lens, M, B_c, start, count):
    """packed language rows of the chunk, slot by slot (NOT the kernel's closed form)"""
    return sum(lens[(start + min(j, count - 1)) // M] for j in range(B_c))


def expected_expand(vis, lang, off, N, M, V, L, d, start, count, B_c, packed, rows_pad):
    """(visual rows, language rows [rows_pad, d], chunk_off, chunk_rows, kmask) of one chunk from index_select / repeat_interleave"""
    dev = vis.device
    p = start + torch.clamp(torch.arange(B_c), max=count - 1)
    n_j, m_j = p // M, p % M
    off_t = torch.as_tensor(off, dtype=torch.int64)
    lens = off_t[1:] - off_t[:-1]
    ln = lens[n_j]
    e_vis = vis.view(M, V, d).index_select(0, m_j.to(dev)).reshape(B_c * V, d)
    slot = torch.repeat_interleave(torch.arange(B_c), ln)                   # slot of every packed row
    c_off = torch.cat([ln.new_zeros(1), ln.cumsum(0)])
    pos = torch.arange(int(ln.sum())) - c_off[slot]                         # position l of every packed row
    src = off_t[n_j][slot] + pos
    kmask = (torch.arange(L)[None, :] < ln[:, None]).to(torch.uint8)
    if packed:
        e_lang = torch.zeros(rows_pad, d, dtype=lang.dtype, device=dev)
        e_lang[:src.numel()] = lang.index_select(0, src.to(dev))
        rows = torch.full((rows_pad,), -1, dtype=torch.int32)
        rows[:src.numel()] = (slot * L + pos).to(torch.int32)
        return e_vis, e_lang, c_off.to(torch.int32), rows, kmask
    e_lang = torch.zeros(B_c * L, d, dtype=lang.dtype, device=dev)
    e_lang[(slot * L + pos).to(dev)] = lang.index_select(0, src.to(dev))
    return e_vis, e_lang, None, None, kmask


def check_expand(ops, dev, dtype, N, M, V, L, d, lens, B_c, packed, alloc=None, row_pad=8, two=False):
    """every chunk of the N*M pairs through ops.pair_expand into poisoned buffers, every output compared bit for bit.  alloc(name,
    shape, dtype) -> tensor (the GPU tests hand out views between guards)."""
    gen = torch.Generator().manual_seed(1234 + N * 7 + M)
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    src_rows = off[-1] + 3                                                   # (a padded source: rows beyond the last caption)
    alloc = alloc or (lambda name, shape, dt: torch.zeros(*shape, dtype=dt, device=dev))
    dts = [dtype] + ([torch.bfloat16] if two else [])
    vis = [torch.randn(M * V, d, generator=gen).to(dt).to(dev) for dt in dts]
    lang = [torch.randn(src_rows, d, generator=gen).to(dt).to(dev) for dt in dts]
    off_dev = torch.tensor(off, dtype=torch.int32, device=dev)
    cap = (B_c * L + row_pad - 1) // row_pad * row_pad if packed else B_c * L
    for start in range(0, N * M, B_c):
        count = min(B_c, N * M - start)
        rows = chunk_rows(lens, M, B_c, start, count) if packed else B_c * L
        rows_pad = min(cap, (rows + row_pad - 1) // row_pad * row_pad) if packed else rows
        x0 = [alloc(f"x0_{i}", (B_c * V + cap, d), dt) for i, dt in enumerate(dts)]
        c_off, c_rows, km = alloc("off", (B_c + 1,), torch.int32), alloc("rows", (cap,), torch.int32), alloc("kmask", (B_c, L), torch.uint8)
        for t in x0:
            t.fill_(7.0)
        c_off.fill_(-7), c_rows.fill_(-7), km.fill_(7)
        ops.pair_expand(vis[0], lang[0], off_dev, x0[0], c_off if packed else None, c_rows if packed else None, km, N, M, V, L, d, start,
                        count, B_c, packed, src_rows, rows, rows_pad, vis2=vis[1] if two else None, lang2=lang[1] if two else None,
                        x0_2=x0[1] if two else None)
        what = f"pairs [{start}, {start + count}) B_c={B_c} packed={packed}"
        for i, dt in enumerate(dts):
            e_vis, e_lang, e_off, e_rows, e_km = expected_expand(vis[i], lang[i], off, N, M, V, L, d, start, count, B_c, packed, rows_pad)
            assert same_bits(x0[i][:B_c * V], e_vis), f"{what}: visual rows (copy {i})"
            assert same_bits(x0[i][B_c * V:B_c * V + rows_pad], e_lang), f"{what}: language rows (copy {i})"
            assert bool((x0[i][B_c * V + rows_pad:].float() == 7.0).all()), f"{what}: rows beyond lang_rows_pad were written (copy {i})"
        assert torch.equal(km.cpu(), e_km), f"{what}: kmask"
        if packed:
            assert torch.equal(c_off.cpu(), e_off), f"{what}: chunk offsets {c_off.tolist()} != {e_off.tolist()}"
            assert torch.equal(c_rows[:rows_pad].cpu(), e_rows), f"{what}: chunk row list"
            assert bool((c_rows[rows_pad:] == -7).all()), f"{what}: row list beyond lang_rows_pad was written"
        else:
            assert bool((c_off == -7).all()) and bool((c_rows == -7).all()), f"{what}: the dense layout wrote offsets / rows"


# ---------------------------------------------------------------------------------------------- xl_match_rank
def rank_margins(N, M):
    """hand-built margins: ties (also a tie of the probabilities alone: 20 and 30 both give prob == 1.0f), extremes of +-60"""
    gen = torch.Generator().manual_seed(99 + N + M)
    mg = torch.randint(-3, 4, (N, M), generator=gen).float() * 0.5           # few distinct values: many ties
    flat = mg.view(-1)
    if N >= 4 and M >= 3:
        mg[N // 2, :] = 1.0                                                  # a whole row and a whole column of equal margins
        mg[:, M // 2] = 1.0
        mg[0, 0], mg[1, 0], mg[3, 0], mg[N - 1, M - 1] = 60.0, 20.0, 30.0, -60.0
    else:
        flat[0], flat[1], flat[2], flat[-1] = 60.0, 20.0, 30.0, -60.0
    return mg


def expected_ranking(margin, k, image_of_caption, caption_of_image):
    """top-k lists and target ranks from a stable descending sort (ties to the lower index)"""
    out = {}
    for name, dim, tgt, rname in (("topk_images", 1, image_of_caption, "rank_t2i"), ("topk_captions", 0, caption_of_image, "rank_i2t")):
        idx = torch.sort(margin.double(), dim=dim, descending=True, stable=True).indices
        idx = idx if dim == 1 else idx.t()                                  # [queries, candidates]
        out[name] = idx[:, :k].to(torch.int32) if k else None
        if tgt is not None:
            t = tgt.long()
            pos = (idx == t.clamp(min=0)[:, None]).to(torch.uint8).argmax(1)
            out[rname] = torch.where(t >= 0, pos, torch.full_like(pos, -1)).to(torch.int32)
    return out


def prob_bound(margin64):
    p = 1.0 / (1.0 + torch.exp(-margin64))
    return p, U32 * p + SLACK * (2 * EXP_ULP * U32 * (1.0 - p) + U32) * p + TINY


def check_rank(ops, dev, N, M, k, B_c, alloc=None):
    """the margins of rank_margins through the scatter stage chunk by chunk (rel buffers with B_c slots, a ragged last chunk whose
    padding slots hold poison) and the rank stage on the last call; margin exact, prob within its bound, lists and ranks exact,
    nothing else written.  A direction with fewer than k candidates gets no top-k buffer."""
    alloc = alloc or (lambda name, shape, dt: torch.zeros(*shape, dtype=dt, device=dev))
    mg = rank_margins(N, M)
    gen = torch.Generator().manual_seed(5)
    a = torch.randint(-4, 5, (N * M,), generator=gen).float() * 0.5           # (halves: the sum and the difference below are exact)
    rel_all = torch.zeros(N * M, 8)
    rel_all[:, 0], rel_all[:, 1] = a, (a + mg.view(-1))
    want = rel_all[:, 1] - rel_all[:, 0]                                    # the fp32 subtraction the kernel must reproduce
    ioc = torch.arange(N, dtype=torch.int32) % M
    coi = torch.arange(M, dtype=torch.int32) % N
    ioc[N // 2], coi[M // 2] = M // 2, N // 2       # rank_margins' all-equal row / column: the target ties with lower AND higher indices
    if N > 1:
        ioc[N - 1] = -1
    margin, prob = alloc("margin", (N, M), torch.float32), alloc("prob", (N, M), torch.float32)
    margin.fill_(-777.0), prob.fill_(-777.0)
    ti = alloc("topk_i", (N, k), torch.int32) if k <= M else None
    tc = alloc("topk_c", (M, k), torch.int32) if k <= N else None
    r1, r2 = alloc("rank_t2i", (N,), torch.int32), alloc("rank_i2t", (M,), torch.int32)
    for t in (ti, tc, r1, r2):
        if t is not None:
            t.fill_(-7)
    ioc_d, coi_d = ioc.to(dev), coi.to(dev)
    if B_c > 1 and N * M > 1:               # a ragged chunk that is NOT the last one: one real pair, poison in the other slots
        rel = torch.full((B_c, 8), 1e30)
        rel[0] = rel_all[0]
        before = margin.clone()
        ops.match_rank(rel.to(dev), 0, 1, margin, prob, N, M)
        assert same_bits(margin.view(-1)[1:], before.view(-1)[1:]), "the scores of padding slots were written"
    for start in range(0, N * M, B_c):
        count = min(B_c, N * M - start)
        rel = torch.full((B_c, 8), 1e30)                                   # padding slots: poison that must never reach the outputs
        rel[:count] = rel_all[start:start + count]
        final = start + count == N * M
        before = margin.clone()
        ops.match_rank(rel.to(dev), start, count, margin, prob, N, M, rank_stage=final, k=k, **(dict(
            topk_images=ti, topk_captions=tc, image_of_caption=ioc_d, caption_of_image=coi_d, rank_t2i=r1, rank_i2t=r2) if final else {}))
        got, was = margin.view(-1), before.view(-1)
        assert same_bits(got[:start], was[:start]) and same_bits(got[start + count:], was[start + count:]), \
            f"pairs outside [{start}, {start + count}) were written"
    assert same_bits(margin.view(-1).cpu(), want), "margin is not the fp32 subtraction"
    p, b = prob_bound(margin.double().cpu())
    ratio = check(prob.cpu(), p, b, "prob")
    exp = expected_ranking(margin.cpu(), k, ioc, coi)
    for name, t in (("topk_images", ti), ("topk_captions", tc)):
        if t is not None:
            assert torch.equal(t.cpu(), exp[name]), f"{name}: {t.tolist()} != {exp[name].tolist()}"
    assert torch.equal(r1.cpu(), exp["rank_t2i"]), f"rank_t2i: {r1.tolist()} != {exp['rank_t2i'].tolist()}"
    assert torch.equal(r2.cpu(), exp["rank_i2t"]), f"rank_i2t: {r2.tolist()} != {exp['rank_i2t'].tolist()}"
    return ratio


# ---------------------------------------------------------------------------------------------- the tiny model
def tiny_case(N=3, M=2, lens=(1, 8, 5)):
    """lang_tasks_tiny's weights and inputs as N captions (ragged lengths, 1 and L among them) and M images"""
    g = load_golden("lang_tasks_tiny")
    oc = golden_cfg(g)
    cfg = XLxmertConfig(**{k: getattr(oc, k) for k in CFG_KEYS})
    sd = O.make_cls_state_dict(oc, int(g["seed"]))
    ids = torch.from_numpy(g["in_input_ids"]).clone()[:N]
    L = ids.shape[1]
    assert len(lens) == N and max(lens) == L and min(lens) == 1
    att = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]
    ids[~att] = 0
    inp = dict(input_ids=ids, attention_mask=att, token_type_ids=torch.from_numpy(g["in_token_type_ids"])[:N].clone(),
               cluster_ids=torch.from_numpy(g["in_cluster_ids"])[:M].clone(), visual_pos=torch.from_numpy(g["in_visual_pos"])[:M].clone())
    return cfg, oc, sd, inp


def materialised(inp, N, M):
    """the N*M explicit rows, caption-major: what a caller has to build today"""
    rep = lambda t: t.repeat_interleave(M, 0)                               # noqa: E731
    til = lambda t: t.repeat(N, *([1] * (t.dim() - 1)))                     # noqa: E731
    return dict(input_ids=rep(inp["input_ids"]), attention_mask=rep(inp["attention_mask"]), token_type_ids=rep(inp["token_type_ids"]),
                cluster_ids=til(inp["cluster_ids"]), visual_pos=til(inp["visual_pos"]))


_ORACLE = {}


def oracle_margin(N=3, M=2, lens=(1, 8, 5)):
    """margin [N, M] of the oracle's matched forward on the explicitly materialised pairs (computed once per case)"""
    key = (N, M, tuple(lens))
    if key not in _ORACLE:
        cfg, oc, sd, inp = tiny_case(N, M, lens)
        big = materialised(inp, N, M)
        ref = O.xlxmert_matched_forward(sd, oc, big["input_ids"], big["visual_pos"], big["attention_mask"], big["cluster_ids"],
                                        torch.zeros(N * M, dtype=torch.int64), big["token_type_ids"])
        s = ref["score"].detach().double()
        _ORACLE[key] = (s[:, 1] - s[:, 0]).view(N, M)
    return _ORACLE[key]
