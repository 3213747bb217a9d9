"""TEST INFRASTRUCTURE: the Mask-Predict caption loop in plain torch, composed from oracle.lxmert_oracle (lxmert_model +
lm_prediction_head + codebook_features: the modules tests/golden/lang_tasks_tiny.npz pins to the reference) and written the way the
reference writes its image loop (ref tasks/imggen_model.py:199-243): whole-batch tensors, softmax(-1).max(-1), topk(largest=False)
+ scatter_.  It shares no code with tests/fake_ops_caption.py (per-caption loops) or with the kernel.

caption_update  one step's bookkeeping on [B, L] tensors -- the independent check of the restatement and of the kernel
step_logits     one forward: fed ids -> vocabulary scores of every position, banned ids at -inf
sample_words_nar  the loop; `trace` receives the state after every step
"""
import torch

import lxmert_oracle as O


def layout(lengths, L, prefix_ids=(), cls_id=101, sep_id=102, mask_id=103, pad_id=0):
    """(tokens [B, L] with mask_id at the free positions, free [B, L] bool, attention_mask [B, L] bool)"""
    lengths = torch.as_tensor(lengths, dtype=torch.long).reshape(-1)
    B, P = lengths.numel(), len(prefix_ids)
    pos = torch.arange(L)[None, :]
    n = lengths[:, None]
    free = (pos >= P + 1) & (pos < P + 1 + n)
    tok = torch.full((B, L), pad_id, dtype=torch.long)
    tok[:, 0] = cls_id
    if P:
        tok[:, 1:P + 1] = torch.as_tensor(list(prefix_ids), dtype=torch.long)[None, :]
    tok = torch.where(free, torch.full_like(tok, mask_id), tok)
    tok = torch.where(pos == P + 1 + n, torch.full_like(tok, sep_id), tok)
    return tok, free, pos < P + n + 2


def order_key(conf, free):
    """int64 [B, L], distinct within a row, ascending exactly as (conf ascending, position ascending) over the free positions:
    the fp32 bit pattern of a non-negative confidence is monotonic in its value, -1 (the repeat rule's value) sorts below all of
    them, non-free positions above all of them"""
    L = conf.shape[1]
    c = conf.float()
    bits = torch.where(c < 0, torch.full_like(c, -1.0).to(torch.int64), c.clamp(min=0).contiguous().view(torch.int32).to(torch.int64))
    bits = torch.where(free, bits, torch.full_like(bits, 2 ** 40))
    return bits * 64 + torch.arange(L, device=conf.device)[None, :]


def caption_update(pred_prob, pred_id, lengths, tokens, word_mask, L, P, step, n_steps, mask_id, suppress_repeats=False, pad_id=0):
    """pred_prob / pred_id [B, L]: the forward's probability / id at every position (whatever at the non-free ones).  Returns the new
    (tokens, fed_ids, word_mask, conf, score [float64]) -- the six rules of include/xlxmert_hip.h xl_caption_step."""
    B = tokens.shape[0]
    pos = torch.arange(L)[None, :]
    n = torch.as_tensor(lengths, dtype=torch.long).reshape(B).clamp(0, L - 2 - P)
    free = (pos >= P + 1) & (pos < P + 1 + n[:, None])
    word_mask = word_mask.bool()
    tokens = torch.where(word_mask & free, pred_id.long(), tokens)
    conf = torch.where(free, pred_prob.float(), torch.zeros(B, L))
    score = torch.where(free, torch.log(conf.double()), torch.zeros(B, L, dtype=torch.float64)).sum(1) / n.clamp(min=1)
    if suppress_repeats:
        same = tokens[:, 1:] == tokens[:, :-1]
        conf[:, 1:] = torch.where(same & free[:, 1:], torch.full_like(conf[:, 1:], -1.0), conf[:, 1:])
    if step + 1 < n_steps:
        n_mask = (n * (n_steps - step - 1)) // n_steps
        key = order_key(conf, free)
        word_mask = torch.zeros(B, L, dtype=torch.bool)
        for b in range(B):                                          # (one k per caption: the image loop has one for the batch)
            k = int(n_mask[b])
            if k > 0:
                _, lowest_arg = key[b].topk(k, largest=False)
                word_mask[b].scatter_(0, lowest_arg, True)
    real = pos < P + n[:, None] + 2
    fed = torch.where(word_mask, torch.full_like(tokens, mask_id), tokens)
    fed = torch.where(real, fed, torch.full_like(tokens, pad_id))
    return tokens, fed, word_mask, conf, score


def step_logits(sd, cfg, fed_ids, attention_mask, visual_feats, visual_pos, banned_ids=()):
    """[B, L, vocab] scores of the MLM head on one forward, banned ids at -inf"""
    with torch.no_grad():
        lang, _, _ = O.lxmert_model(sd, cfg, fed_ids, visual_feats, visual_pos, attention_mask.long())
        scores = O.lm_prediction_head(sd, cfg, lang).clone()
    if len(banned_ids):
        scores[..., torch.as_tensor(list(banned_ids), dtype=torch.long)] = -float("inf")
    return scores


def sample_words_nar(sd, cfg, visual_feats, visual_pos, lengths, n_steps, L, prefix_ids=(), banned_ids=(), cls_id=101, sep_id=102,
                     mask_id=103, suppress_repeats=False, cluster_ids=None):
    """greedy Mask-Predict caption decoding.  Returns (tokens, score, conf, trace); trace[i] = dict of the state after step i
    (tokens, fed_ids, word_mask, conf, score, pred_id, pred_prob, scores)."""
    if cluster_ids is not None:
        visual_feats = O.codebook_features(sd, cluster_ids, None)
    P = len(prefix_ids)
    tokens, free, att = layout(lengths, L, prefix_ids, cls_id, sep_id, mask_id)
    word_mask, fed = free.clone(), tokens.clone()
    trace = []
    for i in range(n_steps):
        scores = step_logits(sd, cfg, fed, att, visual_feats, visual_pos, banned_ids)
        pred_prob, pred_id = torch.softmax(scores, dim=2).max(dim=2)
        tokens, fed, word_mask, conf, score = caption_update(pred_prob, pred_id, lengths, tokens, word_mask, L, P, i, n_steps, mask_id,
                                                             suppress_repeats)
        trace.append(dict(tokens=tokens.clone(), fed_ids=fed.clone(), word_mask=word_mask.clone(), conf=conf.clone(), score=score.clone(),
                          pred_id=pred_id.clone(), pred_prob=pred_prob.clone(), scores=scores))
    return tokens, score, conf, trace
