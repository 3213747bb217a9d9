"""TEST INFRASTRUCTURE: the in-painting loop in plain torch, composed from oracle.lxmert_oracle (lxmert_model + visual_obj_head +
codebook_features: the modules tests/golden/sampler_tiny.npz pins to the reference) and written the way the reference writes its
image loops (ref tasks/imggen_model.py:49-153, 199-243): whole-batch tensors, softmax(-1).max(-1), topk + scatter_ on an exact
integer key.  It shares no code with tests/fake_ops_inpaint.py (per-image loops) or with the kernel.

grid_update     one step's bookkeeping on [B, V] tensors -- the independent check of the restatement and of the kernel
step_logits     one forward: code ids + mask -> codebook scores of every cell
inpaint_codes   the greedy loop; `trace` receives the state after every step
"""
import torch

import lxmert_oracle as O

NAR, AR_CONF, AR_ORDER = 0, 1, 2


def conf_key(conf, live):
    """int64 [B, V], distinct within a row, ascending exactly as (conf ascending, cell ascending) over the `live` cells: the fp32 bit
    pattern of a non-negative confidence is monotonic in its value; cells that are not live sort above all of them"""
    V = conf.shape[1]
    bits = conf.float().clamp(min=0).contiguous().view(torch.int32).to(torch.int64)
    bits = torch.where(live, bits, torch.full_like(bits, 2 ** 40))
    return bits * 64 + torch.arange(V)[None, :]


def grid_update(pred_prob, pred_id, free, order, code_ids, vis_mask, conf, mode, step, n_steps):
    """pred_prob / pred_id [B, V]: the forward's probability / id at every cell.  Returns the new (code_ids, vis_mask [bool], conf,
    score [float64]) -- the rules of include/xlxmert_hip.h xl_grid_step."""
    B, V = code_ids.shape
    free, vis_mask = free.bool(), vis_mask.bool()
    n = free.sum(1)
    pred_prob = pred_prob.float()
    if mode == NAR:
        code_ids = torch.where(free & vis_mask, pred_id.long(), code_ids)
        conf = torch.where(free, pred_prob, torch.zeros(B, V))
        counted = free
        if step + 1 < n_steps:
            n_mask = (n * (n_steps - step - 1)) // n_steps
            key = conf_key(conf, free)
            vis_mask = torch.zeros(B, V, dtype=torch.bool)
            for b in range(B):                                      # (one k per image: the reference's loop has one for the batch)
                k = int(n_mask[b])
                if k > 0:
                    _, lowest_arg = key[b].topk(k, largest=False)
                    vis_mask[b].scatter_(0, lowest_arg, True)
    else:
        cand = free & vis_mask
        if mode == AR_CONF:                                         # highest probability first, the lower cell among equals
            bits = pred_prob.clamp(min=0).contiguous().view(torch.int32).to(torch.int64)
            key = (2 ** 32 - bits) * 64 + torch.arange(V)[None, :]
        else:
            o = torch.arange(V)[None, :].expand(B, V) if order is None else order.long()
            key = (o - o.min()) * 64 + torch.arange(V)[None, :]
        key = torch.where(cand, key, torch.full_like(key, 2 ** 62))
        _, top_arg = key.topk(1, dim=1, largest=False)
        update = torch.zeros(B, V, dtype=torch.bool)
        update.scatter_(1, top_arg, True)
        update &= cand                                              # a row without candidates updates nothing
        code_ids = torch.where(update, pred_id.long(), code_ids)
        conf = torch.where(update, pred_prob, conf.float())
        vis_mask = vis_mask & ~update
        counted = free & ~vis_mask
    logs = torch.where(counted, torch.log(conf.double()), torch.zeros(B, V, dtype=torch.float64))
    score = torch.where(n > 0, logs.sum(1) / n.clamp(min=1), torch.zeros(B, dtype=torch.float64))
    return code_ids, vis_mask, conf, score


def step_logits(sd, cfg, input_ids, code_ids, vis_mask, visual_pos):
    """[B, V, K] scores of the codebook head on one forward over where(mask, mask_feat, centroids[code_ids])"""
    with torch.no_grad():
        feats = O.codebook_features(sd, code_ids, vis_mask.long())
        _, vis, _ = O.lxmert_model(sd, cfg, input_ids, feats, visual_pos, input_ids > 0)
        _, obj = O.visual_obj_head(sd, cfg, vis)
    return obj


def inpaint_codes(sd, cfg, input_ids, init_codes, free_mask, n_steps, grid_size, mode=NAR, order=None):
    """greedy in-painting.  Returns (code_ids, score, conf, trace); trace[i] = dict of the state after step i (code_ids, vis_mask, conf,
    score, pred_id, pred_prob, scores) and of the mask the forward read (fed_mask)."""
    B = input_ids.shape[0]
    V = grid_size ** 2
    dtype = sd["vis_emb.weight"].dtype
    visual_pos = torch.from_numpy(O.box_position(grid_size)).unsqueeze(0).expand(B, -1, -1).to(dtype)
    free = torch.as_tensor(free_mask) != 0
    code_ids = torch.where(free, torch.zeros(B, V, dtype=torch.long), torch.as_tensor(init_codes).long())
    vis_mask, conf = free.clone(), torch.zeros(B, V)
    score = torch.zeros(B, dtype=torch.float64)
    trace = []
    for i in range(n_steps):
        scores = step_logits(sd, cfg, input_ids, code_ids, vis_mask, visual_pos)
        pred_prob, pred_id = torch.softmax(scores, dim=2).max(dim=2)
        fed = vis_mask.clone()
        code_ids, vis_mask, conf, score = grid_update(pred_prob, pred_id, free, order, code_ids, vis_mask, conf, mode, i, n_steps)
        trace.append(dict(code_ids=code_ids.clone(), vis_mask=vis_mask.clone(), conf=conf.clone(), score=score.clone(), fed_mask=fed,
                          pred_id=pred_id.clone(), pred_prob=pred_prob.clone(), scores=scores))
    return code_ids, score, conf, trace
