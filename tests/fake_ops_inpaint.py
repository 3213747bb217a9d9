"""TEST INFRASTRUCTURE: the host restatement of the in-painting grid step (include/xlxmert_hip.h xl_grid_step) on top of
tests/fake_ops_caption.CaptionFakeOps -- the rules of the header restated one by one, an image at a time, in plain loops.

  free      the cells v with free_mask[b, v] != 0; n_b = their number (0 is legal)
  mode 0 (Mask-Predict)
    1 commit  code_ids = row_id at the free cells whose vis_mask is set
    2 conf    row_prob at every free cell, 0 elsewhere
    3 score   mean over the free cells of log conf (in the compute dtype; float64 = the reference of the device's fp32 sum); 0 if n_b = 0
    4 re-mask n_mask = (n_b (T - step - 1)) // T lowest (conf, v) among the free cells; every other cell 0; skipped after the last step
  modes 1, 2 (one cell per image)
    candidates  free and vis_mask set; none: nothing but the score is written
    choice      mode 1: highest row_prob, ties to the lower v; mode 2: lowest (order[b, v], v), order None = v
    fill        code_ids = row_id, vis_mask = 0, conf = row_prob at the chosen cell
    score       mean over n_b of log conf at the free cells with vis_mask clear

InpaintFakeOps(dtype, compute, fault=...) selects ONE deliberately wrong rule for the injected-fault tests:
  "ties"        equal confidences go to the HIGHER cell (re-masking and the confidence policy)
  "count"       one cell too many is re-masked
  "commit"      predictions are committed at every free cell, masked or not
  "fixed"       the ranking runs over all V cells, so a given cell can be re-masked
  "float"       the schedule in floating point, int((T - step - 1) / T * n_b), as the reference's image loop writes it
  "score_all"   the score averaged over all V cells
  "ar_empty"    a row without candidates commits cell 0, which is what xl_sampler_ar_update would do
  "order_ties"  ties in `order` go to the HIGHER cell
"""
import torch

from fake_ops_caption import CaptionFakeOps, n_mask_of

FAULTS = ("ties", "count", "commit", "fixed", "float", "score_all", "ar_empty", "order_ties")
GRID_NAR, GRID_AR_CONF, GRID_AR_ORDER = 0, 1, 2


class InpaintFakeOps(CaptionFakeOps):
    def __init__(self, dtype, compute=torch.float32, noise="ok", fault=None):
        assert fault is None or fault in FAULTS, fault
        super().__init__(dtype, compute, noise, None)
        self.grid_fault = fault

    def _mean_log(self, values, n):
        if n == 0:
            return 0.0
        logs = torch.log(torch.stack(values).to(self.compute)) if values else torch.zeros(1, dtype=self.compute)
        return float(logs.sum() / n)

    def grid_step(self, row_prob, row_id, free_mask, order, code_ids, vis_mask, conf, score, B, V, mode, step, n_steps):
        assert 1 <= V <= 64 and B >= 1 and mode in (0, 1, 2) and 0 <= step < n_steps, (B, V, mode, step, n_steps)
        f = self.grid_fault
        self.calls.append(("grid_step", B, V, mode, step, n_steps, order is not None))
        cid, vm, cf, fm = code_ids.view(B, V), vis_mask.view(B, V), conf.view(B, V), free_mask.view(B, V)
        for b in range(B):
            free = [v for v in range(V) if fm[b, v] != 0]
            n = len(free)
            denom = V if f == "score_all" else n
            if mode == GRID_NAR:
                for v in free:                                                      # 1
                    if vm[b, v] != 0 or f == "commit":
                        cid[b, v] = int(row_id[b * V + v])
                cf[b].zero_()                                                       # 2
                for v in free:
                    cf[b, v] = row_prob[b * V + v]
                score[b] = self._mean_log([cf[b, v] for v in free], denom if n else 0)   # 3
                if step + 1 < n_steps:                                              # 4
                    k = n_mask_of(n, step, n_steps)
                    if f == "float":
                        k = int((n_steps - step - 1) / n_steps * n)
                    if f == "count":
                        k = min(n, k + 1)
                    pool = list(range(V)) if f == "fixed" else free
                    ranked = sorted(pool, key=lambda v: (float(cf[b, v]), -v if f == "ties" else v))
                    vm[b].zero_()
                    for v in ranked[:k]:
                        vm[b, v] = 1
                continue
            cand = [v for v in free if vm[b, v] != 0]
            pick = None
            if cand:
                if mode == GRID_AR_CONF:
                    pick = min(cand, key=lambda v: (-float(row_prob[b * V + v]), -v if f == "ties" else v))
                else:
                    pick = min(cand, key=lambda v: (v if order is None else int(order.view(B, V)[b, v]), -v if f == "order_ties" else v))
            elif f == "ar_empty":
                pick = 0
            if pick is not None:
                cid[b, pick] = int(row_id[b * V + pick])
                vm[b, pick] = 0
                cf[b, pick] = row_prob[b * V + pick]
            score[b] = self._mean_log([cf[b, v] for v in free if vm[b, v] == 0], denom if n else 0)
