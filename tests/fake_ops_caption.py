"""TEST INFRASTRUCTURE: the host restatement of the Mask-Predict caption step (include/xlxmert_hip.h xl_caption_step) on top of
tests/fake_ops_truncation.TruncationFakeOps -- the six rules of the header restated one by one, a caption at a time, in plain loops.

  n_b       lengths[b] clamped to [0, L-2-P]; with packed rows also to the rows example b owns
  row       b*L + l dense, lang_off[b] + l packed
  1 commit  tokens = row_id at the free positions whose word_mask is set
  2 conf    row_prob at every free position, 0 elsewhere
  3 score   mean over the free positions of log conf (in the compute dtype; float64 = the reference of the device's fp32 sum)
  4 repeats conf = -1 where a free token equals its left neighbour, all positions judged on the committed tokens at once
  5 re-mask n_mask = (n_b (T - step - 1)) // T lowest (conf, l); skipped after the last step
  6 fed ids mask_token_id / token for l < P+n_b+2, 0 beyond

CaptionFakeOps(dtype, compute, fault=...) selects ONE deliberately wrong rule for the injected-fault tests:
  "ties"        equal confidences go to the HIGHER position
  "count"       one position too many is re-masked
  "commit"      predictions are committed at every free position, masked or not
  "float"       the schedule in floating point, int((T - step - 1) / T * n_b), as the reference's image loop writes it
  "offset"      packed offsets ignored: rows b*L + l whatever lang_off says
  "sequential"  the repeat rule applied left to right, a flagged token no longer counting as a left neighbour
  "score_all"   the score averaged over all L positions
"""
import math

import torch

from fake_ops_truncation import TruncationFakeOps

FAULTS = ("ties", "count", "commit", "float", "offset", "sequential", "score_all")


def n_mask_of(n, step, n_steps):
    """positions re-masked for step + 1 out of n free ones: integer division, exact"""
    return (n * (n_steps - step - 1)) // n_steps


class CaptionFakeOps(TruncationFakeOps):
    def __init__(self, dtype, compute=torch.float32, noise="ok", fault=None):
        assert fault is None or fault in FAULTS, fault
        super().__init__(dtype, compute, noise, None)
        self.cap_fault = fault

    def caption_step(self, row_prob, row_id, lang_off, lengths, tokens, fed_ids, word_mask, conf, score, B, L, P, step, n_steps,
                     mask_token_id, suppress_repeats=False):
        assert L <= 64 and P >= 0 and L - 2 - P >= 1 and 0 <= step < n_steps, (L, P, step, n_steps)
        f = self.cap_fault
        self.calls.append(("caption_step", B, L, P, step, n_steps, mask_token_id, bool(suppress_repeats), lang_off is not None))
        tok, fed, wm, cf = tokens.view(B, L), fed_ids.view(B, L), word_mask.view(B, L), conf.view(B, L)
        for b in range(B):
            n = min(max(int(lengths[b]), 0), L - 2 - P)
            row0 = b * L
            if lang_off is not None:
                own = int(lang_off[b + 1]) - int(lang_off[b])
                n = min(n, max(own - 2 - P, 0))
                if f != "offset":
                    row0 = int(lang_off[b])
            free = list(range(P + 1, P + 1 + n))
            for l in free:                                                          # 1
                if wm[b, l] != 0 or f == "commit":
                    tok[b, l] = int(row_id[row0 + l])
            cf[b].zero_()                                                           # 2
            for l in free:
                cf[b, l] = row_prob[row0 + l]
            logs = torch.log(cf[b, P + 1:P + 1 + n].to(self.compute))               # 3
            score[b] = float(logs.sum() / (L if f == "score_all" else n)) if n > 0 else 0.0
            if suppress_repeats:                                                    # 4
                flagged = [l for l in free if int(tok[b, l]) == int(tok[b, l - 1])]
                if f == "sequential":
                    flagged = []
                    for l in free:
                        if int(tok[b, l]) == int(tok[b, l - 1]) and (l - 1) not in flagged:
                            flagged.append(l)
                for l in flagged:
                    cf[b, l] = -1.0
            if step + 1 < n_steps:                                                  # 5
                k = n_mask_of(n, step, n_steps)
                if f == "float":
                    k = int((n_steps - step - 1) / n_steps * n)
                if f == "count":
                    k = min(n, k + 1)
                order = sorted(free, key=lambda l: (float(cf[b, l]), -l if f == "ties" else l))
                wm[b].zero_()
                for l in order[:k]:
                    wm[b, l] = 1
            for l in range(L):                                                      # 6
                fed[b, l] = (mask_token_id if wm[b, l] != 0 else int(tok[b, l])) if l < P + n + 2 else 0


def score_bound(n_terms, logs_abs_sum):
    """|device score - float64 score| for the MEAN of n <= 64 fp32 terms log c: each logf within 2 ulp of its value (4 u relative,
    u = 2^-24), the terms added in fp32 in any order (at most n u relative to the sum of magnitudes), one division (u); all of it
    doubled (tests/bounds.SLACK), plus the absolute floor of tests/bounds.LOG_ABS = 2^-21 for terms near log 1 = 0"""
    u = 2.0 ** -24
    n = max(int(n_terms), 1)
    return 2.0 * ((4 * u + n * u + u) * logs_abs_sum / n + 2.0 ** -21) + 1e-37


assert math.isfinite(score_bound(64, 640.0))
