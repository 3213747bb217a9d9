"""TEST INFRASTRUCTURE: the host restatement of the on-chip attention entry points as a KERNEL stand-in (tests/test_bounds_cpu.py
runs tests/sdpa_edge_cases.py over it), honest or with ONE planted kernel fault.

What it adds to FakeOps, from csrc/sdpa.hip: a non-zero sdpa_keep_bits_bytes under the library's conditions and a keep_bits
buffer filled (forward) and read (backward) in the layout documented at struct KeepBits; lse written for the queries that exist
only; a zero output row (and lse = -inf) for a query without a valid key; rows of an example beyond the capacity left alone;
bias_grad accumulated; the argument checks of check_common and of the entry points (SdpaOps(..., checks=True)).  fp32 arithmetic on
bf16 / fp32 storage, reading the logical extents only and storing into the logical views only.

Faults (SdpaOps(dtype, fault=...)): `applied` counts the calls whose result the fault changed; the recorder run must fail at
exactly those.
  key32_dropped                 key 32 does not attend when nk > 32 (forward)
  mask_by_length                the key mask of a packed k side indexed by k_off[b] + j instead of b * nk + j
  mask_255_off                  a mask byte is read as a signed char: 255 is off
  pad_not_zeroed                the pad rows [off[B], pad) keep their content
  pad_one_row_too_far           the pad zeroing runs to row pad inclusive
  store_next_head               the last head's store of the last row runs one column into what follows its dh columns (forward)
  lse_missing_query             lse written for every query of the capacity
  dropout_row_by_length         the dropout row counter is bh * len + q instead of bh * nq + q on a packed q side
  step_seed_ignored_bwd         the hashing backward does not add the step seed
  keep_bit_halves_swapped       halves h of the keep_bits layout swapped, by the forward and the backward alike
  bias_overwritten              bias_grad = instead of +=
  bias_stale_pad_row            the bias sums of a packed side run one row beyond the zeroed pad rows
  dv_without_dropout_scale      dV from the 0 / 1 mask without 1 / (1 - p)
  delta_second_fragment_lost    delta summed over keys 0..31 only
  generic_tail_features_dropped the generic forward's q.k stops at the last whole 8 features of dh
  fp32_through_bf16             an fp32 output rounded through bf16
  round_toward_zero             the generic kernels' bf16 stores round toward zero (on the MFMA path the designed bf16 rounding of
                                P, U16 |P'||V| >= U16 |O|, is larger than the difference between the two rounding modes)"""
import torch

from fake_ops import FakeOps, keep_scale

FAULTS = ("key32_dropped", "mask_by_length", "mask_255_off", "pad_not_zeroed", "pad_one_row_too_far", "store_next_head",
          "lse_missing_query", "dropout_row_by_length", "step_seed_ignored_bwd", "keep_bit_halves_swapped", "bias_overwritten",
          "bias_stale_pad_row", "dv_without_dropout_scale", "delta_second_fragment_lost", "generic_tail_features_dropped",
          "fp32_through_bf16", "round_toward_zero")


class Refused(RuntimeError):
    pass


def rtz(x):
    """round toward zero to bf16 (drop the low 16 bits of the fp32 pattern)"""
    i = x.float().contiguous().view(torch.int32) & -65536
    return i.view(torch.float32).to(torch.bfloat16)


def _al16(t):
    return t.data_ptr() % 16 == 0


class SdpaOps(FakeOps):
    def __init__(self, dtype, fault=None, checks=False):
        super().__init__(dtype)
        assert fault is None or fault in FAULTS, fault
        self.fault, self.applied, self.checks = fault, 0, checks

    # ------------------------------------------------------------------------------------------------ dispatch and argument checks
    def _eligible(self, dh, lds, ptrs):
        return (self.dtype == torch.bfloat16 and dh in (16, 32, 64) and all(ld % 8 == 0 for ld in lds) and all(_al16(t) for t in ptrs))

    def sdpa_keep_bits_bytes(self, B, H, nq, nk, dh):
        if min(B, H, nq, nk) <= 0 or nq > 64 or nk > 64 or self.dtype != torch.bfloat16 or dh not in (16, 32, 64):
            return 0
        return B * H * ((nq + 31) // 32) * ((nk + 31) // 32) * 32 * 4

    def _check(self, fn, B, H, nq, nk, dh, p_drop, tensors, keep_bits=None, eligible=True, bias_lds=None):
        if not self.checks:
            return
        if not (B > 0 and H > 0 and 0 < nq <= 512 and 0 < nk <= 512):
            raise Refused(f"{fn} failed (-1): need 1 <= nq,nk <= 512")
        if not 0 < dh <= 64:
            raise Refused(f"{fn} failed (-1): head size {dh}")
        if not 0.0 <= p_drop < 1.0:
            raise Refused(f"{fn} failed (-2): p_drop {p_drop}")
        if any(t is None for t in tensors):
            raise Refused(f"{fn} failed (-2): null pointer")
        if keep_bits is not None and not (self.sdpa_keep_bits_bytes(B, H, nq, nk, dh) > 0 and eligible and _al16(keep_bits)):
            raise Refused(f"{fn} failed (-2): keep_bits only exists on the on-chip bf16 path")
        assert nq <= 64 and nk <= 64, "the long-sequence kernels are not restated here"
        if bias_lds is not None:                # bias_grad without fused partials: xl_colsum of the stored gradients, whole vectors only
            vec = 8 if self.dtype == torch.bfloat16 else 4
            if any(x % vec for x in (H * dh,) + tuple(bias_lds)):
                raise Refused(f"{fn} failed (-1): bias_grad from column sums needs H * dh and lddq, lddk, lddv to be multiples of {vec}")

    # ------------------------------------------------------------------------------------------------ pieces
    @staticmethod
    def _lens(off, n, B):
        if off is None:
            return [n] * B
        o = [int(x) for x in off.view(-1)[:B + 1]]
        return [min(n, o[b + 1] - o[b]) for b in range(B)]

    def _valid(self, key_mask, B, nq, nk, q_off, k_off, H=1, lse=None):
        """[B, 1, nq, nk]: the (query, key) pairs that exist and attend"""
        lq, lk = self._lens(q_off, nq, B), self._lens(k_off, nk, B)
        j = torch.arange(nk)
        valid = torch.stack([(torch.arange(nq) < lq[b])[:, None] & (j < lk[b])[None, :] for b in range(B)])[:, None]
        if key_mask is not None:
            m = key_mask.reshape(-1)[:B * nk].view(B, nk)
            on = m != 0
            if self.fault == "mask_255_off":
                on = m.to(torch.int8) > 0
            if self.fault == "mask_by_length" and k_off is not None:
                o = [int(x) for x in k_off.view(-1)[:B + 1]]
                flat = torch.cat([key_mask.reshape(-1), torch.zeros(nk + o[B], dtype=key_mask.dtype)])
                on = torch.stack([flat[o[b]:o[b] + nk] for b in range(B)]) != 0
            honest = valid & (m != 0).view(B, 1, 1, nk)
            valid = valid & on.view(B, 1, 1, nk)
            # (a backward or attn_probs row whose saved lse is -inf is zero whatever attends: no change to count there)
            live = True if lse is None else torch.isfinite(lse.view(B, H, nq, 1))
            if bool(((valid != honest) & live).any()):
                self.applied += 1
        return valid, lq, lk

    def _keep(self, B, H, nq, nk, p_drop, seed, lq, q_off, use_step=True):
        """the 0 / 1 keep decisions [B, H, nq, nk] by the counter hash: row (b H + h) nq + q, column key"""
        s = self._seed(seed) if use_step else seed
        row = torch.arange(B * H * nq).view(B, H, nq, 1)
        if self.fault == "dropout_row_by_length" and q_off is not None:
            row = torch.stack([(torch.arange(H) + b * H)[:, None] * lq[b] + torch.arange(nq)[None, :] for b in range(B)])[..., None]
        keep = keep_scale(s, row, torch.arange(nk).view(1, 1, 1, nk), p_drop) > 0
        honest = keep_scale(self._seed(seed), torch.arange(B * H * nq).view(B, H, nq, 1), torch.arange(nk).view(1, 1, 1, nk), p_drop) > 0
        return keep, honest

    def _bit_index(self, B, H, nq, nk):
        """(dword, bit) of every (bh, query, key) in the keep_bits buffer"""
        nqf, nkf = (nq + 31) // 32, (nk + 31) // 32
        bh, q, key = torch.arange(B * H).view(-1, 1, 1), torch.arange(nq).view(1, -1, 1), torch.arange(nk).view(1, 1, -1)
        j, t, i, k31 = q // 32, q % 32, key // 32, key % 32
        h, r = (k31 >> 2) & 1, (k31 & 3) + 4 * (k31 >> 3)
        if self.fault == "keep_bit_halves_swapped":
            h = 1 - h
        word = (bh * nqf + j) * (nkf * 32) + (i * 16 + r) * 2 + h
        return torch.broadcast_tensors(word, t)

    def _store_rows(self, dst, val, B, n, H, dh, ld, off, pad):
        """FakeOps._store with the output rounding and the pad faults"""
        HD = H * dh
        if self.fault == "fp32_through_bf16" and dst.dtype == torch.float32:
            val = val.to(torch.bfloat16).float()
            self.applied_now = True
        if self.fault == "round_toward_zero" and dst.dtype == torch.bfloat16 and self._generic:
            val = rtz(val)
            self.applied_now = True
        if off is None:
            self._heads(dst, B, n, H, dh, ld).copy_(val)
            return
        o = [int(x) for x in off.view(-1)[:B + 1]]
        rows = val.permute(0, 2, 1, 3).reshape(B, n, HD)
        for b in range(B):
            m = min(n, o[b + 1] - o[b])
            torch.as_strided(dst, (m, HD), (ld, 1), dst.storage_offset() + o[b] * ld).copy_(rows[b, :m])
        hi = pad
        if self.fault == "pad_not_zeroed" and pad > o[B]:
            hi, self.applied_now = o[B], True
        if self.fault == "pad_one_row_too_far" and pad >= o[B]:
            hi, self.applied_now = pad + 1, True
        if hi > o[B]:
            torch.as_strided(dst, (hi - o[B], HD), (ld, 1), dst.storage_offset() + o[B] * ld).zero_()

    # ------------------------------------------------------------------------------------------------ entry points
    def sdpa_fwd(self, q, k, v, key_mask, o, lse, B, H, nq, nk, dh, ldq, ldk, ldv, ldo, scale, p_drop=0.0, seed=0,
                 q_off=None, k_off=None, q_pad=0, k_pad=0, keep_bits=None):
        eligible = None not in (q, k, v, o) and self._eligible(dh, (ldq, ldk, ldv, ldo), (q, k, v, o))
        self._check("xl_sdpa_fwd", B, H, nq, nk, dh, p_drop, (q, k, v, o, lse), keep_bits, eligible)
        self._generic, self.applied_now = not eligible, False
        f = self.fault
        (Q, _), (K_, _), (V_, _) = (self._load(t, B, n, H, dh, ld, off)
                                    for t, n, ld, off in ((q, nq, ldq, q_off), (k, nk, ldk, k_off), (v, nk, ldv, k_off)))
        valid, lq, lk = self._valid(key_mask, B, nq, nk, q_off, k_off)
        if f == "key32_dropped" and nk > 32:
            self.applied_now = self.applied_now or bool(valid[..., 32].any())
            valid = valid.clone()
            valid[..., 32] = False
        if f == "generic_tail_features_dropped" and self._generic and dh % 8:
            Q = Q.clone()
            Q[..., dh - dh % 8:] = 0
            self.applied_now = True
        s = (Q @ K_.transpose(-1, -2) * scale).masked_fill(~valid, float("-inf"))
        l = torch.logsumexp(s, -1)
        p = torch.softmax(s, -1).nan_to_num(0.0)
        if p_drop > 0:
            keep, honest = self._keep(B, H, nq, nk, p_drop, seed, lq, q_off)
            self.applied_now = self.applied_now or bool(((keep != honest) & valid).any())
            p = p * keep * float(torch.tensor(1.0 / (1.0 - p_drop), dtype=torch.float32))
            if keep_bits is not None:                       # all 32 x 32 elements of every fragment, like the kernel
                nqf, nkf = (nq + 31) // 32, (nk + 31) // 32
                row = row0 = torch.arange(B * H).view(-1, 1, 1) * nq + torch.arange(nqf * 32).view(1, -1, 1)
                if f == "dropout_row_by_length" and q_off is not None:
                    row = (torch.arange(B * H).view(-1, 1, 1) * torch.tensor(lq).repeat_interleave(H).view(-1, 1, 1)
                           + torch.arange(nqf * 32).view(1, -1, 1))
                full = keep_scale(self._seed(seed), row, torch.arange(nkf * 32).view(1, 1, -1), p_drop) > 0
                if row is not row0:
                    self.applied_now = self.applied_now or not torch.equal(
                        full, keep_scale(self._seed(seed), row0, torch.arange(nkf * 32).view(1, 1, -1), p_drop) > 0)
                word, bit = self._bit_index(B, H, nqf * 32, nkf * 32)
                words = torch.zeros(B * H * nqf * nkf * 32, dtype=torch.int64)
                words.index_add_(0, word.reshape(-1), (full.to(torch.int64) << bit.to(torch.int64)).reshape(-1))
                words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)
                keep_bits.reshape(-1)[:words.numel()].copy_(words.to(torch.int32))
                if f == "keep_bit_halves_swapped":
                    self.applied_now = True
        out = p @ V_
        self._store_rows(o, out, B, nq, H, dh, ldo, q_off, q_pad)
        if f == "store_next_head":
            last = (B * nq if q_off is None else sum(self._lens(q_off, 10 ** 6, B)[:-1]) + lq[-1]) - 1
            if last >= 0 and (q_off is None or lq[-1] > 0):
                torch.as_strided(o, (1,), (1,), o.storage_offset() + last * ldo + H * dh).zero_()
                self.applied_now = True
        lv = lse.view(B, H, nq)
        for b in range(B):
            m = nq if f == "lse_missing_query" else lq[b]
            if f == "lse_missing_query" and lq[b] < nq:
                self.applied_now = True
            lv[b, :, :m] = l[b, :, :m]
        self.applied += int(self.applied_now)

    def attn_probs(self, q, k, key_mask, lse, probs, B, H, nq, nk, dh, ldq, ldk, scale, p_drop=0.0, seed=0, q_off=None, k_off=None):
        self._check("xl_attn_probs", B, H, nq, nk, dh, p_drop, (q, k, lse, probs))
        self.applied_now = False
        (Q, _), (K_, _) = self._load(q, B, nq, H, dh, ldq, q_off), self._load(k, B, nk, H, dh, ldk, k_off)
        valid, lq, _ = self._valid(key_mask, B, nq, nk, q_off, k_off, H, lse)
        p = torch.exp(Q @ K_.transpose(-1, -2) * scale - lse.view(B, H, nq, 1)).masked_fill(~valid, 0.0)
        p = torch.nan_to_num(p, nan=0.0, posinf=0.0)
        if p_drop > 0:
            keep, honest = self._keep(B, H, nq, nk, p_drop, seed, lq, q_off)
            self.applied_now = bool(((keep != honest) & valid).any())
            p = p * keep * float(torch.tensor(1.0 / (1.0 - p_drop), dtype=torch.float32))
        probs.view(B, H, nq, nk).copy_(p)
        self.applied += int(self.applied_now)

    def sdpa_bwd(self, q, k, v, key_mask, dout, lse, dq, dk, dv, B, H, nq, nk, dh, ldq, ldk, ldv, ldo, lddq, lddk,
                 lddv, scale, p_drop=0.0, seed=0, bias_grad=None, ws=None, q_off=None, k_off=None, q_pad=0, k_pad=0, keep_bits=None):
        ts = (q, k, v, dout, dq, dk, dv)
        eligible = None not in ts and self._eligible(dh, (ldq, ldk, ldv, ldo, lddq, lddk, lddv), ts)
        fused = eligible and ws is not None and B * 3 * H * dh <= self.workspace_floats(H * dh)
        self._check("xl_sdpa_bwd", B, H, nq, nk, dh, p_drop, ts + (lse,), keep_bits, eligible,
                    (lddq, lddk, lddv) if (bias_grad is not None and not fused) else None)
        self._generic, self.applied_now = not eligible, False
        f = self.fault
        (Q, _), (K_, _), (V_, _), (dO, _) = (self._load(t, B, n, H, dh, ld, off) for t, n, ld, off in
                                             ((q, nq, ldq, q_off), (k, nk, ldk, k_off), (v, nk, ldv, k_off), (dout, nq, ldo, q_off)))
        valid, lq, lk = self._valid(key_mask, B, nq, nk, q_off, k_off, H, lse)
        p = torch.exp(Q @ K_.transpose(-1, -2) * scale - lse.view(B, H, nq, 1)).masked_fill(~valid, 0.0)
        p = torch.nan_to_num(p, nan=0.0, posinf=0.0)
        inv_keep, keep = 1.0, None
        if p_drop > 0:
            inv_keep = float(torch.tensor(1.0 / (1.0 - p_drop), dtype=torch.float32))
            if keep_bits is not None:
                word, bit = self._bit_index(B, H, nq, nk)
                w = keep_bits.reshape(-1).to(torch.int64) & 0xFFFFFFFF
                keep = ((w[word] >> bit.to(torch.int64)) & 1).bool().view(B, H, nq, nk)
                honest = FakeOps._pmask(B, H, nq, nk, p_drop, self._seed(seed)) > 0
                self.applied_now = self.applied_now or (f is not None and bool(((keep != honest) & valid).any()))
            else:
                ignore = f == "step_seed_ignored_bwd" and self.step_seed is not None
                keep, honest = self._keep(B, H, nq, nk, p_drop, seed, lq, q_off, use_step=not ignore)
                self.applied_now = self.applied_now or bool(((keep != honest) & valid).any())
        msk = 1.0 if keep is None else keep * inv_keep
        dp = (dO @ V_.transpose(-1, -2)) * msk
        pd = p * dp
        if f == "delta_second_fragment_lost" and nk > 32:
            self.applied_now = self.applied_now or bool((pd[..., 32:] != 0).any())
            pd = pd[..., :32]
        delta = pd.sum(-1, keepdim=True)
        ds = p * (dp - delta) * scale
        pk = p * msk
        gq, gk, gv = ds @ K_, ds.transpose(-1, -2) @ Q, pk.transpose(-1, -2) @ dO
        if f == "dv_without_dropout_scale" and p_drop > 0:
            gv, self.applied_now = (p * keep).transpose(-1, -2) @ dO, True
        sides = ((dq, gq, nq, lddq, q_off, q_pad), (dk, gk, nk, lddk, k_off, k_pad), (dv, gv, nk, lddv, k_off, k_pad))
        stale = []
        for dst, g, n, ld, off, pad in sides:
            if off is not None:                             # the row behind the pad rows, before this call writes anything
                o = [int(x) for x in off.view(-1)[:B + 1]]
                stale.append(torch.as_strided(dst, (H * dh,), (1,), dst.storage_offset() + max(pad, o[B]) * ld).float().clone())
            else:
                stale.append(None)
        for dst, g, n, ld, off, pad in sides:
            self._store_rows(dst, g, B, n, H, dh, ld, off, pad)
        if bias_grad is not None:
            HD = H * dh
            for i, ((dst, g, n, ld, off, pad), st) in enumerate(zip(sides, stale)):
                if off is None:
                    sm = g.sum(dim=(0, 2)).reshape(HD)
                else:                                       # rows that exist only (a dense g holds garbage-free zeros elsewhere)
                    ln = self._lens(off, n, B)
                    sm = sum(g[b, :, :ln[b]].sum(1).reshape(HD) for b in range(B))
                    if f == "bias_stale_pad_row":
                        sm, self.applied_now = sm + st, True
                if f == "bias_overwritten":
                    bias_grad[i * HD:(i + 1) * HD] = sm
                    self.applied_now = True
                else:
                    bias_grad[i * HD:(i + 1) * HD] += sm
        self.applied += int(self.applied_now)
