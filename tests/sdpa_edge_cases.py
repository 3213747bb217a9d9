"""The calls of tests/test_sdpa_edges_bounds_gpu.py and of its host twin in tests/test_bounds_cpu.py: xl_sdpa_fwd, xl_sdpa_bwd and
xl_attn_probs on the on-chip path (nq, nk <= 64) at the edges of their dispatch (tests/test_kernel_bounds_gpu.sdpa_kernel restates
it).  Plain functions, no tests: each family takes a recorder-like `rec` (Recorder over HipOps or over the host restatement), a
device and a seeded CPU generator -- the data is drawn on the host and moved, so both sides run the same numbers --, issues its
calls through the ops interface only and returns how many it issued.  Every call has a signature of its own (shape, leading
dimensions, pad counts, which optional tensors are present, dropout on or off, alignment, kernel label), so the recorder checks
every one.

Storage, as the engine lays it out.  q, k and v are column slices of ONE [rows, ld] allocation (ld >= 3 H dh), dq, dk and dv
slices of another; o, dout, lse, bias_grad, the workspace and keep_bits have allocations of their own.  An operand whose leading
dimension or base the case changes alone (the eligibility family) moves into an allocation of its own.  Every allocation has GR
guard rows in front of the base and behind the last row.  What a correct kernel must not READ -- rows at and beyond off[B] of a
packed operand, the pad columns beyond 3 H dh, the guard rows -- holds +-2^12 (POISON): one such element in a 64-deep sum is
orders of magnitude beyond any bound.  What it must not WRITE starts as SENTINEL (never zero: the kernels write zeros into pad
rows), every output is refilled with it before every call, and the recorder holds everything outside the logical views of the
outputs to its earlier bits (the row "outside view")."""
import torch

BF, F32 = torch.bfloat16, torch.float32
GR = 4                      # guard rows in front of and behind a [rows, ld] allocation
G1 = 64                     # guard elements around a flat allocation
POISON = 4096.0
SENTINEL = 12345.0
BITS_FILL = 0x5A5A5A5A
MASK_BYTES = (0, 1, 2, 255)

FRAG_SHAPES = ((1, 1), (32, 32), (33, 32), (32, 33), (33, 33), (31, 64), (64, 31), (1, 64), (64, 1), (64, 64))
ELIG_BASES = ((20, 64, 64), (33, 20, 32))                    # (nq, nk, dh)
ELIG_DH = (1, 8, 24, 48, 63)
FWD_LDS, BWD_LDS = ("ldq", "ldk", "ldv", "ldo"), ("ldq", "ldk", "ldv", "ldo", "lddq", "lddk", "lddv")
FWD_PTRS, BWD_PTRS = ("q", "k", "v", "o"), ("q", "k", "v", "dout", "dq", "dk", "dv")
# (nq capacity, nk capacity, q lengths, k lengths ("same": the q offset vector itself), pad rows beyond off[B])
PACKED = ((64, 20, (1, 32, 33, 64), None, 0),
          (20, 64, None, (67, 0, 33, 1), 1),
          (64, 64, (1, 32, 33, 64), "same", 37),
          (64, 64, (67, 0, 33, 1), "same", 0),
          (64, 64, (33, 1, 64, 0), (1, 67, 32, 33), 1),
          (20, 33, (20, 23, 1, 7), (33, 1, 36, 32), 37))


def _poison(g, n, dtype):
    return ((torch.randint(0, 2, (n,), generator=g) * 2 - 1).float() * POISON).to(dtype)


def flat_out(dev, n, dtype=F32, fill=None):
    """an n-element output between guards of SENTINEL; `fill`: its content before the call"""
    buf = torch.full((G1 + n + G1,), SENTINEL if dtype.is_floating_point else BITS_FILL, dtype=dtype)
    if fill is not None:
        buf[G1:G1 + n] = fill.reshape(-1).to(dtype)
    return buf.to(dev)[G1:G1 + n]


class Case:
    """the operands of one attention geometry.  lens: per-example row counts of a packed side (None: dense); pads: rows beyond off[B]
    that the kernels zero; lds: leading dimensions changed alone; shifts: operands whose base is advanced by 4 elements; uniq: widens
    every leading dimension by 8 * uniq (a signature of its own for calls that differ in content only)."""

    def __init__(self, g, dev, B, H, nq, nk, dh, dtype=BF, uniq=0, q_lens=None, k_lens=None, pads=(0, 0), mask=False, lds=None,
                 shifts=(), extreme=False):
        self.g, self.dev, self.B, self.H, self.nq, self.nk, self.dh, self.dtype = g, dev, B, H, nq, nk, dh, dtype
        HD = self.HD = H * dh
        ld3, ld1 = 3 * HD + 8 * uniq, HD + 8 * uniq
        self.ld = dict(ldq=ld3, ldk=ld3, ldv=ld3, ldo=ld1, lddq=ld3, lddk=ld3, lddv=ld3)
        self.ld.update(lds or {})
        self.scale = dh ** -0.5
        self.q_len = [nq] * B if q_lens is None else list(q_lens)
        same = isinstance(k_lens, str)
        self.k_len = [nk] * B if k_lens is None else self.q_len if same else list(k_lens)

        def offsets(lens):
            off = torch.zeros(B + 1, dtype=torch.int32)
            off[1:] = torch.cumsum(torch.tensor(lens), 0)
            return off
        self.q_off_h = None if q_lens is None else offsets(self.q_len)
        self.k_off_h = None if k_lens is None else self.q_off_h if same else offsets(self.k_len)
        self.q_off = None if q_lens is None else self.q_off_h.to(dev)
        self.k_off = None if k_lens is None else self.q_off if same else self.k_off_h.to(dev)
        self.vq = B * nq if q_lens is None else int(self.q_off_h[B])                # rows that hold data
        self.vk = B * nk if k_lens is None else int(self.k_off_h[B])
        self.q_pad = 0 if q_lens is None else self.vq + pads[0]
        self.k_pad = 0 if k_lens is None else self.vk + pads[1]
        self.rq, self.rk = max(self.vq, self.q_pad), max(self.vk, self.k_pad)      # rows a side's outputs span
        R = max(self.rq, self.rk, 1)

        amp = 4.0 if extreme else 1.0
        data = {"q": torch.randn(self.vq, HD, generator=g) * amp, "k": torch.randn(self.vk, HD, generator=g) * amp,
                "v": torch.randn(self.vk, HD, generator=g), "dout": torch.randn(self.vq, HD, generator=g)}
        if extreme:                                           # example 0: every score strongly negative
            data["q"][:self.q_len[0] if q_lens is not None else nq].abs_()
            data["k"][:self.k_len[0] if k_lens is not None else nk].abs_().neg_()
        self.host = {k: v.to(dtype) for k, v in data.items()}
        bufs, where = {}, {}

        def alloc(key, rows, ld, poison):
            n = (2 * GR + rows) * ld + 16
            bufs[key] = _poison(g, n, dtype) if poison else torch.full((n,), SENTINEL, dtype=dtype)
            return GR * ld

        base_in = alloc("in", R, ld3, True)
        base_g = alloc("grad", R, ld3, False)
        plan = (("q", "ldq", 0, self.rq, self.vq, "in", base_in), ("k", "ldk", HD, self.rk, self.vk, "in", base_in),
                ("v", "ldv", 2 * HD, self.rk, self.vk, "in", base_in), ("dout", "ldo", 0, self.rq, self.vq, None, 0),
                ("o", "ldo", 0, self.rq, 0, None, 0), ("dq", "lddq", 0, self.rq, 0, "grad", base_g),
                ("dk", "lddk", HD, self.rk, 0, "grad", base_g), ("dv", "lddv", 2 * HD, self.rk, 0, "grad", base_g))
        for nm, key, col, rows, valid, fused, base in plan:
            ld, sh = self.ld[key], 4 if nm in shifts else 0
            if fused is None or ld != ld3 or sh:
                fused, col, base = nm, 0, alloc(nm, rows, ld, nm in self.host) + sh
            if nm in self.host:
                torch.as_strided(bufs[fused], (valid, HD), (ld, 1), base + col).copy_(self.host[nm])
            where[nm] = (fused, base + col)
        self._bufs = {k: b.to(dev) for k, b in bufs.items()}
        self._outs = {where[nm][0] for nm in ("o", "dq", "dk", "dv")}
        for nm, (key, start) in where.items():
            setattr(self, nm, self._bufs[key][start:])
        self.lse = flat_out(dev, B * H * nq)
        self.mask_h = self._mask() if mask else None
        self.mask = None if self.mask_h is None else self.mask_h.reshape(-1).to(dev)

    def _mask(self):
        """bytes from {0, 1, 2, 255}; example 0: only key 0 on; example 1: every key off"""
        B, nk = self.B, self.nk
        m = torch.tensor(MASK_BYTES, dtype=torch.uint8)[torch.randint(0, 4, (B, nk), generator=self.g)]
        m[:, 0] = 255
        m[0, 1:] = 0
        m[1] = 0
        return m

    def reset(self):
        """every output back to SENTINEL (a store that does not happen must not find the previous call's value)"""
        for k in self._outs:
            self._bufs[k].fill_(SENTINEL)

    def host_lse(self):
        """the float64 log-sum-exp of the scores, on the host, into self.lse: what a backward or attn_probs call READS (the
        reference reads the same buffer), for the calls that have no forward of their own kernel family in front of them; the
        entries of missing queries keep SENTINEL, those of a query without a key get -inf"""
        B, H, nq, nk, dh = self.B, self.H, self.nq, self.nk, self.dh
        out = torch.full((B, H, nq), SENTINEL, dtype=torch.float64)
        q, k = self.host["q"].double(), self.host["k"].double()
        q0 = self.q_off_h if self.q_off_h is not None else torch.arange(B + 1) * nq
        k0 = self.k_off_h if self.k_off_h is not None else torch.arange(B + 1) * nk
        if self.q_off_h is None and self.k_off_h is None:
            s = torch.einsum("bqhd,bkhd->bhqk", q.view(B, nq, H, dh), k.view(B, nk, H, dh)) * self.scale
            if self.mask_h is not None:
                s = s.masked_fill(self.mask_h.view(B, 1, 1, nk) == 0, -float("inf"))
            out = torch.logsumexp(s, -1)
        else:
            for b in range(B):
                lq, lk = min(nq, self.q_len[b]), min(nk, self.k_len[b])
                qb = q[int(q0[b]):int(q0[b]) + lq].view(lq, H, dh)
                kb = k[int(k0[b]):int(k0[b]) + lk].view(lk, H, dh)
                s = torch.einsum("qhd,khd->hqk", qb, kb) * self.scale
                if self.mask_h is not None:
                    s = s.masked_fill(self.mask_h[b, :lk].view(1, 1, lk) == 0, -float("inf"))
                out[b, :, :lq] = torch.logsumexp(s, -1) if lk else -float("inf")
        self.lse.copy_(out.reshape(-1).float().to(self.dev))

    def keep_bits(self, rec):
        n = rec.sdpa_keep_bits_bytes(self.B, self.H, self.nq, self.nk, self.dh)
        assert n > 0 and n % 4 == 0, n
        return flat_out(self.dev, n // 4, torch.int32)

    def fwd(self, rec, p=0.0, seed=0, kb=None):
        self.reset()
        self.lse.fill_(SENTINEL)
        L = self.ld
        rec.sdpa_fwd(self.q, self.k, self.v, self.mask, self.o, self.lse, self.B, self.H, self.nq, self.nk, self.dh, L["ldq"], L["ldk"],
                     L["ldv"], L["ldo"], self.scale, p_drop=p, seed=seed, q_off=self.q_off, k_off=self.k_off, q_pad=self.q_pad,
                     k_pad=self.k_pad, keep_bits=kb)
        return 1

    def bwd(self, rec, p=0.0, seed=0, kb=None, bias=None, ws=None):
        self.reset()
        L = self.ld
        rec.sdpa_bwd(self.q, self.k, self.v, self.mask, self.dout, self.lse, self.dq, self.dk, self.dv, self.B, self.H, self.nq, self.nk,
                     self.dh, L["ldq"], L["ldk"], L["ldv"], L["ldo"], L["lddq"], L["lddk"], L["lddv"], self.scale, p_drop=p, seed=seed,
                     bias_grad=bias, ws=ws, q_off=self.q_off, k_off=self.k_off, q_pad=self.q_pad, k_pad=self.k_pad, keep_bits=kb)
        return 1

    def probs(self, rec, p=0.0, seed=0):
        out = flat_out(self.dev, self.B * self.H * self.nq * self.nk)
        rec.attn_probs(self.q, self.k, self.mask, self.lse, out, self.B, self.H, self.nq, self.nk, self.dh, self.ld["ldq"], self.ld["ldk"],
                       self.scale, p_drop=p, seed=seed, q_off=self.q_off, k_off=self.k_off)
        return 1

    def three_backwards(self, rec, seed=11, **kw):
        """the three instantiations of the backward, each behind the forward that goes with it: no dropout; dropout hashed in both
        directions; dropout with the forward's saved keep_bits read back"""
        n = self.fwd(rec) + self.bwd(rec, **kw)
        n += self.fwd(rec, 0.1, seed) + self.bwd(rec, 0.1, seed, **kw)
        kb = self.keep_bits(rec)
        return n + self.fwd(rec, 0.1, seed, kb) + self.bwd(rec, 0.1, seed, kb, **kw)


def bias_buffers(rec, dev, g, HD, ws=True, amp=2.0):
    """a bias gradient that already holds values of +-amp..2 amp (it is accumulated; amp = 100 at the workspace limit: above the
    bound of a sum over 2732 rows, so that an overwrite shows at every call), and the workspace of rec.workspace_floats(HD) floats"""
    sign = torch.randint(0, 2, (3 * HD,), generator=g) * 2.0 - 1.0
    bias = flat_out(dev, 3 * HD, fill=sign * amp * (1.0 + torch.rand(3 * HD, generator=g)))
    return bias, (flat_out(dev, rec.workspace_floats(HD)) if ws else None)


# ------------------------------------------------------------------------------------------------------------------------ families
def fragments(rec, dev, g, dhs=(16, 32, 64), shapes=FRAG_SHAPES, masks=(False, True), B=3, H=2):
    """both sides of every XL_CASE boundary x head size x key mask x the three backward instantiations"""
    n = 0
    for dh in dhs:
        for nq, nk in shapes:
            for mask in masks:
                n += Case(g, dev, B, H, nq, nk, dh, mask=mask).three_backwards(rec)
    return n


def eligibility(rec, dev, g, dtype=BF, bases=ELIG_BASES, dhs=ELIG_DH, B=3, H=2):
    """bf16: every condition of mfma_eligible broken alone (a leading dimension of 8 k + 4, a base advanced by 8 bytes), and the
    head sizes without an MFMA instance.  fp32: the same shapes.  The backward reads a host log-sum-exp, so no call of this family
    runs on another kernel family."""
    n = 0
    for nq, nk, dh0 in bases:
        runs = [(dh0, {}, ())] if dtype == F32 else []
        if dtype == BF:
            runs += [(dh0, {k: (H * dh0 if k == "ldo" else 3 * H * dh0) + 4}, ()) for k in BWD_LDS]
            runs += [(dh0, {}, (p,)) for p in ("q", "k", "v", "o", "dout", "dq", "dk", "dv")]
        runs += [(dh, {}, ()) for dh in dhs]
        for i, (dh, lds, shifts) in enumerate(runs):
            c = Case(g, dev, B, H, nq, nk, dh, dtype, lds=lds, shifts=shifts, mask=i % 2 == 1)
            p = 0.1 if i % 3 == 0 else 0.0
            if dtype == F32 or dh != dh0 or any(k in FWD_LDS for k in lds) or any(s in FWD_PTRS for s in shifts):
                n += c.fwd(rec, p, 5)
            if dtype == F32 or dh != dh0 or lds or any(s in BWD_PTRS for s in shifts):
                c.host_lse()
                n += c.bwd(rec, p, 5)
    return n


def packed(rec, dev, g, dtype=BF, path="mfma", configs=PACKED, B=4, H=2, dh=32):
    """packed q, packed k, one shared offset vector, two different ones; lengths 1 / 32 / 33 / capacity / capacity + 3 / 0; pads of
    0, 1 and 37 rows; with a key mask (indexed by capacity) and dropout.  path "generic": bf16 with an odd ldo (and, every other
    case, odd gradient strides), the element-wise branch of zero_pad_rows."""
    n = 0
    for i, (nq, nk, ql, kl, pad) in enumerate(configs):
        HD = H * dh
        lds = {}
        if path == "generic":
            lds = {"ldo": HD + 1} if i % 2 == 0 else {"ldo": HD + 3, "lddq": 3 * HD + 1, "lddk": 3 * HD + 1, "lddv": 3 * HD + 3}
        for mask, p in ((False, 0.0), (True, 0.1)):
            c = Case(g, dev, B, H, nq, nk, dh, dtype, uniq=i + 1, q_lens=ql, k_lens=kl, pads=(pad, pad), mask=mask, lds=lds)
            kb = c.keep_bits(rec) if (p > 0 and path == "mfma" and dtype == BF) else None
            n += c.fwd(rec, p, 21 + i, kb) + c.bwd(rec, p, 21 + i, kb)
    return n


def bias_gradients(rec, dev, g, B=3, H=2, dh=32, nq=20, nk=33):
    """bias_grad (accumulated: it starts non-zero) through the fused partials, through the three column sums of the stored
    gradients with and without a workspace, on the generic path, with packed rows, and on both sides of the workspace limit
    B * 3 * H * dh <= workspace_floats(H * dh); then once with deferred second stages and a flush.  The generic path is reached
    through an INPUT stride of 8 k + 4: the column sums take whole 16-byte vectors of the stored gradients, so a gradient stride
    off 8 with bias_grad is a call the entry point refuses (the rejected family)."""
    n = 0
    HD = H * dh
    for i, (ws, lds, packed_) in enumerate(((True, {}, False), (False, {}, False), (True, {"ldq": 3 * HD + 4}, False),
                                            (False, {"ldq": 3 * HD + 4}, False), (True, {}, True), (True, {"ldk": 3 * HD + 4}, True),
                                            (False, {}, True))):
        ql = (20, 1, 7) if packed_ else None
        c = Case(g, dev, B, H, nq, nk, dh, uniq=i, q_lens=ql, k_lens=(33, 30, 2) if packed_ else None, pads=(5, 1), mask=i % 2 == 1, lds=lds)
        c.host_lse()
        bias, w = bias_buffers(rec, dev, g, HD, ws)
        n += c.bwd(rec, 0.1 if i % 2 == 0 else 0.0, 31, bias=bias, ws=w)
    limit = rec.workspace_floats(16) // (3 * 16)                  # the last B with fused partials (H = 1, dh = 16)
    for Bb in (limit, limit + 1):
        c = Case(g, dev, Bb, 1, 2, 2, 16)
        c.host_lse()
        bias, w = bias_buffers(rec, dev, g, 16, amp=100.0)
        n += c.bwd(rec, bias=bias, ws=w)
    rec.set_deferred_reduce(1)
    try:
        for i, lds in enumerate(({}, {"ldv": 3 * HD + 4})):       # fused partials; three column sums in flight on thirds of the workspace
            c = Case(g, dev, B, H, nq, nk, dh, uniq=8 + i, lds=lds)
            c.host_lse()
            bias, w = bias_buffers(rec, dev, g, HD)
            n += c.bwd(rec, 0.1, 33, bias=bias, ws=w)
            rec.flush_reductions()
    finally:
        rec.set_deferred_reduce(0)
    return n


def dropout(rec, dev, g, B=3, H=2, dh=64):
    """p_drop 0.1 and 0.5 under a seed above 2^32; the step seed (a device int64 holding 3) added in the hashed forward, the hashed
    backward and -- through the forward's bits -- the backward from keep_bits; keep_bits passed with p_drop = 0 (never written)"""
    n = 0
    seed = (1 << 33) + 5
    for p, (nq, nk) in ((0.1, (33, 33)), (0.5, (31, 64))):
        c = Case(g, dev, B, H, nq, nk, dh, mask=True)
        kb = c.keep_bits(rec)
        n += c.fwd(rec, p, seed, kb) + c.bwd(rec, p, seed, kb) + c.fwd(rec, p, seed) + c.bwd(rec, p, seed)
    step = torch.tensor([3], dtype=torch.int64).to(dev)
    rec.set_step_seed_ptr(step)
    try:
        c = Case(g, dev, B, H, 64, 31, dh)
        kb = c.keep_bits(rec)
        n += c.fwd(rec, 0.1, seed) + c.bwd(rec, 0.1, seed) + c.fwd(rec, 0.1, seed, kb) + c.bwd(rec, 0.1, seed, kb)
    finally:
        rec.set_step_seed_ptr(None)
    c = Case(g, dev, B, H, 20, 20, dh)
    kb = c.keep_bits(rec)
    n += c.fwd(rec, 0.0, seed, kb) + c.bwd(rec, 0.0, seed, kb)
    return n


def extremes(rec, dev, g, B=3, H=2):
    """q and k scaled by 4: scale * q.k reaches about +-60 (a one-hot softmax, a large lse); example 0 has every score strongly
    negative; both directions, with and without dropout, on the MFMA kernels and on the generic one"""
    n = 0
    for i, (nq, nk, dh, lds) in enumerate(((64, 64, 64, {}), (33, 20, 32, {}), (20, 33, 64, {"ldv": 3 * H * 64 + 4}))):
        c = Case(g, dev, B, H, nq, nk, dh, uniq=i, lds=lds, extreme=True)
        n += c.fwd(rec) + c.bwd(rec) + c.fwd(rec, 0.1, 41) + c.bwd(rec, 0.1, 41)
    return n


def attn_probs(rec, dev, g, dtype=BF, B=3, H=2):
    """xl_attn_probs at nq, nk <= 64: dense / packed / masked / with dropout / with odd leading dimensions"""
    n = 0
    for i, (nq, nk, dh, kw, p) in enumerate((
            (20, 33, 64, {}, 0.0), (64, 64, 32, dict(mask=True), 0.1), (1, 64, 16, dict(mask=True), 0.0),
            (33, 20, 24, dict(lds={"ldq": 3 * 2 * 24 + 1, "ldk": 3 * 2 * 24 + 3}), 0.1),
            (64, 20, 32, dict(q_lens=(1, 64, 33), pads=(3, 0)), 0.0),
            (20, 64, 32, dict(q_lens=(23, 0, 7), k_lens=(67, 1, 32), pads=(0, 2), mask=True), 0.1))):
        c = Case(g, dev, B, H, nq, nk, dh, dtype, uniq=i, **kw)
        c.host_lse()
        n += c.probs(rec, p, 51)
    return n


def rejected(ops, dev, g, dtype, error):
    """only calls that the entry points' own argument checks refuse before any launch: each raises `error` and leaves every output
    storage as it was -> cases run.  (No call that the checks accept but that would read or write out of range.)"""
    import pytest
    n = 0
    B, H, nq, nk, dh = 3, 2, 20, 33, 32
    c = Case(g, dev, B, H, nq, nk, dh, dtype)
    c.host_lse()
    L = c.ld
    kb = flat_out(dev, 3 * 2 * 2 * 64, torch.int32)
    probs = flat_out(dev, B * H * nq * nk)
    bias = flat_out(dev, 3 * H * dh, fill=torch.ones(3 * H * dh))
    outs = [c.o, c.dq, c.lse, kb, probs, bias]

    def raw(t):
        st = t.untyped_storage()
        return torch.tensor([], dtype=torch.uint8, device=t.device).set_(st, 0, (st.nbytes(),), (1,))

    def refuse(fn):
        nonlocal n
        before = [raw(t).clone() for t in outs]
        with pytest.raises(error):
            fn()
        assert all(torch.equal(raw(t), was) for t, was in zip(outs, before)), "a refused call wrote to an output"
        n += 1

    def fwd(**kw):
        a = dict(q=c.q, k=c.k, v=c.v, key_mask=None, o=c.o, lse=c.lse, B=B, H=H, nq=nq, nk=nk, dh=dh, ldq=L["ldq"], ldk=L["ldk"],
                 ldv=L["ldv"], ldo=L["ldo"], scale=c.scale, p_drop=0.0, seed=1)
        a.update(kw)
        return lambda: ops.sdpa_fwd(**a)

    def bwd(**kw):
        a = dict(q=c.q, k=c.k, v=c.v, key_mask=None, dout=c.dout, lse=c.lse, dq=c.dq, dk=c.dk, dv=c.dv, B=B, H=H, nq=nq, nk=nk, dh=dh,
                 ldq=L["ldq"], ldk=L["ldk"], ldv=L["ldv"], ldo=L["ldo"], lddq=L["lddq"], lddk=L["lddk"], lddv=L["lddv"], scale=c.scale,
                 p_drop=0.0, seed=1)
        a.update(kw)
        return lambda: ops.sdpa_bwd(**a)

    def prb(**kw):
        a = dict(q=c.q, k=c.k, key_mask=None, lse=c.lse, probs=probs, B=B, H=H, nq=nq, nk=nk, dh=dh, ldq=L["ldq"], ldk=L["ldk"],
                 scale=c.scale, p_drop=0.0, seed=1)
        a.update(kw)
        return lambda: ops.attn_probs(**a)
    for bad in (dict(nq=0), dict(nk=0), dict(nq=513), dict(nk=513), dict(dh=0), dict(dh=65), dict(p_drop=1.0), dict(p_drop=-0.1)):
        for mk in (fwd, bwd, prb):
            refuse(mk(**bad))
    refuse(fwd(q=None)), refuse(fwd(o=None)), refuse(fwd(lse=None))
    refuse(bwd(dout=None)), refuse(bwd(dv=None)), refuse(prb(probs=None)), refuse(prb(k=None))
    # bias_grad through column sums of the stored gradients (no workspace: no fused partials) with a gradient stride or H * dh that
    # is not a whole number of 16-byte vectors: refused before the backward is launched, not by xl_colsum after it
    refuse(bwd(bias_grad=bias, lddk=L["lddk"] + (4 if dtype == BF else 2)))
    refuse(bwd(bias_grad=bias, dh=1))
    if dtype == BF:
        refuse(fwd(keep_bits=kb, p_drop=0.1, ldq=L["ldq"] + 4))              # ineligible geometry
        refuse(fwd(keep_bits=kb, p_drop=0.1, dh=24))
        refuse(fwd(keep_bits=kb, p_drop=0.1, nq=65))
        refuse(bwd(keep_bits=kb, p_drop=0.1, nq=65))
        refuse(fwd(keep_bits=kb[2:], p_drop=0.1))                           # 8 bytes off
        refuse(bwd(keep_bits=kb[2:], p_drop=0.1))
        refuse(bwd(keep_bits=kb, p_drop=0.1, lddk=L["lddk"] + 4))
    else:
        refuse(fwd(keep_bits=kb, p_drop=0.1))                               # keep_bits does not exist in fp32
        refuse(bwd(keep_bits=kb, p_drop=0.1))
    return n
