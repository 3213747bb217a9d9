"""Attention with 65..512 tokens per side (--max_text_length above 64) under the per-element float64 bounds of tests/bounds.py, through
the recording proxy of tests/test_kernel_bounds_gpu.py: sdpa_fwd_flash / sdpa_bwd_flash_q / sdpa_bwd_flash_k (the bf16 matrix-core
kernels), their plain fallbacks sdpa_*_long<bf16>, the generic bf16 kernels at nq, nk <= 64, and attn_probs_kernel at long lengths.

Geometry: the real width -- 12 heads of 64 -- with q / k / v as views into one [rows, 3 * 768] fused-projection matrix per side (the
engine's layout), o / dq / dk / dv of stride 768.  Every output buffer starts as 7.0, so a row a kernel forgets shows.  Key masks
carry, in ONE call, an example whose first 64-key block is entirely masked while later keys attend, an example with every key masked
(convention: zero output rows, lse = -inf, zero gradients -- also asserted exactly here), an example with a single valid key in
the last block, and random masks with key 0 valid.  Packed lengths sit on the 64-row block boundaries.

The only elements a comparison leaves out are the lse entries of queries without a valid key; each test counts them from the masks
and lengths it built and compares with what the proxy left out.  The last test runs one full-size training step at L = 100."""
import time

import pytest
import torch

import bounds as BD
from test_kernel_bounds_gpu import SDPA_KERNELS, Recorder, _table

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
H12, DH64 = 12, 64
SHAPES = [(65, 65), (64, 65), (65, 64), (128, 128), (129, 127), (200, 64), (20, 512), (512, 20), (512, 512)]
BLOCK_LENS = (1, 63, 64, 65, 128)


def _recorder(ops=None):
    if ops is None:
        from xlxmert_amd.ops import HipOps
        ops = HipOps(BF)
    return Recorder(ops)


def _rn(g, rows, cols, dev, alloc=None, scale=1.0):
    """bf16 normal draws in the first `rows` rows of an [alloc, cols] matrix (the rest zero)"""
    t = torch.zeros(alloc or rows, cols, dtype=BF)
    t[:rows] = (torch.randn(rows, cols, generator=g) * scale).to(BF)
    return t.to(dev)


def key_masks(g, B, nk):
    """uint8 [B, nk]: random (70 % attend) with key 0 valid; example 1: the first 64-key block ALL masked, every later key valid
    (nk > 64); example 2: every key masked; example 3: one valid key, the last"""
    km = (torch.rand(B, nk, generator=g) > 0.3).to(torch.uint8)
    km[:, 0] = 1
    if B > 1 and nk > 64:
        km[1, :64] = 0
        km[1, 64:] = 1
    if B > 2:
        km[2] = 0
    if B > 3:
        km[3] = 0
        km[3, nk - 1] = 1
    return km


def offsets(lens, n, extra=64):
    """packed side: int32 [B + 1] offsets, the row count and a padded row count with at least `extra` pad rows"""
    lens = torch.as_tensor(lens).clamp(max=n)
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(lens, 0)]).to(torch.int32)
    rows = int(off[-1])
    return off, rows, (rows + 63) // 64 * 64 + extra, lens


class Case:
    """one attention problem: operands, outputs and the calls through the proxy"""

    def __init__(self, g, dev, B, H, dh, nq, nk, p_drop, masks=True, q_lens=None, k_lens=None, ld_extra=0, seed=3):
        self.B, self.H, self.dh, self.nq, self.nk, self.p, self.seed, self.dev = B, H, dh, nq, nk, p_drop, seed, dev
        HD = self.HD = H * dh
        self.ld = ld = 3 * HD + ld_extra
        self.scale = 1.0 / dh ** 0.5
        self.q_off = self.k_off = None
        self.rows_q, self.rows_k, self.q_pad, self.k_pad = B * nq, B * nk, 0, 0
        self.len_q, self.len_k = torch.full((B,), nq), torch.full((B,), nk)
        if q_lens is not None:
            self.q_off, self.rows_q, self.q_pad, self.len_q = offsets(q_lens, nq)
        if k_lens is not None:
            if k_lens is q_lens:
                self.k_off, self.rows_k, self.k_pad, self.len_k = self.q_off, self.rows_q, self.q_pad, self.len_q
            else:
                self.k_off, self.rows_k, self.k_pad, self.len_k = offsets(k_lens, nk)
        self.aq, self.ak = self.q_pad or self.rows_q, self.k_pad or self.rows_k
        xq = _rn(g, self.rows_q, ld, dev, self.aq, scale=1.5)
        same = nq == nk and (k_lens is q_lens)                        # self-attention: q, k, v of one matrix
        xk = xq if same else _rn(g, self.rows_k, ld, dev, self.ak)
        self.q, self.k, self.v = xq[:, :HD], xk[:, HD:2 * HD], xk[:, 2 * HD:3 * HD]
        self.km_host = key_masks(g, B, nk) if masks else None
        self.km = self.km_host.to(dev) if masks else None
        self.dout = _rn(g, self.rows_q, HD, dev, self.aq)
        self.lse = torch.zeros(B * H * nq, device=dev)
        if self.q_off is not None:
            self.q_off = self.q_off.to(dev)
        if self.k_off is not None:
            self.k_off = self.k_off.to(dev) if self.k_off.device.type == "cpu" else self.k_off
        if same and self.q_off is not None:
            self.k_off = self.q_off
        self.vl = dict(q_off=self.q_off, k_off=self.k_off, q_pad=self.q_pad, k_pad=self.k_pad)

    def no_key(self):
        """bool [B]: examples without a single attending key"""
        ar = torch.arange(self.nk)[None, :] < self.len_k[:, None]
        if self.km_host is not None:
            ar = ar & (self.km_host != 0)
        return ~ar.any(1)

    def lse_left_out(self):
        """lse entries no comparison covers: queries beyond a packed example's length and every query of an example without a key"""
        nokey = self.no_key()
        return int(self.H * torch.where(nokey, torch.full_like(self.len_q, self.nq), self.nq - self.len_q).sum())

    def _rows(self, side, b):
        off, n = (self.q_off, self.nq) if side == "q" else (self.k_off, self.nk)
        if off is None:
            return slice(b * n, (b + 1) * n)
        return slice(int(off[b]), int(off[b + 1]))

    def fwd(self, rec):
        c = self
        c.o = torch.full((c.aq, c.HD), 7.0, dtype=BF, device=c.dev)
        rec.sdpa_fwd(c.q, c.k, c.v, c.km, c.o, c.lse, c.B, c.H, c.nq, c.nk, c.dh, c.ld, c.ld, c.ld, c.HD, c.scale, p_drop=c.p,
                     seed=c.seed, **c.vl)
        for b in c.no_key().nonzero().reshape(-1).tolist():      # the convention, exactly: zero rows and lse = -inf
            assert not bool(c.o[c._rows("q", b)].any()), f"example {b} has no key: its output rows are not exactly zero"
            l = c.lse.view(c.B, c.H, c.nq)[b, :, :int(c.len_q[b])]
            assert bool((l == -float("inf")).all()), f"example {b} has no key: lse is not -inf"
        if c.q_pad:
            assert not bool(c.o[c.rows_q:].any()), "pad rows of o are not zero"

    def bwd(self, rec, bias=True, ws=None, bg=None):
        c = self
        c.dq = torch.full((c.aq, c.HD), 7.0, dtype=BF, device=c.dev)
        c.dk, c.dv = (torch.full((c.ak, c.HD), 7.0, dtype=BF, device=c.dev) for _ in range(2))
        if bias:
            c.bg = bg if bg is not None else torch.randn(3 * c.HD, device=c.dev)     # (+= into what is there)
        c.ws = ws if ws is not None else torch.zeros(rec.workspace_floats(c.HD), device=c.dev)
        rec.sdpa_bwd(c.q, c.k, c.v, c.km, c.dout, c.lse, c.dq, c.dk, c.dv, c.B, c.H, c.nq, c.nk, c.dh, c.ld, c.ld, c.ld, c.HD, c.HD,
                     c.HD, c.HD, c.scale, p_drop=c.p, seed=c.seed, bias_grad=c.bg if bias else None, ws=c.ws, **c.vl)
        for b in c.no_key().nonzero().reshape(-1).tolist():
            assert not bool(c.dq[c._rows("q", b)].any()), f"example {b} has no key: dq rows are not exactly zero"
            assert not bool(c.dk[c._rows("k", b)].any()) and not bool(c.dv[c._rows("k", b)].any()), \
                f"example {b} has no key: dk / dv rows are not exactly zero"
        if c.q_pad:
            assert not bool(c.dq[c.rows_q:].any()), "pad rows of dq are not zero"
        if c.k_pad:
            assert not bool(c.dk[c.rows_k:].any()) and not bool(c.dv[c.rows_k:].any()), "pad rows of dk / dv are not zero"

    def probs(self, rec):
        c = self
        c.pr = torch.full((c.B * c.H * c.nq * c.nk,), 7.0, device=c.dev)
        rec.attn_probs(c.q, c.k, c.km, c.lse, c.pr, c.B, c.H, c.nq, c.nk, c.dh, c.ld, c.ld, c.scale, p_drop=c.p, seed=c.seed,
                       q_off=c.q_off, k_off=c.k_off)


def kernels_of(rec, method):
    """the kernel names (first word of the label) the proxy recorded for a method"""
    return {r[3].split()[0] for r in rec.rows if r[0] == method}


def finish(rec, t0, cases, n_min, must=()):
    _table(rec.rows, time.time() - t0)
    assert not rec.unchecked, sorted(rec.unchecked)
    assert not rec.failures, "\n".join(rec.failures)
    assert not rec.leftover(), rec.leftover()
    assert len(rec.rows) >= n_min, len(rec.rows)
    for r in rec.rows:
        if r[0] in ("sdpa_fwd", "sdpa_bwd"):
            assert r[3].split()[0] in SDPA_KERNELS, r[3]
    left, want = sum(x[2] for x in rec.lse_excluded), sum(c.lse_left_out() for c in cases)
    assert len(rec.lse_excluded) == len(cases) and left == want, \
        f"lse entries left out of the comparison: {left} in {len(rec.lse_excluded)} forward calls; the masks and lengths give {want} in {len(cases)}"
    for m, k in must:
        assert k in kernels_of(rec, m), f"{m}: no row of {k} (recorded: {sorted(kernels_of(rec, m))})"
    print(f"kernels recorded: fwd {sorted(kernels_of(rec, 'sdpa_fwd'))}, bwd {sorted(kernels_of(rec, 'sdpa_bwd'))}; "
          f"lse entries left out {left} (= queries without a valid key); run time {time.time() - t0:.1f} s")


FLASH = (("sdpa_fwd", "sdpa_fwd_flash"), ("sdpa_bwd", "sdpa_bwd_flash"))


# ---------------------------------------------------------------------------------------------------------------- scenarios
def dense_shapes(dev="cuda", ops=None, shapes=SHAPES, B=8):
    t0 = time.time()
    rec = _recorder(ops)
    g = torch.Generator().manual_seed(21)
    cases = []
    for nq, nk in shapes:
        for p in (0.1, 0.0):
            c = Case(g, dev, 2 if (nq, nk) == (512, 512) else B, H12, DH64, nq, nk, p)
            c.fwd(rec)
            c.bwd(rec)
            cases.append(c)
    finish(rec, t0, cases, 8 * len(cases), FLASH)
    return rec


def small_heads(dev="cuda", ops=None, B=8):
    t0 = time.time()
    rec = _recorder(ops)
    g = torch.Generator().manual_seed(22)
    cases = []
    for dh, (nq, nk) in ((16, (129, 127)), (32, (129, 127)), (16, (65, 65)), (32, (65, 65))):
        c = Case(g, dev, B, 4, dh, nq, nk, 0.1)
        c.fwd(rec)
        c.bwd(rec)
        cases.append(c)
    finish(rec, t0, cases, 8 * len(cases), FLASH)
    return rec


def packed_rows(dev="cuda", ops=None):
    """lengths 1, 63, 64, 65, 128 and the capacity: both sides packed (language self-attention), the query side alone (language
    queries on 64 dense visual keys, with a key mask) and the key side alone (visual queries on packed language keys)"""
    t0 = time.time()
    rec = _recorder(ops)
    g = torch.Generator().manual_seed(23)
    cap = 200
    lens = torch.tensor(BLOCK_LENS + (cap, 100, cap))
    B = len(lens)
    cases = []
    for p in (0.1, 0.0):
        for nq, nk, ql, kl, masks in ((cap, cap, lens, lens, False), (cap, 64, lens, None, True), (64, cap, None, lens, False),
                                      (128, 128, lens, lens, False)):
            c = Case(g, dev, B, H12, DH64, nq, nk, p, masks=masks, q_lens=ql, k_lens=kl)
            c.fwd(rec)
            c.bwd(rec)
            cases.append(c)
    finish(rec, t0, cases, 8 * len(cases), FLASH)
    return rec


def bench_batch_packed(dev="cuda", ops=None, B=256):
    """the benchmark batch: B = 256, capacity 128, ragged lengths (the block-boundary ones among them), dropout on, the step part
    of the dropout seed read from device memory (xl_set_step_seed_ptr)"""
    t0 = time.time()
    rec = _recorder(ops)
    g = torch.Generator().manual_seed(24)
    L = 128
    lens = torch.randint(6, L + 1, (B,), generator=g)
    lens[:len(BLOCK_LENS)] = torch.tensor(BLOCK_LENS)
    step = torch.tensor([5], dtype=torch.int64, device=dev)
    rec.set_step_seed_ptr(step)
    try:
        c = Case(g, dev, B, H12, DH64, L, L, 0.1, masks=False, q_lens=lens, k_lens=lens)
        c.fwd(rec)
        c.bwd(rec)
    finally:
        rec.set_step_seed_ptr(None)
    finish(rec, t0, [c], 8, FLASH)
    return rec


def deferred_bias_sums(dev="cuda", ops=None, B=8):
    """xl_set_deferred_reduce(1): two long backward calls -- each with its own workspace, which first carries the call's delta and
    then the partials of its three column sums -- pending before ONE flush_reductions; both into the same bias gradient (the
    shared cross-attention's).  The proxy checks the destinations at the flush."""
    t0 = time.time()
    rec = _recorder(ops)
    g = torch.Generator().manual_seed(25)
    a = Case(g, dev, B, H12, DH64, 129, 127, 0.1)
    b = Case(g, dev, B, H12, DH64, 127, 129, 0.1)
    a.fwd(rec)
    b.fwd(rec)
    bg = torch.randn(3 * a.HD, device=dev)
    rec.set_deferred_reduce(1)
    try:
        a.bwd(rec, bg=bg)
        b.bwd(rec, bg=bg)
        assert a.ws.data_ptr() != b.ws.data_ptr()
        rec.flush_reductions()
    finally:
        rec.set_deferred_reduce(0)
    finish(rec, t0, [a, b], 4 + 6 + 3, FLASH)
    assert rec.flushes_checked == 1 and sum(r[1].endswith("@flush") for r in rec.rows) == 3, [r[1] for r in rec.rows]
    return rec


def fallbacks(dev="cuda", ops=None, B=8):
    """the same checks on the kernels a bf16 launch falls back to: transpose read off (plain long kernels), leading dimensions of
    3 * 768 + 4 (rows no longer 16-byte aligned: plain long kernels, and the generic ones at nq, nk <= 64), dh = 48.  Together
    with one flash case the recorded kernel names must hold flash, long and generic in both directions."""
    t0 = time.time()
    rec = _recorder(ops)
    g = torch.Generator().manual_seed(26)
    lens = torch.tensor(BLOCK_LENS + (129, 100, 129))
    cases = []

    def go(*a, **kw):
        c = Case(g, dev, B, *a, **kw)
        c.fwd(rec)
        c.bwd(rec)
        cases.append(c)
    go(H12, DH64, 129, 127, 0.1)                                          # flash
    rec.set_lds_transpose_read(0)
    try:
        go(H12, DH64, 129, 127, 0.1)                                      # sdpa_*_long<bf16>: the same arguments, another kernel
        go(H12, DH64, 200, 64, 0.0)
        go(H12, DH64, 129, 129, 0.1, masks=False, q_lens=lens, k_lens=lens)
    finally:
        rec.set_lds_transpose_read(1)
    go(H12, DH64, 65, 65, 0.1, ld_extra=4)                                # long: rows not 16-byte aligned
    go(H12, DH64, 20, 512, 0.0, ld_extra=4)
    go(H12, DH64, 64, 33, 0.1, ld_extra=4)                                # generic
    go(H12, DH64, 20, 64, 0.0, ld_extra=4, masks=False, q_lens=torch.tensor([1, 20, 7, 20, 13, 20, 2, 19]))
    go(H12, 48, 129, 127, 0.1)                                            # dh = 48: long
    go(H12, 48, 512, 20, 0.0)
    go(H12, 48, 33, 64, 0.1)                                              # dh = 48: generic
    go(H12, 48, 64, 64, 0.0)
    names = {d: kernels_of(rec, f"sdpa_{d}") for d in ("fwd", "bwd")}
    finish(rec, t0, cases, 8 * len(cases), [(f"sdpa_{d}", f"sdpa_{d}_{k}") for d in ("fwd", "bwd") for k in ("flash", "long", "generic")])
    for d in ("fwd", "bwd"):
        assert names[d] == {f"sdpa_{d}_{k}" for k in ("flash", "long", "generic")}, names
    return rec


def attn_probs_long(dev="cuda", ops=None, B=8):
    t0 = time.time()
    rec = _recorder(ops)
    g = torch.Generator().manual_seed(27)
    lens = torch.tensor(BLOCK_LENS + (200, 100, 200))
    cases = []
    for args, kw in (((129, 127, 0.1), {}), ((512, 512, 0.0), {}), ((200, 200, 0.1), dict(masks=False, q_lens=lens, k_lens=lens)),
                     ((200, 64, 0.1), dict(q_lens=lens))):
        c = Case(g, dev, 2 if args[0] == 512 else B, H12, DH64, *args, **kw)
        c.fwd(rec)
        c.probs(rec)
        cases.append(c)
    finish(rec, t0, cases, 3 * len(cases))
    assert len([r for r in rec.rows if r[0] == "attn_probs" and r[1] == "probs"]) == len(cases)
    assert len([r for r in rec.rows if r[0] == "attn_probs" and r[1] == "outside view"]) == len(cases)
    return rec


# ---------------------------------------------------------------------------------------------------------------- tests
def test_flash_kernels_dense_at_every_block_edge_within_bounds():
    """(65, 65) ... (512, 512), dropout 0.1 and 0, the four key-mask examples, bias_grad through the workspace the long path needs
    (eager column sums of the stored gradients)"""
    dense_shapes()


def test_flash_kernels_head_sizes_16_and_32_within_bounds():
    small_heads()


def test_flash_kernels_packed_lengths_on_the_block_boundaries_within_bounds():
    packed_rows()


def test_flash_kernels_at_the_benchmark_batch_packed_with_the_device_step_seed_within_bounds():
    bench_batch_packed()


def test_two_long_backward_calls_pending_before_one_flush_within_bounds():
    deferred_bias_sums()


def test_fallback_kernels_within_bounds_and_the_dispatch_reaches_flash_long_and_generic():
    fallbacks()


def test_attn_probs_at_long_lengths_within_bounds():
    attn_probs_long()


def long_text_step(dev="cuda", ops=None, B=32, L=100, **cfg_kw):
    """one recorded bf16 training step with --max_text_length 100: language rows packed (ragged lengths), 64 visual tokens, dropout
    on, eager, deferred reductions at their default -- the delta scratch of the long backward and the deferred bias sums share the
    engine's workspace regions in the step's real call order"""
    from test_workload_bounds_gpu import _cfgs, _finish, _state_dict, _step
    from xlxmert_amd.trainer import synthetic_batch
    import lxmert_oracle as O
    t0 = time.time()
    cfg, oc = _cfgs(**cfg_kw)
    sd = _state_dict("base", 2718) if not cfg_kw else O.make_state_dict(oc, 2718)
    batch = synthetic_batch(cfg, B, L, 8, seed=33)
    rec, tr = _step("vis_mask", B, batch, sd, cfg, dev, ops, L=L, V=64)
    for _ in range(3):
        if not rec.retry():
            break
        print("one more step: recording both producers of every shared destination", flush=True)
        tr.step({k: v.to(dev) for k, v in batch.items()})
        tr.sync()
    assert tr.engine.packed, "the language rows ran dense"

    def has(method, kernel, nq, nk):
        return any(n == method and a["nq"] == nq and a["nk"] == nk and str(a["_kernel"]).startswith(kernel) for n, a in rec.checked)
    extra = [("no flush was checked", rec.flushes_checked > 0)]
    for nq, nk in ((L, L), (L, 64), (64, L)):
        for m in ("fwd", "bwd"):
            extra.append((f"no checked sdpa_{m}_flash call at {nq} x {nk}", has(f"sdpa_{m}", f"sdpa_{m}_flash", nq, nk)))
    _finish(rec, t0, ("gemm", "gemm_wgrad_group", "sdpa_fwd", "sdpa_bwd", "layernorm_bwd", "flush_reductions", "adamw"), extra)
    print(f"run time {time.time() - t0:.1f} s")
    return rec


def test_training_step_at_text_length_100_every_numeric_call_within_bounds(monkeypatch):
    monkeypatch.delenv("XL_DEFER_REDUCE", raising=False)
    long_text_step()
