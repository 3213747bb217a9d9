"""xl_pair_expand and xl_match_rank alone on the device: every output a view between guards, compared bit for bit with the expected
outputs of tests/match_cases.py (torch.index_select / repeat_interleave of the inputs, a stable descending torch.sort); `prob` against
float64 within the bound derived in tests/match_cases.py; refused arguments write nothing."""
import math

import pytest
import torch

import match_cases as MC

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096          # floats of guard on either side of a buffer, filled with +-2^12 (tests/test_eval_gpu.py::_guarded)


def _ops(dtype=torch.float32):
    from xlxmert_amd.ops import HipOps
    return HipOps(dtype)


class Guarded:
    """alloc(name, shape, dtype) -> a view between two guards; check(): the guards and the slack bytes kept their bits"""

    def __init__(self):
        self.items = []

    def __call__(self, name, shape, dtype):
        n_bytes = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
        n_f = (n_bytes + 3) // 4
        whole = torch.full((n_f + 2 * GUARD,), 4096.0, device=DEV)
        whole[1::2] = -4096.0
        view = whole[GUARD:GUARD + n_f].view(torch.uint8)[:n_bytes].view(dtype).view(*shape)
        self.items.append((name, whole, whole.clone(), n_bytes))
        return view

    def check(self):
        for name, whole, before, n_bytes in self.items:
            w, b = whole.view(torch.uint8), before.view(torch.uint8)
            lo = GUARD * 4
            assert torch.equal(w[:lo], b[:lo]) and torch.equal(w[lo + n_bytes:], b[lo + n_bytes:]), f"{name}: storage outside the view was written"
        self.items = []


SMALL = dict(N=3, M=2, V=4, L=5, d=8, lens=(1, 5, 3))


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("B_c", [1, 4, 6, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_expand_small(dtype, B_c, packed):
    """six pairs in chunks that divide them, that do not, and a capacity above the pair count; row pads of 8 and of the GEMM row tile"""
    ops = _ops(dtype)
    for row_pad in (8, 256):
        g = Guarded()
        MC.check_expand(ops, DEV, dtype, B_c=B_c, packed=packed, alloc=g, row_pad=row_pad, **SMALL)
        torch.cuda.synchronize()
        g.check()


@pytest.mark.parametrize("packed", [True, False])
def test_expand_two_copies_of_an_fp32_stream(packed):
    g = Guarded()
    MC.check_expand(_ops(torch.bfloat16), DEV, torch.float32, B_c=4, packed=packed, alloc=g, two=True, **SMALL)
    torch.cuda.synchronize()
    g.check()


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_expand_full_width(dtype, packed):
    """d = 768, V = 64, L = 20, N = M = 4: 16 pairs in one chunk and in chunks of 5 (more than one block per row class)"""
    lens = (20, 7, 1, 13)
    for B_c in (16, 5):
        g = Guarded()
        MC.check_expand(_ops(dtype), DEV, dtype, N=4, M=4, V=64, L=20, d=768, lens=lens, B_c=B_c, packed=packed, alloc=g, row_pad=256)
        torch.cuda.synchronize()
        g.check()


def test_expand_dense_source_with_lengths():
    """the dense [N*L, d] language source: offsets n*L, the captions' lengths in lang_len (dense chunk layout)"""
    N, M, V, L, d, B_c = 3, 2, 4, 5, 8, 4
    lens = [1, 5, 3]
    ops = _ops()
    gen = torch.Generator().manual_seed(3)
    vis, lang = torch.randn(M * V, d, generator=gen).to(DEV), torch.randn(N * L, d, generator=gen).to(DEV)
    off = torch.arange(N + 1, dtype=torch.int32, device=DEV) * L
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    g = Guarded()
    x0, km = g("x0", (B_c * (V + L), d), torch.float32), g("kmask", (B_c, L), torch.uint8)
    x0.fill_(7.0)
    ops.pair_expand(vis, lang, off, x0, None, None, km, N, M, V, L, d, 4, 2, B_c, False, N * L, B_c * L, B_c * L, lang_len=ln)
    torch.cuda.synchronize()
    g.check()
    exp = torch.zeros(B_c, L, d)
    for j in range(B_c):                            # pairs 4, 5, 5, 5 = caption 2 with images 0, 1, 1, 1
        exp[j, :3] = lang.cpu().view(N, L, d)[2, :3]
    assert MC.same_bits(x0[B_c * V:].cpu(), exp.view(B_c * L, d))
    assert torch.equal(km.cpu(), (torch.arange(L)[None, :] < 3).to(torch.uint8).expand(B_c, L))
    assert MC.same_bits(x0[:B_c * V].cpu(), vis.cpu().view(M, V, d)[[0, 1, 1, 1]].reshape(B_c * V, d))


def test_expand_refuses_bad_arguments_without_writing():
    from xlxmert_amd._lib import XlError
    ops = _ops()
    N, M, V, L, B_c = 3, 2, 4, 5, 4
    g = Guarded()
    off = torch.tensor([0, 1, 6, 9], dtype=torch.int32, device=DEV)

    def call(d=8, N=N, M=M, start=0, count=4, B_c=B_c, packed=True, rows=12, rows_pad=16, L=L, lang_len=None):
        vis, lang = torch.zeros(M * V, 16, device=DEV), torch.zeros(12, 16, device=DEV)
        x0 = g("x0", (B_c * V + 24, 16), torch.float32)
        c_off, c_rows, km = g("off", (B_c + 1,), torch.int32), g("rows", (24,), torch.int32), g("kmask", (B_c, 5), torch.uint8)
        before = [t.clone() for t in (x0, c_off, c_rows, km)]
        with pytest.raises(XlError):
            ops.pair_expand(vis, lang, off, x0, c_off, c_rows, km, N, M, V, L, d, start, count, B_c, packed, 12, rows, rows_pad,
                            lang_len=lang_len)
        torch.cuda.synchronize()
        assert all(MC.same_bits(a, b) for a, b in zip((x0, c_off, c_rows, km), before))
    call(d=12)                      # not a multiple of 8
    call(d=4)
    call(N=4097)
    call(M=0)
    call(count=5)                   # more pairs than slots
    call(count=0)
    call(start=4, count=3)          # beyond N*M
    call(start=-1)
    call(rows=17)                   # rows > rows_pad
    call(rows_pad=B_c * L + 256)    # beyond any capacity
    call(packed=False, rows=12)     # dense: rows must be B_c*L
    call(L=513)
    call(lang_len=off)              # lang_len goes with the dense layout only
    g.check()
    msg = ops.lib.raw("xl_last_error")().decode()
    assert "xl_pair_expand" in msg


# ---------------------------------------------------------------------------------------------- xl_match_rank
@pytest.mark.parametrize("shape", [(5, 3, 1, 4), (5, 3, 3, 4), (5, 3, 3, 15), (5, 3, 3, 1), (1, 70, 1, 64), (1, 70, 32, 70), (70, 1, 1, 9),
                                   (70, 1, 32, 70)])
def test_rank(shape):
    """(N, M, k, chunk capacity): hand-built margins with ties, +-60, the pair 20 / 30 whose probabilities tie at 1.0f, targets that
    tie with lower and higher indices; candidate lists that cross a wave (70); a direction with fewer than k candidates gets no list"""
    N, M, k, B_c = shape
    g = Guarded()
    ratio = MC.check_rank(_ops(), DEV, N, M, k, B_c, alloc=g)
    torch.cuda.synchronize()
    g.check()
    print(f"  xl_match_rank N={N} M={M} k={k}: prob {'exact' if ratio == 0 else f'headroom {1.0 / ratio:.2f}x'}")


def test_rank_refuses_bad_arguments_without_writing():
    from xlxmert_amd._lib import XlError
    ops = _ops()
    N, M = 5, 3
    g = Guarded()
    margin, prob = g("margin", (N, M), torch.float32), g("prob", (N, M), torch.float32)
    ti, tc = g("ti", (N, 3), torch.int32), g("tc", (M, 3), torch.int32)
    r1, tgt = g("r1", (N,), torch.int32), torch.zeros(N, dtype=torch.int32, device=DEV)
    rel = torch.zeros(4, 8, device=DEV)
    outs = (margin, prob, ti, tc, r1)
    before = [t.clone() for t in outs]
    bad = [dict(rel=rel, pair_start=13, pair_count=3),                                    # beyond N*M
           dict(rel=rel, pair_start=0, pair_count=0),
           dict(rel=None, pair_start=0, pair_count=0),                                    # nothing to do
           dict(rel=None, pair_start=0, pair_count=0, rank_stage=True, k=33, topk_images=ti),
           dict(rel=None, pair_start=0, pair_count=0, rank_stage=True, k=4, topk_images=ti),          # k > M candidates
           dict(rel=None, pair_start=0, pair_count=0, rank_stage=True, k=0, topk_captions=tc),
           dict(rel=None, pair_start=0, pair_count=0, rank_stage=True, k=3),                           # no output
           dict(rel=None, pair_start=0, pair_count=0, rank_stage=True, k=3, image_of_caption=tgt),     # target without its rank output
           dict(rel=None, pair_start=0, pair_count=0, rank_stage=True, k=3, rank_t2i=r1)]
    for kw in bad:
        with pytest.raises(XlError):
            ops.match_rank(kw.pop("rel"), kw.pop("pair_start"), kw.pop("pair_count"), margin, prob, N, M, **kw)
    with pytest.raises(XlError):
        ops.match_rank(rel, 0, 1, margin, prob, 4097, M)
    torch.cuda.synchronize()
    assert all(MC.same_bits(a, b) for a, b in zip(outs, before))
    g.check()
