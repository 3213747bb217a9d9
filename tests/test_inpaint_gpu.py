"""In-painting on the device: xl_grid_step against its restatement, the engine loop pinned to the existing samplers with every cell
free, teacher-forced against the oracle with a ragged mask (fp32 and bf16 fused), and the ImggenModel entry point."""
import pytest
import torch

import bounds as Bd
import bounds_sampling as BS
import inpaint_oracle as IO
import test_inpaint_cpu as TI
from _util import golden_cfg, load_golden
from fake_ops_caption import n_mask_of, score_bound
from fake_ops_inpaint import InpaintFakeOps

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64            # guard words on either side of every buffer of the grid step, filled with +-2^12
BF16_MARGIN = 2.0 ** -6


def _ops(dtype=torch.float32):
    from xlxmert_amd.ops import HipOps
    return HipOps(dtype)


def _guard(t, fill):
    """(whole, view): a device copy of t with GUARD elements of +-fill on either side"""
    whole = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype, device=DEV)
    whole[1::2] = -fill if t.dtype != torch.uint8 else fill // 2
    whole[GUARD:GUARD + t.numel()] = t.reshape(-1).to(DEV)
    return whole, whole[GUARD:GUARD + t.numel()].view(t.shape)


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
# (mode, step, n_steps): Mask-Predict at its first step, a middle one, one where n_mask = 0 for the rows with few free cells (step 2
# of 4: n_b = 1 gives 1 * 1 // 4 = 0; step 9 of 10: every n_b < 10), the float-schedule case and the last step; the two one-cell modes
STEPS = ((IO.NAR, 0, 4), (IO.NAR, 1, 4), (IO.NAR, 2, 4), (IO.NAR, 8, 10), (IO.NAR, 4, 11), (IO.NAR, 3, 4),
         (IO.AR_CONF, 0, 64), (IO.AR_CONF, 5, 16), (IO.AR_ORDER, 3, 16), (IO.AR_ORDER, 15, 16))
MASKS = {"all": ("all",), "none": ("none",), "one": ("one",), "ragged": ("all", "none", "one", "ragged", "ragged")}


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("B,V", [(1, 64), (5, 64), (5, 49), (3, 16)])
def test_grid_step_equals_the_restatement(B, V, mask):
    """code_ids and vis_mask exactly, conf bit for bit, score within the bound of a mean of at most 64 logf terms; the inputs and
    +-2^12 guard words around every buffer bit-identical.  make_step_case plants the exactly tied confidences (re-mask cut among them,
    three equal best candidates), one `order` value for a whole row, rows without candidates and vis_mask set at given cells."""
    ops, ref = _ops(), InpaintFakeOps(torch.float32, compute=torch.float64)
    gen = torch.Generator().manual_seed(100 * B + V)
    seen = set()
    for mode, step, T in STEPS:
        for with_order in ((True, False) if mode == IO.AR_ORDER else (True,)):
            c = TI.make_step_case(gen, B, V, mode, T, step, MASKS[mask], with_order)
            if mode == IO.NAR and step + 1 < T:
                seen |= {(n_mask_of(int(n), step, T), int(n)) for n in (c["free_mask"] != 0).sum(1)}
            want = TI.run_step(ref, c)
            TI.check_step(c, want, "restatement")                  # (the restatement itself against the independent statement)
            bufs = {"row_prob": (c["row_prob"], 4096.0), "row_id": (c["row_id"], 4096), "free_mask": (c["free_mask"], 200),
                    "code_ids": (c["code_ids"], 4096), "vis_mask": (c["vis_mask"], 200), "conf": (c["conf"], 4096.0),
                    "score": (torch.full((B,), -7.0), 4096.0)}
            if c["order"] is not None:
                bufs["order"] = (c["order"], 4096)
            dev = {k: _guard(t, fill) for k, (t, fill) in bufs.items()}
            before = {k: w.clone() for k, (w, _) in dev.items()}
            v = {k: x for k, (_, x) in dev.items()}
            ops.grid_step(v["row_prob"], v["row_id"], v["free_mask"], v.get("order"), v["code_ids"], v["vis_mask"], v["conf"], v["score"],
                          B, V, mode, step, T)
            torch.cuda.synchronize()
            for k, (w, x) in dev.items():                              # guards untouched, inputs unchanged
                n = x.numel()
                assert torch.equal(w[:GUARD], before[k][:GUARD]) and torch.equal(w[GUARD + n:], before[k][GUARD + n:]), k
                if k in ("row_prob", "row_id", "free_mask", "order"):
                    assert torch.equal(w, before[k]), k
            what = f"B={B} V={V} mask={mask} mode {mode} step {step}/{T} order={with_order}"
            Bd.check_exact(v["code_ids"].cpu(), want[0], what + " code_ids")
            Bd.check_exact(v["vis_mask"].cpu().long(), want[1].long(), what + " vis_mask")
            Bd.check_exact(v["conf"].cpu().view(torch.int32).long(), want[2].view(torch.int32).long(), what + " conf")
            TI.check_step(c, tuple(t.cpu() for t in (v["code_ids"], v["vis_mask"], v["conf"], v["score"])), what)     # score in its bound
    if mask == "ragged" and B == 5:
        # n_mask = 0 with and without a free cell, and cuts strictly inside a row's free cells
        assert (0, 1) in seen and (0, 0) in seen and any(0 < k < n - 1 for k, n in seen), sorted(seen)


def test_grid_step_bad_arguments_do_not_launch():
    """XL_ERR_BAD_ARG before any launch: the buffers come back untouched"""
    from xlxmert_amd._lib import XlError
    ops = _ops()
    c = TI.make_step_case(torch.Generator().manual_seed(5), 5, 16, IO.NAR, 4, 1)
    v = {k: c[k].to(DEV) for k in ("row_prob", "row_id", "free_mask", "code_ids", "vis_mask", "conf")}
    score = torch.full((5,), -7.0, device=DEV)
    keep = {k: x.clone() for k, x in v.items()}
    for kw in (dict(V=65), dict(V=0), dict(B=0), dict(mode=3), dict(mode=-1), dict(step=4), dict(step=-1), dict(T=0)):
        a = dict(B=5, V=16, mode=0, step=1, T=4)
        a.update(kw)
        with pytest.raises(XlError, match=r"xl_grid_step.*\(-5\)"):
            ops.grid_step(v["row_prob"], v["row_id"], v["free_mask"], None, v["code_ids"], v["vis_mask"], v["conf"], score, a["B"], a["V"],
                          a["mode"], a["step"], a["T"])
    for null in ("row_prob", "free_mask", "code_ids", "conf"):
        args = dict(v, **{null: None})
        with pytest.raises(XlError, match="null argument"):
            ops.grid_step(args["row_prob"], args["row_id"], args["free_mask"], None, args["code_ids"], args["vis_mask"], args["conf"], score,
                          5, 16, 0, 1, 4)
    torch.cuda.synchronize()
    assert all(torch.equal(v[k], keep[k]) for k in v) and bool((score == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- 2. pinned to the old loops
def _trace(eng, out):
    def hook(i):
        out.append((eng.cid.clone(), eng.vmask.clone(), eng.row_maxprob.clone()))
    return hook


@pytest.mark.parametrize("kw", [{}, dict(temperature=1.3, seed=7)], ids=["greedy", "temperature"])
@pytest.mark.parametrize("mode", ["nar", "confidence", "tlbr"])
def test_all_free_inpaint_equals_the_existing_sampler_bit_for_bit(mode, kw):
    """fp32, the tiny fixtures, every cell free: cid, vmask and row_maxprob after every step are those of sample_codes_nar /
    sample_codes_ar on the same engine (Mask-Predict: the old loop re-masks BEFORE its forward, so its mask after step i + 1 is the new
    loop's after step i; the last step leaves it)"""
    from test_sampling_gpu import _engine
    g = load_golden("sampler_tiny" if mode == "nar" else "sampler_ar_tiny")
    eng = _engine(g, torch.float32)
    B, V = eng.B, eng.V
    old, new = [], []
    if mode == "nar":
        T = int(g["n_steps"])
        out_old = [x.clone() for x in eng.sample_codes_nar(T, _trace(eng, old), **kw)]
    else:
        T = V
        out_old = [x.clone() for x in eng.sample_codes_ar(None, mode, on_step=_trace(eng, old), **kw)]
    init = torch.randint(0, eng.K, (B, V), generator=torch.Generator().manual_seed(2)).to(DEV)       # ignored: every cell is free
    cid, code, score, conf = eng.inpaint_codes(init, torch.ones(B, V, dtype=torch.uint8, device=DEV), T if mode == "nar" else None, mode,
                                               None, _trace(eng, new), **kw)
    torch.cuda.synchronize()
    assert len(old) == len(new) == T
    for i in range(T):
        assert torch.equal(new[i][0], old[i][0]), (i, "cid")
        assert torch.equal(new[i][2].view(torch.int32), old[i][2].view(torch.int32)), (i, "row_maxprob")
        assert torch.equal(new[i][1], old[min(i + 1, T - 1)][1] if mode == "nar" else old[i][1]), (i, "vmask")
    assert torch.equal(cid, out_old[0]) and torch.equal(code.view(torch.int16 if code.dtype == torch.bfloat16 else torch.int32),
                                                        out_old[1].view(torch.int16 if code.dtype == torch.bfloat16 else torch.int32))
    if mode == "nar":
        assert torch.equal(conf.reshape(-1).view(torch.int32), out_old[2].view(torch.int32))
    ref = torch.log(conf.double()).mean(1)
    for b in range(B):
        assert abs(float(score[b]) - float(ref[b])) <= score_bound(V, float(torch.log(conf[b].double()).abs().sum())), b


# ---------------------------------------------------------------------------------------------------------------- 3. teacher-forced
def _grab(eng, snaps):
    def hook(i):
        fused = eng.cdtype == torch.bfloat16 and eng.fused_predict_available()
        snaps.append(dict(fused=fused, feat=eng.feat[:eng.MV].clone() if fused else None, logits=None if fused else eng.logits[:eng.MV].clone(),
                          ids=eng.row_argmax.clone(), p=eng.row_maxprob.clone(), lse=eng.row_lse.clone(), code_ids=eng.cid.clone().cpu(),
                          vis_mask=eng.vmask.clone().cpu(), conf=eng.grid_conf.clone().cpu(), score=eng.grid_score.clone().cpu()))
    return hook


def _check_loop(eng, snaps, sd, oc, ids, init, fm, order, mode, T, grid, margin_rel, cap):
    """every step teacher-forced: (a) the predicted codes admissible on the kernel's own head inputs against float64 (tests/bounds.py),
    no row exempted, the share of free rows with more than one admissible column at most `cap`; (b) code ids / masks / confidences
    exactly what the rules make of the device's own predictions, the score within its bound, given cells unchanged; (c) the oracle's
    forward on the state the device fed: the same code wherever the oracle's best logit is decisive"""
    B, V, K = eng.B, eng.V, eng.K
    free = fm != 0
    gmode = TI.MODES[mode]
    state = dict(code_ids=torch.where(free, torch.zeros_like(init), init), vis_mask=free.clone(), conf=torch.zeros(B, V))
    pos = torch.from_numpy(IO.O.box_position(grid)).unsqueeze(0).expand(B, -1, -1).float()
    for i, s in enumerate(snaps):
        M = s["ids"].numel()
        if s["fused"]:
            Kq = eng.code_pred.w_pad.shape[0]
            y, _, e = BS.tempered_reference(s["feat"].view(M, eng.F), eng.code_pred.w_pad, eng.code_pred.bias_pad, 1.0, 0)
            _, n_adm = Bd.check_rowmax_rows(y, e, Kq // 64, s["p"], s["ids"], s["lse"], f"step {i} fused predict")
            assert int(s["ids"].max()) < K
        else:
            y = s["logits"].view(M, -1)[:, :K].double()              # the kernel's own fp32 logits: exact inputs, the exact rule
            n_adm = Bd.check_admissible(y, s["ids"], torch.zeros(M, dtype=torch.float64, device=y.device), f"step {i} argmax")
            pr = torch.exp(y.amax(1) - torch.logsumexp(y, 1))
            assert torch.allclose(s["p"].double(), pr, rtol=1e-5), i
        share, most = Bd.sharpness(n_adm.cpu()[free.reshape(-1)])
        print(f"  step {i}: {100 * share:.1f} % of the free rows with more than one admissible column, at most {most}")
        assert share <= cap, (i, share, most)
        pp, pi = s["p"].cpu().view(B, V), s["ids"].cpu().view(B, V)
        r_cid, r_vm, r_conf, r_score = IO.grid_update(pp, pi, fm, order, state["code_ids"], state["vis_mask"], state["conf"], gmode, i, T)
        assert torch.equal(s["code_ids"], r_cid) and torch.equal(s["vis_mask"].bool(), r_vm), i
        assert torch.equal(s["conf"].view(torch.int32), r_conf.view(torch.int32)), i
        assert torch.equal(s["code_ids"][~free], init[~free]), i
        counted = free if gmode == IO.NAR else free & ~r_vm
        logs = torch.where(counted, torch.log(r_conf.double()).abs(), torch.zeros(1, dtype=torch.float64)).sum(1)
        for b in range(B):
            assert abs(float(s["score"][b]) - float(r_score[b])) <= score_bound(int(counted[b].sum()), float(logs[b])), (i, b)
        scores = IO.step_logits(sd, oc, ids, state["code_ids"], state["vis_mask"], pos)
        top2 = scores.topk(2, dim=2).values
        gap, scale = top2[..., 0] - top2[..., 1], top2[..., 0].abs().clamp_min(1.0)
        live = free & state["vis_mask"] if gmode != IO.NAR else free     # the rows whose prediction can be used in this step
        decisive = live & (gap > scale * margin_rel)
        same = pi.long() == scores.argmax(2)
        print(f"  step {i}: oracle decisive at {int(decisive.sum())} of {int(live.sum())} live cells, same code at {int((same & decisive).sum())}"
              f" of them, {int((same & live).sum())} of all")
        assert int(decisive.sum()) >= 0.5 * int(live.sum()) and bool(same[decisive].all()), i
        state = dict(code_ids=r_cid, vis_mask=r_vm, conf=r_conf)
    assert torch.equal(snaps[-1]["score"][free.sum(1) == 0], torch.zeros(int((free.sum(1) == 0).sum())))


def run_teacher_forced(dtype, mode, ops=None, device=DEV):
    """fp32: the tiny fixture model (B = 3, 4 x 4 cells), rows ragged / none free / one free.  bf16: TI.sharp_model at B = 4, 8 x 8 cells =
    256 head rows, the smallest geometry of the fused predict; rows all free / ragged / one free / ragged"""
    T = 4 if mode == "nar" else None
    if dtype == torch.float32:
        g = load_golden("sampler_tiny")
        oc, grid = golden_cfg(g), int(g["grid"])
        cfg = TI.XLxmertConfig(**{k: getattr(oc, k) for k in TI.CFG_KEYS})
        sd = IO.O.make_state_dict(oc, int(g["seed"]))
        ids = torch.from_numpy(g["in_input_ids"])
        init, fm = TI.ragged_inputs(ids.shape[0], grid * grid, cfg.num_clusters)
        margin, cap = 2.0 ** -12, 0.0
    else:
        cfg, oc, sd = TI.sharp_model()
        ids, init, fm = TI.sharp_inputs()
        grid, margin, cap = TI.SHARP_GRID, BF16_MARGIN, TI.DEVICE_CAP
    B, V = fm.shape
    order = torch.stack([torch.randperm(V, generator=torch.Generator().manual_seed(b)) for b in range(B)]) if mode == "order" else None
    eng = TI.make_inpaint_engine(_ops(dtype) if ops is None else ops, cfg, sd, ids, grid, device, dtype)
    snaps = []
    out = eng.inpaint_codes(init.to(device), fm.to(device), T, mode, None if order is None else order.to(device), _grab(eng, snaps))
    if device != "cpu":
        torch.cuda.synchronize()
    n_steps = int((fm != 0).sum(1).max()) if T is None else T
    assert len(snaps) == n_steps and all(s["fused"] == (dtype == torch.bfloat16) for s in snaps)
    _check_loop(eng, snaps, sd, oc, ids, init, fm, order, mode, n_steps, grid, margin, cap)
    return out


@pytest.mark.parametrize("mode", ["nar", "confidence", "order"])
def test_engine_loop_fp32_teacher_forced_against_the_oracle(mode):
    """fp32, the tiny fixture model, ragged mask.  Decisive = the oracle's best logit leads by more than 2^-12 of its size (2000 fp32
    ulps: the fp32 forward differs from the oracle's by a few ulps per contraction); on the kernel's own fp32 logits the argmax rule
    is exact (cap 0: no row may have two admissible columns)"""
    run_teacher_forced(torch.float32, mode)


def test_engine_loop_bf16_fused_teacher_forced_against_the_oracle():
    """bf16 at the smallest geometry that takes the fused path (B = 4, V = 64: 256 head rows), Mask-Predict, T = 4, ragged mask.  Same
    three checks per step.  Rows where float64 admits more than one column may differ from the oracle; their share among the free
    rows is capped at TI.DEVICE_CAP = 5 % at every step.  Measured on the CPU from the oracle alone
    (test_inpaint_cpu.test_admissible_argmax_rule_is_sharp_on_the_oracle_inpaint_step, step 0's inputs): 0 of the 143 free rows (0.0 %) have more
    than one admissible column (logit std 1.00, worst E 2.9e-05, median top-1/top-2 gap 787 x the acceptance width).
    Decisive = the oracle's best logit leads by more than BF16_MARGIN = 2^-6 of its size (floor 1), the caption test's margin: the
    head input carries the bf16 roundings of ~6 layers (about 5e-3 per element), a logit is a 64-term sum against centroids."""
    run_teacher_forced(torch.bfloat16, "nar")


# ---------------------------------------------------------------------------------------------------------------- 4. nn.Module
def test_inpaint_image_through_the_class():
    """ImggenModel.inpaint_image with an identity generator: given cells keep their centroid rows, the free ones take those of the
    chosen codes; return_intermediate yields one image batch per step whose last entry is the plain result; n_candidates picks the
    replica with the highest score"""
    from test_modeling_gpu import _imggen_model
    g = load_golden("sampler_tiny")
    m, grid = _imggen_model(g)
    V = grid * grid
    ids = torch.from_numpy(g["in_input_ids"]).cuda()
    B = ids.shape[0]
    K = m.config.num_clusters
    init, fm = TI.ragged_inputs(B, V, K)
    init, fm = init.cuda(), fm.cuda()
    free = fm != 0
    m.set_image_generator(lambda x: x)
    img = m.inpaint_image(ids, init, fm, n_steps=4)
    cid = m.code_ids.clone()
    assert torch.equal(cid[~free], init[~free]) and float(m.inpaint_score[1]) == 0.0
    cent = m.vis_emb.weight.float()
    want = m.denorm(cent[cid].permute(0, 2, 1).reshape(B, -1, grid, grid)).cpu()
    assert torch.equal(img, want)
    steps = m.inpaint_image(ids, init, fm, n_steps=4, return_intermediate=True)
    assert len(steps) == 4 and torch.equal(steps[-1], img) and torch.equal(m.code_ids, cid)
    codes, score, conf = m.inpaint_codes(ids, init, fm, 4, grid)
    assert torch.equal(codes, cid) and torch.equal(score, m.inpaint_score)
    r_cid = IO.inpaint_codes(IO.O.make_state_dict(golden_cfg(g), int(g["seed"])), golden_cfg(g), ids.cpu(), init.cpu(), fm.cpu(), 4, grid)[0]
    assert torch.equal(cid.cpu(), r_cid)
    for mode in ("confidence", "tlbr"):
        steps = m.inpaint_image(ids, init, fm, mode=mode, return_intermediate=True)
        assert len(steps) == int(free.sum(1).max()) and torch.equal(m.code_ids[~free], init[~free])
    a = m.inpaint_image(ids, init, fm, n_steps=4, temperature=1.5, sample_seed=11, n_candidates=3)
    sa, ca = m.inpaint_score.clone(), m.code_ids.clone()
    b = m.inpaint_image(ids, init, fm, n_steps=4, temperature=1.5, sample_seed=11, n_candidates=3)
    assert torch.equal(a, b) and torch.equal(ca, m.code_ids) and torch.equal(ca[~free], init[~free])
    all_codes, all_score, _ = m.inpaint_codes(ids.repeat_interleave(3, 0), init.repeat_interleave(3, 0), fm.repeat_interleave(3, 0), 4, grid,
                                              temperature=1.5, seed=11)
    assert torch.equal(sa, all_score.view(B, 3).max(1).values)
    with pytest.raises(ValueError, match="n_candidates"):
        m.inpaint_image(ids, init, fm, n_candidates=2)
