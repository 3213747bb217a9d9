"""In-painting without a GPU: the restatement of xl_grid_step (tests/fake_ops_inpaint.py) against an independent plain-torch
statement (tests/inpaint_oracle.py) with one injected fault at a time, the schedule identity that lets the all-free case equal the
reference loop, the engine's loop over the restatement against the reference fixtures and the oracle's loop, the module entry
points, the C ABI's argument checks, and the sharpness of the admissible-argmax rule at the inputs of the device's bf16 test.  The
kernel itself is held to the restatement in test_inpaint_gpu.py."""
import pytest
import torch

import bounds as BD
import inpaint_oracle as IO
import lxmert_oracle as O
from _util import golden_cfg, load_golden, maxdiff
from fake_ops_caption import n_mask_of, score_bound
from fake_ops_inpaint import FAULTS, InpaintFakeOps
from test_engine_cpu import make_sampler_engine
from xlxmert_amd.config import XLxmertConfig
from xlxmert_amd.engine import Engine
from xlxmert_amd.params import ParamStore

CFG_KEYS = ("vocab_size", "hidden_size", "num_attention_heads", "intermediate_size", "max_position_embeddings", "type_vocab_size",
            "l_layers", "x_layers", "r_layers", "visual_feat_dim", "visual_pos_dim", "num_clusters")
MODES = {"nar": IO.NAR, "confidence": IO.AR_CONF, "tlbr": IO.AR_ORDER, "order": IO.AR_ORDER}


# ---------------------------------------------------------------------------------------------------------------- restatement
def ragged_mask(gen, B, V, kinds=("all", "none", "one", "ragged", "ragged")):
    """free_mask [B, V] uint8 whose rows cycle through `kinds`: every cell, no cell, one cell, a random subset"""
    fm = torch.zeros(B, V, dtype=torch.uint8)
    for b in range(B):
        kind = kinds[b % len(kinds)]
        if kind == "all":
            fm[b] = 1
        elif kind == "one":
            fm[b, int(torch.randint(0, V, (1,), generator=gen))] = 1
        elif kind == "ragged":
            fm[b] = (torch.rand(V, generator=gen) < 0.6).to(torch.uint8)
            fm[b, V - 1], fm[b, 0] = 1, 0                           # (never all, never none)
        elif isinstance(kind, int):
            fm[b, torch.randperm(V, generator=gen)[:kind]] = 1
    return fm


def make_step_case(gen, B, V, mode, T, step, kinds=("all", "none", "one", "ragged", "ragged"), with_order=True):
    """arguments of one grid_step: random predictions, a ragged free mask, vis_mask set at about half of the free cells AND at some
    given cells (they are no candidates and never committed), init codes >= 1000 (no prediction equals them); in the rows b = 0, 3:
    the lowest confidence shared by 5/8 of the free cells (the re-mask cut falls among them), the highest shared by three candidates,
    and one `order` value for all cells; a row whose free cells are all filled already (no candidate)"""
    fm = ragged_mask(gen, B, V, kinds)
    free = fm != 0
    row_prob = torch.rand(B * V, generator=gen) * 0.9 + 0.05
    row_id = torch.randint(0, 90, (B * V,), generator=gen, dtype=torch.int32)
    vm = (torch.rand(B, V, generator=gen) < 0.5)
    vm = torch.where(free, vm, torch.rand(B, V, generator=gen) < 0.3)
    order = torch.randint(0, 6, (B, V), generator=gen, dtype=torch.int32) if mode == IO.AR_ORDER and with_order else None
    for b in (0, 3):
        if b >= B:
            continue
        cells = free[b].nonzero().reshape(-1)
        low = cells[torch.randperm(cells.numel(), generator=gen)[:max(2, 5 * cells.numel() // 8)]]
        row_prob[b * V + low] = 0.01
        top = cells[~torch.isin(cells, low)][-3:]
        row_prob[b * V + top] = 0.99
        vm[b, top] = True
        vm[b, low[:2]] = True
        if order is not None:
            order[b] = 2
    if B > 4:
        vm[4] = vm[4] & ~free[4]                                    # free cells, none of them masked: no candidate, nothing to commit
    codes = torch.randint(1000, 2000, (B, V), generator=gen)
    conf = torch.where(free & ~vm, torch.rand(B, V, generator=gen) * 0.9 + 0.05, torch.zeros(B, V))
    return dict(row_prob=row_prob, row_id=row_id, free_mask=fm, order=order, code_ids=codes, vis_mask=vm.to(torch.uint8), conf=conf,
                B=B, V=V, mode=mode, step=step, n_steps=T)


def step_cases():
    """[(name, arguments of one grid_step)]: the three modes, V = 16 / 49 / 64, n_b = 0, 1, V and ragged, ties, duplicate order values,
    a row without candidates, n_mask = 0 (step 2 of 4 with n_b = 1), the last step, and n_b = 55 of V = 64 at step 4 of T = 11 where
    the float schedule differs"""
    gen = torch.Generator().manual_seed(21)
    return [(name, make_step_case(gen, 5, V, mode, T, step, **kw)) for name, V, mode, T, step, kw in (
        ("nar", 16, IO.NAR, 4, 1, {}), ("nar first", 64, IO.NAR, 4, 0, {}), ("nar odd", 49, IO.NAR, 7, 2, {}),
        ("nar n_mask 0", 16, IO.NAR, 4, 2, {}), ("nar last", 16, IO.NAR, 4, 3, {}),
        ("float schedule", 64, IO.NAR, 11, 4, dict(kinds=(55, "none", "one", "ragged", "all"))),
        ("confidence", 16, IO.AR_CONF, 16, 3, {}), ("confidence 64", 64, IO.AR_CONF, 64, 0, {}),
        ("order", 16, IO.AR_ORDER, 16, 5, {}), ("order 49", 49, IO.AR_ORDER, 49, 48, {}),
        ("raster", 16, IO.AR_ORDER, 16, 2, dict(with_order=False)))]


def run_step(ops, c):
    cid, vm, conf = c["code_ids"].clone(), c["vis_mask"].clone(), c["conf"].clone()
    score = torch.full((c["B"],), -7.0)
    ops.grid_step(c["row_prob"], c["row_id"], c["free_mask"], c["order"], cid, vm, conf, score, c["B"], c["V"], c["mode"], c["step"],
                  c["n_steps"])
    return cid, vm, conf, score


def check_step(c, got, what=""):
    """the outputs of one grid_step against the independent plain-torch statement: integers and conf exact, score in its bound"""
    cid, vm, conf, score = got
    B, V = c["B"], c["V"]
    r_cid, r_vm, r_conf, r_score = IO.grid_update(c["row_prob"].view(B, V), c["row_id"].view(B, V), c["free_mask"], c["order"],
                                                  c["code_ids"], c["vis_mask"], c["conf"], c["mode"], c["step"], c["n_steps"])
    BD.check_exact(cid.cpu(), r_cid, f"{what} code_ids")
    BD.check_exact(vm.cpu().long(), r_vm.long(), f"{what} vis_mask")
    BD.check_exact(conf.cpu().view(torch.int32).long(), r_conf.view(torch.int32).long(), f"{what} conf")
    free = c["free_mask"] != 0
    counted = free if c["mode"] == IO.NAR else free & ~r_vm
    logs = torch.where(counted, torch.log(r_conf.double()).abs(), torch.zeros(1, dtype=torch.float64)).sum(1)
    for b in range(B):
        bound = score_bound(int(counted[b].sum()), float(logs[b]))
        assert abs(float(score[b]) - float(r_score[b])) <= bound, f"{what} score[{b}] {float(score[b])} vs {float(r_score[b])} (bound {bound:.2e})"
    given = ~free
    assert torch.equal(cid.cpu()[given], c["code_ids"][given]), f"{what}: a given cell was written"


def test_step_cases_cover_the_extremes():
    cases = dict(step_cases())
    n = torch.stack([(c["free_mask"] != 0).sum(1) for c in cases.values() if c["V"] == 16])
    assert {0, 1, 16} <= set(n.reshape(-1).tolist())
    c = cases["float schedule"]
    assert int((c["free_mask"][0] != 0).sum()) == 55 and (c["n_steps"], c["step"]) == (11, 4)
    c = cases["nar n_mask 0"]
    assert n_mask_of(1, c["step"], c["n_steps"]) == 0
    c = cases["confidence"]
    assert int(((c["free_mask"][4] != 0) & (c["vis_mask"][4] != 0)).sum()) == 0 and int((c["free_mask"][4] != 0).sum()) > 0
    assert cases["order"]["order"].unique().numel() < 16                                # duplicates


def test_integer_schedule_equals_the_reference_loop_on_the_full_grid():
    """with all 64 cells free the per-row integer schedule is the reference's int(ratio * V) at every step of every T <= 64 (64 is a
    power of two: (T - i) / T * 64 is exact whenever it is an integer, and rounding never crosses one otherwise) -- the condition
    under which inpaint_codes can reproduce sample_codes_nar.  It is NOT so for other free counts: n_b = 55, T = 11 gives
    int(6 / 11 * 55) = 29 where 55 * 6 // 11 = 30 -- why the device schedule is integer"""
    for T in range(1, 65):
        for i in range(T):
            assert (64 * (T - i)) // T == int((T - i) / T * 64), (T, i)
    assert int((11 - 4 - 1) / 11 * 55) == 29 and n_mask_of(55, 4, 11) == 30
    for V in (16, 49):                                            # the grids of the fixtures and the odd one of the kernel test, T = 4 / 7
        assert all((V * (T - i)) // T == int((T - i) / T * V) for T in (4, 7) for i in range(T)), V


@pytest.mark.parametrize("fault", [None] + list(FAULTS))
def test_independent_statement_accepts_the_restatement_and_rejects_each_fault(fault):
    failed = []
    for name, c in step_cases():
        try:
            check_step(c, run_step(InpaintFakeOps(torch.float32, fault=fault), c), name)
        except AssertionError as err:
            assert fault is not None, err
            failed.append((name, str(err)[:70]))
    print(fault, failed)
    assert (fault is None) == (not failed)


# ---------------------------------------------------------------------------------------------------------------- engine
def run_loop(eng, init, free, T, mode="nar", order=None, **kw):
    trace = []

    def hook(i):
        trace.append(dict(code_ids=eng.cid.clone(), vis_mask=eng.vmask.clone(), conf=eng.grid_conf.clone(), score=eng.grid_score.clone(),
                          pred_id=eng.row_argmax.clone(), pred_prob=eng.row_maxprob.clone()))
    cid, code, score, conf = eng.inpaint_codes(init, free, T, mode, order, hook, **kw)
    return cid.clone(), code.clone(), score.clone(), conf.clone(), trace


def test_all_free_nar_reproduces_the_reference_fixture_at_every_step():
    g = load_golden("sampler_tiny")
    T = int(g["n_steps"])
    eng, sd = make_sampler_engine(g, InpaintFakeOps(torch.float32))
    B, V = eng.B, eng.V
    init = torch.randint(0, eng.K, (B, V), generator=torch.Generator().manual_seed(1))   # ignored: every cell is free
    cid, code, score, conf, trace = run_loop(eng, init, torch.ones(B, V, dtype=torch.uint8), T)
    masks, ids = torch.from_numpy(g["step_masks"]), torch.from_numpy(g["step_pred_ids"])
    want = torch.zeros(B, V, dtype=torch.long)
    for i in range(T):
        want = torch.where(masks[i].bool(), ids[i], want)
        assert torch.equal(trace[i]["code_ids"], want), i
        assert torch.equal(trace[i]["vis_mask"].long(), masks[min(i + 1, T - 1)]), i      # the mask of the NEXT forward; the last one stays
        assert maxdiff(trace[i]["conf"], g["step_pred_prob"][i]) < 1e-5, i
    assert maxdiff(code.view(g["code"].shape), g["code"]) == 0.0
    ref = torch.log(torch.from_numpy(g["step_pred_prob"][-1]).double()).mean(1)
    assert torch.allclose(score.double(), ref, atol=1e-4)
    names = [c[0] for c in eng.ops.calls]
    assert names.count("grid_step") == T and "remask_lowest" not in names and "sampler_update" not in names


@pytest.mark.parametrize("mode", ["confidence", "tlbr"])
def test_all_free_ar_reproduces_the_reference_fixture_after_every_step(mode):
    g = load_golden("sampler_ar_tiny")
    eng, sd = make_sampler_engine(g, InpaintFakeOps(torch.float32))
    B, V = eng.B, eng.V
    cid, code, score, conf, trace = run_loop(eng, torch.zeros(B, V, dtype=torch.long), torch.ones(B, V), None, mode)
    ref = torch.from_numpy(g["step_masks_" + mode])
    assert len(trace) == V
    for i, t in enumerate(trace):
        assert torch.equal(t["vis_mask"], ref[i]), (mode, i)                            # the fill order
    assert torch.equal(trace[-1]["pred_id"].view(B, V).long(), torch.from_numpy(g["final_ids_" + mode]))    # (the last forward's predictions)
    assert maxdiff(code.view(g["code_" + mode].shape), g["code_" + mode]) == 0.0
    assert torch.allclose(score.double(), torch.log(conf.double()).mean(1), atol=1e-5) and bool((conf > 0).all())
    # "order" with the raster order spelled out is "tlbr"
    if mode == "tlbr":
        o = torch.arange(V).repeat(B, 1)
        again = run_loop(eng, torch.zeros(B, V, dtype=torch.long), torch.ones(B, V), None, "order", o)
        assert torch.equal(again[0], cid) and torch.equal(again[3], conf)


def ragged_inputs(B, V, K, seed=4):
    """(init_codes, free_mask): row 0 ragged, row 1 no free cell, row 2 one free cell, further rows ragged"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, K, (B, V), generator=gen), ragged_mask(gen, B, V, ("ragged", "none", "one", "ragged"))


@pytest.mark.parametrize("mode,T", [("nar", 4), ("nar", 7), ("confidence", None), ("tlbr", None), ("order", None), ("confidence", 3)])
def test_ragged_mask_engine_loop_matches_the_oracle_loop_and_keeps_the_given_cells(mode, T):
    """fp32 engine over the restatement against the loop composed from the oracle's modules: codes and masks identical after every
    step, confidences to fp32 rounding, score within score_bound of the float64 mean; given cells bit-identical to init_codes after
    every step; the row without free cells comes back untouched with score 0"""
    g = load_golden("sampler_tiny")
    eng, sd = make_sampler_engine(g, InpaintFakeOps(torch.float32))
    B, V, grid = eng.B, eng.V, int(g["grid"])
    oc = golden_cfg(g)
    init, fm = ragged_inputs(B, V, eng.K)
    free = fm != 0
    order = torch.stack([torch.randperm(V, generator=torch.Generator().manual_seed(b)) for b in range(B)]) if mode == "order" else None
    ids = torch.from_numpy(g["in_input_ids"])
    n_steps = int(free.sum(1).max()) if T is None else T
    r_cid, r_score, r_conf, r_trace = IO.inpaint_codes(sd, oc, ids, init, fm, n_steps, grid, MODES[mode], order)
    cid, code, score, conf, trace = run_loop(eng, init, fm, T, mode, order)
    assert len(trace) == n_steps
    for i, (a, r) in enumerate(zip(trace, r_trace)):
        assert torch.equal(a["code_ids"], r["code_ids"]), i
        assert torch.equal(a["vis_mask"].bool(), r["vis_mask"]), i
        assert torch.equal(a["code_ids"][~free], init[~free]), i
        assert torch.allclose(a["conf"], r["conf"], rtol=1e-4, atol=1e-7), i
        counted = free if mode == "nar" else free & ~r["vis_mask"]
        logs = torch.where(counted, torch.log(r["conf"].double().clamp(min=1e-300)).abs(), torch.zeros(1, dtype=torch.float64)).sum(1)
        for b in range(B):
            assert abs(float(a["score"][b]) - float(r["score"][b])) <= score_bound(int(counted[b].sum()), float(logs[b])) + 1e-4, (i, b)
    assert torch.equal(cid, r_cid) and torch.equal(cid[1], init[1]) and float(score[1]) == 0.0 and bool((conf[1] == 0).all())
    if mode == "nar":
        n = free.sum(1).tolist()
        assert [int(t["vis_mask"].sum()) for t in trace[:-1]] == [sum(n_mask_of(k, i, n_steps) for k in n) for i in range(n_steps - 1)]
    else:                                                       # one cell per image per step, while the image has any left
        left = free.sum(1)
        for i, t in enumerate(trace):
            left = (left - 1).clamp(min=0)
            assert t["vis_mask"].sum(1).tolist() == left.tolist(), i
    # the features: centroids of the ids, mask_feat where an AR loop was cut short
    want = O.codebook_features(sd, cid, trace[-1]["vis_mask"] if mode != "nar" else None)
    assert maxdiff(code.view(B, V, -1), want) == 0.0
    if mode == "confidence" and T == 3:
        assert int(trace[-1]["vis_mask"].sum()) > 0


def test_sampling_arguments_reach_the_loop_and_the_loop_is_reproducible():
    g = load_golden("sampler_tiny")
    eng, sd = make_sampler_engine(g, InpaintFakeOps(torch.float32))
    init, fm = ragged_inputs(eng.B, eng.V, eng.K)
    greedy = run_loop(eng, init, fm, 4)
    one = run_loop(eng, init, fm, 4, top_k=1, seed=9)                                     # top_k = 1 is greedy, whatever the seed
    assert torch.equal(one[0], greedy[0])
    a = run_loop(eng, init, fm, 4, temperature=1.5, seed=11)
    b = run_loop(eng, init, fm, 4, temperature=1.5, seed=11)
    c = run_loop(eng, init, fm, 4, temperature=1.5, seed=12)
    assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and not torch.equal(a[0], c[0])
    free = fm != 0
    for out in (a, c, run_loop(eng, init, fm, None, "confidence", temperature=2.0, seed=3, top_k=20, top_p=0.95, min_p=0.01)):
        assert torch.equal(out[0][~free], init[~free]) and bool(((out[3][free] > 0) & (out[3][free] <= 1)).all())
    eng.ops.calls.clear()
    run_loop(eng, init, fm, 2, temperature=1.0, seed=5)
    assert [c for c in eng.ops.calls if c[0] == "grid_step"] == [("grid_step", eng.B, eng.V, 0, i, 2, False) for i in range(2)]


@pytest.mark.parametrize("kw,err", [(dict(mode="best"), "mode"), (dict(mode="order"), "order"), (dict(order=torch.zeros(3, 16, dtype=torch.long)), "order"),
                                    (dict(mode="order", order=torch.zeros(3, 15, dtype=torch.long)), "order"),
                                    (dict(mode="order", order=torch.zeros(3, 16)), "order"), (dict(free=torch.ones(3, 15)), "free_mask"),
                                    (dict(free=torch.ones(16)), "free_mask"), (dict(init=torch.zeros(2, 16, dtype=torch.long)), "init_codes"),
                                    (dict(init=torch.zeros(3, 16)), "init_codes"), (dict(init=torch.full((3, 16), 100)), "init_codes"),
                                    (dict(init=torch.full((3, 16), -1)), "init_codes"), (dict(T=0), "n_steps"),
                                    (dict(temperature=0.0), "temperature"), (dict(top_k=0), "top_k"), (dict(min_p=2.0), "min_p")])
def test_bad_arguments_raise(kw, err):
    g = load_golden("sampler_tiny")
    eng, sd = make_sampler_engine(g, InpaintFakeOps(torch.float32))
    assert (eng.B, eng.V, eng.K) == (3, 16, 50)
    kw = dict(kw)
    init, free = kw.pop("init", torch.zeros(3, 16, dtype=torch.long)), kw.pop("free", torch.zeros(3, 16))
    T, mode, order = kw.pop("T", 2), kw.pop("mode", "nar"), kw.pop("order", None)
    with pytest.raises(ValueError, match=err):
        eng.inpaint_codes(init, free, T, mode, order, **kw)
    assert "grid_step" not in [c[0] for c in eng.ops.calls]


def test_out_of_range_codes_are_refused_at_given_cells_only():
    g = load_golden("sampler_tiny")
    eng, sd = make_sampler_engine(g, InpaintFakeOps(torch.float32))
    init, fm = ragged_inputs(eng.B, eng.V, eng.K)
    wild = torch.where(fm != 0, torch.full_like(init, 10 ** 6), init)                     # whatever the free cells hold is ignored
    assert torch.equal(run_loop(eng, wild, fm, 2)[0], run_loop(eng, init, fm, 2)[0])


# ---------------------------------------------------------------------------------------------------------------- nn.Module
class _StubEngine:
    """stands in for the engine under XLxmertForPretraining.inpaint_codes: records its arguments, returns a fixed score per row"""

    def __init__(self, scores, F=4):
        self.scores, self.F = scores, F

    def set_inputs(self, ids, att, tt, pos, **kw):
        self.ids, self.pos, self.kw = ids.clone(), pos, kw

    def inpaint_codes(self, init_codes, free_mask, n_steps, mode, order, on_step, **kw):
        self.init, self.free, self.args, self.loop_kw = init_codes.clone(), free_mask.clone(), (n_steps, mode, order), kw
        R, V = init_codes.shape
        self.B = R
        if on_step is not None:
            for i in range(n_steps):
                on_step(i)
        rows = torch.arange(R).float()
        return (init_codes + torch.arange(R)[:, None], rows[:, None, None].expand(R, V, self.F).reshape(R * V, self.F), self.scores,
                rows[:, None].expand(R, V) / 100)

    def materialise_codes(self, masked=False):
        return torch.zeros(self.B * 16, self.F)


def _stub_model(eng, cls=None):
    from xlxmert_amd.modeling import XLxmertForPretraining
    cls = XLxmertForPretraining if cls is None else cls
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    m.vis_emb = object()
    m.config = XLxmertConfig(vocab_size=100)
    m._step_engine = lambda B, L, V: eng
    return m


def test_candidates_return_the_best_scoring_replica_per_image():
    B, C, V = 3, 4, 16
    scores = torch.tensor([-1.0, -0.5, -2.0, -0.7, -3.0, -2.5, -2.6, -2.4, -0.1, -0.9, -0.8, -0.05])
    eng = _StubEngine(scores)
    m = _stub_model(eng)
    ids = torch.arange(B * 8).view(B, 8) + 1
    init = torch.arange(B * V).view(B, V) * 10
    fm = (torch.arange(B * V).view(B, V) % 3 == 0).to(torch.uint8)
    cid, score, conf = m.inpaint_codes(ids, init, fm, 3, 4, temperature=0.9, seed=5, n_candidates=C)
    best = scores.view(B, C).argmax(1)
    assert best.tolist() == [1, 3, 3]
    rows = torch.arange(B) * C + best
    assert torch.equal(score, scores[rows]) and torch.equal(cid, init + rows[:, None]) and torch.equal(conf[:, 0], rows.float() / 100)
    assert torch.equal(eng.ids, ids.repeat_interleave(C, 0)) and torch.equal(eng.init, init.repeat_interleave(C, 0))
    assert torch.equal(eng.free, fm.repeat_interleave(C, 0)) and eng.args == (3, "nar", None)
    assert eng.loop_kw == dict(temperature=0.9, seed=5) and eng.pos.shape == (B * C, V, 4)
    assert torch.equal(eng.kw["cluster_ids"], torch.zeros(B * C, V, dtype=torch.long)) and bool(eng.kw["vis_mask"].all())
    # one replica: the loop's rows as they are, greedy: no sampling keyword
    order = torch.arange(V).repeat(B, 1)
    eng.scores = scores[:B]
    cid, score, conf = m.inpaint_codes(ids, init, fm, None, 4, mode="order", order=order)
    assert torch.equal(cid, init + torch.arange(B)[:, None]) and eng.loop_kw == {} and eng.args[:2] == (None, "order")
    assert torch.equal(eng.args[2], order)
    m.inpaint_codes(ids, init, fm, 2, 4, top_p=0.9, n_candidates=1)
    assert eng.loop_kw["top_p"] == 0.9 and isinstance(eng.loop_kw["seed"], int)


def test_module_argument_checks():
    eng = _StubEngine(torch.zeros(2))
    m = _stub_model(eng)
    ids, init, fm = torch.ones(2, 8, dtype=torch.long), torch.zeros(2, 16, dtype=torch.long), torch.ones(2, 16)
    with pytest.raises(ValueError, match="n_candidates"):
        m.inpaint_codes(ids, init, fm, 2, 4, n_candidates=3)                              # greedy replicas would be identical
    with pytest.raises(ValueError, match="n_candidates"):
        m.inpaint_codes(ids, init, fm, 2, 4, n_candidates=0, temperature=1.0)
    for kw, name in ((dict(init=init[:, :15]), "init_codes"), (dict(fm=fm[:1]), "free_mask"), (dict(order=torch.zeros(2, 4)), "order")):
        with pytest.raises(ValueError, match=name):
            m.inpaint_codes(ids, kw.get("init", init), kw.get("fm", fm), 2, 4, order=kw.get("order"))
    with pytest.raises(ValueError, match="temperature"):
        m.inpaint_codes(ids, init, fm, 2, 4, temperature=-1.0)
    with pytest.raises(ValueError, match="top_k"):
        m.inpaint_codes(ids, init, fm, 2, 4, top_k=0)
    m.vis_emb = None
    with pytest.raises(RuntimeError, match="set_visual_embedding"):
        m.inpaint_codes(ids, init, fm, 2, 4)


def test_inpaint_image_hands_the_chosen_replica_to_the_generator():
    from xlxmert_amd.modeling import ImggenModel
    B, C = 2, 3
    scores = torch.tensor([-1.0, -0.2, -0.3, -0.9, -0.8, -0.1])
    eng = _StubEngine(scores)
    m = _stub_model(eng, ImggenModel)
    m.grid_size, m.G, m.tokenizer = 4, None, None
    m._store = type("S", (), {"device": "cpu"})()
    ids, init, fm = torch.ones(B, 8, dtype=torch.long), torch.zeros(B, 16, dtype=torch.long), torch.ones(B, 16)
    with pytest.raises(RuntimeError, match="set_image_generator"):
        m.inpaint_image(ids, init, fm)
    m.set_image_generator(lambda x: x * 2 - 1)                                             # denorm undoes it
    img = m.inpaint_image(ids, init, fm, n_steps=2, temperature=1.0, sample_seed=3, n_candidates=C)
    assert img.shape == (B, 4, 4, 4) and eng.args == (2, "nar", None) and eng.loop_kw == dict(temperature=1.0, seed=3)
    assert img[:, 0, 0, 0].tolist() == [1.0, 1.0]                                          # rows 1 and 5, clamped into (0, 1) by denorm
    assert m.code_ids[:, 0].tolist() == [1, 5] and torch.equal(m.inpaint_score, scores[[1, 5]])
    steps = m.inpaint_image(ids, init, fm, n_steps=2, mode="confidence", return_intermediate=True)
    assert len(steps) == 2 and steps[0].shape == (B, 4, 4, 4) and eng.args[:2] == (2, "confidence")


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_rejects_bad_arguments_before_any_launch_and_is_planable():
    from xlxmert_amd._lib import XlError, get_lib, parse_header
    lib = get_lib()

    def call(B=5, V=16, mode=0, step=0, T=4, null=None):
        ptr = [16] * 8
        ptr[3] = None                                               # order may be NULL
        if null is not None:
            ptr[null] = None
        lib.call("xl_grid_step", *ptr, B, V, mode, step, T, None)
    for kw, text in ((dict(V=65), "V=65 "), (dict(V=0), "V=0 "), (dict(B=0), "B=0 "), (dict(mode=3), "mode=3 "), (dict(mode=-1), "mode=-1 "),
                     (dict(step=4), "step=4 "), (dict(step=-1), "step=-1 "), (dict(T=0), "n_steps=0")):
        with pytest.raises(XlError, match=r"xl_grid_step.*\(-5\).*" + text):
            call(**kw)
    for null in (0, 1, 2, 4, 5, 6, 7):
        with pytest.raises(XlError, match=r"xl_grid_step.*\(-5\).*null argument"):
            call(null=null)
    fid = lib._dll.xl_plan_fn_id(b"xl_grid_step")
    assert fid >= 0 and lib._dll.xl_plan_fn_nargs(fid) == 14 == len(lib.protos["xl_grid_step"][1])
    assert "xl_grid_step" in parse_header(experimental=False) and hasattr(lib._dll, "xl_grid_step")


# ---------------------------------------------------------------------------------------------------------------- sharpness
SHARP_CFG = dict(vocab_size=200, hidden_size=128, num_attention_heads=2, intermediate_size=256, max_position_embeddings=32,
                 visual_feat_dim=64, num_clusters=96, l_layers=2, x_layers=2, r_layers=2)
SHARP_B, SHARP_GRID, SHARP_L, SHARP_SEED = 4, 8, 8, 19          # 4 images of 8 x 8 cells: 256 head rows = the fused path
DEVICE_CAP = 0.05             # the issue's cap on the share of free rows with more than one admissible column


def sharp_model():
    oc = O.OracleConfig(**SHARP_CFG)
    return XLxmertConfig(**SHARP_CFG), oc, O.make_state_dict(oc, SHARP_SEED)


def sharp_inputs():
    """(input_ids [4, 8], init_codes, free_mask): rows all free, ragged, one free cell, ragged"""
    gen = torch.Generator().manual_seed(SHARP_SEED)
    ids = torch.randint(1, SHARP_CFG["vocab_size"], (SHARP_B, SHARP_L), generator=gen)
    ids[1, 6:] = 0
    V = SHARP_GRID ** 2
    return ids, torch.randint(0, SHARP_CFG["num_clusters"], (SHARP_B, V), generator=gen), ragged_mask(gen, SHARP_B, V, ("all", "ragged", "one", "ragged"))


def make_inpaint_engine(ops, cfg, sd, ids, grid, device="cpu", dtype=torch.float32):
    B, L = ids.shape
    V = grid * grid
    dev = torch.device(device)
    store = ParamStore(cfg, device, dtype, task="vis_mask")
    store.load_named(sd)
    eng = Engine(cfg, store, ops, B, L, V, need_lang=False)
    eng.sync_compute_weights()
    pos = torch.from_numpy(O.box_position(grid)).unsqueeze(0).expand(B, -1, -1).float()
    eng.set_inputs(ids.to(dev), (ids > 0).to(dev), None, pos.to(dev), cluster_ids=torch.zeros(B, V, dtype=torch.long, device=dev),
                   vis_mask=torch.ones(B, V, dtype=torch.bool, device=dev))
    return eng


def test_admissible_argmax_rule_is_sharp_on_the_oracle_inpaint_step():
    """The admissible-argmax rule accepts every column within 2 SLACK E of the float64 maximum; it says nothing if many columns are.
    Measured here from the oracle alone (float64 forward of the device bf16 test's model and inputs -- SHARP_CFG, make_state_dict(oc,
    19), sharp_inputs(), every free cell masked = step 0 -- head operands rounded to bf16 as the kernel reads them): 0 of the 143 free
    rows (0.0 %) have more than one admissible column (logit std 1.00, worst E 2.9e-05, median top-1/top-2 gap 787 x the acceptance
    width).  The device test, which sees the other steps' inputs too, applies DEVICE_CAP = 5 % at every step; the oracle alone must
    stay under half of it."""
    cfg, oc, sd = sharp_model()
    sd64 = {k: v.double() for k, v in sd.items()}
    ids, init, fm = sharp_inputs()
    free = fm != 0
    V = SHARP_GRID ** 2
    pos = torch.from_numpy(O.box_position(SHARP_GRID)).unsqueeze(0).expand(SHARP_B, -1, -1).double()
    with torch.no_grad():
        feats = O.codebook_features(sd64, torch.where(free, torch.zeros_like(init), init), fm.long())
        _, vis, _ = O.lxmert_model(sd64, oc, ids, feats, pos, ids > 0)
        feat, _ = O.visual_obj_head(sd64, oc, vis)
    A = feat.reshape(SHARP_B * V, -1)[free.reshape(-1)].to(torch.bfloat16).double()
    W = sd64["vis_emb.weight"].to(torch.bfloat16).double()
    b = sd64["obj_predict_head.out_cluster.bias"]
    pre = A @ W.t() + b
    e = BD.rowmax_logit_error(pre, A.abs() @ W.abs().t(), b.abs()[None, :], A.shape[1])
    E = e.amax(-1)
    _, n_adm = BD.argmax_admissible(pre, pre.argmax(-1), E)
    share, most = BD.sharpness(n_adm)
    top2 = pre.topk(2, -1).values
    print(f"\ninpaint sharpness: {int((n_adm > 1).sum())} of {n_adm.numel()} free rows ({100 * share:.1f} %) with more than one admissible "
          f"column, at most {most} in a row; logit std {float(pre.std()):.2f}, worst E {float(E.max()):.2g}, median top-1/top-2 gap "
          f"{float(((top2[:, 0] - top2[:, 1]) / (2 * BD.SLACK * E)).median()):.1f} x the acceptance width")
    assert share <= DEVICE_CAP / 2, (share, most)                                    # half the cap: room for the other steps' inputs


@pytest.mark.parametrize("dtype,mode", [(torch.float32, "nar"), (torch.float32, "confidence"), (torch.float32, "order"), (torch.bfloat16, "nar")],
                         ids=["fp32-nar", "fp32-confidence", "fp32-order", "bf16-nar"])
def test_device_loop_checks_pass_over_the_host_restatement(dtype, mode):
    """the device loop tests' own checks (test_inpaint_gpu._check_loop), driven here by the host restatement at the same geometries"""
    import test_inpaint_gpu as G
    G.run_teacher_forced(dtype, mode, InpaintFakeOps(dtype), "cpu")
