"""The library calls of every sampler loop and of the two big heads' validation, pinned call by call (tests/ops_trace.py records
them over the fake ops: method, scalar arguments, tensor dtypes), and the RowPredictor both heads share.

tests/golden/sampler_call_trace.json holds, per scenario, the number of calls, the per-method histogram and the SHA-256 of the trace
as `python tools/sampler_call_trace.py --golden` printed them BEFORE the sampler tail moved into xlxmert_amd/sampling.py: a change
of that code that issues other device work, or the same work in another order or with other scalars, fails here.  The full traces
of two commits: `python tools/sampler_call_trace.py [PATTERN]` at each, then diff."""
import json
import os

import pytest
import torch

import ops_trace
from _util import GOLDEN
from xlxmert_amd.engine import Engine, LangHeads
from xlxmert_amd.sampling import RowPredictor

with open(os.path.join(GOLDEN, "sampler_call_trace.json")) as f:
    EXPECTED = json.load(f)
SCENARIOS = ops_trace.scenarios()


def test_the_fixture_names_the_scenarios():
    assert sorted(EXPECTED) == sorted(SCENARIOS) and len(SCENARIOS) == 84


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_call_trace_is_the_recorded_one(name):
    got, want = ops_trace.summary(SCENARIOS[name]()), EXPECTED[name]
    assert got["calls"] == want["calls"], name
    assert got["methods"] == want["methods"], name
    assert got["sha256"] == want["sha256"], f"{name}: same calls per method, other arguments or order (tools/sampler_call_trace.py '{name}')"


def test_scenarios_reach_every_exit():
    """the recorded scenarios between them take the five predict exits and both scoring exits"""
    seen = set().union(*(v["methods"] for v in EXPECTED.values()))
    assert {"rowmax_combine", "rowsample_combine", "ce_fwd_bwd", "sample_rows", "sample_rows_trunc", "rowscore_combine", "score_rows",
            "sampler_update", "sampler_ar_update", "grid_step", "caption_step"} <= seen


def test_both_heads_hold_the_same_predictor_class():
    eng = ops_trace.image_engine(torch.float32)
    cap, _, _ = ops_trace.caption_engine(torch.float32, True)
    assert type(eng.code_pred) is RowPredictor and type(cap.lang_heads.word_pred) is RowPredictor
    for cls in (Engine, LangHeads):
        for gone in ("_prepare_fused_predict", "_prepare_fused_sample", "_prepare_fused_score", "_sample_step", "_sample_step_trunc"):
            assert not hasattr(cls, gone), (cls.__name__, gone)
    # the public names, by inheritance
    for name in ("sample_codes_nar", "sample_codes_ar", "inpaint_codes", "sample_words_nar", "check_truncation", "TRUNC_MAX_CAND",
                 "reuse_vis_stack", "fused_predict_available", "row_kept"):
        assert hasattr(Engine, name) and name not in Engine.__dict__, name
    assert eng.row_kept is None and not eng.fused_predict_available() and not cap.lang_heads.fused_predict_available()


@pytest.mark.parametrize("T", [1e-3, 0.7, 1e3])
def test_where_form_of_the_tempered_bias_equals_the_slice_multiply(T):
    """prepare_temperature's form for both heads against the in-place multiply of the real columns the image side used"""
    n, pad = 10, 6
    bias = torch.full((n + pad,), -1e30)
    bias[:n] = torch.randn(n, generator=torch.Generator().manual_seed(0)) * 3
    where = torch.where(bias > -1e29, bias * (1.0 / T), bias)
    mul = bias.clone()
    mul[:n].mul_(1.0 / T)
    assert where.dtype == torch.float32 and torch.equal(where, mul)
    assert bool((where[n:] == torch.tensor(-1e30)).all()) and bool((where[:n] > -1e29).all())
    # ... and it is what the predictor computes
    pred = RowPredictor(type("E", (), {"cdtype": torch.float32, "dev": torch.device("cpu")})(), n, 8, 4, lambda: torch.zeros(n, 8),
                        lambda: bias[:n], n, n)
    pred.prepare()
    pred.prepare_temperature(T)
    assert pred.bias_pad_T.shape == (256,) and torch.equal(pred.bias_pad_T[:n], mul[:n]) and bool((pred.bias_pad_T[n:] == -1e30).all())
