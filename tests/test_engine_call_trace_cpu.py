"""The library calls of every training step, nn.Module entry point and small-head validation of the engine, pinned call by call
(tests/ops_trace.py records them over the fake ops: method, scalar arguments, tensor dtypes).

tests/golden/engine_call_trace.json holds, per scenario, the number of calls, the per-method histogram and the SHA-256 of the trace as
`python tools/sampler_call_trace.py --set=engine --golden` printed them BEFORE engine.py was split into blocks.py / heads.py / tasks.py
and the heads' transform, row lists and label staging were each given one home: a change of that code that issues other device work,
or the same work in another order or with other scalars, fails here.  The full traces of two commits:
`python tools/sampler_call_trace.py --set=engine [PATTERN]` at each, then diff."""
import json
import os

import pytest

import ops_trace
from _util import GOLDEN

with open(os.path.join(GOLDEN, "engine_call_trace.json")) as f:
    EXPECTED = json.load(f)
SCENARIOS = ops_trace.engine_scenarios()


def test_the_fixture_names_the_scenarios():
    assert sorted(EXPECTED) == sorted(SCENARIOS) and len(SCENARIOS) == 48


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_call_trace_is_the_recorded_one(name):
    got, want = ops_trace.summary(SCENARIOS[name]()), EXPECTED[name]
    assert got["calls"] == want["calls"], name
    assert got["methods"] == want["methods"], name
    assert got["sha256"] == want["sha256"], (f"{name}: same calls per method, other arguments or order "
                                             f"(tools/sampler_call_trace.py --set=engine '{name}')")


def test_scenarios_reach_the_heads_and_the_paired_schedule():
    """the recorded scenarios between them run every head's transform backward, both row-subset spellings, the fine-tune losses, the
    pooler's backward, the feature loss and the paired launches"""
    seen = set().union(*(v["methods"] for v in EXPECTED.values()))
    assert {"layernorm_bwd", "gelu_bwd", "gather_labels", "scatter_rows", "bce_logits_fwd_bwd", "tanh_bwd", "featloss_fwd_bwd",
            "gemm_pair"} <= seen


def test_scenarios_leave_the_environment_alone():
    before = dict(os.environ)
    SCENARIOS["step/vis_mask/pair_blocks/fp32/dense"]()
    SCENARIOS["step/vis_mask/compact_head_off/fp32/dense"]()
    assert dict(os.environ) == before
