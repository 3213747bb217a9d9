"""Library-call traces over the fake ops (tests/ops_trace.py), no GPU needed: the sampler loops and the big heads' validation (the
default set), or -- `--set=engine` -- the training steps, the nn.Module entry points and the small heads' validation.

    python tools/sampler_call_trace.py [--set=engine] [PATTERN]     the full trace of every scenario whose name contains PATTERN
    python tools/sampler_call_trace.py --golden > tests/golden/sampler_call_trace.json
    python tools/sampler_call_trace.py --set=engine --golden > tests/golden/engine_call_trace.json

tests/test_sampler_call_trace_cpu.py and tests/test_engine_call_trace_cpu.py hold every scenario to the committed summary (calls,
per-method histogram, SHA-256 of the trace).  When a digest differs, print the full traces at both commits with this script and
diff them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ops_trace  # noqa: E402


def main(argv):
    golden = "--golden" in argv
    sets = {"sampler": ops_trace.scenarios, "engine": ops_trace.engine_scenarios}
    which = next((a.split("=", 1)[1] for a in argv if a.startswith("--set=")), "sampler")
    pattern = next((a for a in argv if not a.startswith("--")), "")
    out = {}
    for name, run in sets[which]().items():
        if pattern not in name:
            continue
        trace = run()
        if golden:
            out[name] = ops_trace.summary(trace)
        else:
            print(f"== {name}: {len(trace)} calls")
            print("\n".join(trace))
    if golden:
        json.dump(out, sys.stdout, indent=1, sort_keys=True)
        print()


if __name__ == "__main__":
    main(sys.argv[1:])
