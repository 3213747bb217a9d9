"""Library-call traces of the sampler loops and the validation heads over the fake ops (tests/ops_trace.py), no GPU needed.

    python tools/sampler_call_trace.py [PATTERN]            the full trace of every scenario whose name contains PATTERN, to stdout
    python tools/sampler_call_trace.py --golden > tests/golden/sampler_call_trace.json

tests/test_sampler_call_trace_cpu.py holds every scenario to the committed summary (calls, per-method histogram, SHA-256 of the
trace).  When a digest differs, print the full traces at both commits with this script and diff them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ops_trace  # noqa: E402


def main(argv):
    golden = "--golden" in argv
    pattern = next((a for a in argv if not a.startswith("--")), "")
    out = {}
    for name, run in ops_trace.scenarios().items():
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
