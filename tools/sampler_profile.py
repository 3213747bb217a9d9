"""One arm of the T = 4 Mask-Predict sampler (bf16, fused head) and nothing else, for a profiler: same engine set-up as the sampler
rows of tools/task_bench.py.
Usage: rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/sampler_profile.py [--temperature T [--seed S]] [--top-k K]
                                                                            [--top-p P] [--min-p Q] [--bs B] [--loops N]
       python tools/prof_summary.py DIR/NAME_results.db
Without --temperature and without a truncation argument the loop is the greedy one.  One pass per arm: the per-kernel averages of
the summaries are compared."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch
import lxmert_oracle as O
from xlxmert_amd.config import XLxmertConfig
from xlxmert_amd.engine import Engine
from xlxmert_amd.ops import HipOps
from xlxmert_amd.params import ParamStore
from xlxmert_amd.trainer import init_reference_weights

ap = argparse.ArgumentParser()
ap.add_argument("--temperature", type=float, default=None)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--top-k", type=int, default=None)
ap.add_argument("--top-p", type=float, default=None)
ap.add_argument("--min-p", type=float, default=None)
ap.add_argument("--bs", type=int, default=256)
ap.add_argument("--loops", type=int, default=12)
args = ap.parse_args()

cfg, oc, dev, B = XLxmertConfig(), O.OracleConfig(), "cuda", args.bs
store = ParamStore(cfg, dev, torch.bfloat16, task="vis_mask")
init_reference_weights(store, 1)
g = torch.Generator().manual_seed(0)
store.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=g).relu())
eng = Engine(cfg, store, HipOps(torch.bfloat16), B, 20, 64, need_lang=False)
eng.sync_compute_weights()
inp = O.make_inputs(oc, 4, B, 20, 8)
eng.set_inputs(inp["input_ids"].cuda(), inp["attention_mask"].cuda(), None, inp["visual_pos"].cuda(),
               cluster_ids=torch.zeros(B, 64, dtype=torch.long, device=dev), vis_mask=torch.ones(B, 64, dtype=torch.bool, device=dev))
assert eng.fused_predict_available()
trunc = {k: v for k, v in (("top_k", args.top_k), ("top_p", args.top_p), ("min_p", args.min_p)) if v is not None}
for _ in range(args.loops):
    if args.temperature is None and not trunc:
        eng.sample_codes_nar(4)
    else:
        eng.sample_codes_nar(4, temperature=args.temperature, seed=args.seed, **trunc)
torch.cuda.synchronize()
print(f"{args.loops} loops of 4 steps at bs {B}, " + ("greedy" if args.temperature is None and not trunc else
                                                     f"temperature {args.temperature}, seed {args.seed}, truncation {trunc or None}"))
