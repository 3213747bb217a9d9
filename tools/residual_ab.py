"""In-process A/B/A/B of the residual-stream storage type on the plan-replayed bs-256 training step: two PretrainSteps in one process
(A = bf16 stream, the default; B = fp32 stream, residual_dtype="fp32"), same seed, same batches, dropout on, alternated with a settling
run in front of every measurement like tools/abab.py; prints the paired delta (B - mean of the neighbouring A's) in ms per step, its
spread over the alternations, and the activation bytes of both.  The mode is opt-in: there is no pass / fail threshold.

    python tools/residual_ab.py                       # 5 alternations of 40 steps
    python tools/residual_ab.py --alternations 3 --steps 30 --out profiles/residual_fp32/ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from xlxmert_amd.config import XLxmertConfig
from xlxmert_amd.engine import reserve_streams
from xlxmert_amd.trainer import PretrainStep, synthetic_batch

ap = argparse.ArgumentParser()
ap.add_argument("--alternations", type=int, default=5)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--settle", type=int, default=20)
ap.add_argument("--bs", type=int, default=256)
ap.add_argument("--out", default="", help="also write the JSON result line to this file")
args = ap.parse_args()

reserve_streams("cuda:0")
cfg = XLxmertConfig()
B = args.bs
g = torch.Generator().manual_seed(9595)
cents = torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=g).relu()
batches = [{k: v.cuda() for k, v in synthetic_batch(cfg, B, 20, 8, seed=9595 + i).items()} for i in range(4)]


def make(residual_dtype):
    tr = PretrainStep(cfg, B, 20, 64, dtype=torch.bfloat16, device="cuda:0", seed=9595, total_steps=100000, train_dropout=True,
                      plan=True, drop_grads=True, overlap_optimizer=True, residual_dtype=residual_dtype)
    tr.set_centroids(cents)
    return tr


arms = {"A": make("bf16"), "B": make("fp32")}
assert not arms["A"].engine.res32 and arms["B"].engine.res32


def run(name):
    tr = arms[name]
    for i in range(8 + args.settle):
        tr.step(batches[i % 4])
    tr.sync()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(args.steps):
        tr.step(batches[i % 4])
    tr.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / args.steps * 1e3


a_ms, b_ms = [run("A")], []
for i in range(args.alternations):
    b_ms.append(run("B"))
    a_ms.append(run("A"))
    print(f"  bf16 {a_ms[-2]:7.3f}   fp32 {b_ms[-1]:7.3f}   bf16 {a_ms[-1]:7.3f}   paired delta {b_ms[-1] - 0.5 * (a_ms[-2] + a_ms[-1]):+.3f} ms", flush=True)
deltas = [b_ms[i] - 0.5 * (a_ms[i] + a_ms[i + 1]) for i in range(len(b_ms))]
act = {k: tr.engine.act_bytes for k, tr in arms.items()}
tmp = {k: sum(t.numel() * t.element_size() for t in tr.engine._tmp.values()) for k, tr in arms.items()}
out = {"A": "residual_dtype=bf16", "B": "residual_dtype=fp32", "bs": B, "a_ms": [round(x, 3) for x in a_ms], "b_ms": [round(x, 3) for x in b_ms],
       "paired_delta_ms": [round(d, 3) for d in deltas], "mean_delta_ms": round(statistics.mean(deltas), 3),
       "stdev_delta_ms": round(statistics.stdev(deltas), 3) if len(deltas) > 1 else None,
       "a_drift_ms": round(max(a_ms) - min(a_ms), 3), "steps_per_arm": args.steps, "settle_steps": args.settle,
       "act_bytes": {"bf16": act["A"], "fp32": act["B"], "extra": act["B"] - act["A"]},
       "backward_scratch_bytes": {"bf16": tmp["A"], "fp32": tmp["B"], "extra": tmp["B"] - tmp["A"]},
       "final_losses": {k: [float(x) for x in torch.as_tensor(tr.step(batches[0])).reshape(-1)[:2]] for k, tr in arms.items()}}
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out) + "\n")
