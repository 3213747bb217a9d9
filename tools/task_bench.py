"""Throughput of the scope-table 'next' rows on one MI355X (synthetic data, bf16, random-init weights):
VQA fine-tune step (BASELINE config 3), 4-step Mask-Predict sampling (config 4), word_mask / matched pretraining steps.
Usage: python tools/task_bench.py [--rows all|sampler|caption|inpaint|eval|match|generator] [--temperature T [--seed S]] [--top-k K] [--top-p P] [--min-p Q]
--rows eval: the validation pass alone (bs 256): ms per Engine.evaluate_task for vis_mask (`--vis_mask_predict` masks, n ~ U{1..64}) and
word_mask (labelled rows from the loader), on the fused path (XL_EPI_ROWSCORE records) and on the logits path (XL_FUSED_PREDICT=0),
alternating in this process with their yardstick, Engine.task_forward(task, want_grad=False): all rows, fp32 logits.
--rows caption: the Mask-Predict caption sampler alone (bs 256, L = 20, T = 10, ragged lengths): ms per batch and captions/s, greedy on
the fused and on the logits predict path and with the visual stack recomputed every step, in one alternation with the arms below.
--rows inpaint: Engine.inpaint_codes alone (bs 256, Mask-Predict T = 4, half of every grid free): ms per batch, greedy (and drawn, with
--temperature), alternating in this process with the `sampler` row's loop (sample_codes_nar(4) on the same engine), its yardstick.
--rows match: caption-image matching alone (full model, L = 20, V = 64, ragged captions): ms per XLxmertForPretraining-style
match.MatchRunner.run for N = M = 16 and N = M = 32 (stacks once, cross layers per pair, ranking on the device), alternating in this
process with the path that existed before it: the same N*M pairs materialised as rows of an ordinary engine (batches of 256),
encoder_forward + rel_fwd.  The lines also go to --out (default profiles/match/task_bench_match.txt).
--rows generator: the native image generator (xlxmert_amd.generator.Generator, deployed geometry: base_dim 32, 2048 -> 256 codes, 8 -> 256
pixels, bs 64, bf16, noise on) against what a user had before it, the plain-torch statement of the same network on the same GPU (fp32, and
under bf16 autocast), arms alternating in this process; then ImggenModel.sample_image_NAR (T = 4, bs 64) end to end with either generator.
--temperature: the sampler rows are timed greedy AND with temperature sampling, alternating in this process (rounds of 8 loops
each; the line gives the median and the min..max spread of both).
--top-k / --top-p / --min-p (any of them): a third arm in the same alternation, the truncated sampler at that temperature (1 if
--temperature is not given; the untruncated arm then runs at 1 as well)."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch
import lxmert_oracle as O
from xlxmert_amd.config import XLxmertConfig
from xlxmert_amd.trainer import PretrainStep, word_rows_of

ap = argparse.ArgumentParser()
ap.add_argument("--rows", choices=("all", "sampler", "caption", "inpaint", "eval", "match", "generator"), default="all")
ap.add_argument("--temperature", type=float, default=None, help="also time the sampler rows drawing from softmax(logits / T)")
ap.add_argument("--seed", type=int, default=0, help="noise seed of the temperature sampler")
ap.add_argument("--top-k", type=int, default=None, help="truncated arm: at most K candidates (1..256)")
ap.add_argument("--top-p", type=float, default=None, help="truncated arm: nucleus mass in (0, 1]")
ap.add_argument("--min-p", type=float, default=None, help="truncated arm: probability floor relative to the mode, in (0, 1]")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match", "task_bench_match.txt"), help="--rows match / generator: file the lines are written to (generator: profiles/generator/task_bench_generator.txt)")
ap.add_argument("--rounds", type=int, default=5, help="greedy / sampled alternations (with --temperature)")
args = ap.parse_args()
trunc = {k: v for k, v in (("top_k", args.top_k), ("top_p", args.top_p), ("min_p", args.min_p)) if v is not None}
if trunc and args.temperature is None:
    args.temperature = 1.0

cfg, oc = XLxmertConfig(), O.OracleConfig()
dev = "cuda"


def timed(fn, n=8, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


def cuda(d):
    return {k: v.cuda() for k, v in d.items()}


for B in (128, 512) if args.rows == "all" else ():
    tr = PretrainStep(cfg, B, 20, 64, device=dev, task="vqa", num_answers=3129, train_dropout=True, total_steps=1000)
    batch = cuda(O.make_vqa_inputs(oc, 3129, 1, B, 20, 8))
    dt = timed(lambda: tr.step(batch))
    print(f"vqa step        bs {B:4d}: {dt * 1e3:7.2f} ms  {B / dt:9.0f} examples/s")
    del tr
for task in ("word_mask", "matched") if args.rows == "all" else ():
    B = 256
    tr = PretrainStep(cfg, B, 20, 64, device=dev, task=task, train_dropout=True, total_steps=1000)
    g = torch.Generator().manual_seed(0)
    tr.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=g).relu())
    inp = O.make_inputs(oc, 2, B, 20, 8)
    wl, ml = O.make_lang_task_labels(oc, inp["input_ids"], 3)
    batch = cuda({"input_ids": inp["input_ids"], "visual_pos": inp["visual_pos"], "cluster_ids": inp["cluster_ids"],
                  "word_labels": wl, "matched_labels": ml})
    batch["word_rows"] = word_rows_of(wl)          # from the loader, on the host: decoder + loss on the labelled rows only
    dt = timed(lambda: tr.step(batch))
    print(f"{task:10s} step  bs {B:4d}: {dt * 1e3:7.2f} ms  {B / dt:9.0f} examples/s")
    del tr
from xlxmert_amd.engine import Engine
from xlxmert_amd.ops import HipOps
from xlxmert_amd.params import ParamStore
from xlxmert_amd.trainer import init_reference_weights
for B in (64, 256) if args.rows in ("all", "sampler") else ():
    store = ParamStore(cfg, dev, torch.bfloat16, task="vis_mask")
    init_reference_weights(store, 1)
    g = torch.Generator().manual_seed(0)
    store.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=g).relu())
    eng = Engine(cfg, store, HipOps(torch.bfloat16), B, 20, 64, need_lang=False)
    eng.sync_compute_weights()
    inp = O.make_inputs(oc, 4, B, 20, 8)
    eng.set_inputs(inp["input_ids"].cuda(), inp["attention_mask"].cuda(), None, inp["visual_pos"].cuda(),
                   cluster_ids=torch.zeros(B, 64, dtype=torch.long, device=dev), vis_mask=torch.ones(B, 64, dtype=torch.bool, device=dev))
    dt = timed(lambda: eng.sample_codes_nar(4))
    print(f"sampler T=4     bs {B:4d}: {dt * 1e3:7.2f} ms  {B / dt:9.0f} images/s (codes for the GAN decoder)")
    if args.temperature is not None:
        runs = {"greedy": [], "sampled": []}
        if trunc:
            runs["truncated"] = []
        for _ in range(args.rounds):
            runs["greedy"].append(timed(lambda: eng.sample_codes_nar(4), warm=1))
            runs["sampled"].append(timed(lambda: eng.sample_codes_nar(4, temperature=args.temperature, seed=args.seed), warm=1))
            if trunc:
                runs["truncated"].append(timed(lambda: eng.sample_codes_nar(4, temperature=args.temperature, seed=args.seed, **trunc), warm=1))
        for k, v in runs.items():
            v = sorted(v)
            print(f"  {k:9s} bs {B:4d}: median {v[len(v) // 2] * 1e3:7.2f} ms  min {v[0] * 1e3:7.2f}  max {v[-1] * 1e3:7.2f}"
                  + (f"  (temperature {args.temperature}, seed {args.seed})" if k == "sampled" else "")
                  + (f"  ({', '.join(f'{a} {b}' for a, b in trunc.items())})" if k == "truncated" else ""))
    del eng, store


def caption_row(B=256, L=20, T=10):
    store = ParamStore(cfg, dev, torch.bfloat16, task="word_mask")
    init_reference_weights(store, 1)
    g = torch.Generator().manual_seed(0)
    store.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=g).relu())
    eng = Engine(cfg, store, HipOps(torch.bfloat16), B, L, 64, need_lang=True)
    eng.sync_compute_weights()
    lens = torch.randint(4, L - 1, (B,), generator=g)                    # 4 .. 18 free tokens
    pos = torch.arange(L).view(1, L)
    ids = torch.zeros(B, L, dtype=torch.long)
    ids[:, 0] = 101
    ids[pos == lens.view(B, 1) + 1] = 102
    att = pos < lens.view(B, 1) + 2
    inp = O.make_inputs(oc, 4, B, L, 8)
    eng.set_inputs(ids.cuda(), att.cuda(), None, inp["visual_pos"].cuda(), cluster_ids=torch.randint(0, cfg.num_clusters, (B, 64), generator=g).cuda(),
                   lang_rows=att.reshape(-1).nonzero().reshape(-1).cuda(), lang_off=torch.cat([lens.new_zeros(1), (lens + 2).cumsum(0)]).cuda())

    def loop(reuse=True, fused=True, **kw):
        eng.reuse_vis_stack = reuse
        os.environ["XL_FUSED_PREDICT"] = "1" if fused else "0"
        try:
            eng.sample_words_nar(lens, T, **kw)
        finally:
            eng.reuse_vis_stack = True
            os.environ["XL_FUSED_PREDICT"] = "1"
    arms = {"greedy": {}, "greedy logits path": dict(fused=False), "greedy no vis reuse": dict(reuse=False)}
    if args.temperature is not None:
        arms["sampled"] = dict(temperature=args.temperature, seed=args.seed)
        arms["sampled logits path"] = dict(temperature=args.temperature, seed=args.seed, fused=False)
    if trunc:
        arms["truncated"] = dict(temperature=args.temperature, seed=args.seed, **trunc)
    runs = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, kw in arms.items():
            runs[k].append(timed(lambda: loop(**kw), n=4, warm=1))
    print(f"caption T={T}    bs {B:4d}, L {L}, {eng.ML} head rows ({'packed' if eng.packed else 'dense'}), fused predict "
          f"{'available' if eng.lang_heads.fused_predict_available() else 'not available'}")
    for k, v in runs.items():
        v = sorted(v)
        med = v[len(v) // 2]
        print(f"  {k:20s}: median {med * 1e3:7.2f} ms  min {v[0] * 1e3:7.2f}  max {v[-1] * 1e3:7.2f}  {B / med:9.0f} captions/s")


def inpaint_row(B=256, T=4):
    store = ParamStore(cfg, dev, torch.bfloat16, task="vis_mask")
    init_reference_weights(store, 1)
    g = torch.Generator().manual_seed(0)
    store.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=g).relu())
    eng = Engine(cfg, store, HipOps(torch.bfloat16), B, 20, 64, need_lang=False)
    eng.sync_compute_weights()
    inp = O.make_inputs(oc, 4, B, 20, 8)
    eng.set_inputs(inp["input_ids"].cuda(), inp["attention_mask"].cuda(), None, inp["visual_pos"].cuda(),
                   cluster_ids=torch.zeros(B, 64, dtype=torch.long, device=dev), vis_mask=torch.ones(B, 64, dtype=torch.bool, device=dev))
    init = torch.randint(0, cfg.num_clusters, (B, 64), generator=g).cuda()
    free = torch.zeros(B, 64, dtype=torch.uint8)
    for b in range(B):                                                   # half of every grid, other cells per image
        free[b, torch.randperm(64, generator=g)[:32]] = 1
    free = free.cuda()
    arms = {"sampler greedy": lambda: eng.sample_codes_nar(T), "inpaint greedy": lambda: eng.inpaint_codes(init, free, T)}
    if args.temperature is not None:
        kw = dict(temperature=args.temperature, seed=args.seed)
        arms["sampler sampled"] = lambda: eng.sample_codes_nar(T, **kw)
        arms["inpaint sampled"] = lambda: eng.inpaint_codes(init, free, T, **kw)
    runs = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            runs[k].append(timed(fn, warm=1))
    print(f"inpaint T={T}    bs {B:4d}, 32 of 64 cells free, fused predict {'available' if eng.fused_predict_available() else 'not available'}")
    for k, v in runs.items():
        v = sorted(v)
        med = v[len(v) // 2]
        print(f"  {k:16s}: median {med * 1e3:7.2f} ms  min {v[0] * 1e3:7.2f}  max {v[-1] * 1e3:7.2f}  {B / med:9.0f} images/s")


def eval_row(B=256, L=20):
    from xlxmert_amd.trainer import synthetic_batch
    for task in ("vis_mask", "word_mask"):
        store = ParamStore(cfg, dev, torch.bfloat16, task=task)
        init_reference_weights(store, 1)
        g = torch.Generator().manual_seed(0)
        store.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=g).relu())
        eng = Engine(cfg, store, HipOps(torch.bfloat16), B, L, 64, need_lang=task != "vis_mask", train_dropout=False)
        eng.sync_compute_weights()
        b = cuda(synthetic_batch(cfg, B, L, 8, seed=5))
        common = dict(lang_rows=b["lang_rows"], lang_off=b["lang_off"], word_order=b["word_order"])
        if task == "vis_mask":
            eng.set_inputs(b["input_ids"], b["attention_mask"], None, b["visual_pos"], cluster_ids=b["cluster_ids"], vis_mask=b["vis_mask"],
                           obj_labels=b["obj_labels"], masked_rows=b["masked_rows"], **common)
            kw, rows, of = {"feat_loss": False}, eng.n_mrows, eng.MV
        else:
            wl, _ = O.make_lang_task_labels(oc, b["input_ids"].cpu(), 3)
            eng.set_inputs(b["input_ids"], b["attention_mask"], None, b["visual_pos"], cluster_ids=b["cluster_ids"], **common)
            kw = {"word_labels": wl.cuda(), "word_rows": word_rows_of(wl)}
            eng.lang_heads.set_rows(kw["word_rows"])
            rows, of = eng.lang_heads.n_rows, eng.MLd

        def ev(fused):
            os.environ["XL_FUSED_PREDICT"] = "1" if fused else "0"
            try:
                eng.evaluate_task(task, **kw)
            finally:
                os.environ["XL_FUSED_PREDICT"] = "1"
        fkw = {k: v for k, v in kw.items() if k != "word_rows"}
        arms = {"evaluate fused": lambda: ev(True), "evaluate logits path": lambda: ev(False),
                "task_forward(want_grad=False)": lambda: eng.task_forward(task, want_grad=False, **fkw)}
        runs = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                runs[k].append(timed(fn, warm=1))
        print(f"evaluate {task:9s} bs {B:4d}: head on {rows} of {of} rows")
        for k, v in runs.items():
            v = sorted(v)
            med = v[len(v) // 2]
            print(f"  {k:30s}: median {med * 1e3:7.2f} ms  min {v[0] * 1e3:7.2f}  max {v[-1] * 1e3:7.2f}  {B / med:9.0f} examples/s")
        del eng, store


def match_row(L=20, V=64):
    from xlxmert_amd.match import MatchRunner
    from xlxmert_amd.trainer import synthetic_batch
    store = ParamStore(cfg, dev, torch.bfloat16, task="matched")
    init_reference_weights(store, 1)
    g = torch.Generator().manual_seed(0)
    store.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=g).relu())
    ops = HipOps(torch.bfloat16)
    lines = [f"caption-image matching, full model (9/5/5, d = {cfg.hidden_size}), L = {L}, V = {V}, bf16, ragged captions; "
             f"{args.rounds} rounds of 4 calls per arm, arms alternating in one process"]
    for n in (16, 32):
        b = synthetic_batch(cfg, n, L, 8, seed=5)
        x = cuda({k: b[k] for k in ("input_ids", "attention_mask", "cluster_ids", "visual_pos")})
        tgt = torch.arange(n, device=dev)
        runner = MatchRunner(cfg, store, ops, n, n, L, V)
        runner.sync_compute_weights()
        # the path that existed before: the N*M rows, built once on the host (its best case), through an engine of 256 rows
        Bm = min(n * n, 256)
        eng = Engine(cfg, store, ops, Bm, L, V, need_lang=True)
        rep, til = (lambda t: t.repeat_interleave(n, 0)), (lambda t: t.repeat(n, *([1] * (t.dim() - 1))))
        big = cuda({"input_ids": rep(b["input_ids"]), "attention_mask": rep(b["attention_mask"]), "cluster_ids": til(b["cluster_ids"]),
                    "visual_pos": til(b["visual_pos"])})
        am = big["attention_mask"].cpu()
        parts = []
        for s in range(0, n * n, Bm):
            a = am[s:s + Bm]
            parts.append(dict(lang_rows=a.reshape(-1).nonzero().reshape(-1).cuda(),
                              lang_off=torch.cat([torch.zeros(1, dtype=torch.int64), a.sum(1).cumsum(0)]).to(torch.int32).cuda()))
        margin = torch.zeros(n * n, device=dev)

        def materialised():
            for i, s in enumerate(range(0, n * n, Bm)):
                eng.set_inputs(big["input_ids"][s:s + Bm], big["attention_mask"][s:s + Bm], None, big["visual_pos"][s:s + Bm],
                               cluster_ids=big["cluster_ids"][s:s + Bm], **parts[i])
                eng.encoder_forward(want_pooled=True)
                rel = eng.lang_heads.rel_fwd(eng.pooled)
                margin[s:s + Bm] = rel[:, 1] - rel[:, 0]

        def shared():
            runner.run(x["input_ids"], x["attention_mask"], None, cluster_ids=x["cluster_ids"], visual_pos=x["visual_pos"], top_k=5,
                       image_of_caption=tgt, caption_of_image=tgt)
        arms = {"match_scores (shared stacks)": shared, "materialised N*M rows": materialised}
        runs = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                runs[k].append(timed(fn, n=4, warm=1))
        lines.append(f"N = M = {n:3d}: {n * n} pairs, chunks of {runner.B_c}")
        med = {}
        for k, v in runs.items():
            v = sorted(v)
            med[k] = v[len(v) // 2]
            lines.append(f"  {k:30s}: median {med[k] * 1e3:7.2f} ms  min {v[0] * 1e3:7.2f}  max {v[-1] * 1e3:7.2f}  {n * n / med[k]:9.0f} pairs/s")
        a, m_ = med["match_scores (shared stacks)"], med["materialised N*M rows"]
        lines.append(f"  ratio shared / materialised: {a / m_:5.3f}  ({m_ / a:4.2f}x)")
        del runner, eng
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def torch_generator(sd, cfg_g):
    """the same network in stock PyTorch, NCHW, spectral norms folded once (eval mode): what set_image_generator took before"""
    import math
    import torch.nn.functional as F
    from xlxmert_amd.generator import fold_spectral_norm, resolution_channels
    W = {}
    for k in sd:
        if k.endswith(".weight_orig"):
            p = k[:-len(".weight_orig")]
            W[p] = fold_spectral_norm(sd[k], sd[p + ".weight_u"], sd[p + ".weight_v"]).to(dev)
        elif k.endswith(".weight") and not k.endswith(("noise1.weight", "noise2.weight")):
            W[k[:-len(".weight")]] = sd[k].to(dev)
    Bi = {k[:-len(".bias")]: v.to(dev) for k, v in sd.items() if k.endswith(".bias")}
    nw = {k: float(v) for k, v in sd.items() if k.endswith(("noise1.weight", "noise2.weight"))}
    T, r0 = cfg_g["target_size"], cfg_g["init_H"]
    n_up = int(math.log2(T // r0))

    def conv(t, p, pad, groups=1):
        return F.conv2d(t, W[p], Bi[p], padding=pad, groups=groups)

    def spade(t, y, p, weight):
        y = F.interpolate(y, size=t.shape[2:], mode="bilinear", align_corners=False)
        actv = F.relu(conv(y, p + ".shared.0", 1))
        out = F.instance_norm(t) * (1 + conv(actv, p + ".gamma", 1)) + conv(actv, p + ".beta", 1)
        return F.leaky_relu(out + weight * torch.randn(t.shape[0], 1, t.shape[2], t.shape[3], device=t.device, dtype=t.dtype), 0.2)

    def G(x):
        emb = torch.tanh(conv(x, "bottleneck_emb.0", 0))
        h, y = conv(emb, "learned_init_conv.0", 1, 4), conv(emb, "style_init_conv.0", 1, 4)
        out = torch.zeros(x.shape[0], 3, T, T, device=x.device)
        for i in range(n_up):
            p = f"resblocks.{i}"
            t = spade(h, y, p + ".cbn1", nw[p + ".noise1.weight"])
            t = conv(F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False), p + ".conv1", 1)
            t = conv(spade(t, y, p + ".cbn2", nw[p + ".noise2.weight"]), p + ".conv2", 1)
            h = t + conv(F.interpolate(h, scale_factor=2, mode="bilinear", align_corners=False), p + ".res_branch.1", 0)
            rgb = conv(h, f"to_RGB_blocks.{i}.conv", 1)
            out = out + (rgb if rgb.shape[-1] == T else F.interpolate(rgb, size=(T, T), mode="bilinear", align_corners=False)).float()
        return torch.tanh(out)
    return G


def generator_row(B=64, T_steps=4):
    from xlxmert_amd.generator import Generator
    from xlxmert_amd.modeling import ImggenModel
    cfg_g = dict(emb_dim=2048, codebook_dim=256, base_dim=32, init_H=8, init_W=8, target_size=256, extra_layers=0)
    native = Generator(**cfg_g, device=dev, dtype=torch.bfloat16)
    sd = native.state_dict()
    g = torch.Generator().manual_seed(0)
    for k in sd:
        if k.startswith("to_RGB_blocks") and k.endswith("conv.weight"):
            sd[k] = sd[k] * 0.05
        if k.endswith(("noise1.weight", "noise2.weight")):
            sd[k] = torch.full((1,), 0.3)
        if k.endswith(".weight_orig"):          # u = the normalised image of v: sigma = |W v| is O(1)
            p = k[:-len(".weight_orig")]
            sd[p + ".weight_u"] = torch.nn.functional.normalize(torch.mv(sd[k].flatten(1), sd[p + ".weight_v"]), dim=0)
    native.load_state_dict(sd)
    stock = torch_generator(sd, cfg_g)
    x = torch.randn(B, 2048, 8, 8, generator=g).to(dev)
    rows = x.permute(0, 2, 3, 1).reshape(B * 64, 2048).to(torch.bfloat16).contiguous()

    def stock_bf16(t):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return stock(t)
    with torch.no_grad():
        a, b_ = native(x, noise_seed=1, train=False), stock(x[:4])
        lines = [f"image generator, deployed geometry (base_dim 32, 2048 -> 256 codes, 8 x 8 -> 256 x 256), bs {B}, noise on; "
                 f"{args.rounds} rounds of 4 calls per arm, arms alternating in one process",
                 f"  (sanity: native image std {float(a.std()):.3f}, stock torch image std {float(b_.std()):.3f})"]
        arms = {"native (bf16, code rows in)": lambda: native.render_codes(rows, B), "stock torch fp32": lambda: stock(x),
                "stock torch bf16 autocast": lambda: stock_bf16(x)}
        runs = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                runs[k].append(timed(fn, n=4, warm=1))
        med = {}
        for k, v in runs.items():
            v = sorted(v)
            med[k] = v[len(v) // 2]
            lines.append(f"  {k:30s}: median {med[k] * 1e3:8.2f} ms  min {v[0] * 1e3:8.2f}  max {v[-1] * 1e3:8.2f}  {B / med[k]:8.0f} images/s")
        n_ = med["native (bf16, code rows in)"]
        lines.append(f"  ratio native / stock fp32: {n_ / med['stock torch fp32']:5.3f}   native / stock bf16 autocast: {n_ / med['stock torch bf16 autocast']:5.3f}")
        # end to end: the Mask-Predict sampler (T steps) and the generator behind it
        m = ImggenModel(cfg, args=None, num_clusters=cfg.num_clusters, dtype=torch.bfloat16, grid_size=8)
        m.set_visual_embedding(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=g).relu())
        ids = torch.randint(1000, 20000, (B, 20), generator=g).to(dev)
        e2e = {"native": native, "stock torch fp32": stock, "stock torch bf16 autocast": stock_bf16}
        runs = {k: [] for k in e2e}
        for _ in range(args.rounds):
            for k, G in e2e.items():
                m.set_image_generator(G)
                runs[k].append(timed(lambda: m.sample_image_NAR(ids, n_steps=T_steps), n=2, warm=1))
        lines.append(f"sample_image_NAR end to end (T = {T_steps}, bs {B}, image on the host at the end):")
        for k, v in runs.items():
            v = sorted(v)
            lines.append(f"  {k:30s}: median {v[len(v) // 2] * 1e3:8.2f} ms  min {v[0] * 1e3:8.2f}  max {v[-1] * 1e3:8.2f}")
    print("\n".join(lines))
    out = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "generator", "task_bench_generator.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if args.rows == "generator":
    generator_row()
if args.rows == "eval":
    eval_row()
if args.rows == "match":
    match_row()
if args.rows in ("all", "caption"):
    caption_row()
if args.rows == "inpaint":
    inpaint_row()
