"""Training-state continuity on the HIP path: what carries a run from one step to the next is spread over ParamStore buffers,
trainer attributes, engine flags set in Python and the pointers / scalars a recorded launch plan has frozen -- and a plan replay
re-executes C-ABI calls only.  Stated here on the real kernels, streams and plans:

  * an eager step, a recording step and a replayed step are the same launch list (bit-equal parameters, K-split weight gradients
    through slabs: the configuration test_training_step_is_bit_reproducible has shown to repeat itself);
  * a run stopped after step 4, rebuilt in a fresh trainer and continued equals the uninterrupted run -- and a restore that
    leaves a piece out differs;
  * a plan-mode trainer goes through gradient-accumulation windows (which force it onto the eager path) and back;
  * the partial-master guard of the sharded exchange's bf16 gather is up again after a REPLAYED step.

snapshot() / restore() are the ones of tests/test_continuity_cpu.py (the recipe of PretrainStep.state()'s docstring)."""
import os

import pytest
import torch

import lxmert_oracle as O

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=200, hidden_size=128, num_attention_heads=2, intermediate_size=256, max_position_embeddings=32,
             visual_feat_dim=64, num_clusters=96, l_layers=3, x_layers=2, r_layers=2)
# size -> (config, batch size).  "d128": the configuration test_training_step_is_bit_reproducible runs.  Its 128-wide weight
# gradients never fill a 256 x 256 tile, so no bf16 launch there has one writer per tile and NO gradient range ever becomes "kept"
# (ParamStore.mark_overwritten): the kept-range state the eager and the replayed path must agree on stays empty.  "d256" is the
# smallest model where it does not: 256 / 512-wide matrices, and 4 x 64 = 256 visual rows (K <= 512: no K split), so every Linear
# weight gradient is stored by the first backward after an optimizer pass and left uncleared by the pass.
SIZES = {"d128": (SMALL, 16), "d256": (dict(SMALL, hidden_size=256, num_attention_heads=4, intermediate_size=512), 4)}
L, GRID = 20, 8
BUFS = ("master", "exp_avg", "exp_avg_sq")
_cache = {}


def small_cfg(size):
    from xlxmert_amd.config import XLxmertConfig
    return XLxmertConfig(**SIZES[size][0])


def small_batches(size):
    """three batches, cycled: three launch geometries at most, uploaded once"""
    if size not in _cache:
        from xlxmert_amd.trainer import synthetic_batch
        _cache[size] = [{k: v.cuda() for k, v in synthetic_batch(small_cfg(size), SIZES[size][1], L, GRID, seed=70 + i).items()}
                        for i in range(3)]
    return _cache[size]


def small_trainer(size, plan, overlap, seed=5):
    """bf16, dropout on, AdamW clears the gradients, slabs on.  Weights AND codebook follow `seed`: a trainer built from another
    seed shares nothing with the run it is about to continue."""
    from xlxmert_amd.trainer import PretrainStep
    cfg, B = small_cfg(size), SIZES[size][1]
    tr = PretrainStep(cfg, B, L, GRID * GRID, dtype=torch.bfloat16, device="cuda", seed=seed, lr=1e-3, total_steps=20, warmup_ratio=0.3,
                      train_dropout=True, plan=plan, drop_grads=True, overlap_optimizer=overlap)
    assert tr.plan_mode == plan and tr.drop_grads and (tr.opt_stream is not None) == overlap and tr.overwrite_grads
    tr.set_centroids(torch.randn(cfg.num_clusters, cfg.visual_feat_dim, generator=torch.Generator().manual_seed(seed)).relu())
    tr.ops.set_gemm_wgrad_slabs(1)
    return tr


def bufs_of(tr):
    tr.sync()
    return {k: getattr(tr.store, k).clone() for k in BUFS + ("compute",)}


def differing(x, y):
    return f"max |d| {(x.float() - y.float()).abs().max().item():.3e}, {(x != y).float().mean().item():.2%} of the elements differ"


def grads_cleared_outside_kept_chunks(tr, size):
    """the optimizer pass cleared every chunk it does not leave to the next backward (flag bit 2) -- and the size keeps what its
    comment says it keeps"""
    n = tr.store.n_used
    cleared = ((tr.store.decay_flags[:n // 256] & 4) == 0).repeat_interleave(256)
    kept = 1.0 - cleared.float().mean().item()
    assert (kept > 0.25) if size == "d256" else (kept == 0.0), (size, kept)
    return tr.store.grad[:n][cleared].abs().max().item() == 0


# ---------------------------------------------------------------- eager == record == replay
@pytest.mark.parametrize("overlap", [False, True], ids=["plain", "overlap"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_eager_recorded_and_replayed_steps_are_one_launch_list(size, overlap):
    """A plan=False and a plan=True trainer from the same seed, no state copied between them: after each of 5 steps (plan: warm,
    record x3 geometries at most, replay) the master weights are BIT-equal.  test_plan_replay_equals_eager_steps_bf16 runs without
    slabs and so only to a tolerance; this is the exact statement."""
    te, tp = small_trainer(size, False, overlap), small_trainer(size, True, overlap)
    bs = small_batches(size)
    replayed = 0
    for i in range(5):
        n_plans = len(tp._plans)
        le, lp = te.step(bs[i % 3]), tp.step(bs[i % 3])
        replayed += int(i > 0 and len(tp._plans) == n_plans)
        e, p = bufs_of(te), bufs_of(tp)
        for k in BUFS + ("compute",):
            assert torch.equal(e[k], p[k]), (i + 1, k, differing(e[k], p[k]))
        assert torch.allclose(le, lp, rtol=1e-5, atol=1e-7), (i + 1, le, lp)
        assert te.grad_norm() == tp.grad_norm(), (i + 1, te.grad_norm(), tp.grad_norm())
        assert grads_cleared_outside_kept_chunks(te, size) and grads_cleared_outside_kept_chunks(tp, size), i + 1
    assert replayed >= 1 and 1 <= len(tp._plans) <= 3 and tp.t == te.t == 5
    te.close(), tp.close()


# ---------------------------------------------------------------- stop and resume
N_STEPS, CUT = 8, 4


def uninterrupted(size, plan, overlap):
    """8 steps; buffers, losses and gradient norm after each; the snapshot taken after step 4 (a copy: the run goes on)"""
    from test_continuity_cpu import snapshot
    tr = small_trainer(size, plan, overlap)
    bs = small_batches(size)
    after, snap, replayed = [], None, 0
    for i in range(N_STEPS):
        n_plans = len(tr._plans)
        loss = tr.step(bs[i % 3])
        replayed += int(plan and i > 0 and len(tr._plans) == n_plans)
        rec = bufs_of(tr)
        rec["loss"], rec["norm"] = loss.clone(), tr.grad_norm()
        after.append(rec)
        if i + 1 == CUT:
            snap = snapshot(tr)
    if plan:                                   # plans of every geometry were replayed on both sides of the cut
        assert replayed >= N_STEPS - 1 - 3 and len(tr._plans) <= 3
    final = snapshot(tr)
    tr.close()
    return after, snap, final


@pytest.mark.parametrize("overlap", [False, True], ids=["plain", "overlap"])
@pytest.mark.parametrize("plan", [False, True], ids=["eager", "plan"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_resumed_run_equals_uninterrupted_run_on_the_device(size, plan, overlap):
    """8 steps against 4 steps + snapshot + a fresh trainer (other weights, other codebook) + restore + 4 steps: master, both
    moments and the compute copy bit-equal after each of steps 5-8, compute == bf16(master), equal gradient norm, losses to 1e-5
    (the one documented atomic sum).  With plan=True the resumed trainer runs step 5 eagerly and records from step 6 on while the
    uninterrupted one replays.  Negative controls: a restore without load_state (the dropout masks of step 1 repeat) and one
    without step_dev (the schedule restarts at rate 0) must DIFFER after step 5."""
    from test_continuity_cpu import restore, snapshot
    after, snap, final = uninterrupted(size, plan, overlap)
    bs = small_batches(size)
    tr = small_trainer(size, plan, overlap, seed=8)
    assert not torch.equal(tr.store.master.cpu(), snap["master"]) and not torch.equal(tr.store.centroids.cpu(), snap["centroids"])
    restore(tr, snap)
    for i in range(CUT, N_STEPS):
        loss = tr.step(bs[i % 3])
        got, want = bufs_of(tr), after[i]
        for k in BUFS + ("compute",):
            assert torch.equal(got[k], want[k]), (i + 1, k, differing(got[k], want[k]))
        assert torch.equal(got["compute"], got["master"].to(torch.bfloat16)), i + 1
        assert tr.grad_norm() == want["norm"], (i + 1, tr.grad_norm(), want["norm"])
        assert torch.allclose(loss, want["loss"], rtol=1e-5, atol=1e-7), (i + 1, loss, want["loss"])
        assert grads_cleared_outside_kept_chunks(tr, size), i + 1
    got = snapshot(tr)
    for k in ("t", "micro", "step_dev"):
        assert int(got[k]) == int(final[k]) == N_STEPS, k
    tr.close()
    for piece in ("load_state", "step_dev"):
        tr = small_trainer(size, plan, overlap, seed=8)
        restore(tr, snap, without=piece)
        tr.step(bs[CUT % 3])
        m = bufs_of(tr)["master"]
        print(f"control {size} plan={plan} overlap={overlap} without {piece}: {differing(m, after[CUT]['master'])} after step {CUT + 1}")
        assert not torch.equal(m, after[CUT]["master"]), piece
        assert torch.isfinite(m).all()
        tr.close()


# ---------------------------------------------------------------- plan mode through accumulation windows
# (batch, update): warm, record, replay | window of two | replays | window of three | replays
CALLS = [(0, True), (1, True), (2, True), (0, False), (1, True), (2, True), (0, True), (1, False), (2, False), (0, True), (1, True)]


@pytest.mark.parametrize("overlap", [False, True], ids=["plain", "overlap"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_plan_mode_through_accumulation_windows(size, overlap):
    """step(update=False) routes a plan-mode trainer through the eager path and back: the two paths meet with different
    grad_is_zero / dw_overwrite / kept-range state.  Against a plan=False trainer on the same calls, after every update: master,
    both moments and the compute copy bit-equal, step_dev = number of updates, micro = number of calls, the recorded plans still
    there, and the gradient buffer zero outside the kept chunks.

    Measured: bit-equal after all 8 updates at "d256" (kept ranges, no K split anywhere), and at "d128" after every update that
    does not close a window.  The two updates that close a window at "d128" are NOT bit-reproducible -- not between the eager and
    the plan trainer, and just as little between two plan=False trainers from the same seed (max |d| 3.7e-9 on 0.01 % of the
    master weights; only the visual side's Linear weights differ).  The launch: xl_gemm's K-split weight gradient on the 128 x 128
    MFMA kernel -- the visual side's dW[M, N] += dY[1024, M]^T X[1024, N] with M, N <= 384 is below the ping-pong kernel's tile
    threshold, so xl_gemm_wgrad_group hands every problem to xl_gemm, which cuts K = B * V = 1024 into two slices that meet in C
    through fp32 atomics (xl_set_gemm_wgrad_slabs covers the ping-pong kernel's K splits only: csrc/gemm.hip).  Into a cleared
    buffer two addends commute -- which is why single-batch steps repeat themselves at this size -- but a window's second micro-
    batch adds them to the first one's gradient: three addends in arrival order, the unordered fp32 atomic sum DESIGN.md
    documents for K-split weight gradients.  With 8 examples (K = 512: no split) the same calls are bit-equal.  So at "d128" a
    window's closing update is held to the bounds of test_plan_replay_equals_eager_steps_bf16 instead (loss 2e-5, gradient norm
    2e-4 relative, parameter difference <= 2e-3 of the step's parameter movement), and as there the eager trainer's state is
    copied over afterwards, so that every following replay is again compared bit for bit."""
    te, tp = small_trainer(size, False, overlap), small_trainer(size, True, overlap)
    bs = small_batches(size)
    n_used = te.store.n_used
    updates, recorded, replayed = 0, set(), 0
    for n, (b, update) in enumerate(CALLS, start=1):
        n_plans = len(tp._plans)
        before = te.store.master[:n_used].clone()
        le, lp = te.step(bs[b], update=update), tp.step(bs[b], update=update)
        if not update:
            assert len(tp._plans) == n_plans                # (a window records nothing)
            continue
        updates += 1
        closes_window = not CALLS[n - 2][1]
        replayed += int(n > 1 and not closes_window and len(tp._plans) == n_plans)
        e, p = bufs_of(te), bufs_of(tp)
        if closes_window and size == "d128":
            ne, np_ = te.grad_norm(), tp.grad_norm()
            moved = (e["master"][:n_used] - before).norm().item()
            diff = (e["master"][:n_used] - p["master"][:n_used]).norm().item()
            print(f"window closed by call {n} ({size}, overlap={overlap}): {differing(e['master'], p['master'])}; |dp| {diff:.3e} of "
                  f"movement {moved:.3e}; norm {ne!r} vs {np_!r}; loss {le[0].item()!r} vs {lp[0].item()!r}")
            assert abs(le[0].item() - lp[0].item()) <= 2e-5 * abs(le[0].item()), (n, le, lp)
            assert abs(ne - np_) <= 2e-4 * ne, (n, ne, np_)
            assert moved > 0 and diff <= 2e-3 * moved, (n, diff, moved)
            for k in BUFS + ("compute",):                   # same starting point for the steps that follow
                getattr(tp.store, k).copy_(getattr(te.store, k))
        else:
            for k in BUFS + ("compute",):
                assert torch.equal(e[k], p[k]), (n, k, differing(e[k], p[k]))
            assert te.grad_norm() == tp.grad_norm(), (n, te.grad_norm(), tp.grad_norm())
        for tr in (te, tp):
            assert int(tr.step_dev.item()) == updates == tr.t and tr.micro == n, (n, int(tr.step_dev.item()), tr.t, tr.micro)
            assert grads_cleared_outside_kept_chunks(tr, size), n
        assert recorded <= set(tp._plans), (n, recorded, set(tp._plans))      # a window drops no recorded geometry
        recorded |= set(tp._plans)
    assert updates == 8 and 1 <= len(recorded) <= 3 and replayed >= 3, (updates, recorded, replayed)
    te.close(), tp.close()


def test_accumulation_window_stores_then_adds_fp32():
    """fp32, dropout off, learning rate 0, the TINY model: a plan-mode trainer runs warm / record / replay, then a window of two
    micro-batches -- afterwards the gradient buffer holds the SUM of the oracle's gradients of the two batches (the first
    micro-batch stored over what the replay left, the second added), to the 1e-4 * max(1, |g|max) of
    test_edge_case_batches_match_oracle_fp32; the replay that follows holds its own batch's gradient alone."""
    from test_trainer_cpu import TINY, oracle_cfg, oracle_grads
    from xlxmert_amd.config import XLxmertConfig
    from xlxmert_amd.params import ParamStore
    from xlxmert_amd.trainer import PretrainStep, synthetic_batch
    cfg = XLxmertConfig(**TINY)
    sd = O.make_state_dict(oracle_cfg(cfg), 11)
    host = [synthetic_batch(cfg, 3, 8, 4, seed=610 + i) for i in range(3)]
    dev = [{k: v.cuda() for k, v in b.items()} for b in host]
    store = ParamStore(cfg, "cuda", torch.float32)
    store.load_named(sd)
    tr = PretrainStep(cfg, 3, 8, 16, dtype=torch.float32, device="cuda", store=store, lr=0.0, total_steps=10, plan=True,
                      drop_grads=False, visual_losses="obj,feat", train_dropout=False)
    assert tr.plan_mode and tr.overwrite_grads and not tr.drop_grads
    want = [oracle_grads(cfg, sd, b)[0] for b in host]

    def check(expect, what):
        tr.sync()
        n = 0
        for k, g in expect.items():
            if k == "obj_predict_head.out_cluster.weight":
                continue
            got = store.gview(k).cpu()
            assert torch.isfinite(got).all(), (what, k)
            d = (got - g).abs().max().item()
            assert d < 1e-4 * max(1.0, g.abs().max().item()), (what, k, d)
            n += 1
        assert n > 80

    for i in range(3):
        tr.step(dev[i])
    assert len(tr._plans) >= 1
    check(want[2], "after warm, record, replay")
    tr.step(dev[0], update=False)
    check(want[0], "first micro-batch: stored")
    tr.step(dev[1])
    check({k: want[0][k] + want[1][k] for k in want[0]}, "second micro-batch: added")
    n_plans = len(tr._plans)
    tr.step(dev[2])
    check(want[2], "the step after the window starts over")
    assert len(tr._plans) >= n_plans and int(tr.step_dev.item()) == 5 and tr.micro == 6
    tr.close()


# ---------------------------------------------------------------- the partial-master guard survives a replay
def _guard_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from test_trainer_cpu import TINY, oracle_cfg
    from xlxmert_amd.config import XLxmertConfig
    from xlxmert_amd.engine import reserve_streams
    from xlxmert_amd.params import ParamStore
    from xlxmert_amd.trainer import PretrainStep, synthetic_batch
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), XL_COMM="torch")
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    reserve_streams(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = XLxmertConfig(**TINY)
    store = ParamStore(cfg, dev, torch.bfloat16, task="vis_mask")
    store.load_named(O.make_state_dict(oracle_cfg(cfg), 3))
    tr = PretrainStep(cfg, 2, 8, 16, dtype=torch.bfloat16, device=dev, store=store, total_steps=10, lr=1e-2, bucket_mb=0.05,
                      visual_losses="obj,feat", plan=True, drop_grads=False, collective="rs+ag", gather="bf16")
    tr.ops.set_gemm_wgrad_slabs(1)
    assert tr.sharded and tr.gather_bf16 and tr.plan_mode and not store.master_partial
    n = store.n_used
    out = {}

    def step(t):
        tr.step({k: v.to(dev) for k, v in synthetic_batch(cfg, 2, 8, 4, seed=500 + 10 * t + rank).items()})
        tr.sync()

    def raises():
        try:
            store.named_state()
        except RuntimeError as e:
            return "gather_state" in str(e)
        return False

    step(0), step(1)                                         # warm, record
    assert len(tr._plans) == 1
    assert raises(), "named_state() after the recorded step"
    tr.gather_state()
    assert not store.master_partial and store.named_state()
    out["master_after_record"] = store.master[:n].cpu().clone()
    step(1)                                                  # REPLAY (the recorded step's batch: the same launch geometry for
    assert len(tr._plans) == 1 and tr.t == 3                 # certain): no Python of the recorded body runs
    assert raises(), "named_state() after the REPLAYED step: the guard was not armed again"
    # a stale master copy must not reach the compute copy
    before, compute = store.master.clone(), store.compute.clone()
    store.master.add_(1.0)
    tr.engine.sync_compute_weights()
    tr.sync()
    assert torch.equal(store.compute, compute), "sync_compute_weights() cast a partial master copy over the compute copy"
    store.master.copy_(before)
    tr.gather_state()
    assert not store.master_partial and store.named_state()
    out["master_after_replay"] = store.master[:n].cpu().clone()
    out["compute_after_replay"] = store.compute[:n].cpu().clone()
    assert torch.equal(store.compute[:n], store.master[:n].to(torch.bfloat16))
    assert not torch.equal(out["master_after_replay"], out["master_after_record"])
    tr.close()
    torch.save(out, os.path.join(out_dir, f"c{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_partial_master_guard_survives_replay_two_ranks_sharing_one_gpu_gloo(tmp_path):
    """plan=True + collective="rs+ag" + gather="bf16", two ranks on one GPU over gloo: after warm + record named_state() raises;
    gather_state() makes the master copy whole (equal on both ranks); the REPLAYED step must raise the guard again -- the flag
    used to be set only inside the recorded Python body, which a replay skips -- sync_compute_weights() must leave the compute
    copy alone meanwhile, and the second gather_state() gives equal master copies with compute == bf16(master)."""
    import torch.multiprocessing as mp
    from test_trainer_cpu import _free_port
    world, port = 2, _free_port()
    mp.spawn(_guard_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "c0.pt"), torch.load(tmp_path / "c1.pt")
    assert sorted(r0) == ["compute_after_replay", "master_after_record", "master_after_replay"]
    for k in r0:
        assert torch.equal(r0[k], r1[k]), k


# ---------------------------------------------------------------- a sharded plan-mode run stopped and resumed
def _sharded_resume_worker(rank, world, port, out_dir, gather):
    import torch.distributed as dist
    from test_continuity_cpu import SH_BUFS, SH_CUT, SH_STEPS, resume_sharded, save_checkpoint, sharded_bufs, sharded_step, sharded_trainer
    from xlxmert_amd.engine import reserve_streams
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), XL_COMM="torch")
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    reserve_streams(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    kw = dict(dev=dev, plan=True, drop_grads=False)

    def refused(fn):
        try:
            fn()
        except RuntimeError as e:
            return "gather_state" in str(e)
        return False

    # the uninterrupted run; batches of period 2: warm (b0), record (b1), record or replay (b0), REPLAY (b1: recorded for certain)
    ref = sharded_trainer(gather, 3, **kw)
    ref.ops.set_gemm_wgrad_slabs(1)
    assert ref.plan_mode
    for t in range(SH_STEPS):
        if t == SH_STEPS - 1:
            ref.gather_state()                               # (the guard comes down: the replay alone must raise it again)
            assert not ref.store.moments_partial and ref.state()["t"] == t
        n_plans = len(ref._plans)
        sharded_step(ref, t, rank, cycle=2)
    ref.sync()
    assert len(ref._plans) == n_plans and n_plans in (1, 2) and ref.t == SH_STEPS, "the last step was to be a replay"
    assert ref.store.moments_partial, "the partial-moments guard was not armed by the REPLAYED step"
    assert refused(ref.state) and refused(ref.store.moments)
    want = sharded_bufs(ref)
    ref.close()
    # cut after the recorded step, checkpoint from rank 0, fresh trainers: step 3 runs eagerly (warm), step 4 records
    tr = sharded_trainer(gather, 3, **kw)
    tr.ops.set_gemm_wgrad_slabs(1)
    for t in range(SH_CUT):
        sharded_step(tr, t, rank, cycle=2)
    tr.sync()
    assert refused(tr.state) and refused(tr.store.moments)
    tr.gather_state()
    path = os.path.join(out_dir, "ckpt.pt")
    if rank == 0:
        save_checkpoint(tr, path)
    tr.close()
    dist.barrier()
    tr2 = resume_sharded(gather, rank, path, **kw)
    tr2.ops.set_gemm_wgrad_slabs(1)
    assert (tr2.t, tr2.micro, int(tr2.step_dev.item())) == (SH_CUT, SH_CUT, SH_CUT)
    for t in range(SH_CUT, SH_STEPS):
        sharded_step(tr2, t, rank, cycle=2)
    tr2.sync()
    assert len(tr2._plans) == 1 and tr2.store.moments_partial
    got = sharded_bufs(tr2)
    assert tr2.verify_replicas() == []
    for k in SH_BUFS:
        assert torch.equal(got[k], want[k]), (gather, rank, k, differing(got[k], want[k]))
    tr2.close()
    torch.save(got, os.path.join(out_dir, f"got{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("gather", ["fp32", "bf16"])
def test_sharded_plan_run_resumes_bit_for_bit_two_ranks_sharing_one_gpu_gloo(tmp_path, gather):
    """tests/test_continuity_cpu.py's sharded resume on the real kernels with plan=True, two ranks on one GPU over gloo (fp32 store
    with the fp32 gather, bf16 store with the bf16 gather; K-split weight gradients through slabs): two steps, gather_state(), rank 0
    saves, fresh trainers resume and run two more -- the third eagerly, the fourth recording, where the uninterrupted run records
    and REPLAYS.  Compute copy, gathered master weights and both moments bit-equal on both ranks.  state() and ParamStore.moments()
    raise until gather_state(), also after the replayed step."""
    import torch.multiprocessing as mp
    from test_continuity_cpu import SH_BUFS
    from test_trainer_cpu import _free_port
    world, port = 2, _free_port()
    mp.spawn(_sharded_resume_worker, args=(world, port, str(tmp_path), gather), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "got0.pt"), torch.load(tmp_path / "got1.pt")
    for k in SH_BUFS:
        assert torch.equal(r0[k], r1[k]), k
