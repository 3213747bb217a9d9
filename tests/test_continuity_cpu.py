"""Training-state continuity on the CPU (kernels replaced by FakeOps): a run that is stopped, saved, rebuilt in a fresh trainer and
continued must equal the run that was never stopped, bit for bit -- and every piece of the saved state must be OBSERVED (a restore
that leaves one out must differ).  Second half: the partial-master guard of the sharded exchange's bf16 gather (gloo, world 2), and a
SHARDED run stopped and resumed on three ranks: bit for bit after gather_state(), refused (the partial-moments guard) without it.

snapshot() / restore() below are what PretrainStep.state()'s docstring tells a user to do, through public names only; the GPU
twin (tests/test_continuity_gpu.py) imports them."""
import functools
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import lxmert_oracle as O
from fake_ops import FakeOps
from test_trainer_cpu import TINY, _free_port, make_step, oracle_cfg
from xlxmert_amd.config import XLxmertConfig
from xlxmert_amd.params import ParamStore
from xlxmert_amd.trainer import PretrainStep, synthetic_batch

BUFS = ("master", "exp_avg", "exp_avg_sq")
COUNTERS = ("t", "micro", "step_dev", "chunk_steps")


def snapshot(tr):
    """everything a resumed run needs, as a dict of CPU tensors: the three flat buffers, the codebook, PretrainStep.state()"""
    tr.sync()
    st = tr.store
    snap = {k: getattr(st, k).detach().cpu().clone() for k in BUFS}
    snap["centroids"] = st.centroids.detach().cpu().clone()
    snap.update({k: torch.as_tensor(v).clone() for k, v in tr.state().items()})
    return snap


def restore(tr, snap, without=None):
    """the docstring's recipe: buffers in place, set_centroids, load_state, sync_compute_weights.  `without` leaves ONE piece out
    (the negative controls): "codebook"; "step_dev" / "chunk_steps" (the key is dropped from the dict load_state gets); or
    "load_state" -- load_state is not called at all, and so that the control isolates what ONLY load_state can restore (the host
    counters `t` and `micro`) the device counters are written through their public attributes instead."""
    assert without in (None, "codebook", "step_dev", "chunk_steps", "load_state"), without
    st = tr.store
    for k in BUFS:
        getattr(st, k).copy_(snap[k])
    if without != "codebook":
        tr.set_centroids(snap["centroids"])
    if without == "load_state":
        tr.step_dev.fill_(int(snap["step_dev"]))
        if "chunk_steps" in snap:
            tr.chunk_steps.copy_(snap["chunk_steps"])
    else:
        tr.load_state({k: snap[k] for k in COUNTERS if k in snap and k != without})
    tr.engine.sync_compute_weights()


# ---------------------------------------------------------------- 1. stop and resume, six arms
B, L, GRID = 3, 8, 4
N_STEPS, CUT = 6, 3
ALL_ORDER = ["vis_mask", "word_mask", "matched", "vis_mask", "word_mask", "vis_mask"]
ARMS = {f"{task}-{name}": (task, kw) for task in ("vis_mask", "all")
        for name, kw in (("plain", {}), ("overlap", {"overlap_optimizer": True}), ("dropout", {"train_dropout": True}))}
HYPER = dict(lr=1e-2, weight_decay=0.01, warmup_ratio=0.3)          # (total_steps = 10: the rate still rises at the cut, then falls)


def build(task, kw, seed):
    cfg = XLxmertConfig(**TINY)
    if task == "vis_mask":
        return make_step(cfg, B, L, GRID, seed=seed, **HYPER, **kw)[0]
    store = ParamStore(cfg, "cpu", torch.float32, task="all")
    store.load_named(O.make_cls_state_dict(oracle_cfg(cfg), seed))
    return PretrainStep(cfg, B, L, GRID * GRID, dtype=torch.float32, device="cpu", store=store, ops=FakeOps(torch.float32),
                        total_steps=10, task="all", visual_losses="obj,feat", **HYPER, **kw)


@functools.lru_cache(maxsize=None)
def batches():
    cfg = XLxmertConfig(**TINY)
    out = []
    for t in range(1, N_STEPS + 1):
        b = synthetic_batch(cfg, B, L, GRID, seed=300 + t)
        b["word_labels"], b["matched_labels"] = O.make_lang_task_labels(oracle_cfg(cfg), b["input_ids"], 400 + t)
        out.append(b)
    return out


def run_step(tr, task, i):
    """step i (0-based) of the arm's schedule"""
    return tr.step(batches()[i], task=ALL_ORDER[i]) if task == "all" else tr.step(batches()[i])


def clone_bufs(tr):
    return {k: getattr(tr.store, k).clone() for k in BUFS}


@functools.lru_cache(maxsize=None)
def reference(arm):
    """the uninterrupted run (buffers after every step, final counters) and the snapshot of a second trainer stopped after CUT
    steps -- computed once per arm, read-only from then on"""
    task, kw = ARMS[arm]
    tr = build(task, kw, seed=3)
    after = []
    for i in range(N_STEPS):
        run_step(tr, task, i)
        after.append(clone_bufs(tr))
    final = snapshot(tr)
    tr2 = build(task, kw, seed=3)
    for i in range(CUT):
        run_step(tr2, task, i)
    assert all(torch.equal(getattr(tr2.store, k), after[CUT - 1][k]) for k in BUFS)       # (the CPU path repeats itself)
    return after, final, snapshot(tr2)


@pytest.mark.parametrize("arm", sorted(ARMS))
def test_resumed_run_equals_uninterrupted_run(arm):
    """6 steps against 3 steps + snapshot + a FRESH trainer from other weights and another codebook + restore + 3 steps: master
    weights and both Adam moments bit-identical after each of steps 4, 5, 6, and the counters at the end.  The warm-up ends at the
    cut (warmup_ratio 0.3 of 10 steps), so the learning rate differs on either side of it; task="all" has skipped different
    tensors a different number of times by then (chunk_steps); the dropout arms draw their masks from `micro`."""
    task, kw = ARMS[arm]
    after, final, snap = reference(arm)
    tr = build(task, kw, seed=8)
    assert not torch.equal(tr.store.master, snap["master"]) and not torch.equal(tr.store.centroids, snap["centroids"])
    restore(tr, snap)
    for i in range(CUT, N_STEPS):
        run_step(tr, task, i)
        for k in BUFS:
            got, want = getattr(tr.store, k), after[i][k]
            assert torch.equal(got, want), (arm, i + 1, k, (got - want).abs().max().item())
    got = snapshot(tr)
    assert int(got["t"]) == int(final["t"]) == N_STEPS and int(got["micro"]) == int(final["micro"]) == N_STEPS
    assert int(got["step_dev"]) == int(final["step_dev"]) == N_STEPS
    assert ("chunk_steps" in got) == (task == "all")
    if task == "all":
        assert got["chunk_steps"].dtype == torch.int32 and torch.equal(got["chunk_steps"], final["chunk_steps"])
        n = got["chunk_steps"][:tr.store.n_used // 256]
        assert int(n.max()) == N_STEPS and 0 < int(n.min()) < N_STEPS          # per-tensor counts really differ
        assert len(set(snap["chunk_steps"].tolist())) > 2                       # ... already at the cut


CONTROLS = [(arm, piece) for arm in sorted(ARMS) for piece in ("step_dev", "codebook", "chunk_steps", "load_state")
            if (piece != "chunk_steps" or arm.startswith("all")) and (piece != "load_state" or arm.endswith("dropout"))]


@pytest.mark.parametrize("arm,piece", CONTROLS, ids=[f"{a}-without-{p}" for a, p in CONTROLS])
def test_restore_that_leaves_a_piece_out_differs(arm, piece):
    """negative controls: each restored piece is observed by the very next step -- leaving it out MUST change step 4.
    step_dev: the schedule restarts at rate 0; chunk_steps: every tensor's bias correction restarts; codebook: the fresh trainer's
    own centroids feed the inputs and the feature targets; load_state (dropout arms): `micro` restarts, the masks of step 1 repeat."""
    task, kw = ARMS[arm]
    after, _, snap = reference(arm)
    tr = build(task, kw, seed=8)
    restore(tr, snap, without=piece)
    run_step(tr, task, CUT)
    d = (tr.store.master - after[CUT]["master"]).abs().max().item()
    print(f"control {arm} without {piece}: max |master - uninterrupted| after step {CUT + 1} = {d:.3e}")
    assert not torch.equal(tr.store.master, after[CUT]["master"]), (arm, piece)
    assert torch.isfinite(tr.store.master).all()


def test_load_state_accepts_the_two_counter_dict_and_writes_in_place():
    """today's {"t", "micro"} dict still loads and leaves the device counters alone; the new keys land in the EXISTING buffers
    (recorded launch plans hold their addresses)."""
    tr = build("all", {}, seed=3)
    run_step(tr, "all", 0)
    p_step, p_chunk, counts = tr.step_dev.data_ptr(), tr.chunk_steps.data_ptr(), tr.chunk_steps.clone()
    tr.load_state({"t": 5, "micro": 9})
    assert (tr.t, tr.micro) == (5, 9) and int(tr.step_dev) == 1 and torch.equal(tr.chunk_steps, counts)
    tr.load_state({"t": 4})
    assert (tr.t, tr.micro) == (4, 4)
    st = tr.state()
    assert set(st) == {"t", "micro", "step_dev", "chunk_steps"} and st["step_dev"] == 1
    assert st["chunk_steps"].device.type == "cpu" and st["chunk_steps"].dtype == torch.int32
    st["chunk_steps"] += 2                                          # a copy: the trainer's counts do not move with it
    assert torch.equal(tr.chunk_steps, counts)
    tr.load_state(dict(st, step_dev=torch.tensor([7])))
    assert int(tr.step_dev) == 7 and torch.equal(tr.chunk_steps, counts + 2)
    assert tr.step_dev.data_ptr() == p_step and tr.chunk_steps.data_ptr() == p_chunk
    assert set(build("vis_mask", {}, seed=3).state()) == {"t", "micro", "step_dev"}


# ---------------------------------------------------------------- 4. the partial-master guard (gloo, world 2, bf16 store)
def _guard_worker(rank, world, port, out_dir, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    cfg = XLxmertConfig(**TINY)
    oc = oracle_cfg(cfg)
    store = ParamStore(cfg, "cpu", torch.bfloat16, task="vis_mask")
    store.load_named(O.make_state_dict(oc, 3))
    tr = PretrainStep(cfg, 2, 8, 16, dtype=torch.bfloat16, device="cpu", store=store, ops=FakeOps(torch.bfloat16), total_steps=10,
                      lr=1e-2, weight_decay=0.01, bucket_mb=0.05, collective="rs+ag", gather="bf16", visual_losses="obj,feat")
    assert tr.sharded and tr.gather_bf16 and not store.master_partial
    tr.step(synthetic_batch(cfg, 2, 8, 4, seed=500 + rank))
    assert store.master_partial
    with pytest.raises(RuntimeError, match="gather_state"):
        store.named_state()
    if mode == "eager":
        tr.gather_state()
        assert not store.master_partial and store.named_state()
        tr.step(synthetic_batch(cfg, 2, 8, 4, seed=510 + rank))
        assert store.master_partial                          # armed again by the step after the gather
        with pytest.raises(RuntimeError, match="gather_state"):
            store.named_state()
        assert tr.verify_replicas() == [] and not store.master_partial
    else:
        # a state-dict load after a step that skipped gather_state(): the master copy is whole again, so the guard must come down --
        # otherwise sync_compute_weights() returns early and the compute copy stays on the OLD weights
        sd2 = O.make_state_dict(oc, 4)
        assert store.load_named(sd2) == []
        assert not store.master_partial
        tr.engine.sync_compute_weights()
        named = store.named_state()
        for name in store.index:
            assert torch.equal(store.cview(name), sd2[name].to(torch.bfloat16)), name
            assert torch.equal(named[name], sd2[name]), name
        assert torch.equal(named["vis_emb.weight"], sd2["vis_emb.weight"])
        # a load that misses tensors leaves their (possibly stale) values: the guard stays up
        store.master_partial = True
        some = dict(sd2)
        del some["bert.pooler.dense.weight"]
        assert store.load_named(some) == ["bert.pooler.dense.weight"] and store.master_partial
    open(os.path.join(out_dir, f"ok{rank}"), "w").close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["eager", "load_named"])
def test_partial_master_guard_world2_gloo(tmp_path, mode):
    """sharded exchange, gather="bf16": every update leaves the fp32 master matrices current on their owner only.
    eager: step, gather_state(), step -- the guard is up again after the second step (named_state raises).
    load_named: step without gather_state(), then ParamStore.load_named(sd2) -- the guard is down, sync_compute_weights() casts
    (the compute copy equals the bf16 cast of sd2) and named_state() returns sd2's values."""
    world, port = 2, _free_port()
    mp.spawn(_guard_worker, args=(world, port, str(tmp_path), mode), nprocs=world, join=True)
    assert (tmp_path / "ok0").exists() and (tmp_path / "ok1").exists()


# ---------------------------------------------------------------- 5. a SHARDED run stopped and resumed (gloo, world 3)
# rs+ag: a rank's Adam moments -- and with gather="bf16" its master matrices -- are current on its own shards only.  The checkpoint is
# written by rank 0 alone and reaches the other ranks through sync_replicas(): without gather_state() first, two thirds of it are stale.
SH_WORLD, SH_STEPS, SH_CUT = 3, 4, 2
SH_BUFS = ("master", "compute", "exp_avg", "exp_avg_sq")


def sharded_trainer(gather, seed, dev="cpu", ops=None, prepare=None, **kw):
    """the sharded tiny trainer of the resume tests (the GPU twin passes its device and leaves `ops` to the product); `prepare(store)`
    runs between the weight load and the constructor -- where a resuming rank 0 puts the checkpoint in"""
    cfg = XLxmertConfig(**TINY)
    dtype = torch.bfloat16 if gather == "bf16" else torch.float32
    store = ParamStore(cfg, dev, dtype, task="vis_mask")
    store.load_named(O.make_state_dict(oracle_cfg(cfg), seed))
    if prepare is not None:
        prepare(store)
    if ops is None and dev == "cpu":
        ops = FakeOps(dtype)
    tr = PretrainStep(cfg, 2, 8, 16, dtype=dtype, device=dev, store=store, ops=ops, total_steps=10, lr=1e-2, weight_decay=0.01,
                      warmup_ratio=0.3, bucket_mb=0.05, collective="rs+ag", gather=gather, visual_losses="obj,feat", **kw)
    assert tr.sharded and tr.gather_bf16 == (gather == "bf16") and not store.moments_partial
    return tr


def sharded_step(tr, t, rank, cycle=None):
    """step t (0-based) on this rank's own minibatch; cycle: the batches repeat with that period (launch geometries that come back:
    the GPU twin wants plan replays)"""
    cfg = XLxmertConfig(**TINY)
    seed = 500 + 10 * (t % cycle if cycle else t) + rank
    tr.step({k: v.to(tr.device) for k, v in synthetic_batch(cfg, 2, 8, 4, seed=seed).items()})


def sharded_bufs(tr):
    """compute copy as the steps left it, then -- gathered -- master weights and both moments"""
    tr.sync()
    n = tr.store.n_used
    out = {"compute": tr.store.compute[:n].cpu().clone()}
    tr.gather_state()
    m, v = tr.store.moments()
    out.update(master=tr.store.master[:n].cpu().clone(), exp_avg=m[:n].cpu().clone(), exp_avg_sq=v[:n].cpu().clone())
    return out


def save_checkpoint(tr, path, raw=False):
    """what PretrainStep.state() tells a caller to save.  raw: around the guards, as a caller could before they existed -- the buffers
    as this rank holds them and the counters read one by one"""
    st = tr.store
    tr.sync()
    if raw:
        m, v = st.exp_avg, st.exp_avg_sq
        state = {"t": tr.t, "micro": tr.micro, "step_dev": int(tr.step_dev.item())}
    else:
        (m, v), state = st.moments(), tr.state()
    torch.save({"master": st.master.cpu().clone(), "exp_avg": m.cpu().clone(), "exp_avg_sq": v.cpu().clone(),
                "centroids": st.centroids.cpu().clone(), "state": state}, path)


def resume_sharded(gather, rank, path, seed=8, **kw):
    """every rank: a fresh store (other weights, another codebook) and a fresh trainer; rank 0 alone copies the saved buffers in before
    the constructor runs, whose sync_replicas() hands them to the others; all ranks load the counters"""
    ck = torch.load(path)

    def put(store):
        store.ensure_adam_state()
        for k in ("master", "exp_avg", "exp_avg_sq"):
            getattr(store, k).copy_(ck[k])
        store.set_centroids(ck["centroids"])
    tr = sharded_trainer(gather, seed, prepare=put if rank == 0 else None, **kw)
    tr.load_state(ck["state"])
    return tr


def _sharded_resume_worker(rank, world, port, out_dir, gather, with_gather):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    ref = sharded_trainer(gather, 3)
    for t in range(SH_STEPS):
        sharded_step(ref, t, rank)
    want = sharded_bufs(ref)
    tr = sharded_trainer(gather, 3)
    for t in range(SH_CUT):
        sharded_step(tr, t, rank)
    path = os.path.join(out_dir, "ckpt.pt")
    assert tr.store.moments_partial and tr.store.master_partial == (gather == "bf16")
    with pytest.raises(RuntimeError, match="gather_state"):
        tr.state()
    with pytest.raises(RuntimeError, match="gather_state"):
        tr.store.moments()
    if with_gather:
        tr.gather_state()
        assert not tr.store.moments_partial and not tr.store.master_partial
    if rank == 0:
        save_checkpoint(tr, path, raw=not with_gather)
    dist.barrier()
    tr2 = resume_sharded(gather, rank, path)
    assert (tr2.t, tr2.micro, int(tr2.step_dev.item())) == (SH_CUT, SH_CUT, SH_CUT) and not tr2.store.moments_partial
    for t in range(SH_CUT, SH_STEPS):
        sharded_step(tr2, t, rank)
        assert tr2.store.moments_partial                    # up again after every update
    got = sharded_bufs(tr2)
    assert tr2.verify_replicas() == []
    if with_gather:
        for k in SH_BUFS:
            assert torch.equal(got[k], want[k]), (gather, rank, k, (got[k].float() - want[k].float()).abs().max().item())
        assert tr2.state() == {"t": SH_STEPS, "micro": SH_STEPS, "step_dev": SH_STEPS}
    else:
        # the control: rank 0's stale moments went to every rank, nothing raised, the replicas agree -- and the run is another one
        d = (got["master"] - want["master"]).abs().max().item()
        print(f"sharded resume WITHOUT gather_state ({gather}, rank {rank}): max |master - uninterrupted| = {d:.3e}")
        assert not torch.equal(got["master"], want["master"]) and not torch.equal(got["exp_avg"], want["exp_avg"])
        assert torch.isfinite(got["master"]).all()
    torch.save(got, os.path.join(out_dir, f"got{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("gather", ["fp32", "bf16"])
def test_sharded_run_resumes_bit_for_bit_world3_gloo(tmp_path, gather):
    """collective="rs+ag" on three ranks (fp32 store with the fp32 gather, bf16 store with the bf16 gather): two steps, gather_state()
    on every rank, rank 0 alone saves master, moments, codebook and state(); three fresh trainers from other weights, rank 0's filled
    from the file before its constructor broadcasts; two more steps.  Compute copy, master weights and both moments (gathered) equal
    the uninterrupted four-step run bit for bit on every rank.  Before the gather, state() and ParamStore.moments() raise."""
    port = _free_port()
    mp.spawn(_sharded_resume_worker, args=(SH_WORLD, port, str(tmp_path), gather, True), nprocs=SH_WORLD, join=True)
    got = [torch.load(tmp_path / f"got{r}.pt") for r in range(SH_WORLD)]
    for g in got[1:]:
        for k in SH_BUFS:
            assert torch.equal(got[0][k], g[k]), k


@pytest.mark.parametrize("gather", ["fp32", "bf16"])
def test_sharded_checkpoint_without_gather_state_is_refused_world3_gloo(tmp_path, gather):
    """the same sequence with gather_state() left out: state() and ParamStore.moments() raise a RuntimeError that names
    gather_state() -- the guard this test came with.  That it guards something: a checkpoint taken around it (raw buffers of rank 0,
    counters by hand) resumes without any complaint, the replicas agree with each other, verify_replicas() is clean, and the
    parameters after two more steps are NOT the uninterrupted run's (measured: max |d| 2.1e-2 with the fp32 store, 2.7e-2 with the bf16 store, at lr 1e-2)."""
    port = _free_port()
    mp.spawn(_sharded_resume_worker, args=(SH_WORLD, port, str(tmp_path), gather, False), nprocs=SH_WORLD, join=True)
    got = [torch.load(tmp_path / f"got{r}.pt") for r in range(SH_WORLD)]
    for g in got[1:]:
        for k in SH_BUFS:
            assert torch.equal(got[0][k], g[k]), k
