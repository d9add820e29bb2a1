"""Node-partitioned engine on the GPU box: two and three ranks (all on cuda:0, gloo with
CPU staged collectives — RCCL needs one GPU per rank) against the single-GPU RGCN: logits, loss
and parameters after two epochs agree."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _problem(K=6):
    from mrgcn_amd import synth
    g = synth.make_graph("aifb", seed=9, scale=0.5)
    rng = np.random.default_rng(9)
    N = g.num_nodes
    X = rng.standard_normal((N, K)).astype(np.float32)
    idx = np.sort(rng.choice(N, 120, replace=False)).astype(np.int64)
    y = rng.integers(0, 4, 120).astype(np.int64)
    mods = [(K, 8, "mrgcn", torch.nn.ReLU()), (8, 4, "mrgcn", None)]
    return g, X, idx, y, mods


def _single():
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam, train_step
    g, X, idx, y, mods = _problem()
    N, R = g.num_nodes, g.num_relations
    torch.manual_seed(3)
    model = RGCN(mods, R, N, 5, 0.0, False, True, False)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.cuda()
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    Xg = torch.from_numpy(X).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
    logits0 = model(Xg, A).detach().cpu().numpy()
    losses = [float(train_step(model, lambda: model(Xg, A), torch.from_numpy(idx).cuda(),
                               torch.from_numpy(y).cuda(), opt)) for _ in range(2)]
    return state, logits0, losses, {k: v.cpu() for k, v in model.state_dict().items()}


def _worker(rank, world, port, state, out, backend="gloo"):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from mrgcn_amd.partition import NodePartition, PartitionedRGCN, partitioned_train_step
    from mrgcn_amd.train import ClipAdam
    dev = torch.device("cuda:0")
    if backend == "nccl":
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group("gloo")
    g, X, idx, y, mods = _problem()
    N, R = g.num_nodes, g.num_relations
    part = NodePartition(N, world, rank)
    model = PartitionedRGCN(mods, R, N, 5, False, True, part).to(dev)
    model.load_full_state(state)
    model.build_plan(g.rows, g.cols, g.vals, dev)
    Xl = part.shard_rows(torch.from_numpy(X)).to(dev)
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
    opt.set_distributed(None, model.sharded_parameters())
    logits0 = model(Xl).detach().cpu().numpy()[: part.n_local]
    losses = [float(partitioned_train_step(model, Xl, idx, y, opt)) for _ in range(2)]
    # the local shard is node-major (S, B, out): back to [B][own nodes][out]
    wI = model.layers["layer_0"].weight_I.detach().cpu().permute(1, 0, 2)[:, : part.n_local]
    out[rank] = (logits0, losses, wI.numpy(), model.layers["layer_1"].weight_F.detach().cpu().numpy())
    if backend == "nccl":
        # a step submits its work without waiting for the device anywhere: torch raises on any synchronising call
        # (the label shard, the plan and the optimizer state exist after the steps above)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(2):
                partitioned_train_step(model, Xl, idx, y, opt)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_ranks_equal_single_gpu(world):
    """world = 3: N is not a multiple of the rank count, so the last rank's node range is short
    and the reduce-scatter / all-gather payloads carry padding rows."""
    state, logits0, losses, final = _single()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), state, out), nprocs=world, join=True)
    ranks = range(world)
    got_logits = np.concatenate([out[r][0] for r in ranks], 0)
    np.testing.assert_allclose(got_logits, logits0, rtol=1e-4, atol=1e-4)
    for r in ranks:
        np.testing.assert_allclose(out[r][1], losses, rtol=2e-4, atol=2e-5)
    N = logits0.shape[0]
    wI = np.concatenate([out[r][2] for r in ranks], 1).reshape(5 * N, -1)
    d = np.abs(wI - final["layers.layer_0.weight_I"].numpy())
    assert (d > 2e-5).mean() < 5e-3 and d.max() <= 0.045      # Adam: lr-sized moves on noise-level grads
    for r in ranks:
        d = np.abs(out[r][3] - final["layers.layer_1.weight_F"].numpy())
        assert (d > 2e-5).mean() < 5e-3 and d.max() <= 0.045


@pytest.mark.timeout(600)
def test_partitioned_engine_over_rccl_with_one_rank():
    """The RCCL branches of the engine (reduce_scatter_tensor, all_gather_into_tensor, the asynchronous all-reduce
    of the replicated gradients from post-accumulate hooks, the sharded clip norm) executed on the one GPU this box
    has: a process group of world size 1 over the nccl backend.  The collectives are identities there, but tensor
    layouts, contiguity, stream ordering and the work handles are the ones an 8-GPU run uses — and the result must
    equal the single-GPU model's."""
    state, logits0, losses, final = _single()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(1, _free_port(), state, out, "nccl"), nprocs=1, join=True)
    np.testing.assert_allclose(out[0][0], logits0, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(out[0][1], losses, rtol=2e-4, atol=2e-5)
    N = logits0.shape[0]
    d = np.abs(out[0][2].reshape(5 * N, -1) - final["layers.layer_0.weight_I"].numpy())
    assert (d > 2e-5).mean() < 5e-3 and d.max() <= 0.045


def _graphed_worker(rank, world, port, state, out):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from mrgcn_amd.partition import GraphedPartitionedStep, NodePartition, PartitionedRGCN, partitioned_train_step
    from mrgcn_amd.train import ClipAdam
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev)
    g, X, idx, y, mods = _problem()
    N, R = g.num_nodes, g.num_relations
    part = NodePartition(N, world, rank)
    res = []
    for graphed in (False, True):
        model = PartitionedRGCN(mods, R, N, 5, False, True, part).to(dev)
        model.load_full_state(state)
        model.build_plan(g.rows, g.cols, g.vals, dev)
        Xl = part.shard_rows(torch.from_numpy(X)).to(dev)
        opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0, capturable=graphed)
        opt.set_distributed(None, model.sharded_parameters())
        if graphed:
            step = GraphedPartitionedStep(model, Xl, idx, y, opt, warmup=2)
            losses = [float(step()) for _ in range(3)]
        else:
            for _ in range(2):
                partitioned_train_step(model, Xl, idx, y, opt)
            losses = [float(partitioned_train_step(model, Xl, idx, y, opt)) for _ in range(3)]
        res.append((losses, model.layers["layer_1"].weight_F.detach().cpu().numpy()))
    # the optimizer's state loaded after the capture: the captured graph would go on updating the old moments
    kept = (dict(opt.state), dict(opt._dev_step))
    opt.load_state_dict(opt.state_dict())
    try:
        step()
        refused = None
    except Exception as e:  # noqa: BLE001  (its type and text are the parent's to judge)
        refused = (type(e).__name__, str(e))
    del kept
    out[rank] = res, refused, _replays_after_x_changed(part, dev)
    dist.destroy_process_group()


def _replays_after_x_changed(part, dev):
    """24 input columns (> 16) into 8 features: layer 0's dW runs on the pair-sum table of the constant X
    (`functional._dw_pair_sums_table`), which a captured step reads at a fixed address.  Two warm-up steps and one more,
    then X doubled IN PLACE, then two steps — eagerly, and as replays of the step captured before the change."""
    import mrgcn_amd
    import mrgcn_amd.functional as Fn
    from mrgcn_amd.partition import GraphedPartitionedStep, PartitionedRGCN, partitioned_train_step
    from mrgcn_amd.train import ClipAdam
    Fn._DW_PAIR_SUMS_CAP = 1 << 30   # (this worker's own process; more pairs than nodes here: past the default cap)
    g, X, idx, y, mods = _problem(K=24)
    res = {}
    for graphed in (False, True):
        torch.manual_seed(5)
        model = PartitionedRGCN(mods, g.num_relations, g.num_nodes, 5, False, True, part).to(dev)
        model.build_plan(g.rows, g.cols, g.vals, dev)
        Xl = part.shard_rows(torch.from_numpy(X)).to(dev)
        opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0, capturable=graphed)
        opt.set_distributed(None, model.sharded_parameters())

        def count(key):
            return mrgcn_amd.stats().get(key, 0)
        if graphed:
            took = count("backward.dw_pair_sums")
            step = GraphedPartitionedStep(model, Xl, idx, y, opt, warmup=2)
            res["route_taken_in_warmup"] = count("backward.dw_pair_sums") - took
            res["tables_of_the_graph"] = len(step._captured.pair_sums[0])
        else:
            def step():
                return partitioned_train_step(model, Xl, idx, y, opt)
            step(), step()
        step()
        Xl.mul_(2.0)
        builds = count("dw_pair_sums.build")
        losses = [float(step()) for _ in range(2)]
        res[graphed] = (losses, model.layers["layer_0"].weight_F.detach().cpu().numpy(),
                        count("dw_pair_sums.build") - builds)
    return res


@pytest.mark.timeout(600)
def test_graphed_partitioned_step_over_rccl_with_one_rank():
    """GraphedPartitionedStep: the partitioned step with its RCCL collectives captured into a hipGraph and replayed
    gives the eager steps' losses and weights (one rank over the nccl backend: what this box can run); a replay
    refuses an optimizer state loaded after the capture, and sees an in-place change of a wide constant X."""
    state, _, _, _ = _single()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_graphed_worker, args=(1, _free_port(), state, out), nprocs=1, join=True)
    ((l_e, w_e), (l_g, w_g)), refused, changed = out[0]
    np.testing.assert_allclose(l_g, l_e, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(w_g, w_e, rtol=1e-3, atol=2e-5)
    # through the capture helper the step compares the optimizer's generation in front of a replay ...
    assert refused is not None and refused[0] == "MrgcnError", refused
    assert "GraphedPartitionedStep: the optimizer's state was loaded after the capture" in refused[1]
    # ... and re-checks the pair-sum table its layer-0 dW reads: the replay after X changed in place rebuilds it (once)
    # and steps as the eager step does — the loss AFTER that step and layer 0's weights carry the dW
    assert changed["route_taken_in_warmup"] >= 2 and changed["tables_of_the_graph"] == 1, changed
    (l_e, w_e, builds_e), (l_g, w_g, builds_g) = changed[False], changed[True]
    assert builds_g == 1 and builds_e == 1, (builds_g, builds_e)
    np.testing.assert_allclose(l_g, l_e, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(w_g, w_e, rtol=1e-3, atol=2e-5)


def _lp_problem():
    from mrgcn_amd import synth
    g = synth.make_graph("aifb", seed=4, scale=0.25, value_mode="ref_int8")
    rng = np.random.default_rng(4)
    N = g.num_nodes
    n = 900
    tr = np.stack([rng.integers(0, N, n), rng.integers(0, (g.num_relations - 1) // 2, n), rng.integers(0, N, n)], 1)
    y = (rng.random(n) < 0.8).astype(np.float32)
    mods = [(0, 12, "rgcn", torch.nn.ReLU())]
    return g, tr.astype(np.int64), y, mods


def _lp_worker(rank, world, port, state, out):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from mrgcn_amd.partition import NodePartition, PartitionedRGCN, partitioned_lp_step
    from mrgcn_amd.train import ClipAdam
    dist.init_process_group("gloo")
    dev = torch.device("cuda:0")
    g, tr, y, mods = _lp_problem()
    N, R = g.num_nodes, g.num_relations
    part = NodePartition(N, world, rank)
    model = PartitionedRGCN(mods, R, N, 2, True, False, part, link_prediction=True).to(dev)
    with torch.no_grad():
        model.load_full_state(state)
    model.build_plan(g.rows, g.cols, g.vals, dev)
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
    opt.set_distributed(None, model.sharded_parameters())
    t, yy = torch.from_numpy(tr).to(dev), torch.from_numpy(y).to(dev)
    losses = [float(partitioned_lp_step(model, None, t, yy, opt)) for _ in range(3)]
    out[rank] = (losses, model.relations.detach().cpu().numpy())
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_partitioned_link_prediction_equals_single_gpu():
    """BASELINE config 4's shape of computation over two ranks: partitioned featureless encoder,
    all-gathered embeddings, triples scored rank::world, decoder gradients reduce-scattered back."""
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    g, tr, y, mods = _lp_problem()
    N, R = g.num_nodes, g.num_relations
    torch.manual_seed(5)
    model = RGCN(mods, R, N, 2, 0.0, True, False, True)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.cuda()
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
    t, yy = torch.from_numpy(tr).cuda(), torch.from_numpy(y).cuda()
    losses = []
    for _ in range(3):
        sc = lp.score_distmult_bc((t[:, 0], t[:, 1], t[:, 2]), model(None, A), model.relations)
        loss = lp.binary_crossentropy(sc, yy)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_lp_worker, args=(2, _free_port(), state, out), nprocs=2, join=True)
    for r in (0, 1):
        np.testing.assert_allclose(out[r][0], losses, rtol=2e-4, atol=2e-5)
        d = np.abs(out[r][1] - model.relations.detach().cpu().numpy())
        assert (d > 2e-5).mean() < 5e-3 and d.max() <= 0.07


@pytest.mark.timeout(900)
def test_bench_runs_the_partitioned_engine_for_the_partitioned_workload():
    """`bench.py --gpus 2` on the workload BASELINE names as partitioned (config 5, here shrunk): launched exactly
    as the driver does (torch.distributed.run, one process per rank; two ranks on the one GPU of this box, so
    the collectives go over gloo), it must take the node-partitioned engine without being told to, say so in
    the line, and reach the loss of the single-process run of the same workload."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--workload", "synth10m", "--scale", "0.002", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline",
              "--no-literal-spmm", "--no-renumbered-extra", "--spmm-iters", "3"]
    env = dict(os.environ, MRGCN_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    multi = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                            os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                           capture_output=True, text=True, cwd=root, env=env, timeout=800)
    assert multi.returncode == 0, multi.stderr[-2000:]
    lines = [ln for ln in multi.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, multi.stdout[-2000:]          # rank 0 prints ONE line
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "strong"
    assert j["config"]["parallelism"] == "node-partitioned x2"
    assert j["roofline"]["frac"] > 0 and j["value"] > 0
    single = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--no-graph"] + common,
                            capture_output=True, text=True, cwd=root, timeout=800)
    assert single.returncode == 0, single.stderr[-2000:]
    j1 = json.loads([ln for ln in single.stdout.splitlines() if ln.startswith("{")][-1])
    assert j1["config"]["parallelism"] == "1 GPU" and j1["scaling"] == "weak"
    # different initial values (every rank draws its own shard), same problem: both sit at the untrained loss
    assert abs(j["extra"]["final_loss"] - j1["extra"]["final_loss"]) < 0.05 * abs(j1["extra"]["final_loss"])
    # an explicit --no-partition runs replicas
    rep = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                          os.path.join(root, "bench.py"), "--gpus", "2", "--no-partition"] + common,
                         capture_output=True, text=True, cwd=root, env=env, timeout=800)
    assert rep.returncode == 0, rep.stderr[-2000:]
    jr = json.loads([ln for ln in rep.stdout.splitlines() if ln.startswith("{")][-1])
    assert jr["config"]["parallelism"] == "replicas x2" and jr["scaling"] == "weak"


@pytest.mark.timeout(900)
def test_bench_link_prediction_workload_single_and_partitioned():
    """`bench.py --workload fb15k` (BASELINE config 4: R-GCN encoder + DistMult decoder, one step = one full-batch
    epoch of tasks/link_prediction.py:231-326 with device-drawn negatives, plus the ranking pass of :398-404): one
    process prints a line with the encoder product's roofline and the ranking figures; launched as the driver
    launches N > 1 it takes the node-partitioned encoder (`partitioned_lp_step`: all-gathered embeddings, triples
    scored rank::world) unprompted — two ranks on this box's one GPU, collectives over gloo — and reaches the same
    loss as the single process (same seed: identical replicated parameters and negatives; the node table's shards
    are drawn per rank, so the trajectories are close, not equal)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--workload", "fb15k", "--scale", "0.1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline",
              "--spmm-iters", "3"]
    single = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + common,
                            capture_output=True, text=True, cwd=root, timeout=800)
    assert single.returncode == 0, single.stderr[-2000:]
    j1 = json.loads([ln for ln in single.stdout.splitlines() if ln.startswith("{")][-1])
    assert "link-prediction" in j1["metric"] and j1["config"]["parallelism"] == "1 GPU"
    assert j1["roofline"]["frac"] > 0 and j1["value"] > 0 and j1["config"]["layers"] == [[0, 200]]
    assert j1["extra"]["rank_500_raw_ms"] > 0 and 0 < j1["extra"]["mrr_filtered"] <= 1
    env = dict(os.environ, MRGCN_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    multi = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                            os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                           capture_output=True, text=True, cwd=root, env=env, timeout=800)
    assert multi.returncode == 0, multi.stderr[-2000:]
    lines = [ln for ln in multi.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, multi.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["config"]["parallelism"] == "node-partitioned x2"
    assert abs(j["extra"]["final_loss"] - j1["extra"]["final_loss"]) < 0.05 * abs(j1["extra"]["final_loss"])


@pytest.mark.gpu
def test_bench_replicas_also_run_the_partitioned_engine_in_child_processes():
    """`bench.py --gpus 2` on the DEFAULT workload (replicas) as the driver launches it: after the replica timing every
    rank spawns a child that joins a process group of its own and runs the node-partitioned engine on the same graph
    (`extra.partitioned`).  The children must not inherit the elastic agent's rendezvous variables (they would wait for
    a store nobody hosts: the probe then only ever reported "timed out")."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MRGCN_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", MRGCN_BENCH_PROBE_TIMEOUT="200")
    multi = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                            os.path.join(root, "bench.py"), "--gpus", "2", "--scale", "0.02", "--steps", "2", "--warmup", "1",
                            "--full", "--no-cpu-baseline", "--spmm-iters", "3"],
                           capture_output=True, text=True, cwd=root, env=env, timeout=900)
    assert multi.returncode == 0, multi.stderr[-2000:]
    lines = [ln for ln in multi.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, multi.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["config"]["parallelism"].startswith("replicas")
    rec = j["extra"]["partitioned"]["am"]
    assert "error" not in rec, rec
    assert rec["rccl_world"] == 2 and rec["ms_per_step"] > 0 and rec["logits_maxdiff_vs_single"] < 1e-4
    # both engines of SURVEY §8e are priced, and the one with the smaller measured halo is named
    assert "halo_error" not in rec, rec.get("halo_error")
    assert rec["halo_ms_per_step"] > 0 and rec["halo_logits_maxdiff_vs_column_engine"] < 1e-4
    ch = rec["partition_choice"]
    assert ch["by_received_bytes_per_forward"] == ("halo" if ch["halo_bytes"] < ch["column_bytes"] else "column")


# ---- the row partition with operand-row halo exchange (mrgcn_amd.partition_halo) ------------------------------------
def _halo_worker(rank, world, port, state, out, lp_mode=False, backend="gloo", replicate_env=False):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if replicate_env:   # the library's default would replicate lukewarm operand rows: the halo plans must not
        os.environ["MRGCN_REPLICATE"] = "1"
    import torch.distributed as dist
    from mrgcn_amd.partition import NodePartition
    from mrgcn_amd.partition_halo import HaloPartitionedRGCN, halo_lp_step, halo_train_step
    from mrgcn_amd.train import ClipAdam
    dev = torch.device("cuda:0")
    if backend == "nccl":
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group("gloo")
    if lp_mode:
        g, facts, Y, mods = _lp_problem()
        N, R = g.num_nodes, g.num_relations
        part = NodePartition(N, world, rank)
        model = HaloPartitionedRGCN(mods, R, N, 2, True, False, part, link_prediction=True).to(dev)
        model.load_full_state(state)
        hp = model.build_plan(g.rows, g.cols, g.vals, dev)
        opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
        opt.set_distributed(None, model.sharded_parameters())
        tr, yy = torch.from_numpy(facts).to(dev), torch.from_numpy(Y).to(dev)
        emb0 = model(None).detach().cpu().numpy()[: part.n_local]
        losses = [float(halo_lp_step(model, None, tr, yy, opt))]
        # the second step with the exchange calls and the own product logged (the dense route: the product over this
        # rank's own columns is a Python call)
        from mrgcn_amd import _lib as L
        from mrgcn_amd import partition_halo as ph
        log = []
        real_start, real_wait, real_spmm = ph.start_rows_exchange, ph.wait_rows_exchange, hp.p_own.spmm

        def logged_start(*a):
            log.append("exchange started")
            return real_start(*a)

        def logged_wait(p):
            log.append("exchange awaited")
            return real_wait(p)

        def logged_spmm(view, *a, **k):
            log.append("own transposed product" if view == L.VIEW_TRANSPOSED else "own product")
            return real_spmm(view, *a, **k)
        ph.start_rows_exchange, ph.wait_rows_exchange, hp.p_own.spmm = logged_start, logged_wait, logged_spmm
        try:
            losses.append(float(halo_lp_step(model, None, tr, yy, opt)))
        finally:
            ph.start_rows_exchange, ph.wait_rows_exchange = real_start, real_wait
            del hp.p_own.spmm
        out[rank] = (emb0, losses, model.relations.detach().cpu().numpy(), hp.halo_columns, log)
        dist.destroy_process_group()
        return
    g, X, idx, y, mods = _problem()
    N, R = g.num_nodes, g.num_relations
    part = NodePartition(N, world, rank)
    model = HaloPartitionedRGCN(mods, R, N, 5, False, True, part).to(dev)
    model.load_full_state(state)
    hp = model.build_plan(g.rows, g.cols, g.vals, dev)
    Xl = part.shard_rows(torch.from_numpy(X)).to(dev)
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
    opt.set_distributed(None, model.sharded_parameters())
    import mrgcn_amd
    logits0 = model(Xl).detach().cpu().numpy()[: part.n_local]
    mrgcn_amd.reset_stats()
    losses = [float(halo_train_step(model, Xl, idx, y, opt)) for _ in range(2)]
    st = dict(mrgcn_amd.stats())
    wI = model.layers["layer_0"].weight_I.detach().cpu().permute(1, 0, 2)[:, : part.n_local]
    out[rank] = (logits0, losses, wI.numpy(), model.layers["layer_1"].weight_F.detach().cpu().numpy(), hp.halo_columns,
                 st, (hp.p_col.n_rep, hp.p_own.n_rep, hp.p_halo.n_rep))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 3])
def test_halo_engine_ranks_equal_single_gpu(world):
    """The row partition with operand-row halo exchange (SURVEY §8e's second form; north_star's wording) with 2 and 3
    ranks against the single-GPU RGCN: logits before training, the losses of two epochs, the sharded node table and a
    replicated parameter after them.  The exchange moved exactly the distinct remote columns the probe counts."""
    from mrgcn_amd.partition_halo import choose_partition
    state, logits0, losses, final = _single()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_halo_worker, args=(world, _free_port(), state, out), nprocs=world, join=True)
    ranks = range(world)
    np.testing.assert_allclose(np.concatenate([out[r][0] for r in ranks], 0), logits0, rtol=1e-4, atol=1e-4)
    for r in ranks:
        np.testing.assert_allclose(out[r][1], losses, rtol=2e-4, atol=2e-5)
    N = logits0.shape[0]
    wI = np.concatenate([out[r][2] for r in ranks], 1).reshape(5 * N, -1)
    d = np.abs(wI - final["layers.layer_0.weight_I"].numpy())
    assert (d > 2e-5).mean() < 5e-3 and d.max() <= 0.045
    for r in ranks:
        d = np.abs(out[r][3] - final["layers.layer_1.weight_F"].numpy())
        assert (d > 2e-5).mean() < 5e-3 and d.max() <= 0.045
    g = _problem()[0]
    ch = choose_partition(g.rows, g.cols, g.num_nodes, world, [8, 4])
    assert ch["halo_columns_per_rank"] == [out[r][4] for r in ranks]
    for r in ranks:   # both layers of both epochs ran their backward on gradient supports, on every rank — with the
        st = out[r][5]   # row-sparse weight_I gradient and the fused row Adam of the single-GPU path
        assert st.get("halo.backward.support") == 4 and "halo.backward.dense" not in st, (r, st)
        assert st.get("weight_I.fused_rows") == 2 or st.get("weight_I.rows") == 2, (r, st)


@pytest.mark.timeout(600)
def test_halo_engine_with_the_replicate_default_set_in_the_environment():
    """MRGCN_REPLICATE=1 makes plans replicate lukewarm operand rows by default; the halo plans fill their operands
    through index maps and are built without replicas whatever the default says (round-5 ADVICE): same results."""
    state, logits0, losses, final = _single()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_halo_worker, args=(2, _free_port(), state, out, False, "gloo", True), nprocs=2, join=True)
    np.testing.assert_allclose(np.concatenate([out[r][0] for r in range(2)], 0), logits0, rtol=1e-4, atol=1e-4)
    for r in range(2):
        np.testing.assert_allclose(out[r][1], losses, rtol=2e-4, atol=2e-5)
        assert out[r][6] == (0, 0, 0)


@pytest.mark.timeout(600)
def test_halo_engine_over_rccl_with_one_rank():
    """The halo engine's collectives as they run on a multi-GPU node — device tensors over the nccl (= RCCL) backend,
    the operand-row exchange started asynchronously and waited for after the local product — with the one rank this
    box has: the exchanges are empty, the model equals the single-GPU RGCN."""
    state, logits0, losses, final = _single()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_halo_worker, args=(1, _free_port(), state, out, False, "nccl"), nprocs=1, join=True)
    np.testing.assert_allclose(out[0][0], logits0, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(out[0][1], losses, rtol=2e-4, atol=2e-5)
    assert out[0][4] == 0


@pytest.mark.timeout(600)
def test_halo_engine_link_prediction_equals_single_gpu():
    """BASELINE config 4's computation on the halo engine with two ranks (a wide featureless encoder layer, F = 12;
    all-gathered embeddings, triples scored rank::world): the embeddings before training, the losses of two epochs and
    the decoder's relation table against the single-GPU model."""
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    g, tr, y, mods = _lp_problem()
    N, R = g.num_nodes, g.num_relations
    torch.manual_seed(5)
    model = RGCN(mods, R, N, 2, 0.0, True, False, True)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.cuda()
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
    t, yy = torch.from_numpy(tr).cuda(), torch.from_numpy(y).cuda()
    emb0 = model(None, A).detach().cpu().numpy()
    losses = []
    for _ in range(2):
        sc = lp.score_distmult_bc((t[:, 0], t[:, 1], t[:, 2]), model(None, A), model.relations)
        loss = lp.binary_crossentropy(sc, yy)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_halo_worker, args=(2, _free_port(), state, out, True), nprocs=2, join=True)
    np.testing.assert_allclose(np.concatenate([out[r][0] for r in (0, 1)], 0), emb0, rtol=1e-4, atol=1e-4)
    for r in (0, 1):
        np.testing.assert_allclose(out[r][1], losses, rtol=2e-4, atol=2e-5)
        d = np.abs(out[r][2] - model.relations.detach().cpu().numpy())
        assert (d > 2e-5).mean() < 5e-3 and d.max() <= 0.05
    # the ORDER of a step on every rank: each layer's forward sends its operand rows off before the product over its own
    # columns, and each layer's backward STARTS the reverse exchange of gradient rows, then runs the transposed product
    # over its own columns, and only then waits for the rows (over RCCL: in flight under that product).  The values — a
    # row's gradient comes back from the rank that read it — are what the comparisons above check.
    fwd = ["exchange started", "own product", "exchange awaited"]
    bwd = ["exchange started", "own transposed product", "exchange awaited"]
    for r in (0, 1):
        assert out[r][4] == fwd * len(mods) + bwd * len(mods), out[r][4]
