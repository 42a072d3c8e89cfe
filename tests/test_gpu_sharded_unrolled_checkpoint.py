"""GPU: activation checkpointing across steps over spatial shards, ``dist.sharded_unrolled_loss(checkpoint="steps")``,
against the plain path (``checkpoint="none"``) of the same call: the frames and the global loss bit for bit, every
parameter gradient within ``GTOL = 2e-5`` of the tensor's largest entry (the same kernels on the same inputs; autograd may
add a frame's or a parameter's contributions in another order).  Every distance is printed before it is asserted.

Several ranks are real processes over gloo on one GPU (tests/test_gpu_sharded_unrolled_training.py's harness); one pair of
workers runs every job, so the start-up is paid once.  A worker that fails ends its job list; nothing is tried again."""
import datetime
import os
import socket
import traceback

import pytest
import torch

import unroll_checks as uc
from cosmology_gnn_simulation_amd import dist as cdist, graph_network, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
GTOL = uc.GTOL
DT, BOX = 0.01, 1.0
LATENT, ROUNDS, NH = 32, 2, 2
WEIGHTS = (1.0, 1.0, 0.1)       # acc, temp_rate, momentum
MODES = {"x_j-fp32": ("x_j", "fp32", False), "x_j-fp32x3": ("x_j", "fp32x3", False), "edge-fp32": ("edge", "fp32", True)}


def _model(w, source, precision, device=DEV):
    m = graph_network.EncodeProcessDecode(LATENT, LATENT, NH, ROUNDS, 3)
    m.load_state_dict(synthetic.make_state_dict(LATENT, LATENT, NH, ROUNDS, 3, node_in=4 * w - 3))
    m = m.to(device).train()
    m.message_source, m.train_precision = source, precision
    m.train_edge_messages = source == "edge"
    return m


def _data(n, w, s, seed, squeeze=False):
    snap = synthetic.make_snapshot(n, window=w + s - 1, seed=seed)
    c, e = snap["Coordinates"].clone(), snap["InternalEnergy"]
    if squeeze:         # x <- 0.05 + 0.4 x: at world 2 the tile x >= box / 2 holds no particle
        c[..., 0] = 0.05 + 0.4 * c[..., 0]
    return c[:w], e[:w], c[w:w + s], e[w:w + s]


def _sharded(model, data, k, min_image, checkpoint, device=DEV):
    p, t, tp, tt = (v.to(device) for v in data)
    model.zero_grad(set_to_none=True)
    out = cdist.sharded_unrolled_loss(model, p, t, tp, tt, uc.META, dt=DT, box_size=BOX, num_neighbors=k,
                                      momentum_loss_weight=WEIGHTS[2], min_image_edge_attr=min_image, checkpoint=checkpoint)
    out.loss.backward()
    grads = {name: (None if q.grad is None else q.grad.detach().cpu().clone()) for name, q in model.named_parameters()}
    return out, grads


def _gradient_distance(what, got, want):
    """Largest ``rel_to_largest`` over the parameters; ``None`` gradients are ``None`` in both."""
    assert set(got) == set(want)
    worst = 0.0
    for name in want:
        if want[name] is None or got[name] is None:
            assert want[name] is None and got[name] is None, name
            continue
        worst = max(worst, uc.rel_to_largest(got[name], want[name]))
    print(f"{what}: largest gradient distance, of the tensor's largest entry = {worst:.3e}")
    return worst


# ---- no process group: a world of one ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
def test_no_process_group_checkpointed_is_the_plain_call(mode):
    source, precision, min_image = MODES[mode]
    n, k, w, s = 600, 8, 2, 3
    model = _model(w, source, precision)
    data = _data(n, w, s, 21)
    none, g_none = _sharded(model, data, k, min_image, "none")
    steps, g_steps = _sharded(model, data, k, min_image, "steps")
    assert steps.loss.grad_fn is not None and steps.graphs is None
    assert torch.equal(steps.frames["Coordinates"], none.frames["Coordinates"])
    assert torch.equal(steps.frames["InternalEnergy"], none.frames["InternalEnergy"])
    assert torch.equal(steps.value, none.value) and torch.equal(steps.step_losses, none.step_losses)
    assert torch.equal(steps.loss, none.loss)
    assert any(g is not None and float(g.abs().max()) > 0.0 for g in g_steps.values())
    for name in g_none:
        if ".edge_model." in name:
            assert (g_steps[name] is None) == (source == "x_j"), name
    assert _gradient_distance(f"world 1 {mode} W {w} S {s}", g_steps, g_none) <= GTOL


# ---- two processes over gloo, one GPU ------------------------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_job(job, rank, world, dev):
    """One job of a worker: the plain and the checkpointed call; what goes back through the queue is numpy or plain Python."""
    source, precision, min_image = MODES[job["mode"]]
    model = _model(job["w"], source, precision, dev)
    data = _data(job["n"], job["w"], job["s"], job["seed"], job.get("squeeze", False))
    res = {}
    for checkpoint in ("none", "steps"):
        out, grads = _sharded(model, data, job["k"], min_image, checkpoint, dev)
        res[checkpoint] = dict(frames={name: v.cpu().numpy() for name, v in out.frames.items()}, value=float(out.value),
                               step_losses=out.step_losses.cpu().numpy(),
                               grads={name: (None if g is None else g.numpy()) for name, g in grads.items()})
    return res


def _worker(rank, world, port, jobs, q):
    results = {}
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        # a rank that leaves the common order of collectives ends the peer's wait with an error, not with a hang
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))
        try:
            dev = torch.device("cuda", 0)
            torch.cuda.set_device(dev)
            for job in jobs:
                try:
                    results[job["name"]] = (None, _run_job(job, rank, world, dev))
                except Exception:
                    results[job["name"]] = (traceback.format_exc(), None)
                    break       # the ranks may be out of step from here on
        finally:
            dist.destroy_process_group()
        q.put((rank, None, results))
    except Exception:
        q.put((rank, traceback.format_exc(), results))


def _two_processes(jobs, timeout=420):
    import torch.multiprocessing as mp
    torch.cuda.synchronize()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, jobs, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=timeout) for _ in procs), key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    for rank, err, _ in res:
        assert err is None, f"rank {rank}:\n{err}"
    assert all(p.exitcode == 0 for p in procs)
    out = {}
    for job in jobs:
        per_rank = []
        for rank, _, results in res:
            assert job["name"] in results, f"rank {rank} did not reach job {job['name']}: {list(results)}"
            err, val = results[job["name"]]
            assert err is None, f"rank {rank}, job {job['name']}:\n{err}"
            per_rank.append(val)
        out[job["name"]] = per_rank
    return out


@pytest.fixture(scope="module")
def two_ranks():
    """Every job through one pair of workers."""
    jobs = [dict(name="edge", mode="edge-fp32", n=3000, k=8, w=3, s=3, seed=3),
            dict(name="x_j", mode="x_j-fp32x3", n=3000, k=8, w=3, s=3, seed=3),
            dict(name="empty-edge", mode="edge-fp32", n=600, k=8, w=3, s=3, seed=21, squeeze=True),
            dict(name="empty-x_j", mode="x_j-fp32", n=600, k=8, w=3, s=3, seed=21, squeeze=True)]
    return _two_processes(jobs)


def _grads(res):
    return {name: (None if g is None else torch.from_numpy(g)) for name, g in res["grads"].items()}


def _check_ranks(what, ranks):
    for rank, res in enumerate(ranks):
        none, steps = res["none"], res["steps"]
        for name in ("Coordinates", "InternalEnergy"):
            assert torch.equal(torch.from_numpy(steps["frames"][name]), torch.from_numpy(none["frames"][name])), (rank, name)
        assert steps["value"] == none["value"], rank
        assert torch.equal(torch.from_numpy(steps["step_losses"]), torch.from_numpy(none["step_losses"])), rank
        assert _gradient_distance(f"rank {rank} {what}", _grads(steps), _grads(none)) <= GTOL, rank
    assert ranks[0]["steps"]["value"] == ranks[1]["steps"]["value"]
    g0, g1 = _grads(ranks[0]["steps"]), _grads(ranks[1]["steps"])
    assert any(g is not None and float(g.abs().max()) > 0.0 for g in g0.values())
    for name in g0:         # the all-reduced gradients: the same bits on both ranks
        assert (g0[name] is None and g1[name] is None) or torch.equal(g0[name], g1[name]), name


@pytest.mark.parametrize("job", ["edge", "x_j"])
def test_two_processes_checkpointed_train_like_the_plain_call(two_ranks, job):
    _check_ranks(job, two_ranks[job])


@pytest.mark.parametrize("job", ["empty-edge", "empty-x_j"])
def test_a_rank_that_owns_nothing_takes_part_in_every_recomputed_collective(two_ranks, job):
    ranks = two_ranks[job]
    # rank 1's tile x >= box / 2 stays empty for all S steps
    frames = torch.from_numpy(ranks[0]["none"]["frames"]["Coordinates"])
    assert float(torch.remainder(frames, BOX)[..., 0].max()) < 0.5 * BOX
    _check_ranks(job, ranks)
