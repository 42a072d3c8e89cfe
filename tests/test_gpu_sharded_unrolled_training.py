"""GPU: multi-step training over spatial shards (``dist.sharded_unrolled_loss``) and its three kernels
(cgnn_edge_attr_backward_rows, cgnn_rows_to_frames, cgnn_frame_grad_rows) against the one-GPU ``training.unrolled_loss``
and torch autograd of the plain-torch restatement in tests/unroll_checks.py, run in float64 on the CPU.

Bounds, all those of tests/test_gpu_unrolled_training.py and tests/test_gpu_sharded_training.py.  A link kernel's output is a
sum of float32 terms in a fixed order: ``GTOL = 2e-5`` of the tensor's largest entry; the two row <-> frame kernels are
copies (``torch.equal``).  End to end the predicted frames are those of the one-GPU call bit for bit (a rank's predictions
are the unsharded ones' bits), the global loss and each step's total lie within 1e-5 relative of the one-GPU ones, and
every parameter gradient within ``max(GTOL, 3 e_ref)`` of the float64 restatement on the one-GPU run's graphs, ``e_ref``
being the distance of the float32 restatement to the float64 one.  Every figure is printed before it is asserted.  The three
kernels are also gated exactly (ghost rows on both sides of a block edge, invalid ids, order and guard probes) in
tests/test_gpu_unroll_link_gates.py.

Several ranks are real processes over gloo on one GPU (tests/test_gpu_sharded_training_edge.py's pattern); one pair of
workers runs a list of jobs, so the start-up is paid once."""
import datetime
import functools
import os
import socket
import traceback

import pytest
import torch

import unroll_checks as uc
from cosmology_gnn_simulation_amd import dist as cdist, graph_network, ops, synthetic, training
from cosmology_gnn_simulation_amd._lib import CgnnError

pytestmark = pytest.mark.gpu
DEV = "cuda"
GTOL = uc.GTOL
DT, BOX = 0.01, 1.0
LATENT, ROUNDS, NH = 32, 2, 2
WEIGHTS = (1.0, 1.0, 0.1)       # acc, temp_rate, momentum
MODES = {"x_j-fp32": ("x_j", "fp32", False), "x_j-fp32x3": ("x_j", "fp32x3", False), "edge-fp32": ("edge", "fp32", True)}


def _err(got, want, what):
    e = uc.rel_to_largest(got, want)
    print(f"{what}: max |got - want| / max |want| = {e:.3e}")
    return e


# ---- 1. cgnn_edge_attr_backward_rows ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _positions(n=3000, seed=11):
    pos = torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * BOX
    for axis in range(3):       # a particle within 1e-3 of each face
        pos[2 * axis, axis] = 5e-4
        pos[2 * axis + 1, axis] = BOX - 5e-4
    return pos


@functools.lru_cache(maxsize=None)
def _shards(k, min_image, world=4):
    pos = _positions().to(DEV)
    return [cdist.build_shard(pos, BOX, k, world, r, min_image_edge_attr=min_image, row_order="spatial")
            for r in range(world)]


def _autograd_rows(sh, n_recv, d_ea, min_image):
    """float64 torch autograd of the edge features of the first ``n_recv`` receivers of a shard with respect to its local
    position rows [owned | ghosts]."""
    k = sh.k
    l2g = torch.cat([sh.owned_global, sh.ghost_global]).cpu()
    local = _positions()[l2g]
    ne = n_recv * k
    ei = torch.stack([sh.src_local[:ne].long().cpu(), sh.dst_local[:ne].long().cpu()])
    ea = sh.edge_attr[:ne].cpu()
    shift = uc.image_shifts(ea, local, ei, BOX) if min_image else None
    p64 = local.double().requires_grad_(True)
    ref = uc.edge_features(p64, ei, shift)
    if ne and float(ref.abs().max()) > 0.0:
        assert uc.rel_to_largest(ea, ref) <= 1e-6          # the shard's features are the restatement's
    want, = torch.autograd.grad(ref, p64, d_ea[:ne].double().cpu(), allow_unused=True)
    return torch.zeros_like(p64) if want is None else want


@pytest.mark.parametrize("min_image", [False, True])
@pytest.mark.parametrize("k", [1, 4, 16])
def test_edge_attr_backward_rows_matches_autograd_on_shards(k, min_image):
    shards = _shards(k, min_image)
    n = _positions().shape[0]
    assert sum(sh.n_owned for sh in shards) == n
    sh = shards[1]
    assert sh.n_owned > 257
    if k > 1:
        assert sh.n_ghost > 0           # k = 1: every particle's only neighbour is itself
    gen = torch.Generator().manual_seed(100 + k)
    d_global = torch.randn(n * k, 4, generator=gen).to(DEV)
    edge_ids = lambda s: (s.owned_global.view(-1, 1) * k + torch.arange(k, device=DEV)).reshape(-1)  # noqa: E731
    d_ea = d_global[edge_ids(sh)].contiguous()
    for n_recv in (1, 257, sh.n_owned):
        ne = n_recv * k
        src = sh.src_local[:ne].contiguous()
        csr = ops.SenderCsr(src, None, sh.n_local)
        got = ops.edge_attr_backward_rows(d_ea[:ne], sh.edge_attr[:ne], src, k, n_recv, csr)
        assert tuple(got.shape) == (sh.n_local, 3) and bool(torch.isfinite(got).all())
        want = _autograd_rows(sh, n_recv, d_ea, min_image)
        if float(want.abs().max()) == 0.0:      # self edges only (length 0): a finite, zero contribution
            assert k == 1 and float(got.abs().max()) == 0.0
        else:
            assert _err(got, want, f"k {k} min_image {min_image} n_recv {n_recv}") <= GTOL
            # rows past the receivers take only what they send
            assert _err(got[n_recv:], want[n_recv:], "  rows past n_recv") <= GTOL
        again = ops.edge_attr_backward_rows(d_ea[:ne], sh.edge_attr[:ne], src, k, n_recv, ops.SenderCsr(src, None, sh.n_local))
        assert torch.equal(got, again)
    # n_pos == n_recv: the one-graph entry, bit for bit
    pos = _positions().to(DEV)
    snd, ea, _ = ops.knn_periodic(pos, BOX, k, min_image_edge_attr=min_image)
    csr = ops.SenderCsr(snd, None, n)
    one_gpu = ops.edge_attr_backward(d_global, ea, snd, k, csr)
    assert torch.equal(ops.edge_attr_backward_rows(d_global, ea, snd, k, n, csr), one_gpu)
    # the ranks' results, scattered to global ids and summed, are the one-graph result
    total = torch.zeros(n, 3, dtype=torch.float64)
    for s in shards:
        part = ops.edge_attr_backward_rows(d_global[edge_ids(s)].contiguous(), s.edge_attr, s.src_local, k, s.n_owned,
                                           ops.SenderCsr(s.src_local, None, s.n_local))
        total.index_add_(0, torch.cat([s.owned_global, s.ghost_global]).cpu(), part.double().cpu())
    if float(one_gpu.abs().max()) == 0.0:
        assert float(total.abs().max()) == 0.0
    else:
        assert _err(total, one_gpu, f"k {k} min_image {min_image}: sum over the ranks against one graph") <= GTOL


# ---- 2. rows <-> frames ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frames", [1, 6])
@pytest.mark.parametrize("rows", [0, 1, 257])
def test_row_and_frame_kernels_are_index_copies(rows, frames):
    n = 1000
    gen = torch.Generator().manual_seed(rows + frames)
    ids = torch.randperm(n, generator=gen)[:rows]               # unordered, unique
    bad = ids.clone()
    if rows > 1:
        bad[rows // 2] = n + 5                                  # outside [0, N): skipped
        bad[0] = -1
    keep = (bad >= 0) & (bad < n)
    rp, rt = torch.randn(frames, rows, 3, generator=gen), torch.randn(frames, rows, generator=gen)
    want_p, want_t = torch.zeros(frames, n, 3), torch.zeros(frames, n)
    want_p[:, bad[keep]] = rp[:, keep]
    want_t[:, bad[keep]] = rt[:, keep]
    got_p, got_t = ops.rows_to_frames(bad.to(DEV), n, rp.to(DEV), rt.to(DEV))
    assert torch.equal(got_p.cpu(), want_p) and torch.equal(got_t.cpu(), want_t)
    only_p, none = ops.rows_to_frames(bad.to(DEV), n, rp.to(DEV), None)
    assert none is None and torch.equal(only_p, got_p)
    none, only_t = ops.rows_to_frames(bad.to(DEV), n, None, rt.to(DEV))
    assert none is None and torch.equal(only_t, got_t)
    if frames == 1:         # a single frame may come without the frame axis
        one_p, one_t = ops.rows_to_frames(bad.to(DEV), n, rp[0].to(DEV), rt[0].to(DEV))
        assert torch.equal(one_p, got_p) and torch.equal(one_t, got_t)
        # the transpose of cgnn_frame_unpack: the whole-frame gradient read at the rows
        grad = torch.randn(n, 4, generator=gen)
        d_pos, d_temp = ops.frame_grad_rows(grad.to(DEV), bad.to(DEV))
        want = torch.zeros(rows, 4)
        want[keep] = grad[bad[keep]]
        assert tuple(d_pos.shape) == (rows, 3) and tuple(d_temp.shape) == (rows,)
        assert torch.equal(d_pos.cpu(), want[:, :3]) and torch.equal(d_temp.cpu(), want[:, 3])


# ---- end to end: shared inputs and references -------------------------------------------------------------------------------

def _model(w, source, precision, device=DEV):
    m = graph_network.EncodeProcessDecode(LATENT, LATENT, NH, ROUNDS, 3)
    sd = synthetic.make_state_dict(LATENT, LATENT, NH, ROUNDS, 3, node_in=4 * w - 3)
    m.load_state_dict(sd)
    m = m.to(device).train()
    m.message_source, m.train_precision = source, precision
    m.train_edge_messages = source == "edge"
    return m, sd


def _data(n, w, s, seed, squeeze=False):
    snap = synthetic.make_snapshot(n, window=w + s - 1, seed=seed)
    c, e = snap["Coordinates"].clone(), snap["InternalEnergy"]
    if squeeze:         # x <- 0.05 + 0.4 x: at world 2 the tile x >= box / 2 holds no particle
        c[..., 0] = 0.05 + 0.4 * c[..., 0]
    return c[:w], e[:w], c[w:w + s], e[w:w + s]


def _grads_of(model):
    return {name: (None if q.grad is None else q.grad.detach().cpu().clone()) for name, q in model.named_parameters()}


def _restate(sd, source, data, graphs, min_image, dtype, k):
    p, t, tp, tt = data
    sdr = uc.state_dict_of(sd, dtype)
    eis = [g.edge_index.cpu() for g in graphs]
    shifts = [uc.image_shifts(g.edge_attr.detach().cpu(), g.pos.cpu(), ei, BOX) for g, ei in zip(graphs, eis)] \
        if min_image else None
    out = uc.unrolled(sdr, NH, ROUNDS, source, p, t, tp, tt, uc.META, DT, BOX, eis, shifts=shifts, weights=WEIGHTS, dtype=dtype)
    out["loss"].backward()
    return {name: q.grad for name, q in sdr.items()}


@functools.lru_cache(maxsize=None)
def _reference(mode, n, k, w, s, seed, squeeze=False):
    """The one-GPU run of a case and the float64 / float32 restatements on its graphs, once per case: dict(frames, loss,
    step_totals, grads (HIP, one GPU), ref (float64), e_ref per parameter, owners per step, ghosts per step and rank)."""
    source, precision, min_image = MODES[mode]
    model, sd = _model(w, source, precision)
    data = _data(n, w, s, seed, squeeze)
    p, t, tp, tt = (v.to(DEV) for v in data)
    out = training.unrolled_loss(model, p, t, tp, tt, uc.META, dt=DT, box_size=BOX, num_neighbors=k,
                                 momentum_loss_weight=WEIGHTS[2], min_image_edge_attr=min_image, keep_graphs=True)
    out.loss.backward()
    assert all(uc.valid_knn_lists(g.edge_index, n, k) for g in out.graphs)
    ref = _restate(sd, source, data, out.graphs, min_image, torch.float64, k)
    e_ref = dict.fromkeys(ref, 0.0)
    if s > 1:
        f32 = _restate(sd, source, data, out.graphs, min_image, torch.float32, k)
        e_ref = {name: (0.0 if ref[name] is None else uc.rel_to_largest(f32[name], ref[name])) for name in ref}
    sl = out.step_losses.double().cpu()
    # who owns what at world 2, read off the one-GPU run's frames (not off the code under test)
    recents = [g.pos.cpu() for g in out.graphs]
    owners = [cdist.owner_of(r, BOX, 2) for r in recents]
    ghosts = []
    for g, own in zip(out.graphs, owners):
        ei = g.edge_index.cpu()
        cross = own[ei[0]] != own[ei[1]]
        ghosts.append([int(torch.unique(ei[0][cross & (own[ei[1]] == r)]).numel()) for r in range(2)])
    return dict(frames={name: v.cpu() for name, v in out.frames.items()}, loss=float(out.loss),
                step_totals=(WEIGHTS[0] * sl[:, 0] + WEIGHTS[1] * sl[:, 1] + sl[:, 2]).tolist(), grads=_grads_of(model),
                ref=ref, e_ref=e_ref, owners=owners, ghosts=ghosts, sd=sd, data=data)


def _sharded(model, data, k, min_image, group=None, **kw):
    p, t, tp, tt = (v.to(DEV) for v in data)
    model.zero_grad(set_to_none=True)
    out = cdist.sharded_unrolled_loss(model, p, t, tp, tt, uc.META, dt=DT, box_size=BOX, num_neighbors=k,
                                      momentum_loss_weight=WEIGHTS[2], min_image_edge_attr=min_image, group=group, **kw)
    out.loss.backward()
    return out, _grads_of(model)


def _check_against_one_gpu(what, want, frames, value, step_losses, grads, source):
    """The checks of cases 3, 4, 6 and 7 on one rank's result (CPU tensors / floats).  -> the names outside the gate."""
    assert torch.equal(frames["Coordinates"], want["frames"]["Coordinates"]), what
    assert torch.equal(frames["InternalEnergy"], want["frames"]["InternalEnergy"]), what
    rel = abs(value - want["loss"]) / abs(want["loss"])
    print(f"{what} value: {value:.9e} against one GPU {want['loss']:.9e}, relative {rel:.2e}")
    assert rel <= 1e-5, what
    sl = torch.as_tensor(step_losses).double()
    totals = (WEIGHTS[0] * sl[:, 0] + WEIGHTS[1] * sl[:, 1] + sl[:, 2]).tolist()
    for s, (got, ref) in enumerate(zip(totals, want["step_totals"])):
        print(f"{what} step {s} total: {got:.9e} against one GPU {ref:.9e}")
        assert abs(got - ref) <= 1e-5 * abs(ref), (what, s)
    assert set(grads) == set(want["ref"])
    failures, worst_hip = [], 0.0
    for name, ref in want["ref"].items():
        if ".edge_model." in name and source == "x_j":
            assert grads[name] is None and ref is None, name
            continue
        assert grads[name] is not None and float(grads[name].abs().max()) > 0.0, name
        err, bound = uc.rel_to_largest(grads[name], ref), max(GTOL, 3 * want["e_ref"][name])
        hip = uc.rel_to_largest(grads[name], want["grads"][name])
        worst_hip = max(worst_hip, hip)
        print(f"{what} grad {name}: error {err:.3e}, e_ref {want['e_ref'][name]:.3e}, bound {bound:.3e}; "
              f"to the one-GPU HIP gradient {hip:.3e}")
        if err > bound:
            failures.append((name, err, bound))
    print(f"{what} SUMMARY: largest distance to the one-GPU HIP gradients {worst_hip:.3e}; outside the gate: {failures}")
    return failures


def test_no_process_group_is_a_world_of_one_with_noise_and_cut_links():
    """Without a process group the call runs as a world of one (no collective); with noise, ``step_weights`` and
    ``backprop_steps`` it gives the one-GPU call's frames and, within the link bound, its gradients."""
    n, k, w, s = 600, 8, 4, 3
    model, _ = _model(w, "x_j", "fp32")
    data = _data(n, w, s, 21)
    kw = dict(noise_std=3e-4, noise_seed=77, noise_draw=3, backprop_steps=1, step_weights=[0.2, 0.3, 0.5])
    p, t, tp, tt = (v.to(DEV) for v in data)
    one = training.unrolled_loss(model, p, t, tp, tt, uc.META, dt=DT, box_size=BOX, num_neighbors=k,
                                 momentum_loss_weight=WEIGHTS[2], **kw)
    one.loss.backward()
    want = _grads_of(model)
    out, grads = _sharded(model, data, k, False, **kw)
    assert torch.equal(out.frames["Coordinates"], one.frames["Coordinates"])
    assert torch.equal(out.frames["InternalEnergy"], one.frames["InternalEnergy"])
    assert abs(float(out.value) - float(one.loss)) <= 1e-5 * abs(float(one.loss))
    for name, g in want.items():
        if g is not None:
            assert _err(grads[name], g, name) <= GTOL, name


# ---- 3. RCCL, a world of one ------------------------------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def nccl_world_of_one():
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a process group is already up in this process")
    dev = torch.device("cuda", torch.cuda.current_device())
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=dev)
    try:
        yield dev
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


@pytest.mark.parametrize("w,s", [(3, 1), (6, 2), (2, 3)])
@pytest.mark.parametrize("mode", list(MODES))
def test_world_of_one_over_rccl_is_the_one_gpu_call(nccl_world_of_one, mode, w, s):
    source, precision, min_image = MODES[mode]
    n, k = 600, 8
    want = _reference(mode, n, k, w, s, 21)
    model, _ = _model(w, source, precision)
    out, grads = _sharded(model, want["data"], k, min_image)
    assert out.loss.dtype == torch.float32 and out.loss.dim() == 0 and out.loss.grad_fn is not None
    assert out.value.dtype == torch.float64 and out.value.dim() == 0 and not out.value.requires_grad
    assert out.step_losses.shape == (s, 3) and not out.step_losses.requires_grad and out.graphs is None
    assert out.frames["Coordinates"].shape == (s, n, 3) and out.frames["InternalEnergy"].shape == (s, n, 1)
    frames = {name: v.cpu() for name, v in out.frames.items()}
    what = f"world 1 {mode} W {w} S {s}"
    assert _check_against_one_gpu(what, want, frames, float(out.value), out.step_losses.cpu(), grads, source) == []
    again, grads2 = _sharded(model, want["data"], k, min_image)
    assert torch.equal(out.loss, again.loss) and torch.equal(out.value, again.value)
    assert torch.equal(out.step_losses, again.step_losses)
    for name in grads:
        assert (grads[name] is None and grads2[name] is None) or torch.equal(grads[name], grads2[name]), name


# ---- 4 - 8. two processes over gloo, one GPU --------------------------------------------------------------------------------

N2, K2, W2, S2, SEED2 = 3000, 8, 3, 3, 3


def _run_job(job, rank, world, dev):
    """One job of a worker; everything that goes back through the queue is numpy or plain Python."""
    kind = job["kind"]
    if kind == "publish":
        n, cap = job["n"], job["cap"]
        gen = torch.Generator().manual_seed(5)
        ids = torch.randperm(n, generator=gen)
        ids = ids[ids % world == rank].to(dev)                 # unordered: this rank integrated these
        base_p, base_t = torch.randn(n, 3, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev)
        g_p, g_t = torch.randn(n, 3, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev)
        rows_p = base_p[ids].clone().requires_grad_(True)
        rows_t = base_t[ids].clone().requires_grad_(True)
        pos, temp = cdist.publish_frame(rows_p, rows_t, ids, n, cap)
        assert torch.equal(pos, base_p) and torch.equal(temp, base_t)
        # a full-frame gradient that depends on the rank
        torch.autograd.backward([pos, temp], [g_p * float(rank + 1), g_t * float(rank + 1)])
        return dict(ids=ids.cpu().numpy(), d_pos=rows_p.grad.cpu().numpy(), d_temp=rows_t.grad.cpu().numpy())
    source, precision, min_image = MODES[job["mode"]]
    model, _ = _model(job["w"], source, precision, dev)
    data = _data(job["n"], job["w"], job["s"], job["seed"], job.get("squeeze", False))
    kw = dict(decomposition=job.get("decomposition", "uniform"), knn_grid=job.get("knn_grid", "uniform"))
    if kind == "guard":
        launched = []
        saved = (ops.training_sample, ops.mlp_rows, torch.cuda.mem_get_info, torch.cuda.memory_reserved)

        def sample_spy(*a, **k):            # after the guard the first launch is the sample of the owned rows
            if (a[10] if len(a) > 10 else k.get("rows")) is not None:
                launched.append("training_sample(rows)")
            return saved[0](*a, **k)

        def mlp_spy(*a, **k):
            launched.append("mlp_rows")
            return saved[1](*a, **k)
        ops.training_sample, ops.mlp_rows = sample_spy, mlp_spy
        if rank == job["short_rank"]:       # below this rank's estimate: not even the replicated frames fit
            torch.cuda.mem_get_info = lambda *a, **k: (0, saved[2](*a, **k)[1])
            torch.cuda.memory_reserved = torch.cuda.memory_allocated      # reserved - allocated = 0
        try:
            _sharded(model, data, job["k"], min_image, **kw)
            raised = None
        except CgnnError as exc:
            raised = str(exc)
        finally:
            ops.training_sample, ops.mlp_rows, torch.cuda.mem_get_info, torch.cuda.memory_reserved = saved
        return dict(raised=raised, launched=launched)
    if job.get("no_reduce"):        # the frame-gradient reduction replaced by the identity: the gate must bite
        real = cdist.reduce_frame_gradient
        cdist.reduce_frame_gradient = lambda grad, group=None: grad
    try:
        out, grads = _sharded(model, data, job["k"], min_image, **kw)
    finally:
        if job.get("no_reduce"):
            cdist.reduce_frame_gradient = real
    res = dict(frames={name: v.cpu().numpy() for name, v in out.frames.items()}, value=float(out.value),
               loss_part=float(out.loss), step_losses=out.step_losses.cpu().numpy(),
               grads={name: (None if g is None else g.numpy()) for name, g in grads.items()})
    if job.get("twice"):
        again, grads2 = _sharded(model, data, job["k"], min_image, **kw)
        res["same_bits"] = bool(torch.equal(out.loss, again.loss) and torch.equal(out.value, again.value) and all(
            (grads[name] is None and grads2[name] is None) or torch.equal(grads[name], grads2[name]) for name in grads))
    if job.get("adam"):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        opt.step()
        res["params"] = {name: q.detach().cpu().numpy() for name, q in model.named_parameters()}
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


def _case(name, mode, **kw):
    return dict(dict(kind="loss", name=name, mode=mode, n=N2, k=K2, w=W2, s=S2, seed=SEED2), **kw)


@pytest.fixture(scope="module")
def two_ranks():
    """Every job of cases 4, 5, 7 and 8 through one pair of workers."""
    jobs = [_case("edge", "edge-fp32", twice=True, adam=True), _case("edge-no-reduce", "edge-fp32", no_reduce=True),
            _case("x_j", "x_j-fp32x3", adam=True), dict(kind="publish", name="publish", n=1001, cap=600),
            _case("balanced", "edge-fp32", decomposition="balanced"), _case("adaptive", "edge-fp32", knn_grid="adaptive"),
            _case("guard", "edge-fp32", kind="guard", short_rank=1), _case("after-guard", "x_j-fp32x3")]
    return _two_processes(jobs)


def _preconditions(want, s):
    """Asserted on the one-GPU run's frames: both ranks have ghosts at every step, and at least one particle changes
    owner between consecutive steps."""
    assert len(want["ghosts"]) == s and all(min(g) > 0 for g in want["ghosts"]), want["ghosts"]
    moved = [int((a != b).sum()) for a, b in zip(want["owners"][:-1], want["owners"][1:])]
    print(f"ghost rows per step and rank {want['ghosts']}; particles that change owner between steps {moved}")
    assert len(moved) == s - 1 and min(moved) >= 1, moved


def _rank_result(res):
    frames = {name: torch.from_numpy(v) for name, v in res["frames"].items()}
    grads = {name: (None if g is None else torch.from_numpy(g)) for name, g in res["grads"].items()}
    return frames, grads


@pytest.mark.parametrize("job,mode", [("edge", "edge-fp32"), ("x_j", "x_j-fp32x3")])
def test_two_processes_train_like_one_gpu(two_ranks, job, mode):
    want = _reference(mode, N2, K2, W2, S2, SEED2)
    _preconditions(want, S2)
    ranks = two_ranks[job]
    for rank, res in enumerate(ranks):
        frames, grads = _rank_result(res)
        failures = _check_against_one_gpu(f"rank {rank} {mode}", want, frames, res["value"], res["step_losses"], grads,
                                          MODES[mode][0])
        assert failures == [], (rank, failures)
    (f0, g0), (f1, g1) = _rank_result(ranks[0]), _rank_result(ranks[1])
    assert ranks[0]["value"] == ranks[1]["value"]
    assert ranks[0]["loss_part"] != ranks[1]["loss_part"]      # each rank differentiates its own part
    for name in g0:         # the all-reduced gradients: the same bits on both ranks
        assert (g0[name] is None and g1[name] is None) or torch.equal(g0[name], g1[name]), name
    p0, p1 = ranks[0]["params"], ranks[1]["params"]
    assert set(p0) == set(p1) and all(torch.equal(torch.from_numpy(p0[n]), torch.from_numpy(p1[n])) for n in p0)
    if job == "edge":
        assert ranks[0]["same_bits"] and ranks[1]["same_bits"]


def test_the_gate_bites_without_the_frame_gradient_reduction(two_ranks):
    """The same call with ``dist.reduce_frame_gradient`` replaced by the identity: a rank then misses what the other
    rank's rows contribute to the gradient of a predicted frame (particles that changed tile, ghost senders' positions),
    and at least one parameter gradient leaves the gate the complete call passes."""
    want = _reference("edge-fp32", N2, K2, W2, S2, SEED2)
    for rank, res in enumerate(two_ranks["edge-no-reduce"]):
        frames, grads = _rank_result(res)
        assert torch.equal(frames["Coordinates"], want["frames"]["Coordinates"])        # the forward is untouched
        missed = []
        for name, ref in want["ref"].items():
            err, bound = uc.rel_to_largest(grads[name], ref), max(GTOL, 3 * want["e_ref"][name])
            print(f"rank {rank} without the reduction, {name}: error {err:.3e}, bound {bound:.3e}")
            if err > bound:
                missed.append(name)
        assert missed, rank


def test_publish_link_returns_the_sum_of_both_ranks_rows(two_ranks):
    n = 1001
    gen = torch.Generator().manual_seed(5)
    perm = torch.randperm(n, generator=gen)
    torch.randn(n, 3, generator=gen), torch.randn(n, generator=gen)          # the frame's values
    g_p, g_t = torch.randn(n, 3, generator=gen), torch.randn(n, generator=gen)
    want_p, want_t = g_p * 1.0 + g_p * 2.0, g_t * 1.0 + g_t * 2.0           # both ranks' full-frame gradients, summed
    for rank, res in enumerate(two_ranks["publish"]):
        ids = torch.from_numpy(res["ids"])
        assert torch.equal(ids, perm[perm % 2 == rank]) and ids.numel() > 0
        assert torch.equal(torch.from_numpy(res["d_pos"]), want_p[ids]), rank
        assert torch.equal(torch.from_numpy(res["d_temp"]), want_t[ids]), rank


@pytest.mark.parametrize("job", ["balanced", "adaptive"])
def test_other_decomposition_and_grid_give_the_defaults_results(two_ranks, job):
    want = _reference("edge-fp32", N2, K2, W2, S2, SEED2)
    for rank, res in enumerate(two_ranks[job]):
        frames, grads = _rank_result(res)
        assert _check_against_one_gpu(f"rank {rank} {job}", want, frames, res["value"], res["step_losses"], grads,
                                      "edge") == [], rank


def test_memory_guard_is_agreed_by_all_ranks(two_ranks):
    """Free memory below ONE rank's estimate: both ranks raise together after the flag all-reduce and launch nothing
    more; the next call on the same process group runs."""
    for rank, res in enumerate(two_ranks["guard"]):
        assert res["raised"] is not None and "device memory" in res["raised"], (rank, res)
        assert res["launched"] == [], (rank, res["launched"])
    want = _reference("x_j-fp32x3", N2, K2, W2, S2, SEED2)
    for res in two_ranks["after-guard"]:
        assert torch.equal(torch.from_numpy(res["frames"]["Coordinates"]), want["frames"]["Coordinates"])


# ---- 6. a rank that owns nothing ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["edge-fp32", "x_j-fp32"])
def test_a_rank_that_owns_nothing_takes_part_in_every_collective(mode):
    n, k, w, s, seed = 600, 8, 3, 3, 21
    want = _reference(mode, n, k, w, s, seed, True)
    # rank 1's tile x >= box / 2 stays empty for all S steps, on the one-GPU frames
    assert all(int((own == 1).sum()) == 0 for own in want["owners"])
    assert float(torch.remainder(want["frames"]["Coordinates"], BOX)[..., 0].max()) < 0.5 * BOX
    res = _two_processes([dict(kind="loss", name="empty", mode=mode, n=n, k=k, w=w, s=s, seed=seed, squeeze=True,
                               adam=True)], timeout=240)["empty"]
    for rank, r in enumerate(res):
        frames, grads = _rank_result(r)
        assert _check_against_one_gpu(f"rank {rank} (rank 1 owns nothing) {mode}", want, frames, r["value"],
                                      r["step_losses"], grads, MODES[mode][0]) == [], rank
    # rank 1's part to differentiate is the replicated momentum term alone
    assert res[1]["loss_part"] == pytest.approx(float(res[1]["step_losses"][:, 2].mean()), rel=1e-5)
    (_, g0), (_, g1) = _rank_result(res[0]), _rank_result(res[1])
    for name in g0:
        assert (g0[name] is None and g1[name] is None) or torch.equal(g0[name], g1[name]), name
    p0, p1 = res[0]["params"], res[1]["params"]
    assert all(torch.equal(torch.from_numpy(p0[n_]), torch.from_numpy(p1[n_])) for n_ in p0)
