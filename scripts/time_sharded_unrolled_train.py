"""Developer tool: multi-step training over spatial shards (dist.sharded_unrolled_loss) on ONE GPU, for S in --steps:
  (a) a world of one against training.unrolled_loss on the same inputs, alternating in one process (median of --iters
      after warm-up, host clock around a synchronise), next to a separate timing of the per-step build_shard;
  (b) one rank's share of a --world-way split, every collective replaced by a stand-in that moves nothing (the halo as in
      scripts/time_sharded_train.py; the peers' requests taken as large as this rank's own; the all-gather's other rows
      taken from the unsharded run's frames; all-reduces the identity): step time and peak memory against (a)'s;
  (c) the HIP-event time of the three new kernels in (b)'s step (cgnn_edge_attr_backward_rows also on its own: x_j mode
      never launches it) and the bytes of the frame-gradient all-reduce.
``--checkpoint steps`` adds activation checkpointing across steps to (a) and (b): the world of one and the rank's share
run plain and checkpointed alternating in this process.  Not part of the product or tests.
    python scripts/time_sharded_unrolled_train.py [--particles 1000000] [--latent 128] [--mp-steps 10] [--steps 1 2 4]
                                                  [--world 8] [--rank 0] [--message-source x_j|edge]
                                                  [--checkpoint steps]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import _lib, dist as cdist, graph_network, ops, synthetic, training  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--particles", type=int, default=1_000_000)
ap.add_argument("--neighbors", type=int, default=16)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--mp-steps", type=int, default=10)
ap.add_argument("--window", type=int, default=5)
ap.add_argument("--steps", type=int, nargs="+", default=[1, 2, 4])
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--world", type=int, default=8)
ap.add_argument("--rank", type=int, default=0)
ap.add_argument("--train-precision", default="fp32x3", choices=["fp32", "fp32x3"])
ap.add_argument("--message-source", default="x_j", choices=["x_j", "edge"])
ap.add_argument("--noise-std", type=float, default=3e-4)
ap.add_argument("--checkpoint", default="none", choices=list(training.CHECKPOINTS))
a = ap.parse_args()
dev = torch.device("cuda")
n, k, d, L, w = a.particles, a.neighbors, a.latent, a.mp_steps, a.window
edge = a.message_source == "edge"
snap = synthetic.make_snapshot(n, window=w + max(a.steps) - 1, seed=1236)
meta = synthetic.make_metadata()
c, e = snap["Coordinates"].to(dev), snap["InternalEnergy"].to(dev)
m = graph_network.EncodeProcessDecode(d, d, 2, L, 3)
m.load_state_dict(synthetic.make_state_dict(d, d, 2, L, 3, node_in=4 * w - 3))
m = m.to(dev).train()
m.train_precision, m.message_source, m.train_edge_messages = a.train_precision, a.message_source, edge
opt = torch.optim.Adam(m.parameters(), lr=0.0)         # the step's cost without moving the weights between the variants
kw = dict(dt=0.01, box_size=1.0, num_neighbors=k, noise_std=a.noise_std, noise_seed=1236, momentum_loss_weight=0.1,
          min_image_edge_attr=edge)
last = {}


def step(fn, s, checkpoint="none"):
    out = fn(m, c[:w], e[:w], c[w:w + s], e[w:w + s], meta, checkpoint=checkpoint, **kw)
    opt.zero_grad()
    out.loss.backward()
    opt.step()
    last["frames"] = out.frames


def median_ms(fns, iters):
    """The variants alternate; -> per variant (median ms, peak GiB of its own calls)."""
    for fn in fns:
        fn()
    times, peaks = [[] for _ in fns], [0.0 for _ in fns]
    for _ in range(iters):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[j].append((time.perf_counter() - t0) * 1e3)
            peaks[j] = max(peaks[j], torch.cuda.max_memory_allocated() / 2 ** 30)
    return [(sorted(t)[len(t) // 2], p) for t, p in zip(times, peaks)]


# ---- stand-ins for (b): one rank of a --world-way split, nothing moves ----------------------------------------------------

class NoExchange:
    def __init__(self, sh, group=None):
        self.sh = sh

    def start(self, table):
        return None

    def finish(self, handle):
        return None

    def start_return(self, grad_ghost):
        return grad_ghost.new_zeros((sum(self.sh.send_counts), grad_ghost.shape[1]))

    def finish_return(self, handle):
        return handle


def fake_requests(sh, group=None, finish=None):
    """Every peer asks this rank for as many (boundary) rows as this rank asks of it."""
    b = sh.owned_global[sh.n_interior:]
    reqs = [b[:min(cnt, b.numel())] if p != sh.rank else b[:0] for p, cnt in enumerate(sh.recv_counts)]
    return cdist.finish_shard(sh, reqs)


def fake_gather(block, group=None):
    """This rank's block, behind the rows of every particle from the unsharded run's frame of this step (the same bits)."""
    s = fake_gather.step
    fake_gather.step += 1
    ref = torch.empty((n, _lib.ROLLOUT_ROW), dtype=torch.float32, device=dev)
    ref[:, :3] = reference["Coordinates"][s]
    ref[:, 3] = reference["InternalEnergy"][s].reshape(n)
    ref.view(torch.int32)[:, 4] = torch.arange(n, dtype=torch.int32, device=dev)
    return torch.cat([ref, block])


real = {name: getattr(cdist, name) for name in ("_world_of", "_group_up", "exchange_requests", "HaloExchange",
                                                 "all_gather_rows", "_all_reduce_", "_all_reduce_max_", "check_same_data")}
fakes = dict(_world_of=lambda group=None: (a.world, a.rank), _group_up=lambda: True, exchange_requests=fake_requests,
             HaloExchange=NoExchange, all_gather_rows=fake_gather, _all_reduce_=lambda t, group=None: t,
             _all_reduce_max_=lambda t, group=None: t, check_same_data=lambda *args, **kwargs: None)


def rank_step(s, checkpoint="none"):
    for name, fn in fakes.items():
        setattr(cdist, name, fn)
    fake_gather.step = 0
    try:
        step(cdist.sharded_unrolled_loss, s, checkpoint)
    finally:
        for name, fn in real.items():
            setattr(cdist, name, fn)


print(f"{a.message_source}, {a.train_precision}, {n} particles, k={k}, latent {d}, {L} rounds, W={w}", flush=True)
recent = torch.remainder(c[w - 1], 1.0).contiguous()
for world, rank in ((1, 0), (a.world, a.rank)):
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sh = cdist.build_shard(recent, 1.0, k, world, rank, min_image_edge_attr=edge, row_order="spatial")
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    print(f"build_shard(row_order='spatial'), rank {rank} of {world}: {sorted(ts)[1]:.1f} ms ({sh.n_owned} owned, "
          f"{sh.n_ghost} ghosts; the search itself {sh.knn_ms:.1f} ms)", flush=True)
for s in a.steps:
    (one_ms, one_gib), (w1_ms, w1_gib) = median_ms([lambda: step(training.unrolled_loss, s),
                                                    lambda: step(cdist.sharded_unrolled_loss, s)], a.iters)
    print(f"S={s} (a) training.unrolled_loss {one_ms:.1f} ms, peak {one_gib:.2f} GiB; world of one "
          f"{w1_ms:.1f} ms, peak {w1_gib:.2f} GiB: + {w1_ms - one_ms:.1f} ms ({(w1_ms - one_ms) / s:.1f} ms per step)",
          flush=True)
    if a.checkpoint != "none":
        (p_ms, p_gib), (c_ms, c_gib) = median_ms([lambda: step(cdist.sharded_unrolled_loss, s),
                                                  lambda: step(cdist.sharded_unrolled_loss, s, a.checkpoint)], a.iters)
        print(f"S={s} (a) world of one, checkpoint={a.checkpoint}: {c_ms:.1f} ms, peak {c_gib:.2f} GiB against plain "
              f"{p_ms:.1f} ms, peak {p_gib:.2f} GiB", flush=True)
    step(training.unrolled_loss, s)
    reference = {name: v.clone() for name, v in last["frames"].items()}
    torch.cuda.empty_cache()
    (r_ms, r_gib), = median_ms([lambda: rank_step(s)], a.iters)
    est = cdist.sharded_unrolled_training_bytes(sh.n_owned, sh.n_ghost, n, k, w, d, d, 2, L, s, edge) / 2 ** 30
    print(f"S={s} (b) rank {a.rank} of {a.world}, no exchange: {r_ms:.1f} ms ({one_ms / r_ms:.2f} x below the unsharded "
          f"step), peak {r_gib:.2f} GiB against {one_gib:.2f} GiB (the windows, targets and reference frames of all "
          f"particles included; estimate of the rank's need {est:.2f} GiB)", flush=True)
    if a.checkpoint != "none":
        (p_ms, p_gib), (c_ms, c_gib) = median_ms([lambda: rank_step(s), lambda: rank_step(s, a.checkpoint)], a.iters)
        est = cdist.sharded_unrolled_training_bytes(sh.n_owned, sh.n_ghost, n, k, w, d, d, 2, L, s, edge,
                                                    a.checkpoint) / 2 ** 30
        print(f"S={s} (b) rank {a.rank} of {a.world}, checkpoint={a.checkpoint}: {c_ms:.1f} ms, peak {c_gib:.2f} GiB "
              f"against plain {p_ms:.1f} ms, peak {p_gib:.2f} GiB (estimate of the rank's need {est:.2f} GiB)", flush=True)
    with ops.OpTimer() as tm:
        rank_step(s)
    summary = tm.summary()
    total = sum(v[1] for v in summary.values())
    new = {name: summary.get(name, (0, 0.0)) for name in ("rows_to_frames", "frame_grad_rows", "edge_attr_backward_rows")}
    print(f"S={s} (c) " + ", ".join(f"{name} {calls} calls {ms:.3f} ms" for name, (calls, ms) in new.items())
          + f" of {total:.1f} ms in timed ops; frame-gradient all-reduce: {s - 1} x {16 * n / 1e6:.1f} MB", flush=True)
# cgnn_edge_attr_backward_rows on the rank's shard of the first frame
sh = cdist.build_shard(recent, 1.0, k, a.world, a.rank, min_image_edge_attr=True, row_order="spatial")
csr = ops.SenderCsr(sh.src_local, None, sh.n_local)
d_ea = torch.randn_like(sh.edge_attr)
ms = []
for _ in range(7):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ops.edge_attr_backward_rows(d_ea, sh.edge_attr, sh.src_local, k, sh.n_owned, csr)
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
print(f"(c) cgnn_edge_attr_backward_rows alone, {sh.n_owned} receivers x {k}, {sh.n_local} position rows: "
      f"{sorted(ms)[3]:.3f} ms")
