"""Developer tool: one rank's share of a sharded training step (dist.ShardedTraining) on ONE GPU, without the exchanges (a
halo stand-in that moves nothing in either direction), next to the unsharded training step of the same total size on the
same GPU.  Both are forward + backward through the HIP node-stream kernels (``--message-source edge``: both streams, with
``model.train_edge_messages``; where the unsharded edge step is refused for memory, its estimate is printed instead of a
time); HIP-event medians.  Not part of the product or tests.
    python scripts/time_sharded_train.py [--world 8] [--particles 1000000] [--scaling strong] [--train-precision fp32x3]
                                         [--message-source x_j|edge] [--decomposition uniform|balanced]
                                         [--clustered] [--no-unsharded]
--clustered: the snapshot is synthetic.make_clustered_snapshot's (half of the particles in one halo); --no-unsharded
leaves the unsharded step out (a clustered run over every rank needs it once at most)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import data_utils, dist as cdist, graph_network, losses, ops, synthetic  # noqa: E402
from cosmology_gnn_simulation_amd._lib import CgnnError  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--world", type=int, default=8)
ap.add_argument("--rank", type=int, default=0)
ap.add_argument("--particles", type=int, default=1_000_000)
ap.add_argument("--scaling", default="strong", choices=["weak", "strong"])
ap.add_argument("--neighbors", type=int, default=16)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--mp-steps", type=int, default=10)
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--train-precision", default="fp32x3", choices=["fp32", "fp32x3"])
ap.add_argument("--message-source", default="x_j", choices=["x_j", "edge"])
ap.add_argument("--decomposition", choices=cdist.DECOMPOSITIONS, default="uniform")
ap.add_argument("--clustered", action="store_true")
ap.add_argument("--no-unsharded", action="store_true")
a = ap.parse_args()
edge = a.message_source == "edge"
dev = torch.device("cuda")
n_total = a.particles * (a.world if a.scaling == "weak" else 1)
k, d, L = a.neighbors, a.latent, a.mp_steps
dt = 0.01


class NoExchange:
    """The interface ShardedTraining overlaps with; ghost rows keep whatever they hold, nothing is returned."""

    def __init__(self, sh):
        self.sh = sh

    def start(self, table):
        return None

    def finish(self, handle):
        return None

    def start_return(self, grad_ghost):
        return grad_ghost.new_zeros((sum(self.sh.send_counts), grad_ghost.shape[1]))

    def finish_return(self, handle):
        return handle


snap = (synthetic.make_clustered_snapshot if a.clustered else synthetic.make_snapshot)(n_total, seed=1236)
meta = synthetic.make_metadata()
c, e = snap["Coordinates"], snap["InternalEnergy"]
g = data_utils.preprocess(c[:5], e[:5], meta, c[5], e[5], 0.0, k, dt, 1.0, device=dev)
m = graph_network.EncodeProcessDecode(d, d, 2, L, 3)
m.load_state_dict(synthetic.make_state_dict(d, d, 2, L, 3))
m = m.to(dev).train()
m.train_precision = a.train_precision
if edge:
    m.message_source = "edge"
    m.train_edge_messages = True
mse = torch.nn.functional.mse_loss


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2], ms


def unsharded_step():
    m.zero_grad(set_to_none=True)
    pred = m(g)
    (mse(pred["acceleration"], g.y_acc) + mse(pred["temp_rate"], g.y_temp_rate)
     + losses.momentum_conservation_loss(pred["acceleration"], g, dt, 0.1)).backward()


# the shard: every peer's request list is needed to finish the plan; the peers' requests of this rank's rows are taken from
# the other shards of the same box, so that the ghost pass, the return plan and its add have their real sizes
world = a.world
pos = g.pos
sh = cdist.build_shard(pos, 1.0, k, world, a.rank, decomposition=a.decomposition)
wants = []
for p in range(world):
    if p == a.rank:
        wants.append(torch.empty(0, dtype=torch.int64, device=dev))
    else:
        wants.append(cdist.build_shard(pos, 1.0, k, world, p, decomposition=a.decomposition).want_global[a.rank])
cdist.finish_shard(sh, wants)
sh.x_feat = g.x[sh.owned_global].contiguous()
if edge:      # the unsharded graph's edge features, receiver-major with k per receiver
    sh.edge_attr = g.edge_attr[(sh.owned_global.view(-1, 1) * k + torch.arange(k, device=dev)).reshape(-1)].contiguous()
y_acc, y_tr = g.y_acc[sh.owned_global], g.y_temp_rate[sh.owned_global]
runner = cdist.ShardedTraining(m, sh, halo=NoExchange(sh))


def shard_step():
    """One rank's step without the exchanges: forward (interior / boundary split), loss, backward (ghost pass, owned
    pass, return add of a zero buffer of the real size).  The all-reduces of the loss and the gradients are left out."""
    with torch.no_grad():
        acc, tr = runner.run_forward()
    acc.requires_grad_(True)
    tr.requires_grad_(True)
    # the rank's loss terms, with the global element counts (sharded_training_loss without its all-reduces)
    loss = ((acc - y_acc) ** 2).sum() / (3 * n_total) + ((tr - y_tr) ** 2).sum() / n_total + \
        0.1 * (losses._SegmentColsum.apply(acc, None, 1) * dt).pow(2).sum().float()
    loss.backward()
    with torch.no_grad():
        runner.decode_backward(acc.grad, tr.grad)
        for i in range(L - 1, -1, -1):
            handle = runner.halo.start_return(runner.round_backward_local(i))
            runner.round_backward_owned(i)
            runner.round_backward_return(runner.halo.finish_return(handle))
        runner.encode_backward(False)
        runner.local_grads()


split = f", n_split {runner.n_split}" if edge else ""
print(f"{a.decomposition} tiles, {'clustered' if a.clustered else 'uniform'} box; {n_total} particles, k={k}, latent {d}, {L} rounds, message_source {a.message_source}, train_precision "
      f"{a.train_precision}; shard of rank {a.rank}/{world}: {sh.n_owned} owned ({sh.n_interior} interior{split}), "
      f"{sh.n_ghost} ghosts, {sum(sh.send_counts)} rows returned to it per round", flush=True)
med_u = None
try:
    if a.no_unsharded:
        raise CgnnError("left out (--no-unsharded)")
    med_u, all_u = timed(unsharded_step, a.iters)
    print(f"unsharded training step (forward + backward): {med_u:.2f} ms median of {a.iters} "
          f"({', '.join(f'{x:.1f}' for x in all_u)})", flush=True)
except CgnnError as err:          # the edge step's memory guard: its estimate instead of a time
    if not edge and not a.no_unsharded:
        raise
    print(f"unsharded training step refused: {err}", flush=True)
m.zero_grad(set_to_none=True)
torch.cuda.empty_cache()
torch.cuda.reset_peak_memory_stats()
med_s, all_s = timed(shard_step, a.iters)
print(f"one rank's training step, no exchange:        {med_s:.2f} ms median of {a.iters} "
      f"({', '.join(f'{x:.1f}' for x in all_s)})", flush=True)
if med_u is not None:
    print(f"ratio unsharded / rank: {med_u / med_s:.2f} x  (measured without any exchange)")
peak = torch.cuda.max_memory_allocated() / 2**30
with ops.OpTimer() as tm:
    shard_step()
for name, (calls, total) in sorted(tm.summary().items(), key=lambda kv: -kv[1][1]):
    print(f"  {name:16s} {calls:4d} calls {total:9.3f} ms", flush=True)
width = runner.packs.hidden if edge else d         # edge mode returns dPs rows (hidden wide), x_j mode dx rows
reverse_mb = sh.n_ghost * width * 4 / 1e6
print(f"reverse exchange per round: {sh.n_ghost} ghost rows x {width} x 4 B = {reverse_mb:.1f} MB sent by this rank; "
      f"peak memory of the rank's steps {peak:.2f} GiB (the graph and model of the whole box included)")
