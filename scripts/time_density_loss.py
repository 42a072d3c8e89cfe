"""Developer tool: the density-field loss on one frame of 1 M particles, uniform and clustered, mesh 256, CIC and TSC:
the deposit (``ops.mass_assign``), its transpose (``ops.mass_assign_backward``, a gather of 8 or 27 scattered float64
cells per particle from a mesh gradient) and the whole ``losses.density_field_loss`` forward plus backward, without and
with Gaussian smoothing (two deposits, the transposed gather, and with smoothing four 256^3 float64 FFTs), each between two
device events.  Every call is warmed twice, then the calls alternate.  Prints the median, min and max of 7 calls in ms.
Then one multi-step training step (``training.unrolled_loss`` + backward + Adam, S = 4, latent 128, 10 rounds,
``fp32x3``) with the density term on and off, alternating, and the ratio.  Not part of the product or tests.
    python scripts/time_density_loss.py [--iters 7] [--mesh 256] [--inputs uniform:1000000 clustered:1000000]
                                        [--smoothing 0.02] [--steps 4] [--no-training]
clustered:N is synthetic.make_clustered_positions(N) (half of the particles in one Gaussian halo of 0.05 box)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import graph_network, losses, ops, synthetic, training  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--mesh", type=int, default=256)
ap.add_argument("--inputs", nargs="+", default=["uniform:1000000", "clustered:1000000"])
ap.add_argument("--smoothing", type=float, default=0.02, help="Gaussian smoothing length of the smoothed calls, box units")
ap.add_argument("--steps", type=int, default=4, help="S of the training step")
ap.add_argument("--particles", type=int, default=1_000_000, help="particles of the training step")
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--mp-steps", type=int, default=10)
ap.add_argument("--no-training", action="store_true")
a = ap.parse_args()
if a.iters < 7:
    ap.error("--iters: medians of at least 7")
dev = torch.device("cuda")
box = 1.0


def frame(spec):
    kind, n = spec.split(":")
    n = int(n)
    if kind == "clustered":
        return synthetic.make_clustered_positions(n, box, seed=3).to(dev)
    if kind == "uniform":
        return (torch.rand(n, 3, generator=torch.Generator().manual_seed(41)) * box).to(dev)
    raise SystemExit(f"unknown input {spec!r}: uniform:N or clustered:N")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(calls):
    """2 warm-up rounds, then ``--iters`` rounds of every call in turn -> {name: [ms]}"""
    for _ in range(2):
        for fn in calls.values():
            timed(fn)
    times = {name: [] for name in calls}
    for _ in range(a.iters):
        for name, fn in calls.items():
            times[name].append(timed(fn)[0])
    return times


def show(label, times):
    for name, t in times.items():
        print(f"  {label:>18s}  {name:>30s}: median {statistics.median(t):9.3f} ms   min {min(t):9.3f}   max {max(t):9.3f}",
              flush=True)


print(f"mesh {a.mesh}; device events around each call, the calls alternating, {a.iters} timed calls each after 2 warm-up "
      f"calls", flush=True)
for spec in a.inputs:
    pos = frame(spec)
    n = pos.shape[0]
    # the "true" frame of the loss: the same particles displaced by a tenth of a cell
    true = torch.remainder(pos + torch.randn(n, 3, generator=torch.Generator().manual_seed(42)).to(dev) * (0.1 * box / a.mesh),
                           box)
    d_mesh = torch.randn((a.mesh,) * 3, dtype=torch.float64, generator=torch.Generator().manual_seed(43)).to(dev)
    calls = {}
    for order, name in ((2, "CIC"), (3, "TSC")):
        def loss_step(order=order, smoothing=0.0):
            p = pos.detach().requires_grad_(True)
            losses.density_field_loss(p, true, box, a.mesh, order, smoothing).backward()
            return p.grad

        calls[f"{name} mass_assign"] = lambda order=order: ops.mass_assign(pos, box, a.mesh, order)
        calls[f"{name} mass_assign_backward"] = lambda order=order: ops.mass_assign_backward(pos, d_mesh, box, a.mesh, order)
        calls[f"{name} loss fwd+bwd"] = loss_step
        calls[f"{name} loss fwd+bwd, R={a.smoothing:g}"] = lambda order=order: loss_step(order, a.smoothing)
    show(spec, alternate(calls))
    del pos, true, d_mesh, calls
    torch.cuda.empty_cache()

if not a.no_training:
    n, k, d, L, w, s = a.particles, 16, a.latent, a.mp_steps, 5, a.steps
    snap = synthetic.make_snapshot(n, window=w + s - 1, seed=1236)
    meta = synthetic.make_metadata()
    c, e = snap["Coordinates"].to(dev), snap["InternalEnergy"].to(dev)
    m = graph_network.EncodeProcessDecode(d, d, 2, L, 3)
    m.load_state_dict(synthetic.make_state_dict(d, d, 2, L, 3, node_in=4 * w - 3))
    m = m.to(dev).train()
    m.train_precision, m.message_source, m.train_edge_messages = "fp32x3", "x_j", False
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    draws = 0

    def train_step(**density):
        global draws
        out = training.unrolled_loss(m, c[:w], e[:w], c[w:w + s], e[w:w + s], meta, dt=0.01, box_size=1.0, num_neighbors=k,
                                     noise_std=3e-4, noise_seed=1236, noise_draw=draws, momentum_loss_weight=0.1, **density)
        draws += 1
        opt.zero_grad()
        out.loss.backward()
        opt.step()

    on = dict(density_loss_weight=1.0, density_mesh=a.mesh, density_order=2)
    times = alternate({"term off": train_step, "term on (CIC)": lambda: train_step(**on),
                       f"term on (CIC, R={a.smoothing:g})": lambda: train_step(**on, density_smoothing=a.smoothing)})
    show(f"S={s} step, N={n}", times)
    off = statistics.median(times["term off"])
    for name, t in times.items():
        if name != "term off":
            print(f"  {name}: {statistics.median(t) / off:.4f} of the step with the term off ({off:.2f} ms)", flush=True)
