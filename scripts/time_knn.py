"""Developer tool: ``ops.knn_periodic`` on the uniform grid against the density-adaptive one (``grid="adaptive"``), all
queries, in ONE process: every shape is warmed in both modes, then the modes alternate; each call sits between two
device events.  Prints median, min and max per mode and input.  Not part of the product or tests.
    python scripts/time_knn.py [--iters 12] [--neighbors 16] [--inputs uniform:1000000 clustered:1000000 clustered:4000000]
    rocprofv3 --kernel-trace --stats -- python scripts/time_knn.py --iters 10       (build kernels against the search)
clustered:N is synthetic.make_clustered_positions(N) (half of the particles in one Gaussian halo of 0.05 box)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import ops, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=12)
ap.add_argument("--neighbors", type=int, default=16)
ap.add_argument("--inputs", nargs="+", default=["uniform:1000000", "clustered:1000000", "clustered:4000000"])
ap.add_argument("--no-order", action="store_true", help="leave the sorted-order by-product out of the timed call")
a = ap.parse_args()
if a.iters < 10:
    ap.error("--iters: medians of at least 10")
dev = torch.device("cuda")
k, box = a.neighbors, 1.0


def frame(spec):
    kind, n = spec.split(":")
    n = int(n)
    if kind == "clustered":
        return synthetic.make_clustered_positions(n, box, seed=3).to(dev)
    if kind == "uniform":
        return (torch.rand(n, 3, generator=torch.Generator().manual_seed(41)) * box).to(dev)
    raise SystemExit(f"unknown input {spec!r}: uniform:N or clustered:N")


def call(pos, grid):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ops.knn_periodic(pos, box, k, want_order=not a.no_order, grid=grid)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


frames = {spec: frame(spec) for spec in a.inputs}
for pos in frames.values():                          # warm every shape in both modes before any timing
    for grid in ops.KNN_GRIDS:
        for _ in range(2):
            call(pos, grid)
print(f"ops.knn_periodic, k={k}, all queries, edge_attr{'' if a.no_order else ' and order'}; device events around the "
      f"call, modes alternating, {a.iters} timed calls per mode and input", flush=True)
for spec, pos in frames.items():
    times = {grid: [] for grid in ops.KNN_GRIDS}
    same = True
    for _ in range(a.iters):
        outs = {}
        for grid in ops.KNN_GRIDS:
            ms, outs[grid] = call(pos, grid)
            times[grid].append(ms)
        same = same and torch.equal(outs["uniform"][0], outs["adaptive"][0]) \
            and torch.equal(outs["uniform"][1], outs["adaptive"][1])
        del outs
    med = {g: statistics.median(v) for g, v in times.items()}
    for g, v in times.items():
        print(f"  {spec:>18s}  {g:>8s}: median {med[g]:8.3f} ms   min {min(v):8.3f}   max {max(v):8.3f}")
    apart = max(times["adaptive"]) < min(times["uniform"]) or max(times["uniform"]) < min(times["adaptive"])
    print(f"  {spec:>18s}  uniform / adaptive = {med['uniform'] / med['adaptive']:.2f} x; ranges "
          f"{'do not overlap' if apart else 'overlap'}; same bits: {same}", flush=True)
