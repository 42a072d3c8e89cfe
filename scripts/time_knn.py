"""Developer tool: ``ops.knn_periodic`` on the uniform grid against the density-adaptive one (``grid="adaptive"``), all
queries, in ONE process: every shape is warmed in both modes, then the modes alternate; each call sits between two
device events.  Prints median, min and max per mode and input.  Not part of the product or tests.
    python scripts/time_knn.py [--iters 12] [--neighbors 16] [--inputs uniform:1000000 clustered:1000000 clustered:4000000]
    python scripts/time_knn.py --edge-attr reference image      (both edge-feature modes on both grids, all alternating)
    python scripts/time_knn.py --batch 4      (ops.knn_periodic_batched on 4 copies of the first input, nothing else)
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
ap.add_argument("--edge-attr", nargs="+", choices=["reference", "image"], default=["reference"],
                help="edge-feature modes to time: reference (the default of ops.knn_periodic) and / or image "
                     "(min_image_edge_attr=True)")
ap.add_argument("--batch", type=int, default=0, metavar="B",
                help="time ops.knn_periodic_batched (uniform grid) on B copies of the first input instead")
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


VARIANTS = [(grid, mode) for grid in ops.KNN_GRIDS for mode in dict.fromkeys(a.edge_attr)]


def call(pos, grid, mode):
    return timed(lambda: ops.knn_periodic(pos, box, k, want_order=not a.no_order, grid=grid,
                                          min_image_edge_attr=mode == "image"))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


if a.batch:
    one = frame(a.inputs[0])
    n, modes = one.shape[0], list(dict.fromkeys(a.edge_attr))
    pos, offsets = one.repeat(a.batch, 1), [g * one.shape[0] for g in range(a.batch + 1)]
    calls = {mode: (lambda mode=mode: ops.knn_periodic_batched(pos, offsets, box, k, True, not a.no_order,
                                                               min_image_edge_attr=mode == "image")) for mode in modes}
    for fn in calls.values():                        # warm every mode before any timing
        for _ in range(2):
            timed(fn)
    print(f"ops.knn_periodic_batched, {a.batch} x {a.inputs[0]}, k={k}, edge_attr{'' if a.no_order else ' and order'}; "
          f"device events around the call, modes alternating, {a.iters} timed calls per mode", flush=True)
    times = {mode: [timed(fn)[0]] for mode, fn in calls.items()}
    for _ in range(a.iters - 1):
        for mode, fn in calls.items():
            times[mode].append(timed(fn)[0])
    for mode, t in times.items():
        print(f"  {a.batch} x {a.inputs[0]:>14s}   batched {mode:>9s}: median {statistics.median(t):8.3f} ms   "
              f"min {min(t):8.3f}   max {max(t):8.3f}", flush=True)
    raise SystemExit(0)

frames = {spec: frame(spec) for spec in a.inputs}
for pos in frames.values():                          # warm every shape in every mode before any timing
    for grid, mode in VARIANTS:
        for _ in range(2):
            call(pos, grid, mode)
print(f"ops.knn_periodic, k={k}, all queries, edge_attr{'' if a.no_order else ' and order'}; device events around the "
      f"call, modes alternating, {a.iters} timed calls per mode and input", flush=True)
for spec, pos in frames.items():
    times = {v: [] for v in VARIANTS}
    same = True
    for _ in range(a.iters):
        outs = {}
        for v in VARIANTS:
            ms, outs[v] = call(pos, *v)
            times[v].append(ms)
        for mode in a.edge_attr:                     # the two grids give one graph in either edge-feature mode
            same = same and torch.equal(outs["uniform", mode][0], outs["adaptive", mode][0]) \
                and torch.equal(outs["uniform", mode][1], outs["adaptive", mode][1])
        del outs
    med = {v: statistics.median(t) for v, t in times.items()}
    for (grid, mode), t in times.items():
        print(f"  {spec:>18s}  {grid:>8s} {mode:>9s}: median {med[grid, mode]:8.3f} ms   min {min(t):8.3f}   "
              f"max {max(t):8.3f}")
    for mode in dict.fromkeys(a.edge_attr):
        u, ad = times["uniform", mode], times["adaptive", mode]
        apart = max(ad) < min(u) or max(u) < min(ad)
        print(f"  {spec:>18s}  {mode}: uniform / adaptive = {med['uniform', mode] / med['adaptive', mode]:.2f} x; ranges "
              f"{'do not overlap' if apart else 'overlap'}", flush=True)
    if len(set(a.edge_attr)) == 2:
        for grid in ops.KNN_GRIDS:
            r, im = times[grid, "reference"], times[grid, "image"]
            apart = max(im) < min(r) or max(r) < min(im)
            print(f"  {spec:>18s}  {grid}: image / reference = {med[grid, 'image'] / med[grid, 'reference']:.3f} x; ranges "
                  f"{'do not overlap' if apart else 'overlap'}", flush=True)
    print(f"  {spec:>18s}  same bits on both grids: {same}", flush=True)
