"""Developer tool: ``ops.fof_labels`` and ``ops.fof_catalogue`` on one frame of 1 M particles, uniform and clustered, at a
linking length of 0.2 mean interparticle spacings; for context ``ops.pair_counts(pos, L, [0, l])`` of the same frame in
the same process (the existing kernel; it makes the same distance tests).  Every shape is
warmed, then the calls alternate; each call sits between two device events.  Prints the median, min and max of 7 calls
in ms per frame, the ratio to the pair count, the number of groups, the largest group, and the distance evaluations of
the walk under the grid rule of csrc/pair_walk.hpp (every query against every candidate of the cells its cell walks), computed
here from the cell occupancies.  Not part of the product or tests.
    python scripts/time_fof.py [--iters 7] [--spacings 0.2] [--inputs uniform:1000000 clustered:1000000]
clustered:N is synthetic.make_clustered_positions(N) (half of the particles in one Gaussian halo of 0.05 box);
clustered:N:SIGMA makes the halo SIGMA box wide."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import ops, synthetic  # noqa: E402
from cosmology_gnn_simulation_amd import statistics as halo_statistics  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--spacings", type=float, default=0.2, help="linking length in mean interparticle spacings")
ap.add_argument("--cells-per-particle", type=int, default=1,
                help="the cap G^3 <= this x N the library was built with (CGNN_FOF_CELLS_PER_PARTICLE), for the counts")
ap.add_argument("--inputs", nargs="+", default=["uniform:1000000", "clustered:1000000"])
a = ap.parse_args()
if a.iters < 7:
    ap.error("--iters: medians of at least 7")
dev = torch.device("cuda")
box = 1.0


def frame(spec):
    kind, n, *sigma = spec.split(":")
    n = int(n)
    if kind == "clustered":
        return synthetic.make_clustered_positions(n, box, seed=3, blob_sigma=float(sigma[0]) if sigma else 0.05).to(dev)
    if kind == "uniform":
        return (torch.rand(n, 3, generator=torch.Generator().manual_seed(41)) * box).to(dev)
    raise SystemExit(f"unknown input {spec!r}: uniform:N, clustered:N or clustered:N:SIGMA")


def cells_per_axis(n, reach, per_particle=1, largest=512):
    """The grid rule (pair_cells_per_axis of csrc/pair_walk.hpp) with the caps of csrc/fof.hip (per_particle is its
    CGNN_FOF_CELLS_PER_PARTICLE); largest=256: those of csrc/pair_counts.hip."""
    cap = 1
    while cap < largest and (cap + 1) ** 3 <= per_particle * n:
        cap += 1
    g = math.floor(box / (reach * (1 + 1e-5) + 2e-5 * box))
    return max(1, min(g, largest, cap))


def distance_evaluations(pos, g):
    """Sum over cells of (queries in the cell) x (candidates in the cells it walks) on a grid of g cells per axis."""
    n = pos.shape[0]
    c = (pos * (g / box)).floor().long().clamp_(0, g - 1)
    occ = torch.zeros(g * g * g, dtype=torch.float64, device=pos.device)
    occ.index_add_(0, (c[:, 0] * g + c[:, 1]) * g + c[:, 2], torch.ones(n, dtype=torch.float64, device=pos.device))
    occ = occ.view(g, g, g)
    if g <= 3:
        return float(n) * float(n)
    near = occ
    for dim in range(3):
        near = near + near.roll(1, dim) + near.roll(-1, dim)
    return float((occ * near).sum())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


frames = {spec: frame(spec) for spec in a.inputs}
print(f"linking length {a.spacings} mean spacings; device events around each call, the calls alternating, {a.iters} timed "
      f"calls each after 2 warm-up calls", flush=True)
for spec, pos in frames.items():
    n = pos.shape[0]
    ll = halo_statistics.default_linking_length(n, box, a.spacings)
    edges = halo_statistics.default_size_edges(n)
    state = {"labels": ops.fof_labels(pos, box, ll)}

    def label():
        state["labels"] = ops.fof_labels(pos, box, ll)
        return state["labels"]

    calls = {"fof_labels": label,
             "fof_catalogue": lambda: ops.fof_catalogue(pos, state["labels"], box, edges),
             "pair_counts": lambda: ops.pair_counts(pos, box, [0.0, ll])}
    for fn in calls.values():
        for _ in range(2):
            timed(fn)
    times = {name: [] for name in calls}
    first = {}
    same = True
    for _ in range(a.iters):
        for name, fn in calls.items():
            ms, out = timed(fn)
            times[name].append(ms)
            out = out if torch.is_tensor(out) else torch.cat([o.reshape(-1).to(torch.int64) for o in out])
            first.setdefault(name, out)
            same = same and torch.equal(out, first[name])
    g, g_pc = cells_per_axis(n, ll, a.cells_per_particle), cells_per_axis(n, ll, 1, 256)
    evals, evals_pc = distance_evaluations(pos, g), distance_evaluations(pos, g_pc)
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, t in times.items():
        note = ""
        if name == "fof_labels":
            note = f"   {med[name] / med['pair_counts']:.2f} x pair_counts; {evals:.3e} distance evaluations, {g} cells per axis"
        if name == "pair_counts":
            note = f"   {evals_pc:.3e} distance evaluations, {g_pc} cells per axis"
        print(f"  {spec:>18s}  {name:>13s}: median {med[name]:9.3f} ms   min {min(t):9.3f}   max {max(t):9.3f}{note}",
              flush=True)
    size = ops.fof_catalogue(pos, state["labels"], box, want_disp=False)[0]
    print(f"  {spec:>18s}  groups: {int((size > 0).sum())} (of 20 or more: {int((size >= 20).sum())}); largest: "
          f"{int(size.max())}; links counted by pair_counts: {int(first['pair_counts'][0])}; same bits on every call: {same}",
          flush=True)
