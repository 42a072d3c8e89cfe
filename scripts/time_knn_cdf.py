"""Developer tool: the kNN-CDF ops on one frame of 1 M particles, uniform and clustered, with ``ks = (1, 2, 4, 8)``, the 24
default radii and a 100^3 lattice of queries: ``ops.knn_distances`` (the search) and ``ops.knn_cdf_counts`` (the counts)
separately.  Beside them, in the same process, ``ops.knn_periodic(pos, box, 8, want_edge_attr=False)`` of the same frame
and the search with ``queries = pos``: that pair is the meaningful comparison -- the same walk with the same loads, a
list of distances alone against the graph search's (distance, key) list, and one extra sort of the queries.  Each shape
is warmed, then the calls alternate; each call sits between two device events.  Prints the median, min and max of 7 calls
in ms, the ratio of the pair's medians, and whether every call gave the same bits.

Also a chunked torch restatement (``cdist`` against the 27 n images in chunks of queries, then ``topk``) at a size that
fits (``--torch-n`` particles, as many lattice queries), against the search at that size, with the results compared.
Not part of the product or tests.
    python scripts/time_knn_cdf.py [--iters 7] [--inputs uniform:1000000 clustered:1000000] [--lattice 100]
clustered:N is synthetic.make_clustered_positions(N) (half of the particles in one Gaussian halo of 0.05 box)."""
import argparse
import os
import statistics as pystat
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import ops, statistics, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--lattice", type=int, default=100, help="queries per axis")
ap.add_argument("--inputs", nargs="+", default=["uniform:1000000", "clustered:1000000"])
ap.add_argument("--torch-n", type=int, default=32768, help="particles of the torch restatement (0: skip it)")
a = ap.parse_args()
if a.iters < 7:
    ap.error("--iters: medians of at least 7")
dev = torch.device("cuda")
box = 1.0
KS = (1, 2, 4, 8)


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


def alternate(calls, iters):
    """Two warm-up rounds, then ``iters`` rounds of every call in turn -> (times per call, all outputs repeated)."""
    for fn in calls.values():
        for _ in range(2):
            timed(fn)
    times, first, repeat = {name: [] for name in calls}, {}, True
    for _ in range(iters):
        for name, fn in calls.items():
            ms, out = timed(fn)
            times[name].append(ms)
            out = out[0] if isinstance(out, tuple) else out
            repeat = repeat and torch.equal(out, first.setdefault(name, out))
    return times, first, repeat


def report(spec, times, notes=None):
    med = {name: pystat.median(t) for name, t in times.items()}
    for name, t in times.items():
        note = "" if not notes or name not in notes else f"   {med[name] / med[notes[name]]:.2f} x {notes[name]}"
        print(f"  {spec:>18s}  {name:>34s}: median {med[name]:9.3f} ms   min {min(t):9.3f}   max {max(t):9.3f}{note}",
              flush=True)
    return med


def torch_knn_d2(pos, queries, ks, chunk_distances=1 << 24):
    """The 27 n images built, ``cdist`` in chunks of queries (2^24 distances a chunk), ``topk``: what a user does without
    the op (float32; cdist's own arithmetic, so the values agree only to rounding)."""
    s = torch.tensor([-1.0, 0.0, 1.0], device=pos.device) * box
    images = (pos[None] + torch.cartesian_prod(s, s, s)[:, None, :]).reshape(-1, 3)
    cols = torch.tensor([k - 1 for k in ks], device=pos.device)
    out = []
    for q in queries.split(max(1, chunk_distances // images.shape[0])):
        d = torch.cdist(q, images, compute_mode="donot_use_mm_for_euclid_dist")
        out.append(torch.topk(d, ks[-1], dim=1, largest=False).values.index_select(1, cols) ** 2)
    return torch.cat(out)


lattice = statistics.query_lattice(a.lattice, box, dev)
print(f"ks = {KS}, the 24 default radii, {a.lattice}^3 lattice queries; device events around each call, the calls "
      f"alternating, {a.iters} timed calls each after 2 warm-up calls", flush=True)
for spec in a.inputs:
    pos = frame(spec)
    n = pos.shape[0]
    radii = statistics.default_knn_radii(n, box)
    d2 = ops.knn_distances(pos, lattice, box, KS)
    calls = {"knn_distances, lattice": lambda: ops.knn_distances(pos, lattice, box, KS),
             "knn_cdf_counts": lambda: ops.knn_cdf_counts(d2, radii, box),
             "knn_cdf_counts, joint": lambda: ops.knn_cdf_counts(d2, radii, box, d2),
             "knn_periodic k=8, no edge_attr": lambda: ops.knn_periodic(pos, box, 8, want_edge_attr=False),
             "knn_distances, queries = pos": lambda: ops.knn_distances(pos, pos, box, KS)}
    times, first, repeat = alternate(calls, a.iters)
    report(spec, times, {"knn_distances, queries = pos": "knn_periodic k=8, no edge_attr"})
    below = first["knn_cdf_counts"]
    print(f"  {spec:>18s}  vpf at the radii' ends: {1 - int(below[0, 0]) / lattice.shape[0]:.4f} .. "
          f"{1 - int(below[0, -1]) / lattice.shape[0]:.4f}; same bits on every call: {repeat}", flush=True)
if a.torch_n > 0:
    n = a.torch_n
    m = int(round(n ** (1.0 / 3.0)))
    pos = (torch.rand(n, 3, generator=torch.Generator().manual_seed(47)) * box).to(dev)
    q = statistics.query_lattice(m, box, dev)
    calls = {"torch cdist + topk in chunks": lambda: torch_knn_d2(pos, q, KS),
             "knn_distances": lambda: ops.knn_distances(pos, q, box, KS)}
    times, first, _ = alternate(calls, a.iters)
    spec = f"uniform:{n}, {m}^3"
    report(spec, times, {"torch cdist + topk in chunks": "knn_distances"})
    err = (first["torch cdist + topk in chunks"] - first["knn_distances"]).abs().max() / first["knn_distances"].max()
    print(f"  {spec:>18s}  largest difference of the two tables over the largest value: {float(err):.2e}", flush=True)
