"""Developer tool: ``ops.halo_profiles`` on frames of 1 M particles, a uniform and a clustered one, around the centres of
the frame's largest friends-of-friends groups (0.2 mean interparticle spacings, 20 members or more; a frame without such
a group takes its largest groups whatever their size), with the default radii, without values and with one value
channel.  Next to it ``ops.pair_counts(centres, L, edges, pos_b=pos)`` of the same frame -- the same walk with one shared
histogram, hence the natural floor -- and a torch restatement written here (``[h_chunk, N]`` distances, ``bucketize``,
``scatter_add``).  Every call is warmed twice, then the calls alternate; each sits between two device events.  Prints the
median, min and max of 7 calls in ms, the two ratios, and the share of the candidates that the most crowded centre's
neighbourhood holds.  Not part of the product or tests.
    python scripts/time_halo_profiles.py [--iters 7] [--spacings 0.2] [--min-members 20] [--max-halos 1024] [--n 1000000]"""
import argparse
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
ap.add_argument("--min-members", type=int, default=20)
ap.add_argument("--max-halos", type=int, default=1024)
ap.add_argument("--h-chunk", type=int, default=32, help="centres per [h_chunk, N] block of the torch restatement")
ap.add_argument("--n", type=int, default=1000000)
a = ap.parse_args()
if a.iters < 7:
    ap.error("--iters: medians of at least 7")
dev = torch.device("cuda")
box = 1.0
n = a.n
ll = halo_statistics.default_linking_length(n, box, a.spacings)
edges = halo_statistics.default_radial_edges(n, box)
e = ops.check_profile_edges(edges, box, "time_halo_profiles")
nb = len(e) - 1
e2 = torch.tensor(e, dtype=torch.float32, device=dev)
e2 = e2 * e2


def torch_profiles(pos, centres, q=None):
    """counts [H, nb] (and sums [H, nb]) of ops.halo_profiles in torch, h_chunk centres at a time."""
    half = 0.5 * box
    counts = torch.zeros((centres.shape[0], nb + 1), dtype=torch.int64, device=dev)
    sums = None if q is None else torch.zeros_like(counts)
    q64 = None if q is None else q.to(torch.int64)
    for h0 in range(0, centres.shape[0], a.h_chunk):
        c = centres[h0:h0 + a.h_chunk]
        d2 = None
        for ax in range(3):
            d = pos[None, :, ax] - c[:, None, ax]
            d = torch.where(d > half, d - box, torch.where(d < -half, d + box, d))
            d2 = d * d if d2 is None else d2 + d * d
        idx = torch.bucketize(d2, e2, right=True) - 1
        idx = torch.where((idx >= 0) & (idx < nb), idx, torch.full_like(idx, nb))      # the last column takes the rest
        counts[h0:h0 + a.h_chunk].scatter_add_(1, idx, torch.ones_like(idx))
        if q is not None:
            sums[h0:h0 + a.h_chunk].scatter_add_(1, idx, q64[None, :].expand(idx.shape))
    return (counts[:, :nb],) if q is None else (counts[:, :nb], sums[:, :nb])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


frames = {"uniform": (torch.rand(n, 3, generator=torch.Generator().manual_seed(41)) * box).to(dev),
          "clustered": synthetic.make_clustered_positions(n, box, seed=3).to(dev)}
print(f"{n} particles, centres: the up to {a.max_halos} largest groups at {a.spacings} mean spacings, {nb} bins from "
      f"{e[1] / (box / n ** (1 / 3)):.2f} to {e[-1] / (box / n ** (1 / 3)):.2f} spacings; device events around each call, the "
      f"calls alternating, {a.iters} timed calls each after 2 warm-up calls", flush=True)
for name, pos in frames.items():
    labels = ops.fof_labels(pos, box, ll)
    size, disp, _ = ops.fof_catalogue(pos, labels, box)
    listed = int((size >= a.min_members).sum())
    slot = torch.arange(n, dtype=torch.int64, device=dev)
    key = (size.to(torch.int64) << 32) | ((1 << 32) - 1 - slot)
    if listed:
        key = torch.where(size >= a.min_members, key, torch.full_like(key, -1))
    top, root = torch.topk(key, min(a.max_halos, listed if listed else a.max_halos))
    centres, valid = halo_statistics.halo_centres_on_device(pos, size, disp, root, box)
    assert bool(valid.all())
    sizes = size[root]
    values = torch.rand(n, generator=torch.Generator().manual_seed(44)).to(dev) + 0.5
    q = ops.quantize_weights(values, 1.5)
    h = centres.shape[0]

    calls = {"halo_profiles": lambda: (ops.halo_profiles(pos, centres, box, e),),
             "halo_profiles, one value channel": lambda: ops.halo_profiles(pos, centres, box, e, q),
             "pair_counts(centres, pos_b=pos)": lambda: (ops.pair_counts(centres, box, e, pos_b=pos),),
             "torch bucketize / scatter_add": lambda: torch_profiles(pos, centres),
             "torch, one value channel": lambda: torch_profiles(pos, centres, q)}
    for fn in calls.values():
        for _ in range(2):
            timed(fn)
    times = {k: [] for k in calls}
    first, same = {}, True
    for _ in range(a.iters):
        for k, fn in calls.items():
            ms, out = timed(fn)
            times[k].append(ms)
            out = torch.cat([o.reshape(-1) for o in out])
            first.setdefault(k, out)
            same = same and torch.equal(out, first[k])
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in times.items():
        print(f"  {name:>10s}  {k:>33s}: median {med[k]:9.3f} ms   min {min(t):9.3f}   max {max(t):9.3f}", flush=True)
    counts = first["halo_profiles"].reshape(h, nb)
    agree = torch.equal(first["halo_profiles"], first["torch bucketize / scatter_add"]) and \
        torch.equal(first["halo_profiles, one value channel"], first["torch, one value channel"])
    floor = torch.equal(counts.sum(0), first["pair_counts(centres, pos_b=pos)"])
    per = counts.sum(1)
    print(f"  {name:>10s}  halo_profiles / pair_counts: {med['halo_profiles'] / med['pair_counts(centres, pos_b=pos)']:.2f} "
          f"(with values {med['halo_profiles, one value channel'] / med['pair_counts(centres, pos_b=pos)']:.2f});  torch / "
          f"halo_profiles: {med['torch bucketize / scatter_add'] / med['halo_profiles']:.1f} (with values "
          f"{med['torch, one value channel'] / med['halo_profiles, one value channel']:.1f});  centres: {h} (listed groups: "
          f"{listed}), sizes {int(sizes.min())} to {int(sizes.max())};  particles inside the last radius: {int(per.sum())} "
          f"in all, {int(per.max())} around the most crowded centre ({float(per.max()) / max(float(per.sum()), 1.0):.3f} of "
          f"them);  equal to the torch restatement: {agree};  summed over the centres equal to pair_counts: {floor};  same "
          f"bits on every call: {same}", flush=True)
