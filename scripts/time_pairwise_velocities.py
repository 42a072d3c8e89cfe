"""Developer tool: ``ops.pair_velocity_sums`` (auto mode) on one frame of 1 M particles, uniform and clustered, with the 20
log bins up to 4 mean interparticle spacings of ``scripts/time_pair_counts.py`` and Gaussian velocities quantised on their
largest ``|v|``, and ``ops.pair_counts`` of the same frame on the same edges in the same process: the yardstick, the same
walk with no velocities.  Each shape is warmed, then the calls alternate; each call sits between two device events.  The
op's time holds the sorts, the velocity gather, the walk and the epilogue; ``--parts`` also times the walk kernel's share
by difference against a call whose edges hold no pair (everything but the counted pairs' work).  Prints the median, min
and max of 7 calls in ms per frame, the ratio of the medians, whether the counts equal the pair counter's and whether
every call gave the same bits.  Not part of the product or tests.
    python scripts/time_pairwise_velocities.py [--iters 7] [--inputs uniform:1000000 clustered:1000000]
clustered:N is synthetic.make_clustered_positions(N) (half of the particles in one Gaussian halo of 0.05 box)."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import ops, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--bins", type=int, default=20)
ap.add_argument("--spacings", type=float, default=4.0, help="largest radius in mean interparticle spacings")
ap.add_argument("--inputs", nargs="+", default=["uniform:1000000", "clustered:1000000"])
ap.add_argument("--parts", action="store_true", help="also a call with one bin that holds (almost) no pair")
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


def same(x, y):
    if torch.is_tensor(x):
        return torch.equal(x, y)
    return all(torch.equal(p, q) for p, q in zip(x, y))


frames = {spec: frame(spec) for spec in a.inputs}
print(f"{a.bins} log bins up to {a.spacings} mean spacings; device events around each call, the calls alternating, "
      f"{a.iters} timed calls each after 2 warm-up calls", flush=True)
for spec, pos in frames.items():
    n = pos.shape[0]
    reach = a.spacings * box / n ** (1.0 / 3.0)
    edges = torch.logspace(math.log10(reach / 100.0), math.log10(reach), a.bins + 1, dtype=torch.float64)
    vel = torch.randn(n, 3, generator=torch.Generator().manual_seed(43), dtype=torch.float64).to(dev)
    q = ops.quantize_weights(vel, ops._max_abs_scale(vel))
    calls = {"pair_counts": lambda: ops.pair_counts(pos, box, edges),
             "pair_velocity_sums": lambda: ops.pair_velocity_sums(pos, q, box, edges)}
    if a.parts:
        # the same grid and walk (the reach decides them), but only the outermost sliver counts: what is left is the sorts,
        # the gather, the distance tests and the epilogue
        sliver = torch.tensor([reach * (1.0 - 1e-6), reach], dtype=torch.float64)
        calls["pair_counts, a sliver"] = lambda: ops.pair_counts(pos, box, sliver)
        calls["pair_velocity_sums, a sliver"] = lambda: ops.pair_velocity_sums(pos, q, box, sliver)
    for fn in calls.values():
        for _ in range(2):
            timed(fn)
    times = {name: [] for name in calls}
    first, repeat = {}, True
    for _ in range(a.iters):
        for name, fn in calls.items():
            ms, out = timed(fn)
            times[name].append(ms)
            repeat = repeat and same(out, first.setdefault(name, out))
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, t in times.items():
        yardstick = name.replace("pair_velocity_sums", "pair_counts")
        note = "" if name == yardstick else f"   {med[name] / med[yardstick]:.2f} x {yardstick}"
        print(f"  {spec:>18s}  {name:>30s}: median {med[name]:9.3f} ms   min {min(t):9.3f}   max {max(t):9.3f}{note}",
              flush=True)
    counts, sums = first["pair_velocity_sums"]
    r2 = sums[:, 1, 1].to(torch.float64) * 2.0 ** 32 + sums[:, 1, 0].to(torch.float64)
    print(f"  {spec:>18s}  pairs counted: {int(counts.sum())}; R2 total {float(r2.sum()):.4g} (int64 holds 9.22e18); counts "
          f"equal to pair_counts: {torch.equal(counts, first['pair_counts'])}; same bits on every call: {repeat}",
          flush=True)
