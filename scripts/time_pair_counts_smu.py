"""Developer tool: ``ops.pair_counts_smu`` (auto mode) on one frame of 1 M particles, uniform and clustered, with the 20 log
s-bins up to 4 mean interparticle spacings of ``scripts/time_pair_counts.py`` and 20 equal mu-bins, and
``ops.pair_counts`` of the same frame on the same ``s_edges`` in the same process: the yardstick, the same walk with no
mu-bin.  Also the 4096-bin case (64 log s-bins to the same last radius x 64 mu-bins), where the LDS histogram is shared by
pairs of waves, and to tell its parts apart 64 x 1 bins (no mu search) and 64 x 32 (2048 bins: still a histogram per
wave), each against the pair counter with the same 64 s-bins.  Every shape is warmed, then the calls alternate; each call
sits between two device events.  Prints the median, min and max of 7 calls in ms per frame, the ratios of the medians to
the pair counter's, and whether the row sums equal the pair counter's and every call gave the same bits.  Not part of
the product or tests.
    python scripts/time_pair_counts_smu.py [--iters 7] [--inputs uniform:1000000 clustered:1000000]
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
ap.add_argument("--bins", type=int, default=20, help="s-bins, and mu-bins, of the first case")
ap.add_argument("--spacings", type=float, default=4.0, help="largest radius in mean interparticle spacings")
ap.add_argument("--los", type=int, default=2)
ap.add_argument("--inputs", nargs="+", default=["uniform:1000000", "clustered:1000000"])
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


def log_edges(reach, bins):
    return torch.logspace(math.log10(reach / 100.0), math.log10(reach), bins + 1, dtype=torch.float64)


frames = {spec: frame(spec) for spec in a.inputs}
print(f"{a.bins} log s-bins up to {a.spacings} mean spacings x {a.bins} mu-bins, and 64 x 64 bins to the same radius; los "
      f"{a.los}; device events around each call, the calls alternating, {a.iters} timed calls each after 2 warm-up calls",
      flush=True)
for spec, pos in frames.items():
    n = pos.shape[0]
    reach = a.spacings * box / n ** (1.0 / 3.0)
    edges, edges64 = log_edges(reach, a.bins), log_edges(reach, 64)
    mu, mu64 = torch.linspace(0, 1, a.bins + 1, dtype=torch.float64), torch.linspace(0, 1, 65, dtype=torch.float64)
    mu1, mu32 = torch.linspace(0, 1, 2, dtype=torch.float64), torch.linspace(0, 1, 33, dtype=torch.float64)
    small, large = f"pair_counts_smu {a.bins} x {a.bins}", "pair_counts_smu 64 x 64"
    # 64 x 1: no mu search at all; 64 x 32: 2048 bins, the most that still have a histogram per wave
    calls = {"pair_counts": lambda: ops.pair_counts(pos, box, edges),
             small: lambda: ops.pair_counts_smu(pos, box, edges, mu, los=a.los),
             "pair_counts, 64 bins": lambda: ops.pair_counts(pos, box, edges64),
             "pair_counts_smu 64 x 1": lambda: ops.pair_counts_smu(pos, box, edges64, mu1, los=a.los),
             "pair_counts_smu 64 x 32": lambda: ops.pair_counts_smu(pos, box, edges64, mu32, los=a.los),
             large: lambda: ops.pair_counts_smu(pos, box, edges64, mu64, los=a.los)}
    for fn in calls.values():
        for _ in range(2):
            timed(fn)
    times = {name: [] for name in calls}
    first, same = {}, True
    for _ in range(a.iters):
        for name, fn in calls.items():
            ms, out = timed(fn)
            times[name].append(ms)
            same = same and torch.equal(out, first.setdefault(name, out))
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, t in times.items():
        yardstick = "pair_counts" if name == small else "pair_counts, 64 bins"
        note = "" if name.startswith("pair_counts,") or name == "pair_counts" else \
            f"   {med[name] / med[yardstick]:.2f} x {yardstick}"
        print(f"  {spec:>18s}  {name:>24s}: median {med[name]:9.3f} ms   min {min(t):9.3f}   max {max(t):9.3f}{note}",
              flush=True)
    rows = torch.equal(first[small].sum(-1), first["pair_counts"]) and \
        all(torch.equal(out.sum(-1), first["pair_counts, 64 bins"]) for name, out in first.items() if " 64 x " in name)
    print(f"  {spec:>18s}  pairs counted: {int(first[small].sum())}; row sums equal to pair_counts: {rows}; same counts on "
          f"every call: {same}", flush=True)
