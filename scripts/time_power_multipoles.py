"""Developer tool: the shell sums of the redshift-space multipoles on one frame of 1 M particles, uniform and clustered,
mesh 256, CIC, the 128 default bins, each call between two device events:

* ``ops.power_bins``, auto and cross (the existing reduction: four sums);
* ``ops.power_multipoles`` plain and interlaced, auto and cross (twelve sums; interlaced: two more arrays read and
  combined inside the reduction);
* ``ops.redshift_positions`` of the frame;
* a torch composition of the interlaced result: the pair combined in torch (``x = (a + a2 phase) / 2``, the phase table
  made beforehand), multiplied by tables of L2 and L4 (made beforehand), and ``ops.power_bins`` called three times per
  set, ``(x)``, ``(x, x L2)``, ``(x, x L4)`` (row 2 of a cross call is ``sum wt Re(x conj(x L)) = sum wt |x|^2 L``), and
  three times for the cross rows ``(x, y)``, ``(x, y L2)``, ``(x, y L4)``.

Every call is warmed twice, then they alternate.  Prints the median, min and max of 7 calls in ms and the ratios of
``ops.power_multipoles`` to ``ops.power_bins`` and to the torch composition.  Not part of the product or tests.
    python scripts/time_power_multipoles.py [--iters 7] [--mesh 256] [--order 2] [--inputs uniform:1000000 clustered:1000000]
clustered:N is synthetic.make_clustered_positions(N) (half of the particles in one Gaussian halo of 0.05 box)."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import ops, synthetic  # noqa: E402
from cosmology_gnn_simulation_amd import statistics as cstats  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--mesh", type=int, default=256)
ap.add_argument("--order", type=int, default=2)
ap.add_argument("--los", type=int, default=2)
ap.add_argument("--inputs", nargs="+", default=["uniform:1000000", "clustered:1000000"])
a = ap.parse_args()
if a.iters < 7:
    ap.error("--iters: medians of at least 7")
dev = torch.device("cuda")
box, M, los = 1.0, a.mesh, a.los


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


def transform(pos):
    delta = ops.grid_contrast(ops.mass_assign(pos, box, M, a.order), pos.shape[0])
    return torch.fft.rfftn(delta, dim=(-3, -2, -1))


# the tables of the torch composition, over the signed frequencies of cgnn_power_bins
i = torch.arange(M, dtype=torch.float64, device=dev)
full = torch.where(i <= M // 2, i, i - M)
half = torch.arange(M // 2 + 1, dtype=torch.float64, device=dev)
n = (full[:, None, None], full[None, :, None], half[None, None, :])
n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
mu2 = torch.where(n2 > 0, (n[los] * n[los]).expand_as(n2) / n2.clamp(min=1.0), torch.zeros_like(n2))
L2, L4 = 1.5 * mu2 - 0.5, (4.375 * mu2 - 3.75) * mu2 + 0.375
phase = torch.polar(torch.ones_like(n2), math.pi * (n[0] + n[1] + n[2]) / M)
del mu2, n2

edges = cstats.default_k_edges(M)
plan = ops.PowerPlan.of(M, edges, dev)
print(f"mesh {M}, order {a.order}, los {los}, {len(edges) - 1} default bins; device events around each call, the calls "
      f"alternating, {a.iters} timed calls each after 2 warm-up calls", flush=True)
for spec in a.inputs:
    pos = frame(spec)
    jitter = torch.randn(pos.shape, generator=torch.Generator().manual_seed(7)).to(dev) * (0.3 * box / M)
    prev = torch.remainder(pos - jitter, box).clamp(0.0, box)
    other = torch.remainder(pos + jitter, box).clamp(0.0, box)
    ak, bk = transform(pos), transform(other)
    ak2, bk2 = transform(ops.interlace_shift(pos, box, M)), transform(ops.interlace_shift(other, box, M))

    def bins(*args):
        return ops.power_bins(*args[:1], M, a.order, edges, *args[1:], plan=plan)

    def composed_set(x):
        return bins(x)[1][0], bins(x, x * L2)[1][2], bins(x, x * L4)[1][2]

    def composed(cross):
        x = 0.5 * (ak + ak2 * phase)
        if not cross:
            return composed_set(x)
        y = 0.5 * (bk + bk2 * phase)
        return composed_set(x) + composed_set(y) + (bins(x, y)[1][2], bins(x, y * L2)[1][2], bins(x, y * L4)[1][2])

    def multipoles(b=None, a2=None, b2=None):
        return ops.power_multipoles(ak, M, a.order, edges, los, b, a2, b2, plan)

    calls = {"power_bins auto": lambda: bins(ak), "power_bins cross": lambda: bins(ak, bk),
             "multipoles plain auto": lambda: multipoles(), "multipoles plain cross": lambda: multipoles(bk),
             "multipoles interlaced auto": lambda: multipoles(None, ak2),
             "multipoles interlaced cross": lambda: multipoles(bk, ak2, bk2),
             "redshift_positions": lambda: ops.redshift_positions(pos, prev, 1.0, box, los, 1.0),
             "torch composition auto": lambda: composed(False), "torch composition cross": lambda: composed(True)}
    for _ in range(2):
        for fn in calls.values():
            timed(fn)
    times = {name: [] for name in calls}
    for _ in range(a.iters):
        for name, fn in calls.items():
            times[name].append(timed(fn)[0])
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, t in times.items():
        print(f"  {spec:>18s}  {name:>28s}: median {med[name]:9.3f} ms   min {min(t):9.3f}   max {max(t):9.3f}", flush=True)
    for kind in ("auto", "cross"):
        print(f"  {spec:>18s}  {kind}: plain multipoles / power_bins {med['multipoles plain ' + kind] / med['power_bins ' + kind]:.2f}, "
              f"interlaced multipoles / power_bins {med['multipoles interlaced ' + kind] / med['power_bins ' + kind]:.2f}, "
              f"interlaced multipoles / torch composition {med['multipoles interlaced ' + kind] / med['torch composition ' + kind]:.3f}",
              flush=True)
    # the two agree: the composition's rows against the kernel's
    _, sums = multipoles(bk, ak2, bk2)
    got = torch.stack(composed(True))
    want = sums[:9]
    print(f"  {spec:>18s}  composition against the kernel: largest difference "
          f"{float(((got - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max()):.2e} of a row's largest bin", flush=True)
    del ak, bk, ak2, bk2
