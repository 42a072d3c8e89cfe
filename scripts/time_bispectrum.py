"""Developer tool: the stages of ``statistics.bispectrum`` behind the transform of one frame of 1 M particles, uniform and
clustered, CIC, on mesh 128 and mesh 256 with the default 16 shells: the shell filter (``ops.bispectrum_shells``), the
batched inverse transform (``ops.shell_fields``), the triangle sums (``ops.bispectrum_sums``) and, as the yardstick, a
torch composition of the same sums on the same fields, one ``(D[i] * D[j] * D[l]).sum()`` per triangle.  Each between two
device events; every call is warmed twice, then the four alternate.  Prints the median, min and max of 7 calls in ms,
the composition over the kernel, the kernel's bytes/s against the ``nb * 8 * cells`` bytes it must read, how far the two
sums differ, and Q of the equilateral triangles.  Not part of the product or tests.
    python scripts/time_bispectrum.py [--iters 7] [--meshes 128 256] [--order 2] [--inputs uniform:1000000 clustered:1000000]
clustered:N is synthetic.make_clustered_positions(N) (half of the particles in one Gaussian halo of 0.05 box)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import ops, synthetic  # noqa: E402
from cosmology_gnn_simulation_amd import statistics as cstats  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--meshes", type=int, nargs="+", default=[128, 256])
ap.add_argument("--order", type=int, default=2)
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


for mesh in a.meshes:
    edges = cstats.default_bispectrum_edges(mesh)
    plan = ops.BispectrumPlan.of(mesh, edges, dev)
    nb, nt, cells = plan.num_bins, plan.triangles.shape[0], mesh ** 3
    tri = plan.triangles.tolist()
    print(f"mesh {mesh}, order {a.order}, {nb} shells up to {float(edges[-1]):g}, {nt} triangles; device events around "
          f"each call, the calls alternating, {a.iters} timed calls each after 2 warm-up calls", flush=True)
    for spec in a.inputs:
        pos = frame(spec)
        n = pos.shape[0]
        grid = ops.mass_assign(pos, box, mesh, a.order)
        delta_k = torch.fft.rfftn(ops.grid_contrast(grid, n), dim=(-3, -2, -1))
        del grid
        state = {}

        def shells():
            state["filtered"] = ops.bispectrum_shells(delta_k, mesh, a.order, edges, plan)
            return state["filtered"]

        def inverse():
            state["fields"] = ops.shell_fields(state["filtered"], mesh).reshape(nb, -1)
            return state["fields"]

        def kernel():
            return ops.bispectrum_sums(state["fields"], plan.triangles)

        def composition():
            d = state["fields"]
            return torch.stack([(d[i] * d[j] * d[l]).sum() for i, j, l in tri])

        calls = {"bispectrum_shells": shells, "irfftn": inverse, "bispectrum_sums": kernel, "torch composition": composition}
        for _ in range(2):
            for fn in calls.values():
                timed(fn)
        times = {name: [] for name in calls}
        first, same, out = None, True, {}
        for _ in range(a.iters):
            for name, fn in calls.items():
                ms, out[name] = timed(fn)
                times[name].append(ms)
            first = out["bispectrum_sums"] if first is None else first
            same = same and torch.equal(out["bispectrum_sums"], first)
        for name, t in times.items():
            print(f"  {spec:>18s}  {name:>18s}: median {statistics.median(t):9.3f} ms   min {min(t):9.3f}   "
                  f"max {max(t):9.3f}", flush=True)
        k_ms, c_ms = statistics.median(times["bispectrum_sums"]), statistics.median(times["torch composition"])
        apart = float(((out["bispectrum_sums"] - out["torch composition"]).abs() / out["bispectrum_sums"].abs()).max())
        print(f"  {spec:>18s}  composition / kernel: {c_ms / k_ms:.1f}x; the kernel reads nb * 8 * cells = "
              f"{nb * 8 * cells / 1e9:.3f} GB: {nb * 8 * cells / (k_ms * 1e-3) / 1e12:.2f} TB/s; same bits on every call: "
              f"{same}; the composition differs by at most {apart:.1e} relative", flush=True)
        del state, out, first
        res = cstats.bispectrum(pos, box, mesh, edges, a.order)
        eq = [t for t, (i, j, l) in enumerate(tri) if i == j == l and int(res["count"][t]) > 0]
        print(f"  {spec:>18s}  Q of the equilateral triangles, k = " +
              " ".join(f"{float(res['k1'][t]):.0f}" for t in eq) + ":\n  " + " " * 20 +
              " ".join(f"{float(res['reduced_bispectrum'][t]):.3g}" for t in eq), flush=True)
    ops.BispectrumPlan.forget()
