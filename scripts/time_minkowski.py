"""Developer tool: the stages of ``statistics.minkowski_functionals`` for one frame of 1 M particles, uniform and
clustered, CIC, on mesh 128 and mesh 256, smoothed over 2 cells, at the 25 default thresholds: the deposit
(``ops.mass_assign`` and the contrast), the transforms (``rfftn``, the filter, ``irfftn``, the two variances, the division)
and the counts (``ops.excursion_counts``).  ``ops.excursion_counts`` alone is also timed on a white-noise field and on a
constant field (the worst case of its LDS counters: every element of a workgroup in one bin), and, as the yardstick, a
torch composition of the same counts on the same fields (``bucketize``, seven ``roll`` / ``maximum`` chains, eight
``bincount``).  Each between two device events; every call is warmed twice, then the calls alternate.  Prints the median,
min and max of 7 calls in ms, the composition over the kernel, the kernel against the floor of reading the field once,
``8 M^3`` bytes at the 6.3 TB/s a streaming read reaches on an MI355X, and whether the two counts are equal.  Not part of
the product or tests (tests/test_gpu_minkowski.py compares ``torch_excursion_counts`` with the kernel at mesh 33).
    python scripts/time_minkowski.py [--iters 7] [--meshes 128 256] [--order 2] [--inputs uniform:1000000 clustered:1000000]
clustered:N is synthetic.make_clustered_positions(N) (half of the particles in one Gaussian halo of 0.05 box)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import ops, synthetic  # noqa: E402
from cosmology_gnn_simulation_amd import statistics as cstats  # noqa: E402

STREAM_BYTES_PER_S = 6.3e12         # a streaming read of HBM on an MI355X, as measured (8 TB/s is the specification)


def torch_excursion_counts(field: torch.Tensor, nu: torch.Tensor) -> torch.Tensor:
    """The counts of ``ops.excursion_counts`` for one frame ``field [M, M, M]`` (float64) and thresholds ``nu [nt]`` on its
    device, composed of torch calls: int64 ``[4, nt]``."""
    nt = nu.numel()
    idx = torch.bucketize(field, nu, right=True)                        # #{t : nu[t] <= f}; a NaN lands behind them all
    idx = torch.where(torch.isnan(field), torch.zeros_like(idx), idx)

    def low(a, axis):
        return torch.maximum(a, torch.roll(a, 1, axis))

    faces = [low(idx, a) for a in range(3)]
    edges = [low(faces[(a + 1) % 3], (a + 2) % 3) for a in range(3)]
    vertices = low(edges[2], 2)
    rows = []
    for group in ([vertices], edges, faces, [idx]):
        hist = sum(torch.bincount(e.reshape(-1), minlength=nt + 1) for e in group)
        rows.append(hist[1:].flip(0).cumsum(0).flip(0))
    return torch.stack(rows)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def run_calls(label, calls, iters):
    """Two warm-up rounds, then `iters` rounds of the calls in turn -> ({name: median ms}, the last outputs)"""
    for _ in range(2):
        for fn in calls.values():
            timed(fn)
    times, out = {name: [] for name in calls}, {}
    for _ in range(iters):
        for name, fn in calls.items():
            ms, out[name] = timed(fn)
            times[name].append(ms)
    for name, t in times.items():
        print(f"  {label:>18s}  {name:>22s}: median {statistics.median(t):9.3f} ms   min {min(t):9.3f}   max {max(t):9.3f}",
              flush=True)
    return {name: statistics.median(t) for name, t in times.items()}, out


def main():
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
    nu_host = cstats.default_minkowski_thresholds()
    nu = nu_host.to(dev)

    def frame(spec):
        kind, n = spec.split(":")
        n = int(n)
        if kind == "clustered":
            return synthetic.make_clustered_positions(n, box, seed=3).to(dev)
        if kind == "uniform":
            return (torch.rand(n, 3, generator=torch.Generator().manual_seed(41)) * box).to(dev)
        raise SystemExit(f"unknown input {spec!r}: uniform:N or clustered:N")

    def counts_against_composition(label, field, mesh):
        med, out = run_calls(label, {"excursion_counts": lambda: ops.excursion_counts(field, nu_host),
                                     "torch composition": lambda: torch_excursion_counts(field, nu)}, a.iters)
        k_ms, c_ms = med["excursion_counts"], med["torch composition"]
        floor_ms = 8.0 * mesh ** 3 / STREAM_BYTES_PER_S * 1e3
        print(f"  {label:>18s}  composition / kernel: {c_ms / k_ms:.1f}x; floor 8 M^3 bytes / 6.3 TB/s = {floor_ms:.4f} ms: "
              f"kernel / floor {k_ms / floor_ms:.1f}x; equal counts: "
              f"{torch.equal(out['excursion_counts'], out['torch composition'])}", flush=True)
        return k_ms

    for mesh in a.meshes:
        smoothing = 2.0 * box / mesh
        print(f"mesh {mesh}, order {a.order}, smoothing 2 cells, {nu.numel()} thresholds; device events around each call, "
              f"the calls alternating, {a.iters} timed calls each after 2 warm-up calls", flush=True)
        white = torch.randn((mesh,) * 3, dtype=torch.float64, generator=torch.Generator().manual_seed(7)).to(dev)
        white_ms = counts_against_composition("white noise", white, mesh)
        const_ms = counts_against_composition("constant 0.1", torch.full_like(white, 0.1), mesh)
        print(f"  constant field / white noise, kernel: {const_ms / white_ms:.2f}x", flush=True)
        del white
        for spec in a.inputs:
            pos = frame(spec)
            n = pos.shape[0]
            kernel, k2w = cstats._minkowski_filters(mesh, box, smoothing, dev)
            state = {}

            def deposit():
                state["delta"] = ops.grid_contrast(ops.mass_assign(pos, box, mesh, a.order), n)
                return state["delta"]

            def transforms():
                modes = torch.fft.rfftn(state["delta"]) * kernel
                u = torch.fft.irfftn(modes, s=(mesh,) * 3)
                s0 = torch.sqrt((u * u).mean())
                s1 = torch.sqrt((k2w * (modes.real * modes.real + modes.imag * modes.imag)).sum()) / float(mesh) ** 3
                state["field"] = u / s0
                return s0, s1

            def counts():
                return ops.excursion_counts(state["field"], nu_host)

            run_calls(spec, {"deposit": deposit, "transforms": transforms, "excursion_counts": counts}, a.iters)
            counts_against_composition(spec + " smoothed", state["field"], mesh)
            res = cstats.minkowski_functionals(pos, box, mesh, smoothing, order=a.order)
            print(f"  {spec:>18s}  sigma0 {float(res['sigma0']):.4g}, sigma1 {float(res['sigma1']):.4g}; v0, v3 and the "
                  f"Gaussian v3 at nu = -1, 0, 1: " +
                  " ".join(f"{float(res[key][t]):.4g}" for key in ("v0", "v3", "gaussian_v3") for t in (8, 12, 16)), flush=True)
            del state


if __name__ == "__main__":
    main()
