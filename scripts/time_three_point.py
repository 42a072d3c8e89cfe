"""Developer tool: ``ops.triplet_moments`` (auto mode) on one frame of 1 M particles, uniform and clustered, with the
default 8 bins from 0.5 to 4.5 mean interparticle spacings, at ``lmax`` 0, 2 and 4.  Next to it ``ops.pair_counts`` on
the same edges -- the same walk with one shared histogram, hence the natural floor: the ratio is the cost of the
moments -- and the lattice call of ``statistics.three_point_correlation`` (as many query points as particles as
primaries, the frame as neighbours).  Every call is warmed, then the calls alternate; each sits between two device
events.  Prints the median, min and max of 7 calls in ms and the ratios.  ``--lib`` loads another build of the library:
one compiled with ``EXTRA=-DCGNN_TP_TIMING_NO_CONTRACTION`` times stage 1 (the walk and its LDS atomics) without the
float64 contraction.  ``--shapes`` instead prints ``zeta_2 / zeta_0`` of the first off-diagonal bins on a frame of
filaments, on isotropic blobs and on a uniform frame.  Not part of the product or tests.
    python scripts/time_three_point.py [--iters 7] [--n 1000000] [--frames uniform,clustered] [--lmax 0,2,4]
                                       [--last-spacings 4.5] [--lib PATH] [--shapes]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import _lib, ops, synthetic  # noqa: E402
from cosmology_gnn_simulation_amd import statistics as frame_statistics  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--frames", default="uniform,clustered")
ap.add_argument("--lmax", default="0,2,4")
ap.add_argument("--last-spacings", type=float, default=4.5, help="the last radius in mean interparticle spacings")
ap.add_argument("--lib", default=None, help="another build of the library")
ap.add_argument("--shapes", action="store_true", help="zeta_2 / zeta_0 of filaments, blobs and a uniform frame instead")
a = ap.parse_args()
if a.iters < 7 and not a.shapes:
    ap.error("--iters: medians of at least 7")
if a.lib:
    _lib.LIB_PATH = os.path.abspath(a.lib)
dev = torch.device("cuda")
box = 1.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def shapes():
    n, rng = 32768, np.random.default_rng(7)
    spacing = box / n ** (1 / 3)

    def with_background(points):
        rest = rng.random((n - len(points), 3)) * box
        return torch.from_numpy(np.mod(np.concatenate([points, rest]), box).astype(np.float32)).to(dev)

    half = n // 2
    centres = rng.random((64, 3)) * box
    member = rng.integers(0, 64, half)
    direction = rng.standard_normal((64, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    along = (rng.random((half, 1)) - 0.5) * 12.0 * spacing
    filaments = centres[member] + along * direction[member] + rng.standard_normal((half, 3)) * 0.15 * spacing
    blobs = centres[member] + rng.standard_normal((half, 3)) * 1.5 * spacing
    sets = {"filaments": with_background(filaments), "blobs": with_background(blobs),
            "uniform": with_background(np.zeros((0, 3)))}
    print(f"{n} particles, half of them in 64 structures (filaments 12 spacings long and 0.15 thick; Gaussian blobs of 1.5 "
          f"spacings), the rest uniform; default edges, lmax 2", flush=True)
    for name, pos in sets.items():
        res = frame_statistics.three_point_correlation(pos, box, lmax=2)
        z = res["zeta"]
        pairs = [(0, 1), (1, 2), (2, 3)]
        print(f"  {name:>10s}  zeta_2 / zeta_0 at bins (0,1), (1,2), (2,3): "
              + ", ".join(f"{float(z[2, i, j] / z[0, i, j]):+.3f}" for i, j in pairs)
              + ";  zeta_0: " + ", ".join(f"{float(z[0, i, j]):+.4g}" for i, j in pairs)
              + ";  zeta_2: " + ", ".join(f"{float(z[2, i, j]):+.4g}" for i, j in pairs), flush=True)


if a.shapes:
    shapes()
    sys.exit(0)

n = a.n
spacing = box / n ** (1 / 3)
edges = (spacing * torch.linspace(0.5, a.last_spacings, 9, dtype=torch.float64)).to(torch.float32).tolist()
lmaxes = [int(v) for v in a.lmax.split(",")]
queries = frame_statistics.query_lattice(int(round(n ** (1 / 3))), box, dev)
print(f"{n} particles, 8 bins from 0.5 to {a.last_spacings} spacings, library {os.path.basename(_lib.LIB_PATH)}; device "
      f"events around each call, the calls alternating, {a.iters} timed calls each after a warm-up call", flush=True)
for name in a.frames.split(","):
    if name == "uniform":
        pos = (torch.rand(n, 3, generator=torch.Generator().manual_seed(41)) * box).to(dev)
    else:
        pos = synthetic.make_clustered_positions(n, box, seed=3).to(dev)
    calls = {"pair_counts": lambda: (ops.pair_counts(pos, box, edges),)}
    for lm in lmaxes:
        calls[f"triplet_moments, lmax {lm}"] = lambda lm=lm: ops.triplet_moments(pos, box, edges, lm, return_pairs=True)
    calls[f"lattice call, lmax {lmaxes[-1]}"] = lambda: ops.triplet_moments(queries, box, edges, lmaxes[-1], pos,
                                                                          return_pairs=True)
    for k, fn in calls.items():                            # the warm-up call, timed and shown as it ends
        ms, _ = timed(fn)
        print(f"  {name:>10s}  {k:>26s}: warm-up call {ms:10.3f} ms", flush=True)
    times = {k: [] for k in calls}
    first, same = {}, True
    for _ in range(a.iters):
        for k, fn in calls.items():
            ms, out = timed(fn)
            times[k].append(ms)
            out = torch.cat([o.reshape(-1).view(torch.int64) for o in out])
            first.setdefault(k, out)
            same = same and torch.equal(out, first[k])
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in times.items():
        print(f"  {name:>10s}  {k:>26s}: median {med[k]:10.3f} ms   min {min(t):10.3f}   max {max(t):10.3f}   / pair_counts "
              f"{med[k] / med['pair_counts']:6.2f}", flush=True)
    counted = int(2 * first["pair_counts"].sum())
    print(f"  {name:>10s}  counted ordered pairs: {counted} ({counted / n:.1f} per primary);  same bits on every call: {same}",
          flush=True)
