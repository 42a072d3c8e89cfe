"""Developer tool: time ``data_utils.preprocess`` with training noise, CPU-drawn (noise_rng="reference") against made on
the device (noise_rng="device"), windows resident on the GPU.  Both modes alternate in one process after a warm-up; each
call is timed with the host clock around a final synchronise; medians are printed, with the split into the sample
(noise + features + targets) and the k-NN graph build.  Not part of the product or tests.
    python scripts/time_preprocess.py [--particles 1000000] [--window 6] [--iters 10] [--knn-grid uniform|adaptive]
    rocprofv3 --kernel-trace --stats -- python scripts/time_preprocess.py --device-only     (the kernel's own time)"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import data_utils, ops, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--particles", type=int, default=1_000_000)
ap.add_argument("--neighbors", type=int, default=16)
ap.add_argument("--window", type=int, default=6)
ap.add_argument("--noise-std", type=float, default=3e-4)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--knn-grid", choices=ops.KNN_GRIDS, default="uniform")
ap.add_argument("--device-only", action="store_true", help="skip the CPU-drawn mode (for a profiler run)")
a = ap.parse_args()
dev = torch.device("cuda")
n, w, k = a.particles, a.window, a.neighbors
snap = synthetic.make_snapshot(n, window=w, seed=1237)
meta = synthetic.make_metadata()
dt, box = meta["dt"], meta["box_size"]
c, e = snap["Coordinates"].to(dev), snap["InternalEnergy"].to(dev)
draw = 0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def whole(mode):
    global draw
    draw += 1
    # the reference path adds the noise into the targets it is given: hand it copies, as a loader hands over a new sample
    tp, tt = (c[w].clone(), e[w].clone()) if mode == "reference" else (c[w], e[w])
    return data_utils.preprocess(c[:w], e[:w], meta, tp, tt, a.noise_std, k, dt, box, check_bounds=False, noise_rng=mode,
                                 noise_seed=1237, noise_draw=draw, knn_grid=a.knn_grid)


def sample():
    return ops.training_sample(c[:w], e[:w], meta, dt, box, a.noise_std, 1237, draw, c[w], e[w])


modes = ["device"] if a.device_only else ["reference", "device"]
times = {m: [] for m in modes}
times["sample kernel call"], times["k-NN"] = [], []
for it in range(a.iters + 2):                          # two warm-up rounds
    for m in modes:
        ms, g = timed(lambda: whole(m))
        if it >= 2:
            times[m].append(ms)
    ms_s, s = timed(sample)
    ms_k, _ = timed(lambda: data_utils.knn_graph_periodic(s["recent_pos"], box, k, want_order=True,
                                                          grid=a.knn_grid))
    if it >= 2:
        times["sample kernel call"].append(ms_s)
        times["k-NN"].append(ms_k)
med = {name: statistics.median(v) for name, v in times.items()}
nbytes = 4 * n * ((w * 4 + 4) + (4 * w - 3) + 3 + 3 + 1)
print(f"preprocess with noise_std {a.noise_std:g}, k-NN grid {a.knn_grid}: {n} particles, W = {w}, k = {k}, windows on the device; "
      f"medians of {a.iters} (host clock around a synchronise)")
for m in modes:
    print(f"  noise_rng={m!r:12s} whole call {med[m]:9.2f} ms   of which k-NN {med['k-NN']:.2f} ms, "
          f"noise + features + targets {med[m] - med['k-NN']:.2f} ms")
print(f"  ops.training_sample alone (launch to synchronise) {med['sample kernel call']:.3f} ms; it moves "
      f"{nbytes / 1e9:.3f} GB (window, targets, x, last frame, both targets)")
if "reference" in med:
    print(f"  whole call: device path {med['reference'] / med['device']:.1f} x faster")
