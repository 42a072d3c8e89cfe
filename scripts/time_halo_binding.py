"""Developer tool: the halo unbinding on frames of 1 M particles, a uniform and a clustered one (friends-of-friends groups
at 0.2 mean interparticle spacings, 20 members or more, a Plummer softening of 0.05 spacings).  Per frame: the member
ordering (``ops.halo_member_order``: one stable sort and one prefix sum in torch), the potentials
(``ops.halo_potentials`` with the ordering given: the staging kernel, two scans and the all-pairs kernel), the pair terms
per second they amount to, a full unbinding of cold groups (``statistics.halo_unbinding_on_device``: groups, 3 passes and
the evaluation pass, nobody leaves, so every pass costs the whole sum), and ``ops.fof_labels`` for scale.  Then, on the
first ``--sample`` members of the largest group taken as a group of their own (the whole group would not finish in a
minute in torch), ``ops.halo_potentials`` against a chunked torch restatement of the same integer sums.  Every call is
warmed twice, then the calls alternate; each sits between two device events.  Prints the median, min and max of 7 calls
in ms.  Not part of the product or tests.
    python scripts/time_halo_binding.py [--iters 7] [--spacings 0.2] [--softening 0.05] [--sample 32768] [--n 1000000]"""
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
ap.add_argument("--softening", type=float, default=0.05, help="Plummer softening in mean interparticle spacings")
ap.add_argument("--min-members", type=int, default=20)
ap.add_argument("--sample", type=int, default=32768, help="members of the largest group the torch restatement takes")
ap.add_argument("--chunk", type=int, default=2048, help="rows per [chunk, sample] block of the torch restatement")
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--frames", default="uniform,clustered")
a = ap.parse_args()
if a.iters < 7:
    ap.error("--iters: medians of at least 7")
dev = torch.device("cuda")
box = 1.0
n = a.n
spacing = box / n ** (1.0 / 3.0)
ll = halo_statistics.default_linking_length(n, box, a.spacings)
eps, shift = ops.check_softening(a.softening * spacing, box, "time_halo_binding")


def torch_potentials(x):
    """The integer sums of ops.halo_potentials for x [M, 3] as one group, in torch: [chunk, M] blocks."""
    half = 0.5 * box
    eps2 = torch.tensor(eps, dtype=torch.float32, device=dev) ** 2
    scale = 2.0 ** shift
    out = torch.empty(x.shape[0], dtype=torch.int64, device=dev)
    self_term = torch.round(1.0 / torch.sqrt(eps2) * scale).to(torch.int64)
    for r0 in range(0, x.shape[0], a.chunk):
        rows = x[r0:r0 + a.chunk]
        d2 = None
        for ax in range(3):
            d = x[None, :, ax] - rows[:, None, ax]
            d = torch.where(d > half, d - box, torch.where(d < -half, d + box, d))
            d2 = d * d if d2 is None else d2 + d * d
        iw = torch.round(1.0 / torch.sqrt(d2 + eps2) * scale).to(torch.int64)
        out[r0:r0 + a.chunk] = iw.sum(dim=1) - self_term
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def measure(name, calls):
    for fn in calls.values():
        for _ in range(2):
            timed(fn)
    times = {k: [] for k in calls}
    first, same = {}, True
    for _ in range(a.iters):
        for k, fn in calls.items():
            ms, out = timed(fn)
            times[k].append(ms)
            first.setdefault(k, out)
            same = same and torch.equal(out, first[k])
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in times.items():
        print(f"  {name:>10s}  {k:>44s}: median {med[k]:10.3f} ms   min {min(t):10.3f}   max {max(t):10.3f}", flush=True)
    return med, first, same


makers = {"uniform": lambda: (torch.rand(n, 3, generator=torch.Generator().manual_seed(41)) * box).to(dev),
          "clustered": lambda: synthetic.make_clustered_positions(n, box, seed=3).to(dev)}
print(f"{n} particles, groups at {a.spacings} mean spacings with {a.min_members} members or more, softening {a.softening} "
      f"spacings (shift {shift}); device events around each call, the calls alternating, {a.iters} timed calls each after "
      f"2 warm-up calls", flush=True)
for name in a.frames.split(","):
    pos = makers[name]()
    labels = ops.fof_labels(pos, box, ll)
    size, _, _ = ops.fof_catalogue(pos, labels, box, want_disp=False)
    members = ops.halo_member_order(labels, size, a.min_members)
    count = members[2].to(torch.int64)
    listed, largest = int((count > 0).sum()), int(count.max())
    terms = int((count * (count - 1)).sum())
    small = int(((count > 0) & (count <= 64)).sum())
    cold = torch.zeros(n, 3, dtype=torch.float64, device=dev)
    calls = {"halo_member_order": lambda: torch.cat([m.reshape(-1) for m in ops.halo_member_order(labels, size, a.min_members)]),
             "halo_potentials (ordering given)": lambda: ops.halo_potentials(pos, labels, size, box, eps, a.min_members,
                                                                             members=members)[0],
             "unbinding, 3 passes + evaluation, with FoF": lambda: halo_statistics.halo_unbinding_on_device(
                 pos, cold, box, 1.0, eps, ll, a.min_members)["n_bound"],
             "fof_labels": lambda: ops.fof_labels(pos, box, ll)}
    med, first, same = measure(name, calls)
    kernel = med["halo_potentials (ordering given)"]
    bound_all = torch.equal(first["unbinding, 3 passes + evaluation, with FoF"], count)
    print(f"  {name:>10s}  listed groups: {listed} ({small} of at most 64 members), the largest {largest}, members "
          f"{int(count.sum())};  ordered pair terms: {terms:.4g};  {terms / (kernel * 1e-3):.4g} pair terms per second;  "
          f"potentials / fof_labels: {kernel / med['fof_labels']:.2f};  cold groups stay whole: {bound_all};  same bits on "
          f"every call: {same}", flush=True)
    if largest < 2:
        continue
    root = int(count.argmax())
    m = min(a.sample, largest)
    idx = members[0][int(members[1][root]):int(members[1][root]) + m].to(torch.int64)
    sub = pos.index_select(0, idx).contiguous()
    sub_labels = torch.zeros(m, dtype=torch.int32, device=dev)
    sub_size = torch.zeros(m, dtype=torch.int32, device=dev)
    sub_size[0] = m
    sub_members = ops.halo_member_order(sub_labels, sub_size, 1)
    calls = {f"halo_potentials, {m} members as one group": lambda: ops.halo_potentials(sub, sub_labels, sub_size, box, eps, 1,
                                                                                      members=sub_members)[0],
             f"torch restatement, the same {m} members": lambda: torch_potentials(sub)}
    med, first, same = measure(name, calls)
    k0, k1 = list(calls)
    print(f"  {name:>10s}  sub-sample: the first {m} of the largest group's {largest} members ({m * (m - 1):.4g} ordered pair "
          f"terms);  torch / halo_potentials: {med[k1] / med[k0]:.1f};  {m * (m - 1) / (med[k0] * 1e-3):.4g} against "
          f"{m * (m - 1) / (med[k1] * 1e-3):.4g} pair terms per second;  equal to the torch restatement: "
          f"{torch.equal(first[k0], first[k1])};  same bits on every call: {same}", flush=True)
