"""CPU: the contracts of ``cgnn_knn_distances`` and ``cgnn_knn_cdf_counts`` as tests/knn_cdf_checks.py restates them
(against a float64 minimum-image brute force on dyadic inputs, and on a simple-cubic lattice with known answers), the host
arithmetic of ``statistics.knn_cdfs_from_counts``, the argument checks of the ops and of the statistics, the host
refusals of the two C entries, and the bookkeeping of the new entries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import knn_cdf_checks as kc
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib, ops, statistics

ENTRIES = ("cgnn_knn_distances_workspace_bytes", "cgnn_knn_distances", "cgnn_knn_cdf_counts")


def _dyadic(n, seed, box=32):
    """Coordinates that are multiples of 1/64 in [0, box], 0 and box among them: every float32 operation on the images
    within half the box is exact."""
    x = np.random.default_rng(seed).integers(0, 64 * box + 1, size=(n, 3)).astype(np.float32) / np.float32(64)
    x[0, 0], x[1, 1] = 0.0, float(box)
    return x


def test_the_restatement_is_the_float64_minimum_image_on_dyadic_inputs():
    box = 32.0
    pos, q = _dyadic(300, seed=1), _dyadic(70, seed=2)
    q[:5] = pos[:5]                                     # a query on a particle: distance 0
    ks = (1, 2, 3, 8, 16)
    got = kc.knn_distances(pos, q, box, ks)
    assert got.dtype == np.float32 and got.shape == (70, 5)
    # below (box / 2)^2 an image is the minimum image and its float32 distance exact; rounding is monotone, so no farther
    # image comes below it
    assert got.max() < 256.0
    want = np.sort(kc.min_image_d2_f64(pos, q, box), axis=1)[:, [k - 1 for k in ks]]
    assert (got.astype(np.float64) == want).all()
    assert (got[:5, 0] == 0).all() and (got[5:, 0] >= 0).all()
    # the order of the particles and of the queries is immaterial
    perm, qperm = np.random.default_rng(3).permutation(300), np.random.default_rng(4).permutation(70)
    assert (kc.knn_distances(pos[perm], q[qperm], box, ks) == got[qperm]).all()


def test_rank_sums_of_the_restated_counts_are_a_float64_pair_count():
    box = 32.0
    pos, q = _dyadic(300, seed=5), _dyadic(64, seed=6)
    ks = list(range(1, 65))
    radii = np.array([1.5, 3.0, 4.75, 6.0], dtype=np.float32)
    d2 = kc.knn_distances(pos, q, box, ks)
    below = kc.cdf_counts(d2, radii)
    assert below.dtype == np.int64 and below.shape == (64, 4)
    assert below[63, -1] == 0                           # no query has its 64th neighbour inside: the sums are complete
    exact = kc.min_image_d2_f64(pos, q, box)
    want = [(exact < float(r) ** 2).sum() for r in radii]
    assert below.sum(axis=0).tolist() == want and want[0] > 0
    assert (np.diff(below, axis=1) >= 0).all() and (np.diff(below, axis=0) <= 0).all()
    # strict: a radius exactly on a value does not count it
    r_on = np.sqrt(np.float32(d2[7, 3]))
    if np.float32(r_on * r_on) == d2[7, 3]:
        assert kc.cdf_counts(d2[7:8], [r_on])[3, 0] == 0
    # the joint counts are those of the elementwise maximum, and never above either
    d2_b = kc.knn_distances(_dyadic(300, seed=7), q, box, ks)
    joint = kc.cdf_counts(d2, radii, d2_b)
    assert (joint == kc.cdf_counts(np.maximum(d2, d2_b), radii)).all()
    assert (joint <= below).all() and (joint <= kc.cdf_counts(d2_b, radii)).all()


def test_simple_cubic_lattice_has_two_exact_radii():
    """Data on a lattice of spacing a = 4 in box 32, queries at the cell centres: 8 corners at 3 a^2 / 4, then the 24
    corners of the neighbouring cells at 11 a^2 / 4."""
    a, box = 4.0, 32.0
    g = np.arange(8, dtype=np.float32) * np.float32(a)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    q = kc.query_lattice(8, box)
    assert (q == pos + np.float32(a / 2)).all()
    table = kc.knn_table(pos, q, box, 33)
    assert (table[:, :8] == 3 * a * a / 4).all() and (table[:, 8:32] == 11 * a * a / 4).all()
    assert (table[:, 32] > 11 * a * a / 4).all()
    below = kc.cdf_counts(table[:, [0, 7, 8, 31]], [3.0, np.sqrt(12.0), 3.5, np.sqrt(44.0), 6.7])
    # fl32(sqrt(12))^2 rounds to 12 or next to it: leave the two radii on the steps out of the exact statement
    assert below[:, [0, 2, 4]].tolist() == [[0, 512, 512], [0, 512, 512], [0, 0, 512], [0, 0, 512]]


def test_query_lattice():
    q = statistics.query_lattice(3, 6.0)
    assert q.dtype == torch.float32 and q.shape == (27, 3) and q.device.type == "cpu"
    assert q[0].tolist() == [1.0, 1.0, 1.0] and q[1].tolist() == [1.0, 1.0, 3.0] and q[9].tolist() == [3.0, 1.0, 1.0]
    for m, box in ((1, 1.0), (7, 25.0), (10, 0.3)):
        assert np.array_equal(statistics.query_lattice(m, box).numpy(), kc.query_lattice(m, box))
    assert torch.equal(statistics.query_lattice(5, 25.0), statistics.query_lattice(5, 25.0))
    for bad in (dict(m=0), dict(m=-1), dict(m=2.0), dict(m=True), dict(m=1025), dict(box_size=0.0),
                dict(box_size=float("nan")), dict(box_size=float("inf")), dict(box_size=-2.0)):
        kw = dict(m=4, box_size=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            statistics.query_lattice(**kw)


def test_default_radii():
    r = statistics.default_knn_radii(4096, 25.0)
    spacing = 25.0 / 16.0
    assert r.dtype == torch.float64 and r.shape == (24,) and bool((r[1:] > r[:-1]).all())
    np.testing.assert_allclose([float(r[0]), float(r[-1])], [0.1 * spacing, 4.0 * spacing], rtol=1e-6)
    assert ops.check_knn_radii(r, 25.0, "t") == r.tolist()
    few = statistics.default_knn_radii(8, 1.0)          # 4 spacings = 2 boxes: cut at half the box
    assert 1 <= few.numel() < 24 and float(few[-1]) <= 0.5 and float(few[0]) == float(np.float32(0.05))
    assert statistics.default_knn_radii(1, 1.0).numel() >= 1
    for n, box in ((0, 1.0), (10, 0.0), (10, float("nan"))):
        with pytest.raises(ValueError):
            statistics.default_knn_radii(n, box)


def test_check_knn_ranks():
    assert ops.check_knn_ranks((1, 2, 4, 8), "t") == [1, 2, 4, 8]
    assert ops.check_knn_ranks([64], "t") == [64] and ops.check_knn_ranks(range(1, 17), "t") == list(range(1, 17))
    assert ops.check_knn_ranks(torch.tensor([3, 5]), "t") == [3, 5] and ops.check_knn_ranks(np.array([2.0, 7.0]).tolist(), "t") == [2, 7]
    for bad in ((), (0, 1), (1, 1), (2, 1), (65,), (1, 2.5), (True, 2), ("1",), tuple(range(1, 18)), 3, None, (-1,)):
        with pytest.raises(ValueError, match="^t: "):
            ops.check_knn_ranks(bad, "t")


def test_check_knn_radii():
    half = float(np.float32(12.5))
    assert ops.check_knn_radii([0.0, 1.0, half], 25.0, "t") == [0.0, 1.0, half]
    assert ops.check_knn_radii([3.0], 25.0, "t") == [3.0]
    assert ops.check_knn_radii(np.linspace(0.1, 12.0, 256), 25.0, "t")[0] == float(np.float32(0.1))
    above = float(np.nextafter(np.float32(12.5), np.float32(100)))
    for bad in ([], np.linspace(0.1, 12.0, 257), [-0.1, 1.0], [1.0, 1.0], [2.0, 1.0], [1.0, float("nan")],
                [1.0, float("inf")], [1.0, above], [1.0, 1.0 + 1e-9]):              # the last: equal in float32
        with pytest.raises(ValueError, match="^t: "):
            ops.check_knn_radii(bad, 25.0, "t")
    for box in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.check_knn_radii([0.1], box, "t")


def test_cdfs_from_hand_made_counts():
    ks, radii, nq = (1, 2, 3, 8), [0.5, 1.0, 2.0], 10
    below = torch.tensor([[2, 5, 10], [1, 4, 9], [0, 2, 8], [0, 0, 3]])
    res = statistics.knn_cdfs_from_counts(below, nq, ks, radii)
    assert sorted(res) == ["cdf", "counts_in_spheres", "ks", "peaked_cdf", "radii", "vpf"]
    assert res["cdf"].dtype == torch.float64 and res["cdf"].tolist() == (below.double() / 10).tolist()
    assert res["ks"] == [1, 2, 3, 8] and res["radii"].tolist() == radii
    np.testing.assert_allclose(res["peaked_cdf"].numpy(), [[0.2, 0.5, 0.0], [0.1, 0.4, 0.1], [0.0, 0.2, 0.2], [0.0, 0.0, 0.3]],
                               atol=1e-15)
    np.testing.assert_allclose(res["vpf"].numpy(), [0.8, 0.5, 0.0], atol=1e-15)
    assert sorted(res["counts_in_spheres"]) == [1, 2]                  # 3 has no 4, 8 has no 9
    np.testing.assert_allclose(res["counts_in_spheres"][1].numpy(), [0.1, 0.1, 0.1], atol=1e-15)
    np.testing.assert_allclose(res["counts_in_spheres"][2].numpy(), [0.1, 0.2, 0.1], atol=1e-15)
    # without rank 1 there is no void probability
    assert "vpf" not in statistics.knn_cdfs_from_counts(below[1:], nq, ks[1:], radii)
    # a second set
    below_b = torch.tensor([[4, 6, 10], [2, 4, 8], [0, 2, 6], [0, 0, 0]])
    joint = torch.tensor([[1, 3, 10], [1, 2, 8], [0, 1, 5], [0, 0, 0]])
    two = statistics.knn_cdfs_from_counts(below, nq, ks, radii, below_b, joint)
    assert sorted(two) == ["cdf", "cdf_b", "counts_in_spheres", "joint_cdf", "joint_excess", "ks", "peaked_cdf", "radii", "vpf"]
    assert two["cdf_b"].tolist() == (below_b.double() / 10).tolist()
    np.testing.assert_allclose(two["joint_excess"].numpy(),
                               (joint.double() / 10 - (below.double() / 10) * (below_b.double() / 10)).numpy(), atol=1e-15)
    np.testing.assert_allclose(two["joint_excess"][0].numpy(), [0.1 - 0.08, 0.3 - 0.3, 0.0], atol=1e-15)
    # a set with itself: joint_cdf = cdf, excess = cdf (1 - cdf)
    same = statistics.knn_cdfs_from_counts(below, nq, ks, radii, below, below)
    assert torch.equal(same["joint_cdf"], same["cdf"])
    np.testing.assert_allclose(same["joint_excess"].numpy(), (same["cdf"] * (1 - same["cdf"])).numpy(), atol=1e-15)
    # frames
    fr = statistics.knn_cdfs_from_counts(torch.stack([below, below_b]), nq, ks, radii)
    assert fr["cdf"].shape == (2, 4, 3) and fr["vpf"].shape == (2, 3) and fr["counts_in_spheres"][2].shape == (2, 3)
    assert torch.equal(fr["cdf"][0], res["cdf"]) and torch.equal(fr["vpf"][1], 1 - two["cdf_b"][0])
    for bad in (dict(below=below[:3]), dict(below=below[:, :2]), dict(below=below.double()), dict(below=below[0]),
                dict(n_queries=0), dict(n_queries=2.5), dict(n_queries=True), dict(ks=(1, 2, 2, 8)), dict(ks=(1, 2, 3)),
                dict(radii=[0.5, 1.0]), dict(below_b=below_b), dict(below_joint=joint),
                dict(below_b=below_b[:3], below_joint=joint)):
        kw = dict(below=below, n_queries=nq, ks=ks, radii=radii)
        kw.update(bad)
        with pytest.raises(ValueError):
            statistics.knn_cdfs_from_counts(**kw)


def test_the_ops_and_statistics_refuse_on_the_host():
    pos, q = torch.rand(100, 3), torch.rand(10, 3)      # host tensors: refused later, were the arguments right
    for kw in (dict(ks=()), dict(ks=(0,)), dict(ks=(2, 1)), dict(ks=(65,)), dict(ks=tuple(range(1, 18))), dict(box_size=0.0),
               dict(box_size=float("nan"))):
        args = dict(pos=pos, queries=q, box_size=1.0, ks=(1, 2))
        args.update(kw)
        with pytest.raises(ValueError):
            ops.knn_distances(**args)
    with pytest.raises(_lib.CgnnError):                 # the arguments pass; there is no CPU path
        ops.knn_distances(pos, q, 1.0, (1, 2))
    d2 = torch.rand(10, 2)
    for kw in (dict(radii=[]), dict(radii=[0.6]), dict(radii=[0.2, 0.1]), dict(radii=np.linspace(0.01, 0.4, 257)),
               dict(box_size=-1.0)):
        args = dict(d2_a=d2, radii=[0.1, 0.2], box_size=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.knn_cdf_counts(**args)
    with pytest.raises(_lib.CgnnError):
        ops.knn_cdf_counts(d2, [0.1, 0.2], 1.0)
    for kw in (dict(ks=(0, 1)), dict(ks=(1, 1)), dict(radii=[0.7]), dict(radii=[0.2, 0.2]), dict(n_query_axis=0),
               dict(n_query_axis=2.5), dict(queries=q, n_query_axis=4), dict(queries=q[:, :2]), dict(queries=q.numpy()),
               dict(box_size=0.0), dict(pos=pos[:2], ks=(1, 55)), dict(pos=pos[:, :2]), dict(pos_b=pos.view(1, 100, 3)),
               dict(pos_b=pos[:2], ks=(1, 55))):
        args = dict(pos=pos, box_size=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            statistics.knn_cdfs(**args)
    with pytest.raises(_lib.CgnnError):
        statistics.knn_cdfs(pos, 1.0)
    frames = {"Coordinates": pos.view(1, 100, 3).repeat(3, 1, 1)}
    for kw in (dict(ks=(3, 2)), dict(radii=[0.7]), dict(n_query_axis=0), dict(frames=[3]), dict(frames=[]), dict(frames=[-1])):
        args = dict(rollout_data=frames, ground_truth=frames, box_size=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            statistics.rollout_knn_cdfs(**args)
    with pytest.raises(_lib.CgnnError):
        statistics.rollout_knn_cdfs(frames, frames, 1.0)


def test_new_entries_are_declared_exported_built_and_documented():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert name + "(" in header and name in notes
    assert "ranks[nk - 1] <= 27 n" in header and "below[j, b] = #{q : v[q, j] < e2[b]}" in header
    for fn in ("check_knn_ranks", "check_knn_radii", "knn_distances", "knn_cdf_counts"):
        assert callable(getattr(ops, fn))
    for fn in ("query_lattice", "default_knn_radii", "knn_cdfs_from_counts", "knn_cdfs", "rollout_knn_cdfs"):
        assert callable(getattr(statistics, fn))
    csrc = os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert " knn_distances.hip" in makefile and "FLAGS_knn_distances := -ffp-contract=off\n" in makefile
    assert "$(BUILD)/knn.o $(BUILD)/knn_distances.o: knn_grid.hpp" in makefile
    # the host helpers moved, they were not copied
    knn, grid = open(os.path.join(csrc, "knn.hip")).read(), open(os.path.join(csrc, "knn_grid.hpp")).read()
    for helper in ("struct KnnGrid {", "static KnnGrid knn_grid(", "static KnnWorkspace knn_uniform_workspace(",
                   "static int knn_build_uniform(", "static int knn_check_workspace("):
        assert helper in grid and helper not in knn
    assert '#include "knn_grid.hpp"' in knn and '#include "knn_grid.hpp"' in open(os.path.join(csrc, "knn_distances.hip")).read()
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "knn_distances" in text and "rollout_knn_cdfs" in text
    assert (_lib.KNN_DISTANCES_MAX_RANKS, _lib.KNN_DISTANCES_MAX_K, _lib.KNN_CDF_MAX_RADII) == (16, 64, 256)


def test_workspace_size_and_the_host_refusals_of_the_c_entries():
    """The refusals come before any launch: no GPU is needed to meet them, and no pointer is dereferenced."""
    lib = _lib.load()
    wsb, gw = lib.cgnn_knn_distances_workspace_bytes, lib.cgnn_knn_workspace_bytes
    assert wsb(0, 5) == 256 and wsb(-1, 5) == 256 and wsb(5, -1) == 256 and wsb(2 ** 31, 5) == 256 and wsb(5, 2 ** 31) == 256

    def up(x):
        return (x + 255) // 256 * 256

    for n, nq in ((4096, 512), (1, 1), (1000000, 1000000), (300, 0), (7, 100000)):
        # the graph builder's layout for the particles, and the same over the same cells for the queries
        cells_part = gw(n, 8) - up(4 * n) - up(16 * n)
        assert wsb(n, nq) == gw(n, 8) + cells_part + up(4 * nq) + up(16 * nq), (n, nq)
    fake, odd = 1 << 20, (1 << 20) + 4                  # never dereferenced: every call below is refused on the host
    inv, unsup, short = -1, -2, -3                      # CGNN_ERR_INVALID_ARG, _UNSUPPORTED, _WORKSPACE

    def ints(*v):
        return (C.c_int32 * len(v))(*v)

    def floats(*v):
        return (C.c_float * len(v))(*v)

    def dist(pos=fake, n=100, q=fake, nq=10, box=1.0, ranks=ints(1, 2, 4, 8), nk=4, out=fake, w=fake, wb=1 << 30):
        return lib.cgnn_knn_distances(pos, n, q, nq, box, ranks, nk, out, w, wb, None)

    def err():
        return lib.cgnn_last_error().decode()

    for kw in (dict(pos=None), dict(q=None), dict(ranks=None), dict(out=None), dict(w=None), dict(n=0), dict(n=-3),
               dict(nq=-1), dict(box=0.0), dict(box=-1.0), dict(box=float("inf")), dict(box=float("nan"))):
        assert dist(**kw) == inv, kw
    assert err() == "cgnn_knn_distances: invalid argument"
    assert dist(nk=0) == inv and dist(nk=17, ranks=ints(*range(1, 18))) == inv
    assert err() == "cgnn_knn_distances: nk=17 outside [1, 16]"
    for ranks in (ints(0, 1, 2, 3), ints(1, 2, 2, 8), ints(1, 4, 2, 8), ints(1, 2, 4, 65), ints(-1, 2, 4, 8)):
        assert dist(ranks=ranks) == inv
        assert "ranks must lie in [1, 64] and ascend strictly" in err()
    assert dist(n=2, ranks=ints(1, 2, 4, 55)) == inv and "exceeds the 27*n=54 periodic images" in err()
    assert dist(n=2 ** 31) == unsup and dist(nq=2 ** 31) == unsup
    assert dist(w=odd) == inv and err() == "cgnn_knn_distances: workspace must be 16-byte aligned"
    assert dist(wb=wsb(100, 10) - 1) == short
    assert err() == f"cgnn_knn_distances: workspace {wsb(100, 10) - 1} < required {wsb(100, 10)} bytes"
    assert dist(n=2, ranks=ints(1, 2, 4, 54), wb=0) == short        # the limits themselves pass up to there
    assert dist(ranks=ints(*range(49, 65)), nk=16, wb=0) == short
    assert dist(nq=0, q=None, out=None, wb=wsb(100, 0)) == 0        # no query: nothing to do, nothing launched

    def counts(a=fake, b=None, nq=10, nk=4, radii=floats(0.1, 0.2), nr=2, below=fake):
        return lib.cgnn_knn_cdf_counts(a, b, nq, nk, radii, nr, below, None)

    for kw in (dict(a=None), dict(radii=None), dict(below=None), dict(nq=-1)):
        assert counts(**kw) == inv, kw
    assert counts(nk=0) == inv and counts(nk=17) == inv and err() == "cgnn_knn_cdf_counts: nk=17 outside [1, 16]"
    assert counts(nr=0) == inv and counts(nr=257, radii=floats(*np.linspace(0.1, 0.4, 257))) == inv
    assert err() == "cgnn_knn_cdf_counts: nr=257 outside [1, 256]"
    for radii in (floats(-0.1, 0.2), floats(0.2, 0.2), floats(0.3, 0.2), floats(0.1, float("nan")), floats(0.1, float("inf"))):
        assert counts(radii=radii) == inv
        assert "radii must be finite, non-negative and strictly ascending" in err()
    assert counts(nq=2 ** 31) == unsup
