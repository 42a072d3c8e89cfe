"""CPU: the contract of ``cgnn_halo_profiles`` as tests/halo_profile_checks.py restates it, on cases known by hand; the
spherical-overdensity rule of ``statistics.so_masses`` on a profile with an analytic answer; the default radii; the
bookkeeping and the host refusals of the C entry; the refusals of ``ops.halo_profiles`` and of the ``statistics`` layer,
all before any device work."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import halo_profile_checks as hp
import pair_count_checks as pcc
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib, ops, statistics

ENTRIES = ("cgnn_halo_profiles_workspace_bytes", "cgnn_halo_profiles")
MAX_BINS = _lib.HALO_PROFILES_MAX_BINS    # 32: a centre's histogram is a row of LDS counters
SHELLS = [0.0, 0.5, 1.2, 1.6, 1.9]        # around 0, a, a sqrt(2), a sqrt(3) of a lattice with a = 1


def test_a_centre_on_a_lattice_particle_sees_1_6_12_8():
    x = pcc.lattice_points()               # 8^3 points at integer coordinates, box 8
    centres = np.array([[3, 3, 3], [0, 0, 0], [8, 8, 8], [7, 0, 8]], dtype=np.float32)   # inside, corners, an edge
    counts = hp.profiles(x, centres, 8.0, SHELLS)
    assert counts.dtype == np.int64 and counts.tolist() == [[1, 6, 12, 8]] * 4


def test_a_centre_at_a_box_corner_sees_its_neighbours_across_three_faces():
    x = pcc.lattice_points(0.5)            # particles at 0.5 .. 7.5: the corner lies between eight of them
    for corner in ([0, 0, 0], [8, 8, 8], [0, 8, 0]):
        counts = hp.profiles(x, np.array([corner], dtype=np.float32), 8.0, [0.0, 0.8, 0.9, 1.6])
        assert counts.tolist() == [[0, 8, 0]]          # sqrt(0.75) = 0.866; the next shell is at sqrt(2.75) = 1.66


def test_a_positive_first_edge_drops_the_coincident_particle():
    x = pcc.lattice_points()
    c = np.array([[3, 3, 3]], dtype=np.float32)
    assert hp.profiles(x, c, 8.0, [0.0, 0.5]).tolist() == [[1]]
    assert hp.profiles(x, c, 8.0, [0.25, 0.5]).tolist() == [[0]]
    assert hp.profiles(x, c, 8.0, [0.25, 1.2]).tolist() == [[6]]
    # d2 on an edge falls in the UPPER bin (half-open bins)
    assert hp.profiles(x, c, 8.0, [0.0, 1.0, 1.2]).tolist() == [[1, 6]]


def test_the_sums_follow_the_counts():
    x = pcc.lattice_points()
    c = np.array([[3, 3, 3], [0.25, 0, 0]], dtype=np.float32)
    q = np.stack([np.ones(512), -2 * np.ones(512), x[:, 0]], axis=1).astype(np.int32)
    counts, sums = hp.profiles(x, c, 8.0, SHELLS, q)
    assert sums.shape == (2, 4, 3) and sums.dtype == np.int64
    assert (sums[..., 0] == counts).all() and (sums[..., 1] == -2 * counts).all()
    assert sums[0, :, 2].tolist() == [3, 18, 36, 24]   # the shells are symmetric about x = 3
    flat = hp.profiles(x, c, 8.0, SHELLS, q[:, 2])[1]
    assert flat.shape == (2, 4) and (flat == sums[..., 2]).all()


def test_summed_over_the_centres_it_is_the_cross_pair_count():
    rng = np.random.default_rng(5)
    x = rng.random((700, 3), dtype=np.float32) * np.float32(10.0)
    centres = np.concatenate([rng.random((37, 3), dtype=np.float32) * np.float32(10.0), x[:5],
                              np.array([[10.0, 0.0, 5.0]], dtype=np.float32)])
    for edges in ([0.0, 0.7, 1.9, 3.3, 5.0], [0.4, 2.2]):
        assert (hp.profiles(x, centres, 10.0, edges).sum(axis=0) == pcc.cross_counts(centres, x, 10.0, edges)).all()


# ---- so_masses -----------------------------------------------------------------------------------------------------
BOX, N, A = 100.0, 10 ** 6, 20000          # mean density 1; N(< r) = A r, so D(r) = A / (4/3 pi r^2) exactly
RADII = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]


def test_so_masses_returns_the_analytic_crossing_of_a_power_law():
    counts = torch.full((1, 8), A, dtype=torch.int64)
    for delta in (200.0, 500.0, 100.0):
        want_r = math.sqrt(A / (4.0 / 3.0 * math.pi * delta))
        assert RADII[1] < want_r < RADII[-1]
        r, m = statistics.so_masses(counts, N, BOX, RADII, delta)
        assert r.dtype == torch.float64 and r.shape == (1,) and m.shape == (1,)
        assert abs(float(r) / want_r - 1) <= 1e-12
        assert abs(float(m) / (A * want_r) - 1) <= 1e-12          # M = delta rho 4/3 pi R^3 = N(< R) = A R
        rr, mm = hp.so_masses(counts.numpy(), N, BOX, RADII, delta)
        assert abs(rr[0] / want_r - 1) <= 1e-12 and abs(mm[0] / (A * want_r) - 1) <= 1e-12
    # leading axes are kept
    r2, _ = statistics.so_masses(counts.expand(3, 2, 8), N, BOX, RADII)
    assert r2.shape == (3, 2) and bool((r2 == r2[0, 0]).all())


def test_so_masses_is_nan_where_the_rule_finds_nothing_and_passes_over_an_empty_core():
    dense = 4.0 / 3.0 * math.pi * 8.0 ** 3 * 200.0                 # particles that keep D >= 200 out to the last edge
    rows = [[0] * 8,                                               # empty: D = 0 everywhere
            [50] * 8,                                              # too diffuse: D_1 = 50 / 4.19 < 200
            [int(dense) + 1] + [0] * 7,                            # never falls below 200 inside the last edge
            [0, 0, 30000, 0, 0, 0, 0, 0],                          # empty core: D_1 = D_2 = 0, D_3 = 265, D_4 = 112
            [A] * 8]
    counts = torch.tensor(rows, dtype=torch.int64)
    r, m = statistics.so_masses(counts, N, BOX, RADII)
    rr, mm = hp.so_masses(counts.numpy(), N, BOX, RADII)
    assert torch.isnan(r).tolist() == [True, True, True, False, False] == np.isnan(rr).tolist()
    assert torch.isnan(m).tolist() == [True, True, True, False, False]
    assert 3.0 < float(r[3]) < 4.0
    np.testing.assert_allclose(r[3:].numpy(), rr[3:], rtol=1e-12)
    np.testing.assert_allclose(m[3:].numpy(), mm[3:], rtol=1e-12)
    # D constant-count beyond edge 3: N = 30000, D = 30000 / (4/3 pi r^3), so R = (30000 / (4/3 pi 200))^(1/3) exactly
    assert abs(float(r[3]) / (30000 / (4.0 / 3.0 * math.pi * 200.0)) ** (1.0 / 3.0) - 1) <= 1e-12
    # one bin: there is never an edge behind i*
    one = statistics.so_masses(torch.tensor([[10 ** 6]]), N, BOX, [0.0, 1.0])
    assert bool(torch.isnan(one[0]).all()) and bool(torch.isnan(one[1]).all())
    assert np.isnan(hp.so_masses([[10 ** 6]], N, BOX, [0.0, 1.0])[0]).all()


def test_so_masses_refusals():
    counts = torch.zeros((2, 8), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"edges\[0\] must be 0"):
        statistics.so_masses(counts, N, BOX, [0.5] + RADII[1:])
    with pytest.raises(ValueError, match="counts must be"):
        statistics.so_masses(counts[:, :7], N, BOX, RADII)
    for bad in (0.0, -1.0, float("nan"), True):
        with pytest.raises(ValueError, match="delta"):
            statistics.so_masses(counts, N, BOX, RADII, bad)


def test_default_radial_edges():
    e = statistics.default_radial_edges(10 ** 6, 100.0)            # spacing 1: nothing reaches half the box
    assert e.dtype == torch.float64 and e.shape == (25,) and float(e[0]) == 0.0
    assert bool((e[1:] > e[:-1]).all()) and torch.equal(e, e.to(torch.float32).to(torch.float64))
    assert abs(float(e[1]) / 0.05 - 1) < 1e-6 and abs(float(e[-1]) / 8.0 - 1) < 1e-6
    ratio = e[2:] / e[1:-1]
    assert float((ratio / ratio[0] - 1).abs().max()) < 1e-5        # log-spaced
    ops.check_profile_edges(e, 100.0, "test")
    # 512 particles in a box of 8: spacing 1, half the box is 4: the radii above are dropped
    small = statistics.default_radial_edges(512, 8.0)
    assert 2 <= small.numel() < 25 and float(small[-1]) <= 4.0 < float(e[small.numel()])
    np.testing.assert_allclose(small.numpy(), e[:small.numel()].numpy(), rtol=1e-6)     # the same spacing, cut at 4
    ops.check_profile_edges(small, 8.0, "test")
    # one particle: the spacing is the box and still 0.05 of it stays
    assert statistics.default_radial_edges(1, 3.0).numel() >= 2
    for bad in (0, -5):
        with pytest.raises(ValueError):
            statistics.default_radial_edges(bad, 8.0)
    with pytest.raises(ValueError):
        statistics.default_radial_edges(100, 0.0)


# ---- refusals before any device work ---------------------------------------------------------------------------------
def test_ops_halo_profiles_refuses_on_the_host():
    pos, cen = torch.zeros((10, 3)), torch.zeros((2, 3))
    with pytest.raises(ValueError, match="33 bins"):
        ops.halo_profiles(pos, cen, 8.0, np.linspace(0.0, 4.0, MAX_BINS + 2))
    assert len(ops.check_profile_edges(np.linspace(0.0, 4.0, MAX_BINS + 1), 8.0, "test")) == 33      # 32 bins pass
    with pytest.raises(ValueError, match="ascend"):
        ops.halo_profiles(pos, cen, 8.0, [0.0, 2.0, 1.0])
    with pytest.raises(ValueError, match="half the box"):
        ops.halo_profiles(pos, cen, 8.0, [0.0, 4.5])
    with pytest.raises(ValueError, match="box_size"):
        ops.halo_profiles(pos, cen, -8.0, [0.0, 1.0])
    with pytest.raises(ValueError, match="5 channels"):
        ops.halo_profiles(pos, cen, 8.0, [0.0, 1.0], torch.zeros((10, 5)))
    with pytest.raises(ValueError, match="values must be"):
        ops.halo_profiles(pos, cen, 8.0, [0.0, 1.0], torch.zeros(9))
    with pytest.raises(ValueError, match="values must be"):
        ops.halo_profiles(pos, cen, 8.0, [0.0, 1.0], torch.zeros(10, dtype=torch.bool))
    with pytest.raises(ValueError, match="value_scale must be None"):
        ops.halo_profiles(pos, cen, 8.0, [0.0, 1.0], torch.zeros(10, dtype=torch.int32), 2.0)
    with pytest.raises(ValueError, match="value_scale"):
        ops.halo_profiles(pos, cen, 8.0, [0.0, 1.0], torch.zeros(10), -1.0)
    with pytest.raises(ValueError, match="value_scale without values"):
        ops.halo_profiles(pos, cen, 8.0, [0.0, 1.0], None, 1.0)
    with pytest.raises(ValueError, match="pos must be"):
        ops.halo_profiles(torch.zeros((10, 2)), cen, 8.0, [0.0, 1.0])
    for bad in (torch.zeros((2, 2)), torch.zeros((1, 2, 3)), torch.zeros((0, 3))):
        with pytest.raises(ValueError, match="centres must be"):
            ops.halo_profiles(pos, bad, 8.0, [0.0, 1.0])
    with pytest.raises(ValueError, match="centres must be"):                   # T differs
        ops.halo_profiles(torch.zeros((2, 10, 3)), torch.zeros((3, 2, 3)), 8.0, [0.0, 1.0])
    # a CPU tensor that is otherwise fine: there is no CPU path
    with pytest.raises(_lib.CgnnError, match="no CPU path"):
        ops.halo_profiles(pos, cen, 8.0, [0.0, 1.0])
    with pytest.raises(_lib.CgnnError, match="no CPU path"):
        ops.halo_profiles(pos, cen, 8.0, [0.0, 1.0], torch.zeros(10))


def test_statistics_refuse_on_the_host():
    pos = torch.zeros((100, 3))
    with pytest.raises(ValueError, match=r"edges\[0\] must be 0"):
        statistics.halo_profiles(pos, 8.0, [0.5, 1.0])
    with pytest.raises(ValueError, match="33 bins"):
        statistics.halo_profiles(pos, 8.0, np.linspace(0.0, 4.0, MAX_BINS + 2))
    with pytest.raises(ValueError, match="half the box"):
        statistics.halo_profiles(pos, 8.0, [0.0, 5.0])
    with pytest.raises(ValueError, match="one frame"):
        statistics.halo_profiles(torch.zeros((2, 100, 3)), 8.0)
    with pytest.raises(ValueError, match="min_members"):
        statistics.halo_profiles(pos, 8.0, min_members=0)
    with pytest.raises(ValueError, match="values must be"):
        statistics.halo_profiles(pos, 8.0, values=torch.zeros((100, 5)))
    with pytest.raises(ValueError, match="values must be"):
        statistics.halo_profiles(pos, 8.0, values=torch.zeros(99))
    with pytest.raises(ValueError, match="delta"):
        statistics.halo_profiles(pos, 8.0, delta=0.0)
    data = {"Coordinates": torch.zeros((3, 100, 3))}
    with pytest.raises(ValueError, match=r"edges\[0\] must be 0"):
        statistics.rollout_halo_profiles(data, data, 8.0, edges=[0.5, 1.0])
    with pytest.raises(ValueError, match="33 bins"):
        statistics.rollout_halo_profiles(data, data, 8.0, edges=np.linspace(0.0, 4.0, MAX_BINS + 2))
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_halos"):
            statistics.rollout_halo_profiles(data, data, 8.0, max_halos=bad)
    with pytest.raises(ValueError, match="frames must be"):
        statistics.rollout_halo_profiles(data, data, 8.0, frames=[3])
    with pytest.raises(ValueError, match="size_edges"):
        statistics.rollout_halo_profiles(data, data, 8.0, size_edges=[5, 5])
    with pytest.raises(ValueError, match="delta"):
        statistics.rollout_halo_profiles(data, data, 8.0, delta=-200.0)
    # the CPU has no path here either
    with pytest.raises(_lib.CgnnError, match="no CPU path"):
        statistics.halo_profiles(pos, 8.0)
    with pytest.raises(_lib.CgnnError, match="no CPU path"):
        statistics.rollout_halo_profiles(data, data, 8.0)


def test_halo_centres_on_device_is_halo_centres_rounded_and_masks_empty_slots():
    """Plain torch: it runs wherever its tensors live."""
    box = 25.0
    pos = torch.tensor([[24.5, 0.25, 12.0], [1.0, 2.0, 3.0], [5.0, 5.0, 5.0]], dtype=torch.float32)
    size = torch.tensor([4, 0, 1], dtype=torch.int32)
    unit = 2 ** 30 / box
    disp = torch.tensor([[int(4 * 1.0 * unit), int(-4 * 0.5 * unit), 0], [7, 7, 7], [0, 0, 0]], dtype=torch.int64)
    roots = torch.tensor([2, 0, 1], dtype=torch.int64)
    c, valid = statistics.halo_centres_on_device(pos, size, disp, roots, box)
    assert c.dtype == torch.float32 and c.shape == (3, 3) and valid.tolist() == [True, True, False]
    want = statistics.halo_centres(pos[roots[:2]], size[roots[:2]], disp[roots[:2]], box)
    assert torch.equal(c[:2], want.to(torch.float32))
    np.testing.assert_allclose(c[1].numpy(), [0.5, 24.75, 12.0], atol=1e-5)     # wrapped across two faces
    assert c[2].tolist() == [0.0, 0.0, 0.0] and bool(torch.isfinite(c).all())
    # with a frame axis
    cf, vf = statistics.halo_centres_on_device(pos[None], size[None], disp[None], roots[None], box)
    assert torch.equal(cf[0], c) and torch.equal(vf[0], valid)


# ---- the C entry -----------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_built_and_documented():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert name + "(" in header and name in notes
    assert "1 <= num_bins <= 32" in header
    for fn in ("halo_profiles", "check_profile_edges"):
        assert callable(getattr(ops, fn))
    for fn in ("halo_profiles", "rollout_halo_profiles", "so_masses", "default_radial_edges", "halo_centres_on_device"):
        assert callable(getattr(statistics, fn))
    makefile = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "Makefile")).read()
    assert "halo_profiles.hip" in makefile and "FLAGS_halo_profiles := -ffp-contract=off" in makefile
    for doc in ("README.md", "DESIGN.md"):
        assert "halo_profiles" in open(os.path.join(ROOT, doc)).read()
    assert MAX_BINS == 32 and _lib.HALO_PROFILES_MAX_CHANNELS == 4


def test_workspace_size_and_the_host_refusals_of_the_c_entry():
    """The refusals come before any launch: no GPU is needed to meet them, and no pointer is dereferenced."""
    lib = _lib.load()
    wsb = lib.cgnn_halo_profiles_workspace_bytes
    assert wsb(0, 5) == 256 and wsb(5, 0) == 256 and wsb(-1, 5) == 256
    assert wsb(2 ** 31, 5) == 256 and wsb(5, 2 ** 31) == 256
    for n, h in ((1, 1), (4096, 300), (8192, 65), (100, 1000)):
        # per particle and per centre a sorted float4 and a cell id; four tables per set and three for the items over
        # at most 8 n + 1 cell slots; one int per item (up to 8 centres of a cell); every array padded to 256 bytes
        assert 20 * (n + h) <= wsb(n, h) <= 20 * (n + h) + 11 * (8 * n + 1) * 4 + 4 * (h + h // 8 + 1) + 20 * 256
    assert wsb(4096, 300) == wsb(4096, 300)
    assert wsb(8192, 300) > wsb(4096, 300) and wsb(4096, 600) > wsb(4096, 300)
    fake, odd = 1 << 20, (1 << 20) + 4                  # never dereferenced: every call below is refused on the host
    inv, unsup, short = -1, -2, -3                      # CGNN_ERR_INVALID_ARG, _UNSUPPORTED, _WORKSPACE
    half = float(np.float32(0.5))

    def arr(*v):
        return (C.c_float * len(v))(*v)

    def call(pos=fake, n=100, cen=fake, h=7, box=1.0, edges=arr(0.0, 0.1, 0.2), nb=2, q=None, c=0, counts=fake, sums=None,
             w=fake, wb=1 << 30):
        return lib.cgnn_halo_profiles(pos, n, cen, h, box, edges, nb, q, c, counts, sums, w, wb, None)

    for kw in (dict(pos=None), dict(cen=None), dict(edges=None), dict(counts=None), dict(w=None), dict(n=0), dict(n=-4),
               dict(h=0), dict(h=-1), dict(box=0.0), dict(box=-1.0), dict(box=float("inf")), dict(box=float("nan"))):
        assert call(**kw) == inv, kw
    # q and sums go together, with 1 .. 4 channels
    assert call(q=fake, c=1) == inv and call(sums=fake, c=1) == inv
    assert call(q=fake, sums=fake, c=0) == inv and call(q=fake, sums=fake, c=5) == inv
    assert "channels" in lib.cgnn_last_error().decode()
    # bins and edges
    assert call(nb=0) == inv and call(nb=-1) == inv
    assert call(edges=arr(*np.linspace(0, 0.4, MAX_BINS + 2)), nb=MAX_BINS + 1) == inv
    assert "num_bins=33" in lib.cgnn_last_error().decode()
    for e in (arr(-0.1, 0.1, 0.2), arr(0.0, 0.2, 0.2), arr(0.0, 0.3, 0.2), arr(0.0, float("nan"), 0.2),
              arr(0.0, 0.1, float("inf")), arr(0.0, 0.1, float(np.nextafter(np.float32(half), np.float32(1))))):
        assert call(edges=e) == inv
    assert "half the box" in lib.cgnn_last_error().decode()
    # too many particles or centres; a misaligned workspace; a short one (the edges reach exactly half the box)
    assert call(n=2 ** 31) == unsup and call(h=2 ** 31) == unsup
    assert call(w=odd) == inv and "aligned" in lib.cgnn_last_error().decode()
    assert call(edges=arr(0.0, 0.1, half), wb=wsb(100, 7) - 1) == short
    assert call(q=fake, sums=fake, c=4, wb=0) == short
    assert "workspace" in lib.cgnn_last_error().decode()
    # the checks this entry shares with the other pair walks, word for word
    for kw, code, text in (
            (dict(edges=arr(0.0, 0.2, 0.2)), inv, "edges must be finite, non-negative and strictly ascending (edges[2])"),
            (dict(edges=arr(0.0, 0.1, 0.6)), inv, "edges[num_bins]=0.6 exceeds half the box, 0.5"),
            (dict(w=odd), inv, "workspace must be 16-byte aligned"),
            (dict(wb=wsb(100, 7) - 1), short, f"workspace {wsb(100, 7) - 1} < required {wsb(100, 7)} bytes")):
        assert call(**kw) == code and lib.cgnn_last_error().decode() == "cgnn_halo_profiles: " + text, kw
    # the parent's sizes, to the byte
    for n, h, size in ((1, 1, 3584), (4096, 10, 216064), (1000000, 600, 87130368)):
        assert wsb(n, h) == size, (n, h)
