"""CPU: the deposit and binning contracts of ``cgnn_mass_assign`` / ``cgnn_power_bin_ids`` / ``cgnn_power_bins`` as
tests/power_spectrum_checks.py restates them, the host arithmetic of ``statistics.spectra_from_sums``, the host refusals
of ``ops.mass_assign`` / ``ops.power_bins`` and the bookkeeping of the new C entries."""
import math
import os

import numpy as np
import pytest
import torch

import power_spectrum_checks as psc
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib, ops, statistics

ENTRIES = ("cgnn_mass_assign", "cgnn_power_bin_ids", "cgnn_power_bins_workspace_bytes", "cgnn_power_bins")
BOX = 25.0


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("mesh", [2, 4, 5, 9, 16])
def test_every_particle_deposits_exactly_q_cubed_and_no_cell_is_negative(mesh, order):
    x = psc.with_special_positions(psc.uniform(1000, seed=mesh, box=BOX), BOX)
    assert (x == 0).any() and (x == np.float32(BOX)).any()
    grid = psc.mass_assign(x, BOX, mesh, order)
    assert grid.dtype == np.int64 and grid.shape == (mesh, mesh, mesh)
    assert int(grid.sum()) == 1000 * psc.Q ** 3 and psc.Q ** 3 == 2 ** 39 == _lib.MASS_ASSIGN_Q ** 3
    assert grid.min() >= 0                              # the TSC centre weight Q - am - ap never goes below zero
    one = psc.mass_assign(np.full((1, 3), BOX, dtype=np.float32), BOX, mesh, 1)
    assert one[0, 0, 0] == psc.Q ** 3                   # p == L lands in cell 0: a true modulo, no clamp


def _contrast_pair(mesh, n=500):
    a = psc.density_contrast(psc.mass_assign(psc.uniform(n, 1, BOX), BOX, mesh, 2), n)
    b = psc.density_contrast(psc.mass_assign(psc.uniform(n, 2, BOX), BOX, mesh, 2), n)
    return a, b


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("mesh", [4, 5, 8, 9])
def test_half_array_with_hermitian_weights_equals_the_full_cube(mesh, order):
    """Odd meshes have no Nyquist plane and even ones have one that is its own conjugate: the two places where the
    weight goes wrong first.  Edges [0, 1000) cover every mode but n = 0."""
    a, b = _contrast_pair(mesh)
    most = np.linspace(0.0, 1000.0, _lib.POWER_MAX_BINS + 1)               # as many bins as the kernel takes
    for edges in (np.array([0.0, 1000.0]), statistics.default_k_edges(mesh).numpy(), most,
                  np.array([0.0, 1.0, 2.0, 3.5, 1000.0])):
        edges = np.array(ops.check_power_edges(edges, "test"))               # the float32 values the kernel bins by
        modes, sums = psc.power_bins(np.fft.rfftn(a), np.fft.rfftn(b), mesh, order, edges)
        modes_full, sums_full = psc.power_bins_full(np.fft.fftn(a), np.fft.fftn(b), mesh, order, edges)
        assert (modes == modes_full).all()
        if edges[-1] == 1000.0:
            assert modes.sum() == mesh ** 3 - 1
        for row in range(4):
            assert np.abs(sums[row] - sums_full[row]).max() <= 1e-12 * np.abs(sums_full[row]).max()
    ids = psc.bin_ids(mesh, [0.0, 1000.0])
    assert ids.shape == (mesh, mesh, mesh // 2 + 1) and ids[0, 0, 0] == -1 and (ids.reshape(-1)[1:] == 0).all()


def test_an_edge_on_an_integer_frequency_belongs_to_the_upper_bin():
    ids = psc.bin_ids(8, ops.check_power_edges([1.0, 2.0, 3.0], "test"))
    assert ids[1, 0, 0] == 0 and ids[2, 0, 0] == 1 and ids[0, 0, 3] == -1 and ids[7, 0, 0] == 0    # index 7 is n = -1
    assert ids[1, 1, 1] == 0 and ids[0, 0, 0] == -1                                                # n2 = 3 < 4


@pytest.mark.parametrize("order", [1, 2, 3])
def test_a_simple_cubic_lattice_has_no_power_below_its_own_frequency(order):
    """8^3 points, one every second cell of a 16^3 mesh: the only modes with power are multiples of 8 per axis, and
    [0.5, 7.5) holds none of them.  Every deposit puts the same integers around every point and M^3 / (N Q^3) = 2^-36
    is a power of two, so the contrast is exact and the transform cancels exactly."""
    g = np.arange(8, dtype=np.float32) * np.float32(2.0)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    delta = psc.density_contrast(psc.mass_assign(pts, 16.0, 16, order), 512)
    assert psc.Q == _lib.MASS_ASSIGN_Q
    modes, sums = psc.power_bins(np.fft.rfftn(delta), None, 16, order, [0.5, 7.5])
    assert modes.tolist() == [1790] and sums[0, 0] == 0.0
    assert np.isnan(sums[1:3]).all()
    sp = statistics.spectra_from_sums(modes, sums, 512, None, 16.0, 16, [0.5, 7.5], subtract_shot_noise=False)
    assert sp["modes"].tolist() == [1790] and sp["power"].tolist() == [0.0]
    # all seven default bins below the lattice's frequency, and only the shot noise is left to subtract
    edges = statistics.default_k_edges(16)[:8]
    sp = statistics.spectra_from_sums(*psc.power_bins(np.fft.rfftn(delta), None, 16, order, edges.numpy()), 512, None,
                                      16.0, 16, edges)
    assert int(sp["modes"].sum()) == 1790 and sp["power"].tolist() == [-(16.0 ** 3) / 512] * 7


def _spectra(x, y, mesh, order=2, edges=None, **kw):
    edges = psc.default_k_edges(mesh) if edges is None else edges
    a = np.fft.rfftn(psc.density_contrast(psc.mass_assign(x, BOX, mesh, order), x.shape[0]))
    b = None if y is None else np.fft.rfftn(psc.density_contrast(psc.mass_assign(y, BOX, mesh, order), y.shape[0]))
    modes, sums = psc.power_bins(a, b, mesh, order, edges)
    return statistics.spectra_from_sums(modes, sums, x.shape[0], None if y is None else y.shape[0], BOX, mesh, edges, **kw)


def test_cross_of_a_set_with_itself_is_its_auto_spectrum():
    x = psc.uniform(2000, 5, BOX)
    both = _spectra(x, x, 16, subtract_shot_noise=False)
    auto = _spectra(x, None, 16, subtract_shot_noise=False)
    assert set(auto) == {"k_lo", "k_hi", "k_mean", "modes", "power"}
    assert set(both) == set(auto) | {"power_b", "cross", "r", "transfer"}
    for key in ("power_b", "cross"):
        assert torch.equal(both[key], auto["power"]) and both[key].dtype == torch.float64
    np.testing.assert_allclose(both["r"].numpy(), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(both["transfer"].numpy(), 1.0, rtol=0, atol=1e-15)
    sub = _spectra(x, x, 16)
    np.testing.assert_allclose((auto["power"] - sub["power"]).numpy(), BOX ** 3 / 2000, rtol=1e-12)
    assert torch.equal(sub["cross"], both["cross"]) and torch.equal(sub["r"], both["r"])    # only the auto spectra lose it
    assert int(auto["modes"].sum()) == int(psc.power_bins_full(np.zeros((16,) * 3), None, 16, 0, psc.default_k_edges(16))[0].sum())


def test_spectra_from_sums_units_empty_bins_and_cauchy_schwarz():
    x, y = psc.uniform(1500, 7, BOX), psc.uniform(1500, 8, BOX)
    edges = np.array([0.5, 0.75, 1.25, 2.5, 8.5])          # [0.5, 0.75) holds no integer n2: an empty bin
    sp = _spectra(x, y, 16, edges=edges)
    kf = 2 * math.pi / BOX
    np.testing.assert_allclose(sp["k_lo"].numpy(), edges[:-1] * kf, rtol=1e-12)
    np.testing.assert_allclose(sp["k_hi"].numpy(), edges[1:] * kf, rtol=1e-12)
    assert sp["modes"].tolist()[:3] == [0, 6, 12 + 8 + 6 + 24 + 24]             # n2 = 1; n2 = 2 .. 6
    assert sp["modes"].dtype == torch.int64
    for key in ("power", "power_b", "cross", "r", "transfer", "k_mean"):
        assert math.isnan(float(sp[key][0])), key
    assert float(sp["k_mean"][1]) == kf
    assert bool((sp["k_mean"][1:] >= sp["k_lo"][1:]).all()) and bool((sp["k_mean"][1:] < sp["k_hi"][1:]).all())
    assert bool((sp["r"][1:].abs() <= 1.0).all())
    # two independent uniform sets: shot-noise dominated, the subtracted spectra scatter around zero
    raw = _spectra(x, y, 16, edges=edges, subtract_shot_noise=False)
    assert bool((raw["power"][1:] > 0).all())
    # P = L^3 S / modes / M^6 on the first filled bin, by hand
    a = np.fft.rfftn(psc.density_contrast(psc.mass_assign(x, BOX, 16, 2), 1500))
    s = psc.power_bins(a, None, 16, 2, edges)[1][0, 1]
    np.testing.assert_allclose(float(raw["power"][1]), BOX ** 3 * s / 6 / 16 ** 6, rtol=1e-14)
    # frames: a leading axis passes through
    m2 = torch.stack([sp["modes"], sp["modes"]])
    s2 = torch.from_numpy(np.stack([psc.power_bins(a, a, 16, 2, edges)[1]] * 2))
    assert statistics.spectra_from_sums(m2, s2, 1500, 1500, BOX, 16, edges)["power"].shape == (2, 4)
    with pytest.raises(ValueError):
        statistics.spectra_from_sums(m2, s2[:, :3], 1500, 1500, BOX, 16, edges)


@pytest.mark.parametrize("subtract", [True, False])
def test_spectra_from_sums_equals_the_definitions_written_out_in_numpy(subtract):
    """P, cross, r and T against psc.spectra, which shares no code with the package: two frames, unequal set sizes, an
    empty bin, and bins where the subtraction leaves a spectrum negative (T is nan there, and only there)."""
    edges = np.array([0.5, 0.75, 1.5, 2.5, 4.5, 8.5])
    modes, sums = [], []
    for seed in (3, 4):
        x = psc.uniform(1500, seed, BOX)
        y = np.mod(x[:1200] + np.float32(0.4) * psc.uniform(1200, seed + 10, 1.0), np.float32(BOX)).astype(np.float32)
        a = np.fft.rfftn(psc.density_contrast(psc.mass_assign(x, BOX, 16, 2), 1500))
        b = np.fft.rfftn(psc.density_contrast(psc.mass_assign(y, BOX, 16, 2), 1200))
        m, s = psc.power_bins(a, b, 16, 2, edges)
        modes.append(m)
        sums.append(s)
    modes, sums = np.stack(modes), np.stack(sums)
    got = statistics.spectra_from_sums(modes, sums, 1500, 1200, BOX, 16, edges, subtract)
    want = psc.spectra(modes, sums, 1500, 1200, BOX, 16, subtract)
    for key, value in want.items():
        assert got[key].shape == (2, 5)
        np.testing.assert_allclose(got[key].numpy(), value, rtol=1e-13, atol=0, equal_nan=True, err_msg=key)
    assert np.isnan(want["r"][:, 0]).all() and np.isfinite(want["r"][:, 1:]).all() and (want["r"][:, 1:] > 0.5).all()
    if subtract:
        assert np.isnan(want["transfer"][:, 1:]).any() and np.isfinite(want["transfer"][:, 1:]).any()
    else:
        assert np.isfinite(want["transfer"][:, 1:]).all()


def test_uniform_points_have_the_shot_noise_spectrum_within_four_deviations():
    """8192 uniform points, M = 32, CIC, seed 0: P N / L^3 before the shot-noise subtraction is 1 for a Poisson sample,
    with a relative scatter of sqrt(2 / modes) per bin (|delta_k|^2 of a Gaussian mode is exponential, and a bin of
    `modes` modes of the full cube holds modes / 2 independent ones).  Within 4 of those in every default bin with
    upper edge <= M / 4; the largest deviation on this draw is printed.  Bins beyond M / 4 are left out: the CIC window
    is deconvolved but its aliases are not, and they lift the spectrum there."""
    n, mesh = 8192, 32
    sp = _spectra(psc.uniform(n, 0, BOX), None, mesh, subtract_shot_noise=False)
    low = sp["k_hi"] * (BOX / (2 * math.pi)) <= mesh / 4 + 1e-9
    assert int(low.sum()) == 7                          # upper edges 1.5 .. 7.5
    dev = ((sp["power"] * n / BOX ** 3 - 1.0).abs() / torch.sqrt(2.0 / sp["modes"].double()))[low]
    print(f"largest |P N / L^3 - 1| / sqrt(2 / modes): {float(dev.max()):.2f}")
    assert bool((dev < 4.0).all()), dev


def test_default_k_edges():
    e = statistics.default_k_edges(16)
    assert e.dtype == torch.float64 and e.tolist() == [0.5 + i for i in range(9)]
    assert statistics.default_k_edges(5).tolist() == [0.5, 1.5, 2.5]
    np.testing.assert_array_equal(e.numpy(), psc.default_k_edges(16))


@pytest.mark.parametrize("kw", [
    dict(mesh=1), dict(mesh=513), dict(mesh=16.5), dict(order=0), dict(order=4), dict(box_size=0.0), dict(box_size=-1.0),
    dict(box_size=float("nan")), dict(pos=torch.empty(0, 3)), dict(pos=torch.rand(10, 2)),
])
def test_mass_assign_refuses_on_the_host_before_any_device_work(kw):
    args = dict(pos=torch.rand(10, 3), box_size=1.0, mesh=16, order=2)      # a host tensor: refused later, were the rest right
    args.update(kw)
    with pytest.raises(ValueError):
        ops.mass_assign(**args)


def test_mass_assign_refuses_more_than_2_to_the_24_particles_and_has_no_cpu_path():
    big = torch.zeros(1, 3).expand((1 << 24) + 1, 3)                         # a view: no memory behind it
    with pytest.raises(ValueError, match="2\\^24"):
        ops.mass_assign(big, 1.0, 16)
    for mesh, order in ((2, 1), (512, 3)):                                   # the limits pass; the host tensor does not
        with pytest.raises(_lib.CgnnError):
            ops.mass_assign(torch.rand(10, 3), 1.0, mesh, order)


@pytest.mark.parametrize("edges", [
    [0.5], np.linspace(0.0, 100.0, 258), [0.0, float("nan"), 3.0], [0.0, float("inf")], [-0.5, 2.0], [0.5, 1.5, 1.5],
    [0.5, 2.5, 1.5], [1.0, 1.0 + 1e-10],
])
def test_power_bins_refuses_bad_edges_on_the_host(edges):
    dk = torch.zeros(8, 8, 5, dtype=torch.complex128)
    with pytest.raises(ValueError):
        ops.power_bins(dk, 8, 2, edges)
    with pytest.raises(ValueError):
        ops.PowerPlan(8, edges, "cuda")
    with pytest.raises(ValueError):
        statistics.power_spectrum(torch.rand(10, 3), 1.0, 8, edges)


def test_power_bins_refuses_bad_orders_meshes_and_host_tensors():
    dk = torch.zeros(8, 8, 5, dtype=torch.complex128)
    for mesh, order in ((8, 4), (8, -1), (1, 2), (600, 2)):
        with pytest.raises(ValueError):
            ops.power_bins(dk, mesh, order, [0.5, 1.5])
    with pytest.raises(_lib.CgnnError):                                      # everything passes but the host tensor
        ops.power_bins(dk, 8, 0, [0.5, 1.5])
    with pytest.raises(ValueError):
        statistics.power_spectrum(torch.rand(10, 3), 1.0, 8, order=0)
    with pytest.raises(ValueError):
        statistics.rollout_power_spectra({"Coordinates": torch.rand(3, 10, 3)}, {"Coordinates": torch.rand(3, 10, 3)},
                                         1.0, 8, frames=[3])
    with pytest.raises(ValueError):
        statistics.rollout_power_spectra({"Coordinates": torch.rand(3, 10, 3)}, {"Coordinates": torch.rand(3, 11, 3)},
                                         1.0, 8)


def test_new_entries_are_declared_exported_built_and_documented():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert name + "(" in header and name in notes
    assert callable(ops.mass_assign) and callable(ops.power_bins) and callable(ops.PowerPlan.of)
    assert callable(statistics.power_spectrum) and callable(statistics.rollout_power_spectra)
    makefile = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "Makefile")).read()
    assert "power_spectrum.hip" in makefile and "FLAGS_power_spectrum := -ffp-contract=off" in makefile


def test_workspace_size_is_a_function_of_frames_and_bins():
    lib = _lib.load()
    one = lib.cgnn_power_bins_workspace_bytes(1, 16)
    # 64 slices per bin, four float64 sums and one count each, behind the window table of at most 257 doubles
    assert 16 * 64 * 5 * 8 <= one <= 16 * 64 * 5 * 8 + 257 * 8 + 3 * 256
    assert lib.cgnn_power_bins_workspace_bytes(3, 16) > 2 * (one - 257 * 8 - 3 * 256)
    assert lib.cgnn_power_bins_workspace_bytes(0, 16) == 256 and lib.cgnn_power_bins_workspace_bytes(1, 257) == 256
