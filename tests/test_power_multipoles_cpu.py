"""CPU: the contracts of ``cgnn_redshift_positions`` and ``cgnn_power_multipoles`` as tests/multipole_checks.py restates
them -- the half array against a brute force over the full cube, the Legendre sums of cubic shells, white noise up to
the Nyquist frequency with and without interlacing, the Kaiser ratio of a displaced lattice -- the host arithmetic of
``statistics.multipoles_from_sums``, the Python-level refusals and those of the C entries, all before any device work."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import multipole_checks as mc
import power_spectrum_checks as psc
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib, ops, statistics

ENTRIES = ("cgnn_redshift_positions", "cgnn_power_multipoles_workspace_bytes", "cgnn_power_multipoles")
F32 = np.float32


# ---- the shell sums ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [4, 5, 9, 16])
def test_half_array_sums_equal_a_brute_force_over_the_full_cube(mesh):
    """Bins that stay below |n_c| = M/2 on every axis (n2 < (M/2)^2), where the Nyquist convention plays no part."""
    edges = np.linspace(0.5, mesh / 2.0, 4)
    fields = [np.random.default_rng(seed).standard_normal((mesh,) * 3) for seed in range(4)]
    half = [np.fft.rfftn(f) for f in fields]
    full = [np.fft.fftn(f) for f in fields]
    for los in range(3):
        for order in (0, 2):
            for inter in (False, True):
                h = half if inter else half[:2] + [None, None]
                g = full if inter else full[:2] + [None, None]
                modes, sums = mc.power_multipoles(h[0], h[1], mesh, order, los, edges, h[2], h[3])
                modes_f, sums_f = mc.power_multipoles_full(g[0], g[1], mesh, order, los, edges, g[2], g[3])
                assert modes.sum() > 0 and np.array_equal(modes, modes_f)
                for row in range(mc.ROWS):
                    scale = max(np.abs(sums_f[row]).max(), 1.0)
                    assert np.abs(sums[row] - sums_f[row]).max() <= 1e-12 * scale, (los, order, inter, row)


def test_plain_rows_are_the_sums_of_power_bins():
    mesh, edges = 9, psc.default_k_edges(9)
    a, b = mc.real_field_modes(mesh, 0), mc.real_field_modes(mesh, 1)
    modes, sums = mc.power_multipoles(a, b, mesh, 2, 1, edges)
    want_modes, want = psc.power_bins(a, b, mesh, 2, edges)
    assert np.array_equal(modes, want_modes)
    np.testing.assert_allclose(sums[[0, 3, 6, 9]], want, rtol=1e-14)
    _, alone = mc.power_multipoles(a, None, mesh, 2, 1, edges)
    assert np.isnan(alone[3:9]).all() and np.array_equal(alone[[0, 1, 2, 9, 10, 11]], sums[[0, 1, 2, 9, 10, 11]])


def test_legendre_sums_of_cubic_shells():
    """sum h L2 = 0 over a shell with the cube's symmetry (mu^2 averages 1/3); the shell n = 1 has mu^4 averaging 1/3, so
    L4 averages (35/3 - 10 + 3) / 8 = 7/12."""
    mesh = 9                                                    # odd: every shell of the default bins is symmetric
    edges = [math.sqrt(v - 0.5) for v in range(1, 14)]         # one bin per n2 = 1 .. 12
    a = mc.real_field_modes(mesh, 3)
    for los in range(3):
        modes, sums = mc.power_multipoles(a, None, mesh, 0, los, edges)
        assert modes.tolist()[:6] == [6, 12, 8, 6, 24, 24] and modes[6] == 0          # no n2 = 7
        assert np.abs(sums[10]).max() <= 1e-12 * modes.max()
        sp = mc.multipoles(modes, sums, 1, None, 1.0, mesh)
        assert abs(sp["legendre_mean_4"][0] - 7.0 / 12.0) <= 1e-14
        assert np.isnan(sp["legendre_mean_4"][6]) and np.isnan(sp["power_0"][6])


# ---- white noise up to the Nyquist frequency -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("order", [2, 3])
def test_white_noise_keeps_every_bin_to_nyquist_when_interlaced(seed, order):
    """8192 uniform points, M = 32, the default bins: |P_l N / L^3 - (2 l + 1) legendre_mean_l| stays within 4 Poisson
    sigma = 4 sqrt(2 (2 l + 1) / modes) in every bin and for l = 0, 2, 4 (measured with float weights: at most 3.21 /
    2.16 / 2.49).  Not interlaced, the same frame's worst l = 0 bin exceeds 8: a kernel that ignores a2 fails."""
    n, mesh, box = 8192, 32, 1.0
    pos = mc.white_noise(n, seed, box)
    edges = psc.default_k_edges(mesh)
    worst_plain = None
    for inter in (True, False):
        modes, sums = mc.frame_sums(pos, box, mesh, order, 2, edges, interlace=inter)
        sp = mc.multipoles(modes, sums, n, None, box, mesh, subtract_shot_noise=False)
        for ell in (0, 2, 4):
            mean = 1.0 if ell == 0 else sp[f"legendre_mean_{ell}"]
            dev = np.abs(sp[f"power_{ell}"] * n / box ** 3 - (2 * ell + 1) * mean) / np.sqrt(2.0 * (2 * ell + 1) / modes)
            print(f"seed {seed} order {order} interlace {inter} l = {ell}: worst {dev.max():.2f} sigma")
            if inter:
                assert dev.max() <= 4.0, (ell, dev)
            elif ell == 0:
                worst_plain = dev.max()
    assert worst_plain > 8.0


# ---- the Kaiser ratio of a displaced lattice ---------------------------------------------------------------------------
def _lattice_frames(n0, amplitude=1e-3, box=1.0, side=16):
    i = (np.arange(side) + 0.25) * box / side
    q = np.stack(np.meshgrid(i, i, i, indexing="ij"), axis=-1).reshape(-1, 3)
    n0 = np.asarray(n0, dtype=np.float64)
    psi = amplitude * box * (n0 / np.linalg.norm(n0)) * np.sin(2.0 * np.pi * (q @ n0) / box)[:, None]
    return (q + psi).astype(np.float32), (q + 0.6 * psi).astype(np.float32)


@pytest.mark.parametrize("los", [0, 2])
@pytest.mark.parametrize("n0", [(1, 1, 2), (2, 0, 1), (1, 2, 2)])
def test_kaiser_ratio_of_a_displaced_lattice(n0, los):
    """pos = q + psi, pos_prev = q + 0.6 psi, velocity_scale / dt = 1.5: the displacement along the line of sight grows
    by c = 0.6, so the amplitude of mode n0 grows by 1 + c mu0^2 (measured: within 9.3e-4)."""
    box, mesh = 1.0, 32
    pos, prev = _lattice_frames(n0)
    red = mc.redshift_positions(pos, prev, box, los, mc.redshift_shift(2.0, 3.0))
    real_k, red_k = mc.contrast_modes(pos, box, mesh, 2), mc.contrast_modes(red, box, mesh, 2)
    mu2 = n0[los] ** 2 / float(np.dot(n0, n0))
    ratio = abs(red_k[n0]) / abs(real_k[n0])
    print(f"n0 {n0} los {los}: ratio {ratio:.6f}, 1 + c mu^2 = {1 + 0.6 * mu2:.6f}")
    assert abs(ratio - (1.0 + 0.6 * mu2)) <= 3e-3


def test_kaiser_ratio_is_exactly_one_without_a_line_of_sight_displacement():
    box, mesh = 1.0, 32
    pos, prev = _lattice_frames((0, 3, 0))
    real_k = mc.contrast_modes(pos, box, mesh, 2)
    for los in (0, 2):                                   # psi lies along y
        red = mc.redshift_positions(pos, prev, box, los, 1.5)
        assert np.array_equal(red, pos)
        assert abs(mc.contrast_modes(red, box, mesh, 2)[0, 3, 0]) / abs(real_k[0, 3, 0]) == 1.0
    pos, prev = _lattice_frames((1, 1, 2))
    for los in range(3):                                 # velocity_scale = 0
        assert np.array_equal(mc.redshift_positions(pos, prev, box, los, mc.redshift_shift(0.5, 0.0)), pos)


# ---- redshift positions ------------------------------------------------------------------------------------------------
def test_a_pair_across_a_box_face_moves_by_its_displacement():
    box = 10.0
    pos = np.array([[0.25, 5.0, 9.75], [9.5, 5.0, 0.5]], dtype=np.float32)
    prev = np.array([[9.75, 5.0, 0.25], [0.5, 5.0, 9.5]], dtype=np.float32)       # steps of +0.5, -1 (x); -0.5, +1 (z)
    out = mc.redshift_positions(pos, prev, box, 0, 2.0)
    np.testing.assert_allclose(out[:, 0], [1.25, 7.5], atol=1e-5)
    assert np.array_equal(out[:, 1:], pos[:, 1:])
    out = mc.redshift_positions(pos, prev, box, 2, 1.0)
    np.testing.assert_allclose(out[:, 2], [9.25, 1.5], atol=1e-5)
    out = mc.redshift_positions(pos, prev, box, 2, 0.5)             # 9.75 - 0.25 = 9.5 and 0.5 + 0.5 = 1.0
    np.testing.assert_allclose(out[:, 2], [9.5, 1.0], atol=1e-5)


def test_outputs_stay_in_the_box_and_equal_positions_come_back():
    box = 25.0
    rng = np.random.default_rng(5)
    pos = (rng.random((4000, 3)) * box).astype(np.float32)
    pos = np.where(pos >= F32(box), F32(0), pos)
    prev = psc.with_special_positions((rng.random((4000, 3)) * box).astype(np.float32), box)
    pos[:4] = [(0, 0, 0), (box, box, box), (0, box, 0), (box, 0, box)]
    for shift in (0.0, 1.0, -1.0, 7.3, -40.0, 250.0, 1e30, -1e30):
        for los in range(3):
            out = mc.redshift_positions(pos, prev, box, los, shift)
            assert out.dtype == np.float32 and (out >= 0).all() and (out <= F32(box)).all(), (shift, los)
    inside = pos[4:]
    for los in range(3):
        assert np.array_equal(mc.redshift_positions(inside, inside, box, los, 3.0).view(np.int32), inside.view(np.int32))
    assert mc.redshift_positions(pos[:4], pos[:4], box, 1, 3.0)[:, 1].tolist() == [0, 0, 0, 0]      # L lands on 0
    bad = np.array([[np.nan, 1, 2], [np.inf, 1, 2], [1, 1, 2], [1, 1, 2]], dtype=np.float32)
    bad_prev = np.array([[1, 1, 2], [1, 1, 2], [np.nan, 1, 2], [-np.inf, 1, 2]], dtype=np.float32)
    out = mc.redshift_positions(bad, bad_prev, box, 0, 1.0)
    assert out[:, 0].tolist() == [0, 0, 0, 0] and np.array_equal(out[:, 1:], bad[:, 1:])


def test_interlace_shift_is_half_a_cell_wrapped():
    box, mesh = 25.0, 16
    pos = np.array([[0.0, 25.0, 24.5], [24.21875, 24.3, 12.0]], dtype=np.float32)
    out = mc.interlace_shift(pos, box, mesh)
    half = F32(25.0 / 32)
    assert out.dtype == np.float32 and (out >= 0).all() and (out < F32(box)).all()
    assert out[0].tolist() == [float(half), float(half), float(F32(24.5) + half - F32(25.0))]
    assert out[1, 0] == 0.0                                  # 24.21875 + 0.78125 = L exactly
    got = ops.interlace_shift(torch.from_numpy(pos), box, mesh)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), out)
    big = psc.with_special_positions(psc.uniform(5000, 2, box), box)
    assert np.array_equal(ops.interlace_shift(torch.from_numpy(big), box, 9).numpy(), mc.interlace_shift(big, box, 9))


# ---- host arithmetic -----------------------------------------------------------------------------------------------------
def test_multipoles_from_sums_against_the_definitions():
    mesh, box, n_a, n_b = 9, 25.0, 1000, 900
    edges = [0.5, 1.5, 2.5, 2.55, 3.5]                       # a bin without modes
    a, b = mc.real_field_modes(mesh, 0), mc.real_field_modes(mesh, 1)
    modes, sums = mc.power_multipoles(a, b, mesh, 2, 0, edges, mc.real_field_modes(mesh, 2), mc.real_field_modes(mesh, 3))
    assert modes[2] == 0
    stacked_m, stacked_s = np.stack([modes, modes]), np.stack([sums, 2.0 * sums])
    for subtract in (True, False):
        got = statistics.multipoles_from_sums(stacked_m, stacked_s, n_a, n_b, box, mesh, edges, subtract)
        want = mc.multipoles(stacked_m, stacked_s, n_a, n_b, box, mesh, subtract)
        assert set(got) == {"k_lo", "k_hi", "k_mean", "modes", "legendre_mean_2", "legendre_mean_4", "r", "transfer"} | {
            f"{name}_{ell}" for name in ("power", "power_b", "cross") for ell in (0, 2, 4)}
        for key, w in want.items():
            assert got[key].shape == (2, 4) and got[key].dtype == torch.float64
            np.testing.assert_allclose(got[key].numpy(), w, rtol=1e-13, equal_nan=True, err_msg=key)
            assert np.isnan(got[key].numpy()[:, 2]).all()
        assert torch.equal(got["modes"], torch.from_numpy(stacked_m))
        k = np.asarray(edges, dtype=np.float32).astype(np.float64) * (2 * np.pi / box)
        np.testing.assert_allclose(got["k_lo"].numpy(), k[:-1], rtol=1e-15)
        np.testing.assert_allclose(got["k_hi"].numpy(), k[1:], rtol=1e-15)
    # the shot noise leaves l = 0 only
    on = statistics.multipoles_from_sums(modes, sums, n_a, n_b, box, mesh, edges, True)
    off = statistics.multipoles_from_sums(modes, sums, n_a, n_b, box, mesh, edges, False)
    keep = torch.from_numpy(modes > 0)
    np.testing.assert_allclose((off["power_0"] - on["power_0"])[keep].numpy(), box ** 3 / n_a, rtol=1e-9)
    np.testing.assert_allclose((off["power_b_0"] - on["power_b_0"])[keep].numpy(), box ** 3 / n_b, rtol=1e-9)
    for key in ("power_2", "power_4", "power_b_2", "power_b_4", "cross_0", "cross_2", "cross_4", "r"):
        assert torch.equal(on[key][keep], off[key][keep]), key
    # one set: no second set's keys; the monopole is spectra_from_sums' power
    alone = statistics.multipoles_from_sums(modes, sums, n_a, None, box, mesh, edges)
    assert not any(k.startswith(("power_b", "cross")) or k in ("r", "transfer") for k in alone)
    four = torch.from_numpy(sums[[0, 3, 6, 9]])
    plain = statistics.spectra_from_sums(modes, four, n_a, n_b, box, mesh, edges)
    for mine, theirs in (("power_0", "power"), ("power_b_0", "power_b"), ("cross_0", "cross"), ("r", "r"),
                         ("transfer", "transfer"), ("k_mean", "k_mean")):
        assert torch.allclose(on[mine][keep], plain[theirs][keep], rtol=0.0, atol=0.0, equal_nan=True), mine


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_python_level_refusals_come_before_any_device_work():
    pos, prev = torch.rand(10, 3), torch.rand(10, 3)
    for kw in (dict(los=3), dict(los=-1), dict(los=True), dict(los=1.5), dict(dt=0.0), dict(dt=-1.0),
               dict(dt=float("nan")), dict(dt=float("inf")), dict(velocity_scale=float("inf")),
               dict(velocity_scale=1e30, dt=1e-30), dict(box_size=0.0), dict(box_size=float("nan"))):
        args = dict(dt=1.0, box_size=1.0, los=2, velocity_scale=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.redshift_positions(pos, prev, **args)
    for p, q in ((pos, torch.rand(11, 3)), (torch.rand(10, 2), torch.rand(10, 2)), (torch.rand(3), torch.rand(3)),
                 (torch.rand(2, 10, 3), torch.rand(10, 3))):
        with pytest.raises(ValueError):
            ops.redshift_positions(p, q, 1.0, 1.0)
    with pytest.raises(_lib.CgnnError):                              # everything passes but the host tensor
        ops.redshift_positions(pos, prev, 1.0, 1.0)
    for kw in (dict(mesh=1), dict(mesh=513), dict(box_size=-1.0)):
        args = dict(box_size=1.0, mesh=8)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.interlace_shift(pos, **args)
    with pytest.raises(ValueError):
        ops.interlace_shift(pos.double(), 1.0, 8)

    dk = torch.zeros(8, 8, 5, dtype=torch.complex128)
    for kw in (dict(mesh=1), dict(order=4), dict(order=-1), dict(los=3), dict(los=None), dict(k_edges=[0.5]),
               dict(k_edges=[1.5, 0.5]), dict(shifted_b=dk), dict(shifted_b=dk, delta_k_b=dk),
               dict(shifted=dk, delta_k_b=dk)):
        args = dict(mesh=8, order=2, k_edges=[0.5, 1.5], los=2)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.power_multipoles(dk, **args)
    for kw in (dict(), dict(shifted=dk.to(torch.complex64)), dict(delta_k_b=torch.zeros(8, 8, 4, dtype=torch.complex128)),
               dict(shifted=dk[None])):
        with pytest.raises(_lib.CgnnError):
            ops.power_multipoles(dk, 8, 2, [0.5, 1.5], **kw)

    frames = torch.rand(3, 10, 3)
    for kw in (dict(pos_prev=frames), dict(pos_prev=frames, dt=0.0), dict(pos_prev=frames, dt=1.0, los=4),
               dict(pos_prev=frames[:2], dt=1.0), dict(order=0), dict(mesh=1), dict(box_size=0.0),
               dict(pos_prev=frames, dt=1.0, velocity_scale=float("nan")), dict(pos_b_prev=frames),
               dict(pos_b=frames, pos_b_prev=frames), dict(pos_b=frames, pos_prev=frames, dt=1.0),
               dict(pos_b=frames[0]), dict(pos_b=frames[:2]), dict(k_edges=[2.0, 1.0])):
        args = dict(box_size=1.0, mesh=8)
        args.update(kw)
        with pytest.raises(ValueError):
            statistics.power_multipoles(frames, **args)
    roll, truth = {"Coordinates": torch.rand(4, 10, 3)}, {"Coordinates": torch.rand(3, 10, 3)}
    for kw in (dict(frames=[3]), dict(frames=[0]), dict(frames=[-1]), dict(frames=[]), dict(dt=0.0), dict(los=5),
               dict(velocity_scale=float("inf")), dict(order=4), dict(mesh=1000)):
        args = dict(box_size=1.0, mesh=8, dt=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            statistics.rollout_redshift_spectra(roll, truth, **args)
    with pytest.raises(ValueError):
        statistics.rollout_redshift_spectra(roll, {"Coordinates": torch.rand(3, 11, 3)}, 1.0, 8, 0.1)
    with pytest.raises(ValueError):                                  # one frame: none has a predecessor
        statistics.rollout_redshift_spectra({"Coordinates": torch.rand(1, 10, 3)}, truth, 1.0, 8, 0.1)
    with pytest.raises(ValueError):
        statistics.multipoles_from_sums(torch.zeros(3, dtype=torch.int64), torch.zeros(4, 3), 10, None, 1.0, 8,
                                        [0.5, 1.5, 2.5, 3.5])


# ---- the C entries -----------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_built_and_documented():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert name + "(" in header and name in notes
    assert "rintf(fl32(d / L))" in header and "sincospi" in header and "+mesh/2" in header
    for fn in ("redshift_positions", "interlace_shift", "power_multipoles", "check_los"):
        assert callable(getattr(ops, fn))
    for fn in ("power_multipoles", "rollout_redshift_spectra", "multipoles_from_sums"):
        assert callable(getattr(statistics, fn))
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "power_multipoles" in text and "redshift_positions" in text
    assert os.path.exists(os.path.join(ROOT, "scripts", "time_power_multipoles.py"))
    assert _lib.POWER_MULTIPOLE_SUMS == mc.ROWS == 12


def test_workspace_size_and_the_host_refusals_of_the_c_entries():
    """The refusals come before any launch: no GPU is needed to meet them, and no pointer is dereferenced."""
    lib = _lib.load()
    wsb = lib.cgnn_power_multipoles_workspace_bytes
    one = wsb(1, 16)
    # 64 slices per bin, twelve float64 sums and one count each, behind the window table of at most 257 doubles
    assert 16 * 64 * 13 * 8 <= one <= 16 * 64 * 13 * 8 + 257 * 8 + 3 * 256
    assert wsb(3, 16) > 2 * (one - 257 * 8 - 3 * 256)
    assert wsb(0, 16) == 256 and wsb(1, 257) == 256 and wsb(-1, 4) == 256 and wsb(1, 0) == 256
    fake, odd = 1 << 20, (1 << 20) + 8                  # never dereferenced: every call below is refused on the host
    inv, unsup, short = -1, -2, -3                      # CGNN_ERR_INVALID_ARG, _UNSUPPORTED, _WORKSPACE

    def multipoles(a=fake, b=None, a2=None, b2=None, frames=2, mesh=8, order=2, los=2, perm=fake, start=fake, nb=4,
                   modes=fake, sums=fake, w=fake, wb=1 << 30):
        return lib.cgnn_power_multipoles(a, b, a2, b2, frames, mesh, order, los, perm, start, nb, modes, sums, w, wb, None)

    for kw in (dict(a=None), dict(perm=None), dict(start=None), dict(modes=None), dict(sums=None), dict(w=None),
               dict(frames=0), dict(frames=-1), dict(mesh=1), dict(mesh=513), dict(order=-1), dict(order=4), dict(nb=0),
               dict(nb=257), dict(los=-1), dict(los=3)):
        assert multipoles(**kw) == inv, kw
    assert "los=3" in lib.cgnn_last_error().decode()
    # b2 goes with b and a2, and must be there when both are
    assert multipoles(b2=fake) == inv and multipoles(b2=fake, b=fake) == inv and multipoles(b2=fake, a2=fake) == inv
    assert multipoles(a2=fake, b=fake) == inv and "b2" in lib.cgnn_last_error().decode()
    for name in ("a", "b", "a2", "b2", "w"):
        kw = dict(b=fake, a2=fake, b2=fake)
        kw[name] = odd
        assert multipoles(**kw) == inv and "aligned" in lib.cgnn_last_error().decode(), name
    for kw in (dict(), dict(b=fake), dict(a2=fake), dict(b=fake, a2=fake, b2=fake)):
        assert multipoles(wb=wsb(2, 4) - 1, **kw) == short
    assert "workspace" in lib.cgnn_last_error().decode()

    def positions(pos=fake, prev=fake, frames=2, n=10, box=1.0, los=2, shift=1.5, out=fake):
        return lib.cgnn_redshift_positions(pos, prev, frames, n, box, los, shift, out, None)

    for kw in (dict(pos=None), dict(prev=None), dict(out=None), dict(frames=0), dict(n=0), dict(n=-3), dict(box=0.0),
               dict(box=-1.0), dict(box=float("nan")), dict(box=float("inf")), dict(los=-1), dict(los=3),
               dict(shift=float("nan")), dict(shift=float("inf")), dict(shift=-float("inf"))):
        assert positions(**kw) == inv, kw
    assert positions(n=(1 << 24) + 1) == unsup
