"""CPU: the contract of ``cgnn_mass_assign_backward`` as tests/density_loss_checks.py restates it is the gradient of the
deposit -- against central finite differences of a float64 unquantised deposit, within the bound the quantisation of the
forward's weights allows -- with its exact properties (a constant mesh, whole-cell translations), and the host-side
contract of ``losses.density_field_loss`` and the density term of ``training.unrolled_loss``: refusals before any device
work, the exported entry, the memory estimate.

The quantisation bound.  The backward uses, for the two axes it does not differentiate, the forward's integer weights
over Q = 2^13: each is off from the unquantised weight by at most 2^-14 (one rint; the TSC centre is Q minus two rints),
plus M 2^-24 from the float32 rounding of u = p s.  Derivative weights are at most 1 in size, value weights sum to 1 per
axis, so a particle's gradient is off by at most  scale s sum|d_mesh over its cells| 2^-12  for M <= 512.

The finite difference.  Central differences with a step of h = 2^-26 cells.  Inside one polynomial piece they are exact
for CIC (linear) and TSC (quadratic): h^2 times a vanishing third derivative.  A TSC stencil that straddles a
breakpoint of the spline (its first derivative is continuous, its second jumps by at most 3) adds at most 2 h per
unit of d_mesh, and float64 roundoff of the two function values 2^-52 / h per unit; both are charged on 27 max|d_mesh|."""
import os

import numpy as np
import pytest
import torch

import density_loss_checks as dlc
import power_spectrum_checks as psc
from cosmology_gnn_simulation_amd import _lib, graph_network, losses, ops, training
from unroll_checks import META

BOX = 25.0
H_CELLS = 2.0 ** -26


def _points(n, mesh, order, seed, box=BOX):
    """float32 [n, 3] in [0, box]; CIC: u kept at least 1e-3 of a cell from every cell boundary; TSC: anywhere,
    the box faces and cell boundaries and centres included"""
    rng = np.random.default_rng(seed)
    s = np.float32(mesh) / np.float32(box)
    if order == 2:
        u = rng.integers(0, mesh, (n, 3)) + rng.uniform(2e-3, 1 - 2e-3, (n, 3))
        x = (u / np.float64(s)).astype(np.float32)
        f = x.astype(np.float64) * np.float64(s)
        f = f - np.floor(f)
        assert (f >= 1e-3).all() and (f <= 1 - 1e-3).all()
        return x
    x = psc.with_special_positions(psc.uniform(n, seed, box), box)
    x[5:5 + mesh, 0] = (np.arange(mesh) / np.float64(s)).astype(np.float32)              # cell boundaries
    x[5:5 + mesh, 1] = ((np.arange(mesh) + 0.5) / np.float64(s)).astype(np.float32)        # cell centres: the breakpoints
    return x


def _bound(x, d_mesh, mesh, order, scale, box=BOX):
    s = np.float64(np.float32(mesh) / np.float32(box))
    return scale * s * dlc.abs_sum_over_cells(x, d_mesh, box, mesh, order) * 2.0 ** -12


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mesh", [4, 5, 16])
def test_restated_gradient_is_the_finite_difference_of_the_unquantised_deposit(mesh, order):
    n, scale = 200, 3.0
    x = _points(n, mesh, order, seed=mesh + order)
    d_mesh = np.random.default_rng(7 + mesh).normal(size=(mesh, mesh, mesh))
    got = dlc.mass_assign_backward(x, d_mesh, BOX, mesh, order, scale).astype(np.float64)
    s = np.float64(np.float32(mesh) / np.float32(BOX))
    h = H_CELLS / s
    x64 = x.astype(np.float64)
    fd = np.empty((n, 3))
    for ax in range(3):
        up, dn = x64.copy(), x64.copy()
        up[:, ax] += h
        dn[:, ax] -= h
        fd[:, ax] = scale * (dlc.contraction_unquantised(up, d_mesh, BOX, mesh, order)
                             - dlc.contraction_unquantised(dn, d_mesh, BOX, mesh, order)) / (2 * h)
    fd_term = scale * s * 27 * np.abs(d_mesh).max() * ((2 * H_CELLS if order == 3 else 0.0) + 2.0 ** -52 / H_CELLS)
    fl32_term = 2.0 ** -24 * np.abs(got)                                  # the restatement's one rounding to float32
    tol = _bound(x, d_mesh, mesh, order, scale)[:, None] + fd_term + fl32_term
    err = np.abs(got - fd)
    print(f"M={mesh} order={order}: largest error / tolerance {np.max(err / tol):.3f}, fd term / bound "
          f"{fd_term / _bound(x, d_mesh, mesh, order, scale).min():.2e}")
    assert (err <= tol).all()
    assert np.abs(got).max() > 0.1                                        # the check is not of zeros


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mesh", [4, 5, 16])
def test_restated_gradient_is_within_the_quantisation_bound_of_the_analytic_one(mesh, order):
    n, scale = 500, mesh ** 3 / 500
    x = _points(n, mesh, order, seed=3 * mesh + order)
    d_mesh = np.random.default_rng(11 + mesh).normal(size=(mesh, mesh, mesh))
    got = dlc.mass_assign_backward(x, d_mesh, BOX, mesh, order, scale).astype(np.float64)
    want = dlc.gradient_unquantised(x.astype(np.float64), d_mesh, BOX, mesh, order, scale)
    tol = _bound(x, d_mesh, mesh, order, scale)[:, None] + 2.0 ** -24 * np.abs(got)
    err = np.abs(got - want)
    print(f"M={mesh} order={order}: largest error / bound {np.max(err / tol):.3f}")
    assert (err <= tol).all()


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mesh", [4, 5, 16])
def test_constant_mesh_gives_exactly_zero(mesh, order):
    """The difference form of the contract takes differences of equal values first: exactly 0.0, not roundoff."""
    x = psc.with_special_positions(psc.uniform(300, 5 + mesh, BOX), BOX)
    for value in (1.0, -0.3, 1e300):
        got = dlc.mass_assign_backward(x, np.full((mesh, mesh, mesh), value), BOX, mesh, order, scale=7.0)
        assert got.dtype == np.float32 and got.shape == (300, 3) and (got == 0.0).all()


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mesh", [4, 5, 16])
def test_whole_cell_translation_with_a_rolled_mesh_leaves_the_gradient_unchanged(mesh, order):
    """s = 1 (box = M) and coordinates on multiples of 2^-8: the translation is exact in float32, the fractional
    parts are the same bits, so every weight is, and the cells move with the mesh."""
    rng = np.random.default_rng(21 + mesh)
    x = (rng.integers(0, mesh * 256, (400, 3)) / 256.0).astype(np.float32)
    d_mesh = rng.normal(size=(mesh, mesh, mesh))
    want = dlc.mass_assign_backward(x, d_mesh, float(mesh), mesh, order, scale=2.0)
    assert np.abs(want).max() > 0.1
    for shift in ((1, 0, 0), (2, mesh - 1, 3), (mesh, mesh, mesh)):
        k = np.asarray(shift)
        moved = np.mod(x.astype(np.float64) + k, mesh).astype(np.float32)
        assert (moved.astype(np.float64) == np.mod(x.astype(np.float64) + k, mesh)).all()
        got = dlc.mass_assign_backward(moved, np.roll(d_mesh, shift, axis=(0, 1, 2)), float(mesh), mesh, order, scale=2.0)
        assert np.array_equal(got, want)


def test_an_axis_the_forward_reads_as_zero_has_no_gradient_and_keeps_its_weights():
    x = psc.uniform(50, 31, BOX)
    d_mesh = np.random.default_rng(32).normal(size=(8, 8, 8))
    for order in (2, 3):
        clean = dlc.mass_assign_backward(x, d_mesh, BOX, 8, order)
        y = x.copy()
        y[10, 1] = np.nan
        y[20, 2] = np.float32(3e9 * BOX / 8)
        got = dlc.mass_assign_backward(y, d_mesh, BOX, 8, order)
        assert got[10, 1] == 0.0 and got[20, 2] == 0.0 and np.isfinite(got).all()
        keep = np.ones(50, dtype=bool)
        keep[[10, 20]] = False
        assert np.array_equal(got[keep], clean[keep])
        zero = x[10].copy()
        zero[1] = 0.0                       # the other axes see the weights of u = 0 on the refused axis
        assert np.array_equal(got[10, [0, 2]], dlc.mass_assign_backward(zero[None], d_mesh, BOX, 8, order)[0, [0, 2]])


def test_the_library_exports_the_entry():
    lib = _lib.load()
    assert "cgnn_mass_assign_backward" in _lib.EXPORTS and hasattr(lib, "cgnn_mass_assign_backward")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cgnn.h")).read()
    assert "int cgnn_mass_assign_backward(" in header
    for name in ("mass_assign_backward", "density_contrast"):
        assert callable(getattr(ops, name))
    assert callable(losses.density_field_loss)


def _touched(*a, **kw):
    raise AssertionError("the device was touched")


def test_density_field_loss_refuses_before_any_device_work(monkeypatch):
    monkeypatch.setattr(ops, "mass_assign", _touched)
    monkeypatch.setattr(_lib, "load", _touched)
    a, b = torch.rand(10, 3, requires_grad=True), torch.rand(10, 3)
    for kw in (dict(smoothing=-1.0), dict(smoothing=float("nan")), dict(smoothing=float("inf")), dict(order=1),
               dict(order=4), dict(order=True)):
        with pytest.raises(ValueError):
            losses.density_field_loss(a, b, 1.0, 8, **kw)
    for mesh in (1, 513, 7.5, True):
        with pytest.raises(ValueError):
            losses.density_field_loss(a, b, 1.0, mesh)
    with pytest.raises(ValueError):
        losses.density_field_loss(a, b[:5], 1.0, 8)
    with pytest.raises(ValueError):                                     # NGP has no gradient to give
        ops.density_contrast(a, 1.0, 8, order=1)
    with pytest.raises(ValueError):
        ops.mass_assign_backward(b, torch.zeros(8, 8, 8, dtype=torch.float64), 1.0, 8, order=1)
    with pytest.raises(ValueError):
        ops.mass_assign_backward(b, torch.zeros(8, 8, 8, dtype=torch.float64), 0.0, 8)


def test_unrolled_loss_refuses_a_bad_density_term_before_any_device_work(monkeypatch):
    monkeypatch.setattr(ops, "training_sample", _touched)
    monkeypatch.setattr(ops, "mass_assign", _touched)
    monkeypatch.setattr(training, "free_device_bytes", _touched)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    model = graph_network.EncodeProcessDecode(32, 32, 2, 2, 3)
    w, n, s = 3, 8, 2
    args = (model, torch.rand(w, n, 3), torch.rand(w, n, 1), torch.rand(s, n, 3), torch.rand(s, n, 1), META)
    kw = dict(dt=0.01, box_size=1.0, num_neighbors=4)
    for bad in (dict(density_loss_weight=1.0),                                            # no mesh
                dict(density_loss_weight=-1.0, density_mesh=8),
                dict(density_loss_weight=float("nan"), density_mesh=8),
                dict(density_loss_weight=float("inf"), density_mesh=8),
                dict(density_loss_weight=1.0, density_mesh=8, density_order=1),
                dict(density_loss_weight=1.0, density_mesh=1),
                dict(density_loss_weight=1.0, density_mesh=513),
                dict(density_loss_weight=1.0, density_mesh=8, density_smoothing=-0.1),
                dict(density_loss_weight=1.0, density_mesh=8, density_smoothing=float("nan"))):
        with pytest.raises(ValueError):
            training.unrolled_loss(*args, **kw, **bad)


def test_memory_estimate_counts_the_density_term():
    est = training.unrolled_training_bytes
    shape = (1000, 16, 5, 128, 128, 2, 10)
    for ckpt in ("none", "steps"):
        base = est(*shape, 4, checkpoint=ckpt)
        assert est(*shape, 4, checkpoint=ckpt, density_mesh=0) == base          # the default leaves the value unchanged
        steps_kept = 4 if ckpt == "none" else 1
        assert est(*shape, 4, checkpoint=ckpt, density_mesh=64) == base + steps_kept * 2 * 8 * 64 ** 3
        smoothed = est(*shape, 4, checkpoint=ckpt, density_mesh=64, density_smoothed=True)
        assert smoothed >= base + steps_kept * (2 * 8 * 64 ** 3 + 2 * 16 * 64 * 64 * 33)
    assert training.density_loss_bytes(256) == 2 * 8 * 256 ** 3


def test_batched_and_sharded_losses_refuse_the_term(monkeypatch):
    """Out of scope there (one box per deposit, no mesh across shards): refused, never silently ignored."""
    from cosmology_gnn_simulation_amd import dist
    monkeypatch.setattr(ops, "training_sample", _touched)
    monkeypatch.setattr(training, "free_device_bytes", _touched)
    model = graph_network.EncodeProcessDecode(32, 32, 2, 2, 3)
    p, t, tp, tt = torch.rand(3, 8, 3), torch.rand(3, 8, 1), torch.rand(2, 8, 3), torch.rand(2, 8, 1)
    kw = dict(dt=0.01, box_size=1.0, num_neighbors=4, density_loss_weight=1.0, density_mesh=8)
    with pytest.raises(TypeError):
        training.unrolled_batch_loss(model, [p], [t], [tp], [tt], META, **kw)
    with pytest.raises(NotImplementedError):
        dist.sharded_unrolled_loss(model, p, t, tp, tt, META, **kw)
    with pytest.raises(ValueError):
        dist.sharded_unrolled_loss(model, p, t, tp, tt, META, **dict(kw, density_loss_weight=-1.0))
