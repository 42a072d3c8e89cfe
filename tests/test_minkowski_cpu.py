"""CPU: the contract of ``cgnn_excursion_counts`` as tests/minkowski_checks.py restates it (exact shapes on mesh 8 with
known counts and Euler characteristics, translations across the box faces, monotony, the threshold rule, NaN), the host
arithmetic of ``statistics.minkowski_from_counts``, ``statistics.gaussian_minkowski`` against the restatement on smoothed
white noise, the argument checks of the op and of the statistics, the host refusals of the C entry, and the bookkeeping
of the new entry."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import minkowski_checks as mk
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib, ops, statistics

SHAPES = mk.shapes()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_exact_shapes_and_their_translations(name):
    field, counts, chi = SHAPES[name]
    got = mk.excursion_counts(field, [mk.SHAPE_THRESHOLD])
    assert got.dtype == np.int64 and got.shape == (4, 1)
    assert tuple(got[:, 0]) == counts
    assert got[0, 0] - got[1, 0] + got[2, 0] - got[3, 0] == chi
    for shift in mk.SHIFTS:                             # across the box faces: the complex is periodic
        assert (mk.excursion_counts(mk.translated(field, shift), [mk.SHAPE_THRESHOLD]) == got).all(), shift
    # the host arithmetic on these integers
    box = 4.0
    a, cells = box / mk.SHAPE_MESH, float(mk.SHAPE_MESH) ** 3
    res = statistics.minkowski_from_counts(got, mk.SHAPE_MESH, box)
    n0, n1, n2, n3 = counts
    assert res["v0"].dtype == torch.float64 and res["euler"].dtype == torch.int64 and res["v0"].shape == (1,)
    assert float(res["v0"]) == n3 / cells
    assert float(res["v1"]) == 2.0 * (n2 - 3 * n3) / (9.0 * a * cells)
    assert float(res["v2"]) == 2.0 * (n1 - 2 * n2 + 3 * n3) / (9.0 * a * a * cells)
    assert float(res["v3"]) == chi / (a ** 3 * cells) and int(res["euler"]) == chi
    assert torch.equal(res["counts"], torch.from_numpy(got))
    want = mk.from_counts(got, mk.SHAPE_MESH, box)
    for key in ("v0", "v1", "v2", "v3", "euler"):
        assert (res[key].numpy() == want[key]).all(), key


def test_a_single_cube_reports_two_thirds_of_its_surface():
    """Crofton's orientation average on a cubic lattice: V1 is a sixth of the surface per unit volume for an isotropic
    body, and a lattice cube, whose faces all lie along the axes, reports 2/3 of its 6 a^2."""
    box, mesh = 4.0, mk.SHAPE_MESH
    a = box / mesh
    res = statistics.minkowski_from_counts(mk.excursion_counts(SHAPES["one voxel"][0], [0.5]), mesh, box)
    assert float(res["v1"]) == pytest.approx((2.0 / 3.0) * 6 * a * a / 6.0 / box ** 3, rel=1e-15)
    assert float(res["v0"]) == pytest.approx(a ** 3 / box ** 3, rel=1e-15)
    assert float(res["v3"]) == pytest.approx(1.0 / box ** 3, rel=1e-15)
    # frames: [F, 4, nt] in, [F, nt] out
    both = statistics.minkowski_from_counts(np.stack([mk.excursion_counts(SHAPES[n][0], [0.5, 0.75]) for n in
                                                      ("one voxel", "the full box")]), mesh, box)
    assert both["v0"].shape == (2, 2) and both["euler"].tolist() == [[1, 1], [0, 0]]
    assert both["v0"][1].tolist() == [1.0, 1.0] and both["v1"][1].tolist() == [0.0, 0.0] and both["v2"][1].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("mesh", (2, 3, 5, 9))
def test_monotony_bounds_and_the_threshold_rule(mesh):
    nu = mk.thresholds(25)
    cells = mesh ** 3
    for field in (mk.integer_field(mesh, seed=mesh), mk.white_field(mesh, seed=mesh + 1), mk.smooth_field(mesh, seed=2)):
        counts = mk.excursion_counts(field, nu)
        assert (np.diff(counts, axis=1) <= 0).all()                     # non-increasing in t
        assert (counts >= 0).all() and (counts <= np.array([cells, 3 * cells, 3 * cells, cells])[:, None]).all()
        # a threshold below the minimum: everything is in
        low = mk.excursion_counts(field, [field.min() - 1.0])[:, 0]
        assert tuple(low) == (cells, 3 * cells, 3 * cells, cells)
        # one above the maximum: nothing is
        assert (mk.excursion_counts(field, [field.max() + 1.0]) == 0).all()
        # the cubes are the voxels at or above the threshold
        assert counts[3].tolist() == [(field >= t).sum() for t in nu]
    # a value equal to a threshold is in
    field = mk.constant_field(mesh, 1.0)
    at = mk.excursion_counts(field, [0.0, 1.0, np.nextafter(1.0, 2.0)])
    assert at[:, 0].tolist() == at[:, 1].tolist() == [cells, 3 * cells, 3 * cells, cells] and (at[:, 2] == 0).all()
    # NaN is in no set, whatever the threshold; -inf neither; +inf in all
    for value, inside in ((np.nan, False), (-np.inf, False), (np.inf, True)):
        got = mk.excursion_counts(mk.constant_field(mesh, value), [-1e300, 0.0, 1e300])
        assert (got == (np.array([cells, 3 * cells, 3 * cells, cells])[:, None] if inside else 0)).all(), value
    assert mk.indices(np.array([np.nan, -np.inf, np.inf, 0.0, -0.0, 0.5]), [0.0, 0.5]).tolist() == [0, 0, 2, 1, 1, 2]


def test_small_meshes_count_by_index_arithmetic():
    """mesh 2: the neighbour at -1 is the neighbour at +1; one voxel still has 8 vertices, 12 edges and 6 faces by index,
    since every one of the 2^3 lower corners touches it."""
    field = np.zeros((2, 2, 2))
    field[1, 0, 1] = 1.0
    assert mk.excursion_counts(field, [0.5])[:, 0].tolist() == [8, 12, 6, 1]
    field = np.zeros((3, 3, 3))
    field[1, 1, 1] = 1.0
    assert mk.excursion_counts(field, [0.5])[:, 0].tolist() == [8, 12, 6, 1]
    frames = np.stack([field, 1.0 - field])
    both = mk.excursion_counts(frames, [0.5])
    assert both.shape == (2, 4, 1) and both[1, :, 0].tolist() == [27, 81, 81, 26]


def test_gaussian_minkowski_against_the_restatement_on_smoothed_white_noise():
    """Mesh 64, a Gaussian of 3 cells, seed 5, 25 thresholds in [-3, 3].  The largest deviation of the counted curves from
    the Gaussian ones, relative to each curve's peak, as the restatement gives it here: 0.01232 (v0), 0.02276 (v1),
    0.07897 (v2), 0.13257 (v3) -- sample variance and pixelisation of one realisation (seed 6: 0.0041, 0.0124, 0.0675,
    0.1372; 2 cells: 0.0093, 0.0234, 0.0804, 0.1144).  The tolerances are 1.5 times these."""
    measured = {"v0": 0.01232, "v1": 0.02276, "v2": 0.07897, "v3": 0.13257}
    mesh, nu = 64, mk.thresholds(25)
    field, s0, s1 = mk.smoothed_white_noise(mesh, 3.0, seed=5)
    res = statistics.minkowski_from_counts(mk.excursion_counts(field, nu), mesh, 1.0)
    gauss = statistics.gaussian_minkowski(nu, s0, s1)
    assert float(gauss["lam"]) == pytest.approx(math.sqrt(s1 * s1 / (6.0 * math.pi * s0 * s0)), rel=1e-14)
    for key, seen in measured.items():
        dev = float((res[key] - gauss[key]).abs().max() / gauss[key].abs().max())
        print(key, "largest deviation / peak:", dev)
        assert dev <= 1.5 * seen, key
    # the curves themselves: closed forms at nu = 0 and their symmetries
    lam = float(gauss["lam"])
    mid = 12
    assert nu[mid] == 0.0
    assert float(gauss["v0"][mid]) == 0.5 and float(gauss["v2"][mid]) == 0.0
    assert float(gauss["v1"][mid]) == pytest.approx(2.0 / 3.0 * lam / math.sqrt(2 * math.pi), rel=1e-14)
    assert float(gauss["v3"][mid]) == pytest.approx(-lam ** 3 / math.sqrt(2 * math.pi), rel=1e-14)
    assert torch.allclose(gauss["v0"] + gauss["v0"].flip(0), torch.ones(25, dtype=torch.float64), atol=1e-15)
    assert torch.equal(gauss["v1"], gauss["v1"].flip(0)) and torch.equal(gauss["v2"], -gauss["v2"].flip(0))
    # frames: sigma [F] -> curves [F, nt]
    two = statistics.gaussian_minkowski(nu, [s0, 2 * s0], [s1, s1])
    assert two["v3"].shape == (2, 25) and two["v0"].shape == (2, 25)
    assert torch.equal(two["v1"][0], gauss["v1"]) and torch.allclose(two["v1"][1], gauss["v1"] / 2, rtol=1e-14)
    for bad in (dict(nu=[]), dict(nu=[float("nan")]), dict(sigma0=0.0), dict(sigma0=-1.0), dict(sigma1=-1.0),
                dict(sigma0=[1.0, 2.0]), dict(sigma0=[[1.0]], sigma1=[[1.0]])):
        args = dict(nu=nu, sigma0=1.0, sigma1=2.0)
        args.update(bad)
        with pytest.raises(ValueError):
            statistics.gaussian_minkowski(**args)


def test_defaults_and_the_host_arithmetic_refusals():
    nu = statistics.default_minkowski_thresholds()
    assert nu.dtype == torch.float64 and nu.shape == (25,) and float(nu[0]) == -3.0 and float(nu[-1]) == 3.0
    assert float(nu[12]) == 0.0 and bool((nu[1:] > nu[:-1]).all())
    good = np.zeros((4, 3), dtype=np.int64)
    for kw in (dict(counts=np.zeros((3, 3), dtype=np.int64)), dict(counts=np.zeros((4, 3))), dict(counts=np.zeros(4, dtype=np.int64)),
               dict(counts=np.zeros((4, 0), dtype=np.int64)), dict(mesh=1), dict(mesh=513), dict(mesh=2.5), dict(box_size=0.0),
               dict(box_size=float("inf"))):
        args = dict(counts=good, mesh=8, box_size=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            statistics.minkowski_from_counts(**args)


def test_the_op_and_the_statistics_refuse_on_the_host():
    field = torch.zeros(4, 4, 4, dtype=torch.float64)   # host tensors: refused later, were the arguments right
    for kw in (dict(field=field.float()), dict(field=field.long()), dict(field=field.numpy()), dict(field=field[:, :, :3]),
               dict(field=field[0]), dict(field=torch.zeros(4, 4, 3, dtype=torch.float64)),
               dict(field=torch.zeros(2, 4, 4, 5, dtype=torch.float64)), dict(field=torch.zeros(0, 4, 4, 4, dtype=torch.float64)),
               dict(field=field.transpose(0, 2)), dict(field=torch.zeros(8, 8, 8, dtype=torch.float64)[::2, ::2, ::2]),
               dict(field=torch.zeros(1, 1, 1, dtype=torch.float64)), dict(field=torch.zeros(1, 513, 1, dtype=torch.float64).expand(513, 513, 513)),
               dict(thresholds=[]), dict(thresholds=[0.0, 0.0]), dict(thresholds=[1.0, 0.0]), dict(thresholds=[float("nan")]),
               dict(thresholds=[0.0, float("inf")]), dict(thresholds=np.linspace(0, 1, 256))):
        args = dict(field=field, thresholds=[0.0, 1.0])
        args.update(kw)
        with pytest.raises(ValueError):
            ops.excursion_counts(**args)
    assert len(ops.check_excursion_thresholds(np.linspace(0, 1, 255), "t")) == 255
    with pytest.raises(_lib.CgnnError):                 # the arguments pass; there is no CPU path
        ops.excursion_counts(field, [0.0, 1.0])
    pos = torch.rand(100, 3)
    for kw in (dict(mesh=1), dict(mesh=513), dict(mesh=8.5), dict(box_size=0.0), dict(box_size=float("nan")), dict(smoothing=-0.1),
               dict(smoothing=float("inf")), dict(smoothing=True), dict(order=0), dict(order=4), dict(order=True),
               dict(threshold_units="nu"), dict(thresholds=[]), dict(thresholds=[0.5, 0.5]), dict(thresholds=[float("nan")]),
               dict(thresholds=np.linspace(-3, 3, 256)), dict(pos=pos[:, :2]), dict(pos=pos.numpy()), dict(pos=pos.view(1, 1, 100, 3))):
        args = dict(pos=pos, box_size=1.0, mesh=8, smoothing=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            statistics.minkowski_functionals(**args)
    with pytest.raises(_lib.CgnnError):
        statistics.minkowski_functionals(pos, 1.0, 8, 0.1)
    frames = {"Coordinates": pos.view(1, 100, 3).repeat(3, 1, 1)}
    for kw in (dict(mesh=1), dict(smoothing=-1.0), dict(order=5), dict(threshold_units="delta"), dict(thresholds=[1.0, 0.0]),
               dict(frames=[3]), dict(frames=[]), dict(frames=[-1]), dict(box_size=-1.0)):
        args = dict(rollout_data=frames, ground_truth=frames, box_size=1.0, mesh=8, smoothing=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            statistics.rollout_minkowski(**args)
    with pytest.raises(_lib.CgnnError):
        statistics.rollout_minkowski(frames, frames, 1.0, 8, 0.1)


def test_host_refusals_of_the_c_entry():
    """The refusals come before any launch: no GPU is needed to meet them, and no pointer is dereferenced."""
    lib = _lib.load()
    fake = 1 << 20                                      # never dereferenced: every call below is refused on the host
    inv, unsup = -1, -2                                 # CGNN_ERR_INVALID_ARG, CGNN_ERR_UNSUPPORTED

    def doubles(*v):
        return (C.c_double * len(v))(*v)

    def call(field=fake, frames=1, mesh=8, nu=doubles(0.0, 1.0), nt=2, counts=fake):
        return lib.cgnn_excursion_counts(field, frames, mesh, nu, nt, counts, None)

    def err():
        return lib.cgnn_last_error().decode()

    for kw in (dict(field=None), dict(nu=None), dict(counts=None), dict(frames=0), dict(frames=-2)):
        assert call(**kw) == inv, kw
        assert err() == "cgnn_excursion_counts: invalid argument (no null pointer, frames positive)"
    for kw in (dict(mesh=1), dict(mesh=0), dict(mesh=-8), dict(mesh=513), dict(nt=0), dict(nt=-1),
               dict(nt=256, nu=doubles(*np.linspace(0, 1, 256)))):
        assert call(**kw) == inv, kw
        assert "outside [2, 512] or num_thresholds=" in err() and "outside [1, 255]" in err()
    for nu in (doubles(0.0, 0.0), doubles(1.0, 0.0), doubles(float("nan"), 1.0), doubles(0.0, float("nan")),
               doubles(0.0, float("inf")), doubles(float("-inf"), 0.0)):
        assert call(nu=nu) == inv
        assert "thresholds must be finite and strictly ascending" in err()
    assert call(frames=(1 << 20) + 1) == unsup and err() == "cgnn_excursion_counts: more than 2^20 frames in one call"
    assert _lib.EX_MAX_THRESHOLDS == 255 and _lib.EX_TILE == (8, 8, 64)


def test_the_new_entry_is_declared_exported_built_and_documented():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    name = "cgnn_excursion_counts"
    assert name in _lib.EXPORTS and hasattr(lib, name)
    assert name + "(" in header and name in notes
    assert "#define CGNN_EX_MAX_THRESHOLDS %d\n" % _lib.EX_MAX_THRESHOLDS in header
    for axis, extent in zip("XYZ", _lib.EX_TILE):
        assert re.search(r"#define CGNN_EX_T%s %d\s" % (axis, extent), header)
    assert "idx(v) = #{t : thresholds[t] <= field(v)}" in header
    makefile = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "Makefile")).read()
    assert " minkowski.hip" in makefile and "FLAGS_minkowski" not in makefile
    source = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "minkowski.hip")).read()
    assert "pair_walk.hpp" not in source and "atomicAdd(&out[i], (unsigned long long)v)" in source
    for fn in ("check_excursion_thresholds", "excursion_counts"):
        assert callable(getattr(ops, fn))
    for fn in ("default_minkowski_thresholds", "minkowski_from_counts", "gaussian_minkowski", "minkowski_functionals",
               "rollout_minkowski", "smoothed_contrast", "minkowski_counts_on_device", "minkowski_on_host"):
        assert callable(getattr(statistics, fn))
    assert os.path.isfile(os.path.join(ROOT, "scripts", "time_minkowski.py"))
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "excursion_counts" in text and "rollout_minkowski" in text and "time_minkowski.py" in text
