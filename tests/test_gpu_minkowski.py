"""GPU: ``cgnn_excursion_counts`` through ctypes, bit for bit against the numpy restatement of tests/minkowski_checks.py --
at meshes on either side of every tile extent, on fields that sit on thresholds, run long, scatter, alternate, are
constant or hold NaN and infinities, at 1 to 255 thresholds and for frames -- with NaN guards around the field, canaries
around the counts and the field checked to be unmodified; the exact shapes; the refusals; and the chain up to
``statistics.minkowski_functionals`` and ``rollout_minkowski`` against the restatement fed with the device's own field."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import minkowski_checks as mk
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib, ops, statistics, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TX, TY, TZ = _lib.EX_TILE
# the smallest meshes (2 and 3: the neighbour at -1 is the one at +1), one mesh on either side of every tile extent
# (x and y: 8, z: 64), and two that are no multiple of any
MESHES = (2, 3, 4, 5, TX - 1, TX, TX + 1, TZ - 1, TZ, TZ + 1, 100, 129)
CANARY = mk.CANARY


def _raw_counts(fields, nu, expect=0):
    """cgnn_excursion_counts on fields [F, M, M, M] (host values) with NaN guards around the field and canaries in and
    around the counts, all checked, the field compared bit for bit afterwards -> counts [F, 4, nt] on the device"""
    fields = np.ascontiguousarray(fields, dtype=np.float64)
    frames, mesh = fields.shape[0], fields.shape[1]
    nu = np.ascontiguousarray(nu, dtype=np.float64)
    nt = len(nu)
    lib = _lib.load()
    f, f_buf = mk.guarded(fields, float("nan"), DEV)
    counts, c_buf = mk.guarded(torch.full((frames, 4, nt), CANARY, dtype=torch.int64), CANARY, DEV)
    rc = lib.cgnn_excursion_counts(f.data_ptr(), frames, mesh, nu.ctypes.data_as(C.POINTER(C.c_double)), nt,
                                   counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == expect, lib.cgnn_last_error().decode()
    torch.cuda.synchronize()
    assert mk.guards_intact(f_buf, float("nan")) and mk.guards_intact(c_buf, CANARY)
    assert torch.equal(f.cpu().view(torch.int64), torch.from_numpy(fields).view(torch.int64))
    return counts


def _check(fields, nu, what):
    got = _raw_counts(fields, nu).cpu().numpy()
    want = mk.excursion_counts(fields, nu)
    assert got.dtype == want.dtype and (got == want).all(), what
    return got


def _families(mesh):
    nu = mk.thresholds(25)
    out = {"integers": mk.integer_field(mesh, seed=mesh), "smooth": mk.smooth_field(mesh, seed=mesh + 1),
           "white": mk.white_field(mesh, seed=mesh + 2), "planted": mk.planted(mk.white_field(mesh, seed=mesh + 3)),
           "constant at a threshold": mk.constant_field(mesh, nu[7])}
    if mesh <= TZ + 1:
        out.update({"checkerboard": mk.checkerboard(mesh), "constant below": mk.constant_field(mesh, -5.0),
                    "constant above": mk.constant_field(mesh, 5.0), "planted smooth": mk.planted(mk.smooth_field(mesh, seed=3))})
    return out


@pytest.mark.parametrize("mesh", MESHES)
def test_counts_equal_the_restatement(mesh):
    fields = _families(mesh)
    for name, field in fields.items():
        _check(field[None], mk.thresholds(25), (mesh, name))
    # the other numbers of thresholds: 1, 2 and the most; on the small meshes for every family
    for nt in (1, 2, 255):
        names = fields if mesh <= TX + 1 else ("integers", "planted") if mesh <= TZ + 1 else ("planted",) if nt == 255 else ()
        for name in names:
            scale = 1.0 if nt > 2 else 0.5              # 0/1-like values around the one or two thresholds
            _check((fields[name] * scale)[None], mk.thresholds(nt), (mesh, name, nt))
    cells = mesh ** 3
    low = _raw_counts(fields["white"][None], [-1e9]).cpu()[0, :, 0].tolist()
    assert low == [cells, 3 * cells, 3 * cells, cells]


def test_more_tiles_than_workgroups():
    """mesh 193 has 25 x 25 x 4 = 2500 tiles for at most 2048 workgroups: some take two tiles and keep their counters."""
    mesh = 193
    assert -(-mesh // TX) * -(-mesh // TY) * -(-mesh // TZ) > 2048
    field = mk.integer_field(mesh, seed=1) + 0.5 * mk.smooth_field(mesh, seed=2).round()
    _check(field[None], mk.thresholds(25), mesh)


@pytest.mark.parametrize("mesh", (3, TX + 1, TZ + 1))
def test_frames_hold_different_data_and_two_runs_give_the_same_bits(mesh):
    frames = np.stack([mk.integer_field(mesh, seed=5), mk.planted(mk.smooth_field(mesh, seed=6)), mk.white_field(mesh, seed=7)])
    for nt in (1, 25, 255):
        nu = mk.thresholds(nt)
        got = _check(frames, nu, (mesh, nt))
        assert (got[0] != got[2]).any()
        again = _raw_counts(frames, nu).cpu().numpy()
        assert (again == got).all()
        one = _raw_counts(frames[1:2], nu).cpu().numpy()
        assert (one[0] == got[1]).all()
        # the op: the frames at once, one frame, host thresholds of any kind
        on_device = torch.from_numpy(frames).to(DEV)
        assert torch.equal(ops.excursion_counts(on_device, nu).cpu(), torch.from_numpy(got))
        assert torch.equal(ops.excursion_counts(on_device[2], torch.from_numpy(nu)).cpu(), torch.from_numpy(got[2]))
        assert torch.equal(ops.excursion_counts(on_device[:1], nu.tolist()).cpu(), torch.from_numpy(got[:1]))


@pytest.mark.parametrize("name", sorted(mk.shapes()))
def test_exact_shapes_on_the_device(name):
    field, counts, chi = mk.shapes()[name]
    every = np.stack([field] + [mk.translated(field, s) for s in mk.SHIFTS])
    got = _raw_counts(every, [mk.SHAPE_THRESHOLD]).cpu().numpy()
    for f in range(len(every)):
        assert tuple(got[f, :, 0]) == counts, (name, f)
    res = statistics.minkowski_from_counts(got[0], mk.SHAPE_MESH, 1.0)
    assert int(res["euler"]) == chi


def test_error_codes_with_the_canaries_untouched():
    lib = _lib.load()
    mesh, nu = 8, np.array([0.0, 1.0])
    f, f_buf = mk.guarded(mk.white_field(mesh, seed=1)[None], float("nan"), DEV)
    counts, c_buf = mk.guarded(torch.full((1, 4, 2), CANARY, dtype=torch.int64), CANARY, DEV)
    st = torch.cuda.current_stream().cuda_stream

    def doubles(*v):
        return (C.c_double * len(v))(*v)

    def call(field=f.data_ptr(), frames=1, mesh=mesh, nu=doubles(*nu), nt=2, out=counts.data_ptr()):
        return lib.cgnn_excursion_counts(field, frames, mesh, nu, nt, out, st)

    inv, unsup = -1, -2
    for kw in (dict(field=None), dict(nu=None), dict(out=None), dict(frames=0), dict(frames=-1), dict(mesh=1), dict(mesh=513),
               dict(nt=0), dict(nt=256, nu=doubles(*np.linspace(0, 1, 256))), dict(nu=doubles(0.0, 0.0)),
               dict(nu=doubles(1.0, 0.0)), dict(nu=doubles(0.0, float("nan"))), dict(nu=doubles(float("-inf"), 0.0)),
               dict(nu=doubles(0.0, float("inf")))):
        assert call(**kw) == inv, kw
    assert call(frames=(1 << 20) + 1) == unsup
    torch.cuda.synchronize()
    assert bool((counts == CANARY).all()) and mk.guards_intact(c_buf, CANARY) and mk.guards_intact(f_buf, float("nan"))
    assert call() == 0                                  # and the same buffers serve a good call
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == mk.excursion_counts(f.cpu().numpy(), nu)).all() and mk.guards_intact(c_buf, CANARY)


def test_the_op_equals_the_torch_composition_of_the_timing_script():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import time_minkowski
    finally:
        sys.path.pop(0)
    mesh = 33
    for nt, field in ((25, mk.planted(mk.white_field(mesh, seed=1))), (25, mk.integer_field(mesh, seed=2)),
                      (255, mk.smooth_field(mesh, seed=3)), (1, mk.checkerboard(mesh))):
        nu = mk.thresholds(nt)
        on_device = torch.from_numpy(field).to(DEV)
        got = ops.excursion_counts(on_device, nu)
        assert torch.equal(got, time_minkowski.torch_excursion_counts(on_device, torch.from_numpy(nu).to(DEV)))
        assert (got.cpu().numpy() == mk.excursion_counts(field, nu)).all()


# ---- the chain ------------------------------------------------------------------------------------------------------------
BOX, MESH, N = 1.0, 32, 4096
SMOOTHING = 2.0 * BOX / MESH


def _positions(kind):
    if kind == "clustered":
        return synthetic.make_clustered_positions(N, BOX, seed=3).to(DEV)
    return (torch.rand(N, 3, generator=torch.Generator().manual_seed(41)) * BOX).to(DEV)


def _restated(frames, units, nu, order=2, smoothing=SMOOTHING):
    """minkowski_from_counts of the restatement's counts of the device's own field, with its sigma0 and sigma1"""
    field, s0, s1 = statistics.smoothed_contrast(frames, BOX, MESH, smoothing, order, units)
    counts = mk.excursion_counts(field.cpu().numpy(), nu)
    return statistics.minkowski_from_counts(counts, MESH, BOX), s0.cpu(), s1.cpu(), field


@pytest.mark.parametrize("units", ("sigma", "contrast"))
@pytest.mark.parametrize("kind", ("clustered", "uniform"))
def test_minkowski_functionals_equal_the_restatement_of_the_device_field(kind, units):
    pos = _positions(kind)
    nu = np.linspace(-3.0, 3.0, 25) if units == "sigma" else np.linspace(-0.9, 3.0, 14)
    res = statistics.minkowski_functionals(pos, BOX, MESH, SMOOTHING, None if units == "sigma" else nu, threshold_units=units)
    want, s0, s1, field = _restated(pos[None], units, nu)
    assert res["v0"].shape == (len(nu),) and res["counts"].shape == (4, len(nu)) and res["sigma0"].dim() == 0
    for key in ("v0", "v1", "v2", "v3", "euler", "counts"):
        assert torch.equal(res[key], want[key][0]), key
    assert torch.equal(res["sigma0"], s0[0]) and torch.equal(res["sigma1"], s1[0])
    assert torch.equal(res["thresholds"], torch.from_numpy(nu))
    assert int(res["counts"][3, 0]) > 0 and float(res["sigma1"]) > float(res["sigma0"]) > 0
    if units == "sigma":
        assert float((field * field).mean()) == pytest.approx(1.0, rel=1e-12)
        gauss = statistics.gaussian_minkowski(nu, s0[0], s1[0])
        for d in range(4):
            assert torch.equal(res["gaussian_v%d" % d], gauss["v%d" % d])
    else:
        assert "gaussian_v0" not in res
        # the field is the contrast itself: its mean is 0 up to rounding
        assert abs(float(field.mean())) < 1e-12
    # frames [T, N, 3]: each equals its own call; order 3 and no smoothing go the same way
    both = torch.stack([pos, _positions("uniform" if kind == "clustered" else "clustered")])
    res2 = statistics.minkowski_functionals(both, BOX, MESH, SMOOTHING, nu, threshold_units=units)
    assert res2["v0"].shape == (2, len(nu)) and res2["sigma0"].shape == (2,)
    for key in ("v0", "v1", "v2", "v3", "euler", "counts", "sigma0", "sigma1"):
        assert torch.equal(res2[key][0], res[key]), key
    raw = statistics.minkowski_functionals(pos, BOX, MESH, 0.0, nu, order=3, threshold_units=units)
    want_raw = _restated(pos[None], units, nu, order=3, smoothing=0.0)[0]
    assert torch.equal(raw["counts"], want_raw["counts"][0]) and torch.equal(raw["v3"], want_raw["v3"][0])


def test_rollout_minkowski_equals_per_frame_calls_without_a_host_synchronisation():
    true = torch.stack([_positions("clustered"), _positions("uniform"), _positions("clustered")])
    pred = torch.stack([_positions("uniform"), _positions("clustered"), _positions("clustered")])
    data, gt = {"Coordinates": pred}, {"Coordinates": true}
    nu = statistics.default_minkowski_thresholds().tolist()
    statistics.rollout_minkowski(data, gt, BOX, MESH, SMOOTHING)        # warm: library, FFT plans, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                 # up to the final transfer
    try:
        dev_side = statistics.minkowski_counts_on_device(true, BOX, MESH, SMOOTHING, nu)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert dev_side.shape == (3, 4 * 25 + 2) and dev_side.dtype == torch.int64 and dev_side.is_cuda
    res = statistics.rollout_minkowski(data, gt, BOX, MESH, SMOOTHING, frames=[0, 2, 1])
    assert res["frames"] == [0, 2, 1]
    counts, s0, s1 = statistics.minkowski_on_host(dev_side.cpu(), 25)
    assert torch.equal(counts[[0, 2, 1]], res["counts_true"]) and torch.equal(s0[[0, 2, 1]], res["sigma0_true"])
    assert torch.equal(s1[[0, 2, 1]], res["sigma1_true"])
    for row, f in enumerate(res["frames"]):
        for side, frames in (("pred", pred), ("true", true)):
            one = statistics.minkowski_functionals(frames[f], BOX, MESH, SMOOTHING)
            for key in ("v0", "v1", "v2", "v3", "euler", "counts", "sigma0", "sigma1"):
                assert torch.equal(res[key + "_" + side][row], one[key]), (key, side, f)
            if side == "true":
                for d in range(4):
                    assert torch.equal(res["gaussian_v%d_true" % d][row], one["gaussian_v%d" % d])
    for d in range(4):
        assert torch.equal(res["v%d_difference" % d], res["v%d_pred" % d] - res["v%d_true" % d])
    assert bool((res["v0_difference"][1] == 0).all())                   # frame 2: the same positions on both sides
    contrast = statistics.rollout_minkowski(data, gt, BOX, MESH, SMOOTHING, [0.0, 1.0], threshold_units="contrast", frames=[1])
    assert "gaussian_v0_true" not in contrast and contrast["v0_pred"].shape == (1, 2)
