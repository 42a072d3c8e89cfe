"""GPU: ``ops.pair_counts`` (``cgnn_pair_counts``) against the numpy restatement of its counting contract
(tests/pair_count_checks.py): integers, so every case is ``torch.equal``.  ``ops.frame_errors`` against float64 numpy, and
``statistics.rollout_statistics`` on a rollout of the ``tiny`` golden model.

Grids the cases reach (G cells per axis: the largest with cells no smaller than the last radius plus its margin,
capped by cbrt(N) and 256): one cell (radius L / 2, N = 1 and 2), G = 2 and 3 (all cells of an axis walked once: a
wrapped 3-cell walk would meet a cell twice), powers of two (4, 8, 16) and others (6, 7, 10, 19) under the 27-cell walk."""
import functools
import math

import numpy as np
import pytest
import torch

import pair_count_checks as pcc
from cosmology_gnn_simulation_amd import graph_network, ops, rollout, statistics

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOX = 25.0
RATIOS = (0.5, 0.3, 0.12, 0.05)
SIZES = (1, 2, 64, 300, 4096, 8192)


def _edges(ratio, box=BOX, nb=8):
    return np.linspace(0.0, ratio * box, nb + 1).astype(np.float32)


def _uniform(n, seed, box=BOX):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32) * np.float32(box)


def _auto(x, box, edges, **kw):
    return ops.pair_counts(torch.from_numpy(x).to(DEV), box, edges, **kw)


def _cross(a, b, box, edges, **kw):
    return ops.pair_counts(torch.from_numpy(a).to(DEV), box, edges, torch.from_numpy(b).to(DEV), **kw)


def _want(counts):
    return torch.from_numpy(np.asarray(counts, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def _sweep_reference(n):
    """One brute force per size for all four radii: counted once over the union of the four edge sets (each set's e2
    thresholds are among the union's), then summed per set."""
    x = _uniform(n, seed=100 + n)
    union = np.unique(np.concatenate([_edges(r) for r in RATIOS]))
    fine = pcc.auto_counts(x, BOX, union)
    out = {}
    for r in RATIOS:
        at = np.searchsorted(union, _edges(r))
        assert (union[at] == _edges(r)).all()
        out[r] = np.array([fine[a:b].sum() for a, b in zip(at[:-1], at[1:])], dtype=np.int64)
    return x, out


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("n", SIZES)
def test_auto_counts_equal_the_brute_force(n, ratio):
    x, want = _sweep_reference(n)
    got = _auto(x, BOX, _edges(ratio))
    assert got.dtype == torch.int64 and got.shape == (8,)
    assert torch.equal(got.cpu(), _want(want[ratio]))
    if n >= 4096:
        assert int(got.sum()) > 0


def test_the_union_reference_is_the_plain_restatement():
    x, want = _sweep_reference(300)
    for r in RATIOS:
        assert (pcc.auto_counts(x, BOX, _edges(r)) == want[r]).all()


def _near_boundaries(n, seed, box=BOX):
    """Particles within 1e-3 L of faces, edges and corners; coordinates of exactly 0 and exactly L among them."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3), dtype=np.float32) * np.float32(box)
    eps = rng.random((n, 3), dtype=np.float32) * np.float32(1e-3 * box)
    near = np.where(rng.random((n, 3)) < 0.5, eps, np.float32(box) - eps).astype(np.float32)
    axes = rng.integers(1, 4, size=n)                   # 1: a face, 2: an edge, 3: a corner
    pick = np.argsort(rng.random((n, 3)), axis=1) < axes[:, None]
    x = np.where(pick, near, x).astype(np.float32)
    exact = rng.integers(0, n, size=(40, 2))
    x[exact[:20, 0], exact[:20, 1] % 3] = 0.0
    x[exact[20:, 0], exact[20:, 1] % 3] = np.float32(box)
    assert (x == 0).any() and (x == np.float32(box)).any() and x.min() >= 0 and x.max() <= np.float32(box)
    return x


@pytest.mark.parametrize("ratio", RATIOS + (0.4,))       # 0.4: two cells per axis
def test_particles_at_faces_edges_and_corners(ratio):
    x = _near_boundaries(600, seed=7)
    edges = _edges(ratio)
    assert torch.equal(_auto(x, BOX, edges, check_bounds=True).cpu(), _want(pcc.auto_counts(x, BOX, edges)))


def test_a_blob_puts_several_workgroups_of_queries_in_one_cell():
    rng = np.random.default_rng(11)
    d = rng.standard_normal((700, 3))
    d *= (0.01 * BOX * rng.random((700, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    x = np.concatenate([(0.35 * BOX + d).astype(np.float32), _uniform(300, seed=12)])      # G = 10: cell 3 holds the blob
    edges = np.geomspace(1e-3 * BOX, 0.05 * BOX, 13).astype(np.float32)
    want = pcc.auto_counts(x, BOX, edges)
    assert want.sum() > 700 * 699 // 4
    assert torch.equal(_auto(x, BOX, edges).cpu(), _want(want))
    y = _uniform(500, seed=13)
    assert torch.equal(_cross(y, x, BOX, edges).cpu(), _want(pcc.cross_counts(y, x, BOX, edges)))
    assert torch.equal(_cross(x, y, BOX, edges).cpu(), _want(pcc.cross_counts(x, y, BOX, edges)))


def _cells_per_axis(partners, box, reach):
    """Restates the grid rule (``pair_cells_per_axis`` of csrc/pair_walk.hpp) with the pair counter's caps, G^3 <= partners
    and G <= 256."""
    cap = 1
    while cap < 256 and (cap + 1) ** 3 <= partners:
        cap += 1
    g = math.floor(box / (float(np.float32(reach)) * (1 + 1e-5) + 2e-5 * box))
    return max(1, min(g, 256, cap))


@pytest.mark.parametrize("m", [256, 257, 512])
def test_a_cell_of_exactly_full_work_items(m):
    """m queries in one cell and nobody else in it: one full item, a full item and one query, two full items.  The cell
    is alone under the grid of the auto count (and of a cross count whose partners are x) and under the grid that y's
    500 partners make, so cross(x, y) walks the same full items."""
    rng = np.random.default_rng(21 + m)
    d = rng.standard_normal((m, 3))
    d *= (0.01 * BOX * rng.random((m, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    blob = (0.35 * BOX + d).astype(np.float32)
    edges = np.geomspace(1e-3 * BOX, 0.05 * BOX, 13).astype(np.float32)
    y = _uniform(500, seed=23)
    grids = (_cells_per_axis(m + 300, BOX, edges[-1]), _cells_per_axis(len(y), BOX, edges[-1]))
    assert min(grids) >= 4

    def in_blob_cell(p, g):
        return (np.floor(p * (g / BOX)) == np.floor(0.35 * g)).all(axis=1)

    others = _uniform(400, seed=22)
    others = others[~(in_blob_cell(others, grids[0]) | in_blob_cell(others, grids[1]))][:300]
    x = np.concatenate([blob, others])
    x = x[rng.permutation(len(x))]
    assert len(x) == m + 300
    for g in grids:
        assert in_blob_cell(x, g).sum() == m
    assert torch.equal(_auto(x, BOX, edges).cpu(), _want(pcc.auto_counts(x, BOX, edges)))
    assert torch.equal(_cross(x, y, BOX, edges).cpu(), _want(pcc.cross_counts(x, y, BOX, edges)))
    assert torch.equal(_cross(y, x, BOX, edges).cpu(), _want(pcc.cross_counts(y, x, BOX, edges)))


def test_partners_at_the_last_radius_test_the_reach_margin():
    """64 centres, each with one partner at edges[nb] (1 +- 3e-7) in a random direction; the radius is the largest for
    which 8 cells per axis are still allowed, so the cells are barely larger than the reach."""
    reach = np.float32((0.125 - 2e-5) / (1 + 1e-5) * (1 - 1e-6) * BOX)
    rng = np.random.default_rng(21)
    c = rng.random((64, 3)) * BOX
    u = rng.standard_normal((64, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = np.float64(reach) * (1 + 3e-7 * np.where(np.arange(64) % 2 == 0, 1.0, -1.0))
    partners = np.mod(c + dist[:, None] * u, BOX)
    x = np.concatenate([c, partners, _uniform(600, seed=22)]).astype(np.float32)
    x = np.minimum(x, np.float32(BOX))
    edges = np.array([0.9 * reach, reach], dtype=np.float32)
    want = pcc.auto_counts(x, BOX, edges)
    beyond = pcc.auto_counts(x, BOX, np.array([reach, reach * np.float32(1.0001)], dtype=np.float32))
    assert want[0] > 0 and beyond[0] > 0                # partners on both sides of the radius
    assert torch.equal(_auto(x, BOX, edges).cpu(), _want(want))


@pytest.mark.parametrize("first_edge", [0.0, 0.01])
def test_coincident_particles_count_in_bin_0_only_when_it_starts_at_zero(first_edge):
    base = _uniform(50, seed=31)
    x = np.concatenate([base, base, base, _uniform(200, seed=32)])
    edges = np.array([first_edge * BOX, 0.05 * BOX, 0.2 * BOX], dtype=np.float32)
    want = pcc.auto_counts(x, BOX, edges)
    got = _auto(x, BOX, edges).cpu()
    assert torch.equal(got, _want(want))
    if first_edge == 0.0:
        assert int(got[0]) >= 150                       # three coincident pairs per triple
    else:
        from_zero = pcc.auto_counts(x, BOX, np.array([0.0, first_edge * BOX, 0.2 * BOX], dtype=np.float32))
        assert from_zero[0] >= 150 and int(got.sum()) == int(from_zero[1])      # the coincident pairs are left out


@pytest.mark.parametrize("shift", [0.0, 0.5])
def test_simple_cubic_lattice_has_its_analytic_counts(shift):
    got = _auto(pcc.lattice_points(shift), 8.0, pcc.LATTICE_EDGES)
    assert got.cpu().tolist() == pcc.LATTICE_COUNTS


@pytest.mark.parametrize("nb", [1, 20, 256])
def test_bin_counts(nb):
    x = _uniform(2000, seed=41)
    if nb == 20:
        edges = np.geomspace(0.004 * BOX, 0.2 * BOX, nb + 1).astype(np.float32)
    else:
        edges = np.linspace(0.0, 0.2 * BOX, nb + 1).astype(np.float32)
    got = _auto(x, BOX, edges)
    assert got.shape == (nb,)
    assert torch.equal(got.cpu(), _want(pcc.auto_counts(x, BOX, edges)))


def test_cross_counts_and_the_identity_with_auto():
    a, b = _uniform(300, seed=51), _uniform(500, seed=52)
    for ratio in (0.5, 0.12):
        edges = _edges(ratio)
        assert torch.equal(_cross(a, b, BOX, edges).cpu(), _want(pcc.cross_counts(a, b, BOX, edges)))
        assert torch.equal(_cross(b, a, BOX, edges).cpu(), _want(pcc.cross_counts(a, b, BOX, edges)))
        xx = _cross(a, a, BOX, edges).cpu()
        xx[0] -= 300                                    # every particle with itself, d2 = 0
        assert torch.equal(xx, 2 * _auto(a, BOX, edges).cpu())
    one = _cross(a[:1], b, BOX, _edges(0.3)).cpu()      # a single query
    assert torch.equal(one, _want(pcc.cross_counts(a[:1], b, BOX, _edges(0.3))))


def test_frames_equal_separate_calls_and_a_repeat_gives_the_same_tensor():
    frames = torch.from_numpy(np.stack([_uniform(1000, seed=60 + t) for t in range(3)])).to(DEV)
    other = torch.from_numpy(np.stack([_uniform(700, seed=70 + t) for t in range(3)])).to(DEV)
    edges = _edges(0.12)
    got = ops.pair_counts(frames, BOX, edges)
    assert got.shape == (3, 8) and got.dtype == torch.int64
    assert torch.equal(got, torch.stack([ops.pair_counts(frames[t], BOX, edges) for t in range(3)]))
    assert torch.equal(got[1].cpu(), _want(pcc.auto_counts(frames[1].cpu().numpy(), BOX, edges)))
    cross = ops.pair_counts(frames, BOX, edges, other)
    assert torch.equal(cross, torch.stack([ops.pair_counts(frames[t], BOX, edges, other[t]) for t in range(3)]))
    assert torch.equal(ops.pair_counts(frames, BOX, edges), got)
    assert torch.equal(ops.pair_counts(frames, BOX, edges, other), cross)


def test_check_bounds_refuses_positions_outside_the_box():
    x = torch.from_numpy(_uniform(100, seed=80)).to(DEV)
    x[3, 1] = BOX
    ops.pair_counts(x, BOX, _edges(0.3), check_bounds=True)              # exactly L is inside
    for bad in (-1e-3, BOX * (1 + 1e-6)):
        y = x.clone()
        y[5, 2] = bad
        with pytest.raises(ValueError):
            ops.pair_counts(y, BOX, _edges(0.3), check_bounds=True)
        with pytest.raises(ValueError):
            ops.pair_counts(x, BOX, _edges(0.3), y, check_bounds=True)


def test_correlation_function_of_uniform_points_is_small():
    x = torch.from_numpy(_uniform(8192, seed=90)).to(DEV)
    edges = np.linspace(0.0, BOX / 2, 17)
    res = statistics.correlation_function(x, BOX, edges)
    assert sorted(res) == ["counts", "r_hi", "r_lo", "xi"]
    expect = pcc.expected_random_pairs(8192, BOX, edges)
    big = expect >= 100
    dev = np.abs(res["counts"].numpy() - expect)[big] / np.sqrt(expect[big])
    assert (dev < 4).all(), dev                         # four Poisson deviations, as on the host
    np.testing.assert_allclose(res["xi"].numpy()[big], (res["counts"].numpy() / expect - 1)[big], atol=1e-12)


# ---- frame errors ------------------------------------------------------------------------------------------------------
def _fold64(d, box):
    """The contract's fold on float32 differences, then float64."""
    box32, half = np.float32(box), np.float32(0.5) * np.float32(box)
    return np.where(d > half, d - box32, np.where(d < -half, d + box32, d)).astype(np.float32).astype(np.float64)


def _frames_with_crossers(t, n, seed, sigma):
    """True frames, and predictions off by about sigma; 5 % of the true particles sit within sigma of a face, so that
    their predictions are likely on the other side (wrapped back into the box)."""
    rng = np.random.default_rng(seed)
    true = rng.random((t, n, 3)) * BOX
    at_face = rng.random((t, n)) < 0.05
    true[at_face, 0] = np.where(rng.random(at_face.sum()) < 0.5, 0.0, BOX) + 0.1 * sigma * rng.standard_normal(at_face.sum())
    true = np.mod(true, BOX).astype(np.float32)
    pred = np.mod(true.astype(np.float64) + sigma * rng.standard_normal((t, n, 3)), BOX).astype(np.float32)
    pred, true = np.minimum(pred, np.float32(BOX)), np.minimum(true, np.float32(BOX))
    ttmp = rng.random((t, n, 1), dtype=np.float32) + 1
    ptmp = (ttmp + 0.1 * rng.standard_normal((t, n, 1))).astype(np.float32)
    return pred, true, ptmp, ttmp


@pytest.mark.parametrize("n", [1, 63, 1000, 8192])
def test_frame_errors_match_float64_numpy_and_repeat_bit_for_bit(n):
    """Bound: the sums of at most 3 n <= 24576 non-negative float64 terms, every addition within 2^-53: relative error
    below 3 n 2^-53 < 3e-12 (the issue's 1e-11 has room to spare)."""
    pred, true, ptmp, ttmp = _frames_with_crossers(4, n, seed=n, sigma=0.01 * BOX)
    dev = [torch.from_numpy(a).to(DEV) for a in (pred, true, ptmp, ttmp)]
    got = ops.frame_errors(*dev, BOX)
    assert got.shape == (4, 2) and got.dtype == torch.float64
    want_p = (_fold64(pred - true, BOX) ** 2).reshape(4, -1).mean(axis=1)
    want_t = ((ptmp - ttmp).astype(np.float64) ** 2).reshape(4, -1).mean(axis=1)
    np.testing.assert_allclose(got[:, 0].cpu().numpy(), want_p, rtol=1e-11, atol=0)
    np.testing.assert_allclose(got[:, 1].cpu().numpy(), want_t, rtol=1e-11, atol=0)
    assert torch.equal(ops.frame_errors(*dev, BOX), got)
    no_tmp = ops.frame_errors(dev[0], dev[1], None, None, BOX)
    assert torch.equal(no_tmp[:, 0], got[:, 0]) and float(no_tmp[:, 1].abs().max()) == 0.0
    squeezed = ops.frame_errors(dev[0], dev[1], dev[2].squeeze(-1), dev[3].squeeze(-1), BOX)
    assert torch.equal(squeezed, got)


def test_minimum_image_error_stays_at_the_size_of_the_perturbation():
    sigma = 1e-3 * BOX
    pred, true, ptmp, ttmp = _frames_with_crossers(2, 4000, seed=5, sigma=sigma)
    crossed = np.abs(pred - true).max(axis=2) > 0.5 * BOX
    assert 0.01 < crossed.mean() < 0.06                 # about half of the 5 % at a face
    data = {"Coordinates": torch.from_numpy(pred).to(DEV), "InternalEnergy": torch.from_numpy(ptmp).to(DEV)}
    truth = {"Coordinates": torch.from_numpy(true), "InternalEnergy": torch.from_numpy(ttmp)}
    got = ops.frame_errors(data["Coordinates"], truth["Coordinates"].to(DEV), data["InternalEnergy"],
                           truth["InternalEnergy"].to(DEV), BOX).cpu()
    raw = rollout.calculate_errors(data, truth)
    for t in range(2):
        assert 0.5 * sigma ** 2 < float(got[t, 0]) < 2 * sigma ** 2
        assert raw["position_errors"][t] > 1e-3 * BOX ** 2                      # a box length for every crosser
        # calculate_errors sums 4000 float32 terms: within n 2^-24 = 2.4e-4 of the float64 mean
        assert abs(float(got[t, 1]) - raw["temperature_errors"][t]) <= 3e-4 * raw["temperature_errors"][t]


def test_rollout_statistics_on_a_rollout_of_the_tiny_golden_model(golden_tiny):
    g = golden_tiny
    model = graph_network.EncodeProcessDecode(int(g["latent"]), int(g["latent"]), int(g["nh"]), int(g["steps"]), 3)
    model.load_state_dict(g["state_dict"])
    model = model.to(DEV).eval()
    box, dt, k, w = float(g["box"]), float(g["dt"]), int(g["k"]), 5
    truth = {"Coordinates": torch.from_numpy(g["coords"]), "InternalEnergy": torch.from_numpy(g["energy"])}
    with torch.no_grad():
        pred = rollout.rollout(model, truth, g["metadata"], 0.0, dt, box, w, k, num_steps=3)
    assert pred["Coordinates"].shape == (w + 3, 256, 3)
    edges = np.linspace(0.0, 0.3 * box, 9)
    stats = statistics.rollout_statistics(pred, truth, box, edges)
    assert stats["frames"] == list(range(6))            # the frames both hold
    for key in ("position_mse", "temperature_mse"):
        assert stats[key].shape == (6,) and stats[key].dtype == torch.float64 and not stats[key].is_cuda
        assert float(stats[key][:w].abs().max()) == 0.0                         # the window is copied from the truth
        assert float(stats[key][w]) > 0.0
    for t in range(6):
        one = statistics.correlation_function(pred["Coordinates"][t], box, edges)
        assert torch.equal(stats["counts_pred"][t], one["counts"]) and torch.equal(stats["xi_pred"][t], one["xi"])
        true_t = statistics.correlation_function(truth["Coordinates"][t].to(DEV), box, edges)
        assert torch.equal(stats["xi_true"][t], true_t["xi"])
        cross = statistics.correlation_function(pred["Coordinates"][t], box, edges, truth["Coordinates"][t].to(DEV))
        assert torch.equal(stats["xi_cross"][t], cross["xi"])
        assert torch.equal(one["counts"], _want(pcc.auto_counts(pred["Coordinates"][t].cpu().numpy(), box, edges)))
    errs = ops.frame_errors(pred["Coordinates"][:6], truth["Coordinates"].to(DEV), pred["InternalEnergy"][:6],
                            truth["InternalEnergy"].to(DEV), box).cpu()
    assert torch.equal(stats["position_mse"], errs[:, 0]) and torch.equal(stats["temperature_mse"], errs[:, 1])
    last = statistics.rollout_statistics(pred, truth, box, edges, frames=[5, 2])
    assert last["frames"] == [5, 2] and torch.equal(last["xi_pred"], stats["xi_pred"][[5, 2]])
    with pytest.raises(ValueError):
        statistics.rollout_statistics(pred, truth, box, edges, frames=[6])
