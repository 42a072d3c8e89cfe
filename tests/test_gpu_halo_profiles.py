"""GPU: ``cgnn_halo_profiles`` against the numpy restatement of its contract (tests/halo_profile_checks.py), bit for bit,
and the ``statistics`` layer on top of it.

Grids the cases reach (``_cells_per_axis`` restates the grid rule, ``pair_cells_per_axis`` of csrc/pair_walk.hpp, with this
kernel's caps: the largest G with cells no smaller than the last edge plus its margin, capped by G^3 <= N and 256): one
cell (last edge L / 2), G = 2 and 3 (all cells of an axis walked once), a power of two and another number under the
27-cell walk.  A work item is up to 8 centres of one cell and a tile is 256 candidates: 2, 65 and 300 centres, 130 centres
in one cell (sixteen full items and one of two) and 4096 particles in one cell (sixteen tiles) pass those edges."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import fof_checks as fc
import halo_profile_checks as hp
from cosmology_gnn_simulation_amd import _lib, ops, statistics, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOX = 25.0
HALF = float(np.float32(0.5) * np.float32(BOX))
SIZES = (1, 64, 300, 4096, 8192)
CENTRES = (1, 2, 65, 300)
GRIDS = (1, 2, 3, 8, 11)           # cells per axis aimed at; the cap G^3 <= N may hold a case below


def _cells_per_axis(n, box, reach):
    cap = 1
    while cap < 256 and (cap + 1) ** 3 <= n:
        cap += 1
    g = math.floor(box / (float(np.float32(reach)) * (1 + 1e-5) + 2e-5 * box))
    return max(1, min(g, 256, cap)), cap


def _reach(g):
    return HALF if g == 1 else float(np.float32(0.98 * BOX / g))


def _uniform(n, seed, box=BOX):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32) * np.float32(box)


def _edges(reach, nb=5, first=0.0):
    e = np.linspace(first, reach, nb + 1).astype(np.float32)
    e[-1] = np.float32(reach)
    return e


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _want(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _check(x, centres, edges, q=None, box=BOX):
    """The counts (and sums) equal the restatement's, and summed over the centres the pair counter's; returns them."""
    pos, cen = _dev(x), _dev(centres)
    if q is None:
        got = ops.halo_profiles(pos, cen, box, edges)
        want = hp.profiles(x, centres, box, edges)
        sums = None
    else:
        got, sums = ops.halo_profiles(pos, cen, box, edges, _dev(q))
        want, want_sums = hp.profiles(x, centres, box, edges, q)
        assert sums.dtype == torch.int64 and sums.shape == want_sums.shape
        assert torch.equal(sums.cpu(), _want(want_sums))
    assert got.dtype == torch.int64 and got.shape == (len(centres), len(edges) - 1)
    assert torch.equal(got.cpu(), _want(want))
    assert torch.equal(got.sum(0), ops.pair_counts(cen, box, edges, pos_b=pos))
    return got, sums


@pytest.mark.parametrize("n", SIZES)
def test_sweep_of_sizes_centres_and_grids(n):
    x = _uniform(n, seed=300 + n)
    met = set()
    for h in CENTRES:
        centres = _uniform(h, seed=400 + h)
        for g in GRIDS:
            reach = _reach(g)
            got_g, cap = _cells_per_axis(n, BOX, reach)
            assert got_g == min(g, cap)
            met.add(got_g)
            _check(x, centres, _edges(reach))
    assert met == {min(g, _cells_per_axis(n, BOX, 0.01)[1]) for g in GRIDS}


def test_more_than_two_work_items_in_one_cell():
    x = _uniform(4096, seed=1)
    reach = _reach(8)                                       # cells of side 3.125
    assert _cells_per_axis(4096, BOX, reach)[0] == 8
    inside = np.float32(3.2) + np.random.default_rng(2).random((130, 3), dtype=np.float32) * np.float32(2.9)
    assert (np.floor(inside / 3.125) == 1).all()            # all in cell (1, 1, 1): sixteen items of 8 and one of 2
    got, _ = _check(x, inside, _edges(reach))
    assert int(got.sum()) > 0
    both = np.concatenate([inside, _uniform(70, seed=3)])   # and further cells behind it in the item table
    _check(x, both, _edges(reach))


def test_a_crowded_neighbourhood_has_many_tiles_per_item():
    rng = np.random.default_rng(4)
    x = (np.float32(6.3) + rng.random((4096, 3), dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    reach = _reach(8)
    assert (np.floor(x / 3.125) == 2).all()                 # 4096 particles in cell (2, 2, 2): 16 tiles per item
    centres = np.concatenate([x[:3], np.array([[7.8, 7.8, 7.8], [5.0, 7.0, 9.5], [20.0, 20.0, 20.0]], dtype=np.float32),
                              _uniform(20, seed=5)])
    got, _ = _check(x, centres, _edges(reach, nb=32))
    assert int(got[3].sum()) == 4096                        # the cell's centre reaches every particle (2.6 < 3.06)
    q = rng.integers(-(1 << 20), (1 << 20) + 1, size=(4096, 4)).astype(np.int32)
    _check(x, centres, _edges(reach, nb=7), q)


def test_special_positions():
    x = _uniform(4096, seed=6)
    x[0] = [BOX, 0.0, BOX]                                  # a particle on the upper faces: the edge cell
    x[1] = [0.0, 0.0, 0.0]
    reach = _reach(8)
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))       # noqa: E731
    down = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))    # noqa: E731
    face = np.float32(3.125)
    centres = np.array([[BOX, BOX, BOX], [BOX, 5.0, 0.0], [0.0, 0.0, 0.0], [up(0.0), 12.0, down(BOX)],
                        [down(BOX), down(BOX), down(BOX)], [up(face), down(face), face], [down(2 * face), 9.0, up(face)]],
                       dtype=np.float32)
    centres = np.concatenate([centres, x[:60]])             # centres ON particles: d2 == 0
    for first in (0.0, 0.05):
        got, _ = _check(x, centres, _edges(reach, first=first))
        got1, _ = _check(x, centres, _edges(HALF, first=first))          # one cell
    zero = ops.halo_profiles(_dev(x), _dev(x[:60]), BOX, [0.0, 1e-6])
    # only the coincident particle -- and x[0] = (L, 0, L) and x[1] = (0, 0, 0) are one point of the periodic box
    assert zero.flatten().tolist() == [2, 2] + [1] * 58
    assert int(ops.halo_profiles(_dev(x), _dev(x[:60]), BOX, [1e-6, 2e-6]).sum()) == 0      # none with edges[0] > 0


@pytest.mark.parametrize("nb", (1, 32))
def test_one_bin_and_thirty_two(nb):
    x = _uniform(4096, seed=7)
    centres = np.concatenate([_uniform(65, seed=8), x[:5]])
    for first in (0.0, 0.3):
        _check(x, centres, _edges(_reach(3), nb=nb, first=first))
        _check(x, centres, _edges(_reach(11), nb=nb, first=first))


@pytest.mark.parametrize("c", (1, 2, 3, 4))
def test_weighted_sums(c):
    rng = np.random.default_rng(10 + c)
    x = _uniform(4096, seed=9)
    centres = np.concatenate([_uniform(70, seed=10), x[:4]])
    q = rng.integers(-(1 << 20), (1 << 20) + 1, size=(4096, c)).astype(np.int32)
    q[:8] = 1 << 20
    q[8:16] = -(1 << 20)
    q[16:24] = 0
    for g in (1, 3, 8):
        got, sums = _check(x, centres, _edges(_reach(g), nb=6), q)
    if c == 1:                                              # [N] values give [H, nb] sums
        flat = ops.halo_profiles(_dev(x), _dev(centres), BOX, _edges(_reach(8), nb=6), _dev(q[:, 0]))[1]
        assert flat.shape == (74, 6) and torch.equal(flat, sums[..., 0])
    # float values go through quantize_weights and equal the int32 path
    vals = torch.from_numpy(rng.standard_normal((4096, c)) * 3.0).to(DEV)
    edges = _edges(_reach(8), nb=6)
    for scale in (2.5, None, torch.tensor(7.0, dtype=torch.float64, device=DEV)):
        used = vals.abs().max() if scale is None else scale          # None: the largest |value| of the call
        weights = ops.quantize_weights(vals, used)
        assert weights.dtype == torch.int32 and int(weights.abs().max()) == 1 << 20
        want = ops.halo_profiles(_dev(x), _dev(centres), BOX, edges, weights)
        have = ops.halo_profiles(_dev(x), _dev(centres), BOX, edges, vals, scale)
        assert torch.equal(have[0], want[0]) and torch.equal(have[1], want[1])
        assert torch.equal(have[0], got)


def test_hygiene_same_bits_guard_rows_no_synchronisation_and_frames():
    x = np.stack([_uniform(4096, seed=20), _uniform(4096, seed=21),
                  synthetic.make_clustered_positions(4096, BOX, seed=2).numpy()])
    centres = np.stack([_uniform(130, seed=22), _uniform(130, seed=23), x[2, :130]])
    q = np.random.default_rng(24).integers(-(1 << 20), (1 << 20) + 1, size=(3, 4096, 3)).astype(np.int32)
    edges = _edges(_reach(8), nb=9)
    pos, cen, qd = _dev(x), _dev(centres), _dev(q)
    fvals = qd.to(torch.float32)
    counts, sums = ops.halo_profiles(pos, cen, BOX, edges, qd)
    assert counts.shape == (3, 130, 9) and sums.shape == (3, 130, 9, 3)
    for f in range(3):                                      # [T, N, 3] is the per-frame calls
        one = ops.halo_profiles(pos[f], cen[f], BOX, edges, qd[f])
        assert torch.equal(one[0], counts[f]) and torch.equal(one[1], sums[f])
        want = hp.profiles(x[f], centres[f], BOX, edges, q[f])
        assert torch.equal(counts[f].cpu(), _want(want[0])) and torch.equal(sums[f].cpu(), _want(want[1]))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = ops.halo_profiles(pos, cen, BOX, edges, qd)
        plain = ops.halo_profiles(pos, cen, BOX, edges)
        floats = ops.halo_profiles(pos, cen, BOX, edges, fvals)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again[0], counts) and torch.equal(again[1], sums) and torch.equal(plain, counts)
    assert torch.equal(floats[0], counts)
    # guard rows around the outputs of the C entry
    lib = _lib.load()
    h, nb, c, n = 130, 9, 3, 4096
    big_c = torch.full((h + 2, nb), -77, dtype=torch.int64, device=DEV)
    big_s = torch.full((h + 2, nb, c), -77, dtype=torch.int64, device=DEV)
    ws_bytes = lib.cgnn_halo_profiles_workspace_bytes(n, h)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    edges_c = (C.c_float * (nb + 1))(*[float(v) for v in edges])
    rc = lib.cgnn_halo_profiles(pos[2].data_ptr(), n, cen[2].data_ptr(), h, BOX, edges_c, nb, qd[2].data_ptr(), c,
                                big_c[1].data_ptr(), big_s[1].data_ptr(), ws.data_ptr(), ws_bytes,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(big_c[1:-1], counts[2]) and torch.equal(big_s[1:-1], sums[2])
    for guard in (big_c[0], big_c[-1], big_s[0], big_s[-1]):
        assert bool((guard == -77).all())
    with pytest.raises(ValueError, match="leaves"):
        ops.halo_profiles(pos[0], cen[0] + 30.0, BOX, edges, check_bounds=True)
    with pytest.raises(ValueError, match="leaves"):
        ops.halo_profiles(pos[0] - 1.0, cen[0], BOX, edges, check_bounds=True)
    assert torch.equal(ops.halo_profiles(pos[0], cen[0], BOX, edges, check_bounds=True), counts[0])


# ---- statistics ----------------------------------------------------------------------------------------------------
def _blobs(n, blobs, seed, box=BOX):
    """n particles: Gaussian blobs (centre, members, sigma) and a uniform rest, shuffled; wrapped into [0, box)."""
    rng = np.random.default_rng(seed)
    parts = [np.asarray(c) + rng.standard_normal((m, 3)) * s for c, m, s in blobs]
    parts.append(rng.random((n - sum(m for _, m, _ in blobs), 3)) * box)
    x = np.mod(np.concatenate(parts), box).astype(np.float32)
    x[x >= np.float32(box)] = 0.0
    return x[rng.permutation(n)]


def _profile_frame(x, temp=None, **kw):
    """statistics.halo_profiles of a frame against the restatement evaluated at the centres it returns."""
    n = len(x)
    res = statistics.halo_profiles(_dev(x), BOX, values=None if temp is None else _dev(temp), **kw)
    edges = torch.cat([res["r_lo"][:1], res["r_hi"]]).numpy()
    assert torch.equal(_want(edges.astype(np.float32).astype(np.float64)), _want(edges))
    ll = statistics.default_linking_length(n, BOX)
    labels = fc.fof_labels(x, BOX, ll)
    size, disp, _ = fc.catalogue(x, labels, BOX)
    roots, _ = hp.largest_groups(size, kw.get("min_members", 20), n)
    assert res["root"].tolist() == roots and res["size"].tolist() == [int(size[r]) for r in roots]
    assert len(roots) >= 2
    centres32 = res["centre"].to(torch.float32)
    assert torch.equal(centres32.to(torch.float64), res["centre"])
    want_c = fc.centres(x, np.asarray(roots), size, disp, BOX).astype(np.float32)
    assert torch.equal(centres32, _want(want_c))
    counts = hp.profiles(x, centres32.numpy(), BOX, edges)
    assert res["counts"].dtype == torch.int64 and torch.equal(res["counts"], _want(counts))
    shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3) * n / BOX ** 3
    np.testing.assert_allclose(res["density"].numpy(), counts / shell, rtol=1e-14)
    rd, md = hp.so_masses(counts, n, BOX, edges, kw.get("delta", 200.0))
    assert torch.isnan(res["r_delta"]).tolist() == np.isnan(rd).tolist()
    assert torch.isnan(res["m_delta"]).tolist() == np.isnan(md).tolist()
    ok = ~np.isnan(rd)
    np.testing.assert_allclose(res["r_delta"].numpy()[ok], rd[ok], rtol=1e-10)
    np.testing.assert_allclose(res["m_delta"].numpy()[ok], md[ok], rtol=1e-10)
    if temp is not None:
        scale = float(np.abs(temp).max())
        q = ops.quantize_weights(torch.from_numpy(temp), scale).numpy()
        _, sums = hp.profiles(x, centres32.numpy(), BOX, edges, q)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(counts > 0, sums / np.maximum(counts, 1) * (scale / 2 ** 20), np.nan)
        np.testing.assert_allclose(res["mean_value"].numpy(), mean, rtol=1e-12, equal_nan=True)
        assert bool(torch.isnan(res["mean_value"]).any()) or bool((res["counts"] > 0).all())
    return res, counts, edges


def test_statistics_halo_profiles_on_a_clustered_frame():
    x = synthetic.make_clustered_positions(8192, BOX, seed=3).numpy()
    temp = (1.0 + np.random.default_rng(30).random(8192) * 4.0).astype(np.float32)
    res, counts, edges = _profile_frame(x, temp)
    assert len(edges) == 25 and res["counts"].shape[1] == 24
    assert int((~torch.isnan(res["m_delta"])).sum()) >= 1


def test_statistics_halo_profiles_on_two_blobs_and_the_so_mass_of_a_compact_one():
    n = 2000
    blobs = [((5.0, 5.0, 5.0), 600, 0.05), ((24.95, 12.0, 0.05), 300, 0.05)]     # the second across two faces
    x = _blobs(n, blobs, seed=31)
    res, counts, edges = _profile_frame(x)
    assert res["size"][:2].tolist() == [600, 300] or res["size"][0] >= 600
    for hh in (0, 1):
        r, m = float(res["r_delta"][hh]), float(res["m_delta"][hh])
        assert not math.isnan(r)
        c = res["centre"][hh].numpy()
        d = x.astype(np.float64) - c
        d -= BOX * np.round(d / BOX)
        inside = int(((d * d).sum(axis=1) < r * r).sum())
        shell = int(np.searchsorted(edges, r, side="right")) - 1
        # m_delta is the power-law interpolation of N(< r) between the two edges around r_delta: it differs from the
        # brute-force count inside r_delta by at most the particles of that shell (and the rounding of the dozen
        # float64 operations behind m_delta, 1e-10 relative as above, where the shell is empty)
        assert abs(m - inside) <= counts[hh, shell] + 1e-10 * m
        assert abs(m - blobs[hh][1]) <= 0.05 * blobs[hh][1]
    # other radii, another delta, a higher minimum
    _profile_frame(x, edges=[0.0, 0.1, 0.3, 1.0, 2.0, 3.0, 6.0], delta=500.0, min_members=100)
    none = statistics.halo_profiles(_dev(_uniform(500, seed=32)), BOX)
    nb = statistics.default_radial_edges(500, BOX).numel() - 1              # the radii beyond half the box are dropped
    assert nb < 24 and none["root"].numel() == 0 and none["counts"].shape == (0, nb) and none["m_delta"].shape == (0,)


def _frame_reference(x, t, scale, edges, min_members, delta):
    """Every listed group of one frame, largest first: roots, sizes, per-halo counts, sums, r_delta and m_delta."""
    n = len(x)
    labels = fc.fof_labels(x, BOX, statistics.default_linking_length(n, BOX))
    size, disp, _ = fc.catalogue(x, labels, BOX)
    roots, _ = hp.largest_groups(size, min_members, n)
    nb = len(edges) - 1
    if roots:
        cen = fc.centres(x, np.asarray(roots), size, disp, BOX).astype(np.float32)
        counts, sums = hp.profiles(x, cen, BOX, edges, ops.quantize_weights(torch.from_numpy(t), scale).numpy())
        rd, md = hp.so_masses(counts, n, BOX, edges, delta)
    else:
        counts = sums = np.zeros((0, nb), dtype=np.int64)
        rd = md = np.zeros(0)
    return dict(roots=roots, sizes=np.asarray([int(size[r]) for r in roots], dtype=np.int64), counts=counts, sums=sums,
                rd=rd, md=md)


def _stacks(ref, size_edges, max_halos):
    """The restatement of one frame of one side of rollout_halo_profiles from the frame's per-halo reference."""
    k = min(max_halos, len(ref["roots"]))
    sizes, md, rd = ref["sizes"][:k], ref["md"][:k], ref["rd"][:k]
    counts, num = hp.stack(ref["counts"][:k], sizes, size_edges)
    sums, _ = hp.stack(ref["sums"][:k], sizes, size_edges)
    ok = ~np.isnan(md)
    msum, nd = hp.stack(md[ok], sizes[ok], size_edges)
    rsum, _ = hp.stack(rd[ok], sizes[ok], size_edges)
    return dict(left=len(ref["roots"]) - k, counts=counts, num=num, sums=sums, msum=msum, rsum=rsum, nd=nd)


def test_rollout_halo_profiles_stacks_truncates_visibly_and_survives_an_empty_frame():
    n = 1000
    two40 = [((5.0, 5.0, 5.0), 200, 0.05), ((24.95, 12.0, 0.05), 120, 0.05), ((12.0, 20.0, 8.0), 40, 0.03),
             ((18.0, 3.0, 15.0), 40, 0.03), ((9.0, 9.0, 20.0), 25, 0.03)]
    other = [((6.0, 5.0, 5.0), 180, 0.08), ((1.0, 12.0, 24.0), 130, 0.05), ((12.0, 20.0, 8.0), 60, 0.03)]
    truth = np.stack([_blobs(n, two40, 40), _blobs(n, other, 41), _uniform(n, seed=42)])
    pred = np.stack([_blobs(n, other, 43), _blobs(n, two40, 44), _uniform(n, seed=45)])
    rng = np.random.default_rng(46)
    t_true = (1.0 + rng.random((3, n)) * 4.0).astype(np.float32)
    t_pred = (2.0 + rng.random((3, n, 1)) * 9.0).astype(np.float32)
    data = {"Coordinates": _dev(pred), "InternalEnergy": _dev(t_pred)}
    gt = {"Coordinates": _dev(truth), "InternalEnergy": _dev(t_true)}
    size_edges = [20, 50, 150, 1000]
    edges = statistics.default_radial_edges(n, BOX).numpy()
    nb = len(edges) - 1
    shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3) * n / BOX ** 3
    sides = {"true": (truth, t_true), "pred": (pred, t_pred.reshape(3, n))}
    scales = {name: float(np.abs(t).max()) for name, (_, t) in sides.items()}
    refs = {name: [_frame_reference(x, t, scales[name], edges, size_edges[0], 200.0) for x, t in zip(*sides[name])]
            for name in sides}
    assert [len(r["roots"]) for r in refs["true"]] == [5, 3, 0] and [len(r["roots"]) for r in refs["pred"]] == [3, 5, 0]
    assert refs["true"][0]["sizes"].tolist() == [200, 120, 40, 40, 25]
    statistics.rollout_halo_profiles(data, gt, BOX, size_edges=size_edges)           # warm: library, allocator
    scale_true = gt["InternalEnergy"].abs().max().to(torch.float64)
    for max_halos in (1024, 3):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                                      # up to the final transfer
        try:
            dev_side = statistics.halo_profile_stacks_on_device(
                gt["Coordinates"], BOX, statistics.default_linking_length(n, BOX), size_edges, [float(v) for v in edges],
                max_halos, 200.0, (gt["InternalEnergy"], scale_true))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        res = statistics.rollout_halo_profiles(data, gt, BOX, size_edges=size_edges, max_halos=max_halos)
        assert res["frames"] == [0, 1, 2] and res["size_lo"].tolist() == [20, 50, 150]
        assert torch.equal(dev_side[0][:, 0].cpu(), res["not_profiled_true"])
        assert torch.equal(dev_side[0][:, 7:7 + 3 * nb].cpu().reshape(3, 3, nb), res["counts_true"])
        for name in sides:
            assert res["counts_" + name].shape == (3, 3, nb) and res["counts_" + name].dtype == torch.int64
            for f in range(3):
                r = _stacks(refs[name][f], size_edges, max_halos)
                assert int(res["not_profiled_" + name][f]) == r["left"] == max(len(refs[name][f]["roots"]) - max_halos, 0)
                assert torch.equal(res["counts_" + name][f], _want(r["counts"]))
                assert res["n_halos_" + name][f].tolist() == r["num"].tolist()
                assert res["n_delta_" + name][f].tolist() == r["nd"].tolist()
                with np.errstate(invalid="ignore", divide="ignore"):
                    np.testing.assert_allclose(res["m_delta_" + name][f].numpy(), r["msum"] / r["nd"], rtol=1e-10)
                    np.testing.assert_allclose(res["r_delta_" + name][f].numpy(), r["rsum"] / r["nd"], rtol=1e-10)
                    np.testing.assert_allclose(res["density_" + name][f].numpy(),
                                               r["counts"] / (r["num"][:, None] * shell), rtol=1e-13)
                    np.testing.assert_allclose(res["temperature_" + name][f].numpy(),
                                               r["sums"] / r["counts"] * (scales[name] / 2 ** 20), rtol=1e-12)
            # the frame without a listed group: zeros and nan, no fault
            assert int(res["counts_" + name][2].sum()) == 0 and res["n_halos_" + name][2].tolist() == [0, 0, 0]
            assert bool(torch.isnan(res["m_delta_" + name][2]).all()) and bool(torch.isnan(res["density_" + name][2]).all())
        if max_halos == 3:
            # exactly the largest groups, the tie of the two groups of 40 to the smaller root: the other one and the
            # group of 25 are counted as not profiled
            assert res["not_profiled_true"].tolist() == [2, 0, 0] and res["not_profiled_pred"].tolist() == [0, 2, 0]
            ref0 = refs["true"][0]
            assert ref0["roots"][2] < ref0["roots"][3] and res["n_halos_true"][0].tolist() == [1, 1, 1]
            assert torch.equal(res["counts_true"][0, 0], _want(ref0["counts"][2]))
            assert not np.array_equal(ref0["counts"][2], ref0["counts"][3])
        else:
            assert int(res["not_profiled_true"].sum()) == 0 and res["n_halos_true"][0].tolist() == [3, 1, 1]
            assert int((res["n_delta_true"] > 0).sum()) > 0
    # frames select and order; without a temperature there is no temperature profile
    sel = statistics.rollout_halo_profiles({"Coordinates": data["Coordinates"]}, {"Coordinates": gt["Coordinates"]}, BOX,
                                           size_edges=size_edges, frames=[1])
    assert "temperature_pred" not in sel and sel["frames"] == [1]
    assert torch.equal(sel["counts_true"][0], res["counts_true"][1])
