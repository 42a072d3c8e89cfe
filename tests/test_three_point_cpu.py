"""CPU: the contract of ``cgnn_triplet_moments`` as tests/three_point_checks.py restates it, on cases known by hand (a
cubic lattice, points on lines, coincident points), the derived bound against float64 directions, the Legendre and
multinomial coefficients, the host arithmetic of ``statistics.three_point_from_sums`` / ``three_point_zeta``, the texts
of the header and the Makefile, and the host refusals of the C entry, of ``ops.triplet_moments`` and of the
``statistics`` layer, all before any device work."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import three_point_checks as tp
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib, ops, statistics

ENTRIES = ("cgnn_triplet_moments_workspace_bytes", "cgnn_triplet_moments")


# ---- the coefficients --------------------------------------------------------------------------------------------------
def test_the_monomial_listing_and_its_multinomials():
    assert [len(tp.monomials(l)) for l in range(5)] == [1, 4, 10, 20, 35] == [ops.triplet_monomials(l) for l in range(5)]
    assert tp.monomials(2) == [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0),
                               (0, 1, 1), (0, 0, 2)]
    assert tp.multinomials(2) == [1, 1, 1, 1, 1, 2, 2, 1, 2, 1]
    for n, sl in enumerate(tp.degree_slices(4)):
        assert all(sum(e) == n for e in tp.monomials(4)[sl]) and sum(tp.multinomials(4)[sl]) == 3 ** n


def test_legendre_coefficients_and_multinomials_reproduce_numpy_on_random_unit_vectors():
    rng = np.random.default_rng(0)
    u, w = rng.standard_normal((2, 200, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    cos = (u * w).sum(axis=1)
    mono, mult = tp.monomials(4), tp.multinomials(4)
    power = np.zeros((5, 200))
    for (a, b, c), m in zip(mono, mult):
        power[a + b + c] += m * (u[:, 0] ** a * u[:, 1] ** b * u[:, 2] ** c) * (w[:, 0] ** a * w[:, 1] ** b * w[:, 2] ** c)
    for n in range(5):
        assert np.abs(power[n] - cos ** n).max() <= 1e-14
    coef = tp.legendre_matrix(4)
    assert torch.equal(statistics.legendre_coefficients(4), torch.from_numpy(coef))
    assert torch.equal(statistics.legendre_coefficients(2), torch.from_numpy(coef[:3, :3]))
    for l in range(5):
        want = np.polynomial.legendre.legval(cos, [0.0] * l + [1.0])
        assert np.abs(coef[l] @ power - want).max() <= 1e-14


# ---- the restatement on cases known by hand ------------------------------------------------------------------------------
@pytest.mark.parametrize("unit_bits", (6, 20))
def test_a_cubic_lattice_has_ddd_36_0_0_0_21_per_primary(unit_bits):
    x, box = tp.cubic_lattice(6, 1.0)
    edges = [0.9, 1.1]                                       # the 6 nearest neighbours and nothing else
    m, pairs = tp.moments(x, box, edges, 4, unit_bits=unit_bits)
    assert m.shape == (216, 1, 35) and (m[:, 0, 0] == 6).all() and pairs.tolist() == [6 * 216]
    one = 1 << unit_bits
    # directions (+-1, 0, 0) and permutations: the odd monomials cancel, x^2, y^2, z^2 and their fourth powers give 2
    for al, (a, b, c) in enumerate(tp.monomials(4)):
        pure_even = sorted((a, b, c))[:2] == [0, 0] and (a + b + c) % 2 == 0 and a + b + c > 0
        assert (m[:, 0, al] == (6 if al == 0 else 2 * one if pure_even else 0)).all(), (a, b, c)
    t, abs_sum, terms = tp.power_sums(m, 4)
    assert terms == [216, 648, 1296, 2160, 3240]
    ddd = tp.ddd_from_power_sums(t, unit_bits)
    assert (ddd[:, 0, 0] / 216 == np.array([36.0, 0.0, 0.0, 0.0, 21.0])).all()
    # without j == k: 30 ordered pairs, 6 opposite and 24 at right angles
    assert (tp.ddd_from_power_sums(t, unit_bits, pairs)[:, 0, 0] / 216 == np.array([30.0, -6.0, -6.0, -6.0, 15.0])).all()
    res = statistics.three_point_from_sums(np.array(t, dtype=np.float64), 216, 216, box, edges, unit_bits)
    assert (res["ddd"][:, 0, 0].numpy() / 216 == np.array([36.0, 0.0, 0.0, 0.0, 21.0])).all()


def test_auto_skips_the_primary_and_coincident_points_count_for_nothing():
    x = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.5, 1.0, 1.0], [7.75, 1.0, 1.0]], dtype=np.float32)
    m, pairs = tp.moments(x, 8.0, [0.0, 1.0, 2.0], 1)
    # 0 and 1 coincide: each sees 2 (+x, bin 0) and 3 (-x across the face, 1.25: bin 1); 2 sees 0 and 1 (-x) and 3 (bin 1)
    assert m[:, :, 0].tolist() == [[1, 1], [1, 1], [2, 1], [0, 3]] and pairs.tolist() == [4, 6]
    one = 1 << 20
    assert m[0, :, 1].tolist() == [one, -one] and m[2, :, 1].tolist() == [-2 * one, -one] and m[3, 1, 1] == 3 * one
    assert (m[:, :, 2:] == 0).all()
    # cross: a query on a particle does not count it, with edges[0] == 0 either
    q = np.array([[1.0, 1.0, 1.0], [4.0, 4.0, 4.0]], dtype=np.float32)
    mq, pq = tp.moments(q, 8.0, [0.0, 1.0, 2.0], 1, pos_b=x)
    assert mq[:, :, 0].tolist() == [[1, 1], [0, 0]] and pq.tolist() == [1, 1]


def test_points_on_lines_have_only_collinear_triplets():
    box, reach = 40.0, 4.0
    x = tp.line_points(box, reach, per_line=14, seed=3)
    edges = [0.3, 1.5, 2.7, 4.0]
    m, pairs = tp.moments(x, box, edges, 4)
    star = tp.float64_moments(x, box, edges, 4)
    assert int(pairs.sum()) > 200
    ddd = tp.ddd_from_power_sums(tp.power_sums(m, 4)[0], 20)
    want = tp.ddd_float64(x, box, edges, 4)
    bound = tp.ddd_bound(m, star, 4, 20)
    assert (np.abs(ddd - want) <= bound).all()
    # every cosine is +-1 (to the rounding of the positions): P_2 = P_4 = P_0 and P_3 = P_1
    for hi, lo in ((2, 0), (4, 0), (3, 1)):
        assert np.abs(want[hi] - want[lo]).max() <= 1e-9 * want[0].max()
        assert (np.abs(ddd[hi] - ddd[lo]) <= bound[hi] + bound[lo] + 1e-9 * want[0].max()).all()
    assert want[0].min() > 0 and np.abs(want[1]).max() < want[0].max()


@pytest.mark.parametrize("unit_bits", (6, 20))
def test_the_derived_bound_against_float64_directions(unit_bits):
    rng = np.random.default_rng(11)
    x = rng.random((300, 3), dtype=np.float32) * np.float32(10.0)
    edges = [0.2, 1.0, 1.8, 2.6]
    m, pairs = tp.moments(x, 10.0, edges, 4, unit_bits=unit_bits)
    star = tp.float64_moments(x, 10.0, edges, 4)
    assert (m[:, :, 0] == np.rint(star[:, :, 0])).all() and int(pairs.min()) > 300
    err = np.abs(m.astype(np.float64) - star * 2.0 ** unit_bits)
    bound = tp.moment_bound(m, 4, unit_bits)
    assert (err[:, :, 1:] <= bound[:, :, 1:]).all()         # alpha = 0 is the count, compared above
    assert err[:, :, 1:].max() > 0                                     # the quantisation is there
    ddd = tp.ddd_from_power_sums(tp.power_sums(m, 4)[0], unit_bits)
    want = tp.ddd_float64(x, 10.0, edges, 4)
    assert (np.abs(ddd - want) <= tp.ddd_bound(m, star, 4, unit_bits)).all()
    assert (ddd[0] == want[0]).all()                         # counts: exact
    # cross mode, other primaries
    q = rng.random((40, 3), dtype=np.float32) * np.float32(10.0)
    mq, _ = tp.moments(q, 10.0, edges, 3, pos_b=x, unit_bits=unit_bits)
    sq = tp.float64_moments(q, 10.0, edges, 3, pos_b=x)
    assert (np.abs(mq.astype(np.float64) - sq * 2.0 ** unit_bits) <= tp.moment_bound(mq, 3, unit_bits))[:, :, 1:].all()
    assert (mq[:, :, 0] == np.rint(sq[:, :, 0])).all()
    # a lower lmax is a prefix of a higher one
    assert (tp.moments(x, 10.0, edges, 2, unit_bits=unit_bits)[0] == m[:, :, :10]).all()


def test_power_sums_are_exact_integers_with_their_precondition():
    rng = np.random.default_rng(12)
    x = rng.random((60, 3), dtype=np.float32) * np.float32(6.0)
    m, _ = tp.moments(x, 6.0, [0.0, 1.5, 3.0], 3, unit_bits=6)
    t, abs_sum, terms = tp.power_sums(m, 3)
    assert tp.exact_in_float64(abs_sum) and terms == [60, 180, 360, 600]
    assert all(isinstance(v, int) for v in t.reshape(-1)) and (t == t.transpose(0, 2, 1)).all()
    assert int(t[0, 0, 1]) == int((m[:, 0, 0] * m[:, 1, 0]).sum())
    assert int(t[1, 0, 0]) == int((m[:, 0, 1:4] ** 2).sum())
    big = np.full((4, 1, 4), 1 << 40, dtype=np.int64)
    assert not tp.exact_in_float64(tp.power_sums(big, 1)[1])


# ---- host arithmetic ---------------------------------------------------------------------------------------------------
def test_three_point_from_sums_on_hand_made_sums():
    box, edges, ub = 10.0, [1.0, 2.0, 3.0], 4
    one = 2.0 ** (2 * ub)
    t = np.zeros((3, 2, 2))
    t[0] = [[8.0, 6.0], [6.0, 18.0]]
    t[1] = np.array([[2.0, -1.0], [-1.0, 3.0]]) * one
    t[2] = np.array([[4.0, 2.0], [2.0, 6.0]]) * one
    pairs = np.array([4, 6], dtype=np.int64)
    res = statistics.three_point_from_sums(t, 5, 50, box, edges, ub)
    assert set(res) == {"ddd", "triplet", "r_lo", "r_hi"} and res["ddd"].dtype == torch.float64
    assert res["r_lo"].tolist() == [1.0, 2.0] and res["r_hi"].tolist() == [2.0, 3.0]
    want = np.stack([t[0], t[1] / one, 1.5 * t[2] / one - 0.5 * t[0]])
    assert np.array_equal(res["ddd"].numpy(), want)
    vol = 4.0 * np.pi / 3.0 * np.array([7.0, 19.0])
    norm = 5 * (50 / 1000.0) ** 2 * vol[:, None] * vol[None, :]
    ell = np.array([1.0, 3.0, 5.0])[:, None, None]
    np.testing.assert_allclose(res["triplet"].numpy(), ell * want / norm, rtol=1e-14)
    # the degenerate triangles leave the diagonal, for every l, and only there
    cut = statistics.three_point_from_sums(t, 5, 50, box, edges, ub, pairs)
    diff = (res["ddd"] - cut["ddd"]).numpy()
    assert np.array_equal(diff, np.broadcast_to(np.diag([4.0, 6.0]), (3, 2, 2)))
    assert np.array_equal(cut["ddd"].numpy(), tp.ddd_from_power_sums(t, ub, pairs))
    # frames
    both = statistics.three_point_from_sums(np.stack([t, 2 * t]), 5, 50, box, edges, ub, np.stack([pairs, pairs]))
    assert both["ddd"].shape == (2, 3, 2, 2) and torch.equal(both["ddd"][0], cut["ddd"])
    for kw, text in ((dict(T=t[:, :, :1]), "T must be"), (dict(edges=[1.0, 2.0]), "bins"), (dict(n_primaries=0), "n_primaries"),
                     (dict(unit_bits=21), "unit_bits"), (dict(pairs=np.zeros(3, dtype=np.int64)), "pairs must hold"),
                     (dict(pairs=np.zeros(2)), "pairs must hold")):
        args = dict(T=t, n_primaries=5, n_partners=50, box_size=box, edges=edges, unit_bits=ub)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            statistics.three_point_from_sums(**args)


def test_zeta_assembled_from_two_hand_made_calls():
    box, edges, n, nq = 10.0, [1.0, 2.0, 3.0], 40, 30
    rng = np.random.default_rng(2)
    one = 2.0 ** 40

    def sums():
        t = rng.random((3, 2, 2)) * 50.0
        t = t + t.transpose(0, 2, 1)
        t[1:] *= one
        return t

    td, tq = sums(), sums()
    pd, pq = np.array([30, 70], dtype=np.int64), np.array([25, 60], dtype=np.int64)
    res = statistics.three_point_zeta(td, pd, tq, pq, n, nq, box, edges)
    zeta, full, trip_q, xi = tp.zeta_on_host(td, pd, tq, pq, n, nq, box, edges)
    for key, want in (("zeta", zeta), ("zeta_full", full), ("triplet_queries", trip_q), ("xi", xi)):
        np.testing.assert_allclose(res[key].numpy(), want, rtol=1e-13, atol=1e-13)
    assert torch.equal(res["pairs"], torch.from_numpy(pd)) and res["r_hi"].tolist() == [2.0, 3.0]
    # delta_{l0}: the xi terms and the 1 enter l = 0 alone
    d = statistics.three_point_from_sums(td, n, n, box, edges, 20, pd)["triplet"]
    q = statistics.three_point_from_sums(tq, nq, n, box, edges, 20, pq)["triplet"]
    assert torch.equal(res["zeta"][1:], (d - q)[1:]) and torch.equal(res["zeta_full"][1:], d[1:])
    np.testing.assert_allclose((d - q - res["zeta"])[0].numpy(), xi[:, None] + xi[None, :], rtol=1e-12)
    np.testing.assert_allclose((d - res["zeta_full"])[0].numpy(), np.ones((2, 2)), rtol=1e-12)
    vol = 4.0 * np.pi / 3.0 * np.array([7.0, 19.0])
    np.testing.assert_allclose(xi, pd / (n * n / 1000.0 * vol) - 1.0, rtol=1e-14)
    # uncorrelated neighbours: S_0 = N (nbar V)^2 off the diagonal, xi = 0, no odd or quadrupole sums -> zeta = 0
    nbar = n / 1000.0
    flat = np.zeros((3, 2, 2))
    flat[0] = n * nbar * nbar * vol[:, None] * vol[None, :]
    flat[2] = flat[0] / 3.0 * one                           # <cos^2> = 1 / 3
    pairs = np.rint(n * nbar * vol).astype(np.int64)
    res = statistics.three_point_zeta(flat, pairs, flat * (nq / n), pairs, n, nq, box, edges)
    off = res["zeta"][:, 0, 1].numpy()
    assert np.abs(off[1:]).max() < 1e-12 and abs(off[0] + float(res["xi"].sum())) < 1e-12
    assert float(res["xi"].abs().max()) < 0.05              # the rounded pair counts


def test_default_three_point_edges():
    e = statistics.default_three_point_edges(10 ** 6, 100.0)       # spacing 1
    assert e.dtype == torch.float64 and e.shape == (9,) and torch.equal(e, e.to(torch.float32).to(torch.float64))
    np.testing.assert_allclose(e.numpy(), np.linspace(0.5, 4.5, 9), rtol=1e-6)
    ops.check_triplet_arguments(e, 100.0, 4, 20, "test")
    small = statistics.default_three_point_edges(512, 8.0)         # spacing 1, half the box is 4
    assert small.tolist() == [0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
    assert statistics.default_three_point_edges(8, 2.0).tolist() == [0.5, 1.0]
    for bad in (7, 0, -1):
        with pytest.raises(ValueError, match="at least 8"):
            statistics.default_three_point_edges(bad, 8.0)
    with pytest.raises(ValueError, match="box_size"):
        statistics.default_three_point_edges(100, 0.0)


# ---- refusals before any device work -----------------------------------------------------------------------------------
def test_ops_and_statistics_refuse_on_the_host():
    pos = torch.zeros((10, 3))
    with pytest.raises(ValueError, match="17 bins"):
        ops.triplet_moments(pos, 8.0, np.linspace(0.0, 4.0, 18))
    assert len(ops.check_triplet_arguments(np.linspace(0.0, 4.0, 17), 8.0, 4, 20, "test")) == 17       # 16 bins pass
    with pytest.raises(ValueError, match="ascend"):
        ops.triplet_moments(pos, 8.0, [0.0, 2.0, 1.0])
    with pytest.raises(ValueError, match="half the box"):
        ops.triplet_moments(pos, 8.0, [0.0, 4.5])
    with pytest.raises(ValueError, match="box_size"):
        ops.triplet_moments(pos, -8.0, [0.0, 1.0])
    for bad in (5, -1, 2.0, True):
        with pytest.raises(ValueError, match="lmax"):
            ops.triplet_moments(pos, 8.0, [0.0, 1.0], bad)
    for bad in (0, 21, 20.0, True):
        with pytest.raises(ValueError, match="unit_bits"):
            ops.triplet_moments(pos, 8.0, [0.0, 1.0], unit_bits=bad)
    with pytest.raises(_lib.CgnnError, match="no CPU path"):
        ops.triplet_moments(pos, 8.0, [0.0, 1.0])
    with pytest.raises(ValueError, match="17 bins"):
        statistics.three_point_correlation(pos, 8.0, np.linspace(0.0, 4.0, 18))
    with pytest.raises(ValueError, match="lmax"):
        statistics.three_point_correlation(pos, 8.0, lmax=5)
    with pytest.raises(ValueError, match="exclude each other"):
        statistics.three_point_correlation(pos, 8.0, queries=torch.zeros((4, 3)), n_query_axis=2)
    with pytest.raises(ValueError, match="queries must be"):
        statistics.three_point_correlation(pos, 8.0, queries=torch.zeros((4, 2)))
    with pytest.raises(ValueError, match="at least 8"):
        statistics.three_point_correlation(torch.zeros((5, 3)), 8.0)
    with pytest.raises(ValueError, match="pos must be"):
        statistics.three_point_correlation(torch.zeros((10, 2)), 8.0, [0.0, 1.0])
    data = {"Coordinates": torch.zeros((3, 100, 3))}
    with pytest.raises(ValueError, match="half the box"):
        statistics.rollout_three_point(data, data, 8.0, edges=[0.0, 5.0])
    with pytest.raises(ValueError, match="frames must be"):
        statistics.rollout_three_point(data, data, 8.0, frames=[3])
    with pytest.raises(_lib.CgnnError, match="no CPU path"):
        statistics.three_point_correlation(pos, 8.0)
    with pytest.raises(_lib.CgnnError, match="no CPU path"):
        statistics.rollout_three_point(data, data, 8.0)


# ---- the C entry -------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_built_and_documented():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert name + "(" in header and name in notes
    assert "1 <= num_bins <= 16, 0 <= lmax <= 4, 1 <= unit_bits <= 20" in header
    assert callable(ops.triplet_moments) and callable(ops.check_triplet_arguments)
    for fn in ("three_point_from_sums", "three_point_zeta", "three_point_correlation", "rollout_three_point",
               "default_three_point_edges", "legendre_coefficients"):
        assert callable(getattr(statistics, fn))
    makefile = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "Makefile")).read()
    assert "three_point.hip" in makefile
    assert "FLAGS_three_point := -ffp-contract=off -DCGNN_PAIR_CONTRACT_OFF\n" in makefile
    deps = [line for line in makefile.splitlines() if line.startswith("$(BUILD)/") and "three_point.o" in line]
    assert sorted(line.split(": ")[1] for line in deps) == ["cell_grid.hpp", "pair_walk.hpp"]
    assert "fast-math" not in makefile.split("FLAGS_three_point :=")[1].split("\n")[0]
    for doc in ("README.md", "DESIGN.md"):
        assert "triplet_moments" in open(os.path.join(ROOT, doc)).read()
    assert (_lib.THREE_POINT_MAX_BINS, _lib.THREE_POINT_MAX_L, _lib.THREE_POINT_MAX_UNIT_BITS) == (16, 4, 20)


def test_workspace_size_and_the_host_refusals_of_the_c_entry():
    """The refusals come before any launch: no GPU is needed to meet them, and no pointer is dereferenced."""
    lib = _lib.load()
    wsb = lib.cgnn_triplet_moments_workspace_bytes
    for bad in ((0, 0, 4, 8), (-1, 0, 4, 8), (5, -1, 4, 8), (2 ** 31, 0, 4, 8), (5, 2 ** 31, 4, 8), (5, 0, 5, 8), (5, 0, -1, 8),
                (5, 0, 4, 0), (5, 0, 4, 17)):
        assert wsb(*bad) == 256, bad
    # the pair job's layout (per particle a sorted float4 and a cell id, the cell tables) plus a second float4 per
    # primary (their order within a cell) and, per workgroup of the
    # walk -- one per possible work item, 2048 at most -- a float64 per (n, b1 <= b2) and an int64 per bin
    for n_a, n_b, lmax, nb in ((1, 0, 0, 1), (4096, 0, 4, 8), (300, 4096, 2, 16), (10 ** 6, 0, 4, 8)):
        partners = n_b or n_a
        blocks = min(2048, min(8 * partners, n_a) + n_a // 8 + 1)
        tables = blocks * ((lmax + 1) * nb * (nb + 1) // 2 + nb) * 8
        assert 36 * n_a + 20 * n_b <= wsb(n_a, n_b, lmax, nb) <= 36 * n_a + 20 * n_b + 11 * (8 * partners + 1) * 4 + \
            4 * (n_a + n_a // 8 + 1) + tables + 24 * 256, (n_a, n_b, lmax, nb)
    assert wsb(4096, 0, 4, 8) > wsb(4096, 0, 2, 8) > wsb(4096, 0, 2, 4) and wsb(300, 4096, 4, 8) > wsb(300, 0, 4, 8)
    fake, odd = 1 << 20, (1 << 20) + 4                  # never dereferenced: every call below is refused on the host
    inv, unsup, short = -1, -2, -3                      # CGNN_ERR_INVALID_ARG, _UNSUPPORTED, _WORKSPACE
    half = float(np.float32(0.5))

    def arr(*v):
        return (C.c_float * len(v))(*v)

    def call(pos=fake, n=100, pos_b=None, n_b=0, box=1.0, edges=arr(0.0, 0.1, 0.2), nb=2, lmax=4, ub=20, sums=fake,
             pairs=fake, moments=None, w=fake, wb=1 << 30):
        return lib.cgnn_triplet_moments(pos, n, pos_b, n_b, box, edges, nb, lmax, ub, sums, pairs, moments, w, wb, None)

    for kw in (dict(pos=None), dict(edges=None), dict(sums=None), dict(pairs=None), dict(w=None), dict(n=0), dict(n=-4),
               dict(pos_b=fake, n_b=0), dict(box=0.0), dict(box=-1.0), dict(box=float("inf")), dict(box=float("nan"))):
        assert call(**kw) == inv, kw
    assert call(nb=0) == inv and call(edges=arr(*np.linspace(0, 0.4, 18)), nb=17) == inv
    assert lib.cgnn_last_error().decode() == "cgnn_triplet_moments: num_bins=17 outside [1, 16]"
    assert call(lmax=5) == inv and lib.cgnn_last_error().decode() == "cgnn_triplet_moments: lmax=5 outside [0, 4]"
    assert call(lmax=-1) == inv
    assert call(ub=21) == inv and lib.cgnn_last_error().decode() == "cgnn_triplet_moments: unit_bits=21 outside [1, 20]"
    assert call(ub=0) == inv
    for e in (arr(-0.1, 0.1, 0.2), arr(0.0, 0.2, 0.2), arr(0.0, float("nan"), 0.2),
              arr(0.0, 0.1, float(np.nextafter(np.float32(half), np.float32(1))))):
        assert call(edges=e) == inv
    assert "half the box" in lib.cgnn_last_error().decode()
    assert call(n=2 ** 31) == unsup and call(pos_b=fake, n_b=2 ** 31) == unsup
    # the checks this entry shares with the other pair walks, word for word
    need = wsb(100, 0, 4, 2)
    for kw, code, text in (
            (dict(edges=arr(0.0, 0.2, 0.2)), inv, "edges must be finite, non-negative and strictly ascending (edges[2])"),
            (dict(edges=arr(0.0, 0.1, 0.6)), inv, "edges[num_bins]=0.6 exceeds half the box, 0.5"),
            (dict(w=odd), inv, "workspace must be 16-byte aligned"),
            (dict(edges=arr(0.0, 0.1, half), wb=need - 1), short, f"workspace {need - 1} < required {need} bytes")):
        assert call(**kw) == code and lib.cgnn_last_error().decode() == "cgnn_triplet_moments: " + text, kw
    assert call(pos_b=fake, n_b=50, wb=wsb(100, 50, 4, 2) - 1) == short and call(moments=fake, wb=0) == short
