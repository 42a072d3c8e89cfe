"""CPU: the counting contract of ``cgnn_pair_counts_smu`` as tests/smu_checks.py restates it, the closed-form Legendre bin
integrals, the host arithmetic of ``statistics.correlation_multipoles_from_counts``, the host refusals of
``ops.pair_counts_smu`` and the bookkeeping of the new C entries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pair_count_checks as pcc
import smu_checks as smc
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib, ops, statistics

ENTRIES = ("cgnn_pair_counts_smu_workspace_bytes", "cgnn_pair_counts_smu")
BOX = 25.0


def _uniform(n, seed, box=BOX):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32) * np.float32(box)


@pytest.mark.parametrize("los", [0, 1, 2])
def test_row_sums_of_the_restatement_are_the_pair_counters(los):
    x, y = _uniform(400, seed=1), _uniform(250, seed=2)
    s_edges = np.linspace(0.0, 0.3 * BOX, 9).astype(np.float32)
    mu_edges = np.linspace(0.0, 1.0, 6)
    auto = smc.auto_counts(x, BOX, s_edges, mu_edges, los)
    assert auto.shape == (8, 5) and auto.dtype == np.int64 and auto[1:].min() > 0
    assert (auto.sum(axis=1) == pcc.auto_counts(x, BOX, s_edges)).all()
    cross = smc.cross_counts(x, y, BOX, s_edges, mu_edges, los)
    assert (cross.sum(axis=1) == pcc.cross_counts(x, y, BOX, s_edges)).all()
    assert (cross == smc.cross_counts(y, x, BOX, s_edges, mu_edges, los)).all()       # symmetric in a and b
    one = smc.auto_counts(x, BOX, s_edges, [0.0, 1.0], los)                           # one mu-bin: no threshold at all
    assert (one[:, 0] == pcc.auto_counts(x, BOX, s_edges)).all()


def test_the_restatement_tells_the_line_of_sight():
    """Pairs along an axis are in the last mu-bin of that axis and in bin 0 of the others; a coincident cross pair is in
    the last mu-bin (every threshold is 0 <= 0)."""
    a = np.array([[1.0, 1.0, 1.0]], dtype=np.float32)
    b = np.array([[1.0, 1.0, 2.0], [1.0, 1.0, 1.0]], dtype=np.float32)
    mu_edges = np.linspace(0.0, 1.0, 5)
    for los in (0, 1, 2):
        got = smc.cross_counts(a, b, BOX, [0.0, 0.5, 1.5], mu_edges, los)
        want = np.zeros((2, 4), dtype=np.int64)
        want[0, 3] = 1                                  # the coincident pair
        want[1, 3 if los == 2 else 0] = 1
        assert (got == want).all(), (los, got)
        assert smc.cross_counts(a, b, BOX, [0.1, 0.5, 1.5], mu_edges, los).sum() == 1   # s_edges[0] > 0: not counted


def test_mu_thresholds_ascend():
    """Rounding is monotone: fl32(m2[j'] d2) ascends with j' for every d2, so a binary search counts them."""
    rng = np.random.default_rng(3)
    d2 = np.concatenate([rng.random(2000, dtype=np.float32) * np.float32(150.0),
                         np.float32(2.0) ** np.arange(-149, 8, dtype=np.float32), np.zeros(1, dtype=np.float32)])
    for mu_edges in (np.linspace(0, 1, 129), np.geomspace(1e-20, 1, 128).tolist(), [0, 0.6, 0.8, 1],
                     [0.0, 1e-30, 1e-20, 1.0]):
        if mu_edges[0] != 0:
            mu_edges = [0.0] + list(mu_edges)
        th = smc.mu_thresholds(mu_edges, d2)
        assert th.shape == (d2.size, len(mu_edges) - 2)
        assert (np.diff(th, axis=1) >= 0).all()
        assert (th <= d2[:, None]).all()                # m2 <= 1: no threshold passes d2, which bounds dl2


def test_the_two_lattice_families_at_the_mu_edges():
    """float32: the separation (2, 0, 1.5) meets the 0.6 edge exactly (the tie goes to the upper bin); (1.5, 0, 2) is one
    ulp short of the 0.8 edge (the lower bin)."""
    m2 = pcc.squared_edges([0.0, 0.6, 0.8, 1.0])
    d2 = np.float32(2.0) * np.float32(2.0) + np.float32(1.5) * np.float32(1.5)
    assert d2 == np.float32(6.25)
    assert m2[1] * d2 == np.float32(2.25)
    assert m2[2] * d2 > np.float32(4.0) and m2[2] * d2 == np.nextafter(np.float32(4.0), np.float32(5.0))


def test_legendre_bin_integrals():
    from numpy.polynomial import legendre
    nodes, weights = legendre.leggauss(8)               # exact for degree 15
    for mu_edges in (np.linspace(0, 1, 21), [0.0, 1.0], [0.0, 0.6, 0.8, 1.0], np.linspace(0, 1, 129) ** 2):
        got = smc.legendre_bin_integrals(mu_edges)
        mu = np.asarray(mu_edges, dtype=np.float32).astype(np.float64)
        np.testing.assert_allclose(got.sum(axis=1), [1.0, 0.0, 0.0], rtol=0, atol=1e-14)
        mid, half = 0.5 * (mu[1:] + mu[:-1]), 0.5 * (mu[1:] - mu[:-1])
        for row, ell in enumerate((0, 2, 4)):
            coef = np.zeros(ell + 1)
            coef[ell] = 1.0
            quad = (legendre.legval(mid[:, None] + half[:, None] * nodes[None, :], coef) * weights[None, :]).sum(axis=1) * half
            np.testing.assert_allclose(got[row], quad, rtol=0, atol=1e-14)
        mine = statistics.legendre_bin_integrals(torch.from_numpy(mu))
        np.testing.assert_allclose(mine.numpy(), got, rtol=0, atol=1e-15)


def test_default_mu_edges():
    mu = statistics.default_mu_edges()
    assert mu.dtype == torch.float64 and mu.shape == (21,) and float(mu[0]) == 0.0 and float(mu[-1]) == 1.0
    assert torch.equal(mu, torch.linspace(0, 1, 21, dtype=torch.float64))
    assert statistics.default_mu_edges(7).shape == (8,)
    assert ops.check_mu_edges(mu, "test") == np.linspace(0, 1, 21).astype(np.float32).tolist()


def test_multipoles_from_counts_equal_to_rr_vanish_and_xi_0_is_the_pair_counters():
    s_edges = np.linspace(0.0, 0.2 * BOX, 9)
    mu_edges = np.linspace(0.0, 1.0, 11)
    n = 5000
    rr = smc.expected_random_pairs(n, BOX, s_edges, mu_edges)
    res = statistics.correlation_multipoles_from_counts(torch.from_numpy(rr), n, None, BOX, s_edges, mu_edges, True)
    assert sorted(res) == ["counts", "mu_hi", "mu_lo", "s_hi", "s_lo", "xi_0", "xi_2", "xi_4", "xi_smu"]
    for key in ("xi_smu", "xi_0", "xi_2", "xi_4"):
        assert res[key].dtype == torch.float64 and float(res[key].abs().max()) < 1e-12
    assert res["xi_smu"].shape == (8, 10) and res["xi_0"].shape == (8,)
    np.testing.assert_array_equal(res["s_lo"].numpy(), s_edges.astype(np.float32)[:-1].astype(np.float64))
    np.testing.assert_array_equal(res["mu_hi"].numpy(), mu_edges.astype(np.float32)[1:].astype(np.float64))
    # integer counts, frames, cross
    counts = torch.from_numpy(np.random.default_rng(5).integers(0, 1000, size=(3, 8, 10)))
    for auto, n_b in ((True, None), (False, 700)):
        res = statistics.correlation_multipoles_from_counts(counts, n, n_b, BOX, s_edges, mu_edges, auto)
        assert res["counts"].dtype == torch.int64 and torch.equal(res["counts"], counts)
        xi = statistics.correlation_from_counts(counts.sum(-1), n, n_b, BOX, s_edges, auto)
        assert res["xi_0"].shape == (3, 8)
        np.testing.assert_allclose(res["xi_0"].numpy(), xi.numpy(), rtol=0, atol=1e-12 * float(xi.abs().max()))
        want = counts.numpy() / smc.expected_random_pairs(n, BOX, s_edges, mu_edges, n_b) - 1.0
        np.testing.assert_allclose(res["xi_smu"].numpy(), want, rtol=1e-12)
        w = smc.legendre_bin_integrals(mu_edges)
        for row, ell in enumerate((0, 2, 4)):
            np.testing.assert_allclose(res[f"xi_{ell}"].numpy(), (2 * ell + 1) * (want * w[row]).sum(-1), rtol=0,
                                       atol=1e-12 * np.abs(want).max())
    # the -1 leaves l = 2, 4: DD / RR alone gives the same
    dd_rr = torch.from_numpy(counts.numpy() / smc.expected_random_pairs(n, BOX, s_edges, mu_edges))
    np.testing.assert_allclose(statistics.correlation_multipoles_from_counts(counts, n, None, BOX, s_edges, mu_edges,
                                                                             True)["xi_2"].numpy(),
                               5 * (dd_rr.numpy() * w[1]).sum(-1), rtol=0, atol=1e-12 * float(dd_rr.max()))
    # no pair expected at all: nan, as in correlation_from_counts
    none = statistics.correlation_multipoles_from_counts(torch.zeros(8, 10), 1, None, BOX, s_edges, mu_edges, True)
    assert bool(torch.isnan(none["xi_smu"]).all()) and bool(torch.isnan(none["xi_0"]).all())
    assert bool(torch.isnan(statistics.correlation_from_counts(torch.zeros(8), 1, None, BOX, s_edges, True)).all())
    with pytest.raises(ValueError):
        statistics.correlation_multipoles_from_counts(torch.zeros(8, 9), n, None, BOX, s_edges, mu_edges, True)


@pytest.mark.parametrize("s_edges,mu_edges,los", [
    ([0.0, 0.2], [0.1, 0.5, 1.0], 2),                   # does not start at 0
    ([0.0, 0.2], [0.0, 0.5, 0.999], 2),                 # does not end at 1
    ([0.0, 0.2], [0.0, 0.5, 1.0 + 1e-6], 2),
    ([0.0, 0.2], [0.0, 0.5, 0.5, 1.0], 2),              # not ascending
    ([0.0, 0.2], [0.0, 0.5, 0.5 + 1e-10, 1.0], 2),      # equal in float32
    ([0.0, 0.2], [0.0, 0.7, 0.5, 1.0], 2),
    ([0.0, 0.2], [0.0, float("nan"), 1.0], 2),
    ([0.0, 0.2], [1.0], 2),                             # no bin
    ([0.0, 0.2], np.linspace(0, 1, 130), 2),            # 129 mu-bins
    (np.linspace(0, 0.5, 130), [0.0, 1.0], 2),          # 129 s-bins
    (np.linspace(0, 0.5, 66), np.linspace(0, 1, 65), 2),    # 65 x 64 bins
    ([0.0, 0.6], [0.0, 1.0], 2),                        # s_edges as in pair_counts: past half the box
    ([0.0, 0.2], [0.0, 1.0], 3),
    ([0.0, 0.2], [0.0, 1.0], -1),
    ([0.0, 0.2], [0.0, 1.0], True),
    ([0.0, 0.2], [0.0, 1.0], 1.5),
])
def test_pair_counts_smu_refuses_on_the_host(s_edges, mu_edges, los):
    pos = torch.rand(10, 3)                             # a host tensor: refused later, were the arguments right
    with pytest.raises(ValueError):
        ops.pair_counts_smu(pos, 1.0, s_edges, mu_edges, los=los)
    with pytest.raises(ValueError):
        statistics.correlation_multipoles(pos, 1.0, s_edges, mu_edges, los=los)
    with pytest.raises(ValueError):
        statistics.rollout_redshift_correlation({"Coordinates": pos.view(1, 10, 3).repeat(3, 1, 1)},
                                                {"Coordinates": pos.view(1, 10, 3).repeat(3, 1, 1)}, 1.0, s_edges, 0.1,
                                                los=los, mu_edges=mu_edges)


def test_pair_counts_smu_accepts_the_limits_and_has_no_cpu_path():
    pos = torch.rand(10, 3)
    for s_edges, mu_edges in (([0.0, 0.5], [0.0, 1.0]), (np.linspace(0, 0.5, 129), [0.0, 1.0]),
                              ([0.25, 0.5], np.linspace(0, 1, 129)), (np.linspace(0, 0.5, 65), np.linspace(0, 1, 65))):
        with pytest.raises(_lib.CgnnError):             # the edges pass; the host tensor does not
            ops.pair_counts_smu(pos, 1.0, s_edges, mu_edges)
    with pytest.raises(ValueError):
        statistics.correlation_multipoles(pos, 1.0, [0.0, 0.2], pos_prev=pos)           # pos_prev needs dt
    with pytest.raises(ValueError):
        statistics.correlation_multipoles(pos, 1.0, [0.0, 0.2], pos_prev=pos, dt=0.0)
    with pytest.raises(ValueError):
        statistics.correlation_multipoles(pos, 1.0, [0.0, 0.2], pos_b=pos, pos_b_prev=pos)
    with pytest.raises(ValueError):
        ops.check_mu_edges([0.0, 0.5], "test")


def test_new_entries_are_declared_exported_built_and_documented():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert name + "(" in header and name in notes
    assert "lands in the LAST mu-bin" in header and "num_s * num_mu <= 4096" in header
    for fn in ("pair_counts_smu", "check_mu_edges"):
        assert callable(getattr(ops, fn))
    for fn in ("default_mu_edges", "correlation_multipoles_from_counts", "correlation_multipoles",
               "rollout_redshift_correlation"):
        assert callable(getattr(statistics, fn))
    makefile = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "Makefile")).read()
    assert "pair_counts_smu.hip" in makefile and "FLAGS_pair_counts_smu := -ffp-contract=off" in makefile
    for doc in ("README.md", "DESIGN.md"):
        assert "pair_counts_smu" in open(os.path.join(ROOT, doc)).read()
    assert _lib.PAIR_COUNTS_SMU_MAX_BINS == 4096 and _lib.PAIR_COUNTS_SMU_MAX_AXIS == 128


def test_workspace_size_and_the_host_refusals_of_the_c_entry():
    """The refusals come before any launch: no GPU is needed to meet them, and no pointer is dereferenced."""
    lib = _lib.load()
    wsb = lib.cgnn_pair_counts_smu_workspace_bytes
    assert wsb(0, 0, 8, 5) == 256 and wsb(-1, 0, 8, 5) == 256 and wsb(2 ** 31, 0, 8, 5) == 256
    for n_a, n_b in ((4096, 0), (4096, 500), (500, 4096), (1, 0)):     # the pair counter's workspace, whatever the bins
        assert wsb(n_a, n_b, 8, 5) == wsb(n_a, n_b, 64, 64) == lib.cgnn_pair_counts_workspace_bytes(n_a, n_b, 8)
    fake, odd = 1 << 20, (1 << 20) + 4                  # never dereferenced: every call below is refused on the host
    inv, unsup, short = -1, -2, -3                      # CGNN_ERR_INVALID_ARG, _UNSUPPORTED, _WORKSPACE
    half = float(np.float32(0.5))

    def arr(*v):
        return (C.c_float * len(v))(*v)

    def lin(hi, n):
        return arr(*np.linspace(0.0, hi, n + 1))

    def call(a=fake, n_a=100, b=None, n_b=0, box=1.0, s=arr(0.0, 0.1, 0.2), ns=2, mu=arr(0.0, 0.5, 1.0), nmu=2, los=2,
             counts=fake, w=fake, wb=1 << 30):
        return lib.cgnn_pair_counts_smu(a, n_a, b, n_b, box, s, ns, mu, nmu, los, counts, w, wb, None)

    for kw in (dict(a=None), dict(s=None), dict(mu=None), dict(counts=None), dict(w=None), dict(n_a=0), dict(n_a=-4),
               dict(b=fake, n_b=0), dict(box=0.0), dict(box=-1.0), dict(box=float("inf")), dict(box=float("nan"))):
        assert call(**kw) == inv, kw
    # bins per axis and in all
    assert call(ns=0) == inv and call(nmu=0) == inv and call(ns=-1) == inv
    assert call(s=lin(0.4, 129), ns=129) == inv and "num_s=129" in lib.cgnn_last_error().decode()
    assert call(mu=lin(1.0, 129), nmu=129) == inv and "num_mu=129" in lib.cgnn_last_error().decode()
    assert call(s=lin(0.4, 65), ns=65, mu=lin(1.0, 64), nmu=64) == inv and "4160" in lib.cgnn_last_error().decode()
    # the line of sight
    assert call(los=3) == inv and call(los=-1) == inv and "los" in lib.cgnn_last_error().decode()
    # s_edges as in cgnn_pair_counts
    for e in (arr(-0.1, 0.1, 0.2), arr(0.0, 0.2, 0.2), arr(0.0, 0.3, 0.2), arr(0.0, float("nan"), 0.2),
              arr(0.0, 0.1, float("inf")), arr(0.0, 0.1, float(np.nextafter(np.float32(half), np.float32(1))))):
        assert call(s=e) == inv
    assert "half the box" in lib.cgnn_last_error().decode()
    # mu_edges from exactly 0 to exactly 1, ascending
    for m in (arr(0.1, 0.5, 1.0), arr(0.0, 0.5, 0.99), arr(0.0, 0.5, float(np.nextafter(np.float32(1), np.float32(2)))),
              arr(-0.0 - 1e-30, 0.5, 1.0), arr(0.0, 0.5, 0.5), arr(0.0, 1.0, 0.5), arr(0.0, float("nan"), 1.0),
              arr(0.0, float("inf"), 1.0)):
        assert call(mu=m) == inv
        assert "mu_edges" in lib.cgnn_last_error().decode()
    # too many particles; a misaligned workspace; a short one (the limits themselves pass up to there)
    assert call(n_a=2 ** 31) == unsup and call(b=fake, n_b=2 ** 31) == unsup
    assert call(w=odd) == inv and "aligned" in lib.cgnn_last_error().decode()
    assert call(s=arr(0.0, 0.1, half), wb=wsb(100, 0, 2, 2) - 1) == short
    assert call(s=lin(0.5, 64), ns=64, mu=lin(1.0, 64), nmu=64, wb=0) == short
    assert call(s=lin(0.5, 128), ns=128, mu=arr(0.0, 1.0), nmu=1, b=fake, n_b=50, wb=wsb(100, 50, 128, 1) - 1) == short
    assert "workspace" in lib.cgnn_last_error().decode()
    # the checks this entry shares with the other pair walks, word for word
    for kw, code, text in (
            (dict(s=arr(0.0, 0.2, 0.2)), inv,
             "s_edges must be finite, non-negative and strictly ascending (s_edges[2])"),
            (dict(s=arr(0.0, 0.1, 0.6)), inv, "s_edges[num_s]=0.6 exceeds half the box, 0.5"),
            (dict(w=odd), inv, "workspace must be 16-byte aligned"),
            (dict(wb=wsb(100, 0, 2, 2) - 1), short, f"workspace {wsb(100, 0, 2, 2) - 1} < required {wsb(100, 0, 2, 2)} bytes")):
        assert call(**kw) == code and lib.cgnn_last_error().decode() == "cgnn_pair_counts_smu: " + text, kw
    # the parent's sizes, to the byte
    for n_a, n_b, size in ((1, 0, 2304), (100, 0, 5376), (4096, 0, 182016), (4096, 500, 113152), (500, 4096, 227584),
                           (1000000, 0, 65964544)):
        assert wsb(n_a, n_b, 8, 5) == size, (n_a, n_b)
