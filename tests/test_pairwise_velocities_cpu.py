"""CPU: the contract of ``cgnn_pair_velocity_sums`` as tests/pairwise_velocity_checks.py restates it (its counts, its
symmetries, its two-word totals), the cap the rigid-rotation GPU test relies on, the host arithmetic of
``statistics.pairwise_velocity_moments``, the host refusals of the op, of the statistics and of the C entry, and the
bookkeeping of the new entries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pair_count_checks as pcc
import pairwise_velocity_checks as pvc
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib, ops, statistics

ENTRIES = ("cgnn_pair_velocity_sums_workspace_bytes", "cgnn_pair_velocity_sums")
BOX = 25.0
Q = pvc.Q_ONE


def _uniform(n, seed, box=BOX):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32) * np.float32(box)


def _velocities(n, seed, limit=Q):
    return np.random.default_rng(seed).integers(-limit, limit + 1, size=(n, 3)).astype(np.int32)


EDGES = np.linspace(0.0, 0.3 * BOX, 9).astype(np.float32)


def test_counts_of_the_restatement_are_the_pair_counters():
    x, y = _uniform(400, seed=1), _uniform(250, seed=2)
    qx, qy = _velocities(400, seed=3), _velocities(250, seed=4)
    counts, sums = pvc.auto_sums(x, qx, BOX, EDGES)
    assert counts == pcc.auto_counts(x, BOX, EDGES).tolist() and min(counts[1:]) > 0
    assert all(0 < r2 < t2 for _, r2, t2 in sums[1:])    # random velocities: T2 is about three times R2
    cross, _ = pvc.cross_sums(x, qx, y, qy, BOX, EDGES)
    assert cross == pcc.cross_counts(x, y, BOX, EDGES).tolist()


def test_swapping_the_sets_changes_nothing():
    """d and dq both change sign, so every product of w, and with it iu, is the same."""
    x, y = _uniform(300, seed=5), _uniform(200, seed=6)
    qx, qy = _velocities(300, seed=7), _velocities(200, seed=8)
    assert pvc.cross_sums(x, qx, y, qy, BOX, EDGES) == pvc.cross_sums(y, qy, x, qx, BOX, EDGES)


@pytest.mark.parametrize("first_edge", [0.0, 0.5])
def test_auto_is_half_of_the_cross_of_a_set_with_itself_without_the_self_pairs(first_edge):
    x, q = _uniform(300, seed=9), _velocities(300, seed=10)
    edges = EDGES.copy()
    edges[0] = first_edge
    counts, sums = pvc.auto_sums(x, q, BOX, edges)
    cc, cs = pvc.cross_sums(x, q, x, q, BOX, edges)
    if first_edge == 0.0:
        cc[0] -= 300                                    # a particle with itself: d2 = 0, bin 0, iu = 0 and t2 = 0
    assert cc == [2 * c for c in counts]
    assert cs == [[2 * v for v in row] for row in sums]


def test_a_constant_added_to_every_velocity_changes_nothing():
    x = _uniform(300, seed=11)
    q = _velocities(300, seed=12, limit=Q // 2)
    shift = np.array([Q // 2, -Q // 3, 12345], dtype=np.int32)
    assert np.abs(q + shift).max() <= Q
    assert pvc.auto_sums(x, q, BOX, EDGES) == pvc.auto_sums(x, q + shift, BOX, EDGES)


def test_zero_velocities_give_zero_sums_and_coincident_particles_no_direction():
    x = _uniform(200, seed=13)
    counts, sums = pvc.auto_sums(x, np.zeros((200, 3), dtype=np.int32), BOX, EDGES)
    assert sum(counts) > 0 and all(v == 0 for row in sums for v in row)
    a = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    qa, qb = np.array([[Q, -Q, Q]], dtype=np.int32), np.array([[-Q, Q, -Q]], dtype=np.int32)
    counts, sums = pvc.cross_sums(a, qa, a, qb, BOX, [0.0, 1.0])
    assert counts == [1] and sums == [[0, 0, 3 * (2 * Q) ** 2]]      # iu = 0; T2 still counts, and passes 2^32
    assert sums[0][2] > 1 << 43
    counts, _ = pvc.cross_sums(a, qa, a, qb, BOX, [0.5, 1.0])
    assert counts == [0]
    # sign: b moves away from a along their separation -> u > 0; towards it -> u < 0 (infall)
    b = np.array([[1.0, 2.0, 5.0]], dtype=np.float32)
    zero = np.zeros((1, 3), dtype=np.int32)
    away, towards = np.array([[0, 0, 1000]], dtype=np.int32), np.array([[0, 0, -1000]], dtype=np.int32)
    assert pvc.cross_sums(a, zero, b, away, BOX, [0.0, 3.0])[1] == [[1000, 10 ** 6, 10 ** 6]]
    assert pvc.cross_sums(a, zero, b, towards, BOX, [0.0, 3.0])[1] == [[-1000, 10 ** 6, 10 ** 6]]


@pytest.mark.parametrize("v", [0, 1, -1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, -(1 << 32), -(1 << 32) - 1, (1 << 63) - 1,
                               1 << 63, (1 << 63) + 12345, 5 * (1 << 70) + 7, -(1 << 45) + 3, -3 * (1 << 40)])
def test_the_two_words_round_trip(v):
    lo, hi = pvc.split_words(v)
    assert 0 <= lo < 1 << 32 and pvc.join_words(lo, hi) == v and (hi < 0) == (v < 0)
    assert -(1 << 63) <= hi < 1 << 63
    w = pvc.words([[v, 0, 1 << 32]])
    assert w.dtype == np.int64 and w.shape == (1, 3, 2) and pvc.totals(w) == [[v, 0, 1 << 32]]
    assert w[0, 2].tolist() == [0, 1]
    # the device's normalisation: any (lo', hi') with lo' < 2^63 has the canonical words of its value; halving an even value
    raw_lo, raw_hi = lo + (3 << 32), hi - 3
    assert pvc.split_words(pvc.join_words(raw_lo, raw_hi)) == (lo, hi)
    lo2, hi2 = pvc.split_words(2 * v)
    assert ((lo2 >> 1) | ((hi2 & 1) << 31), hi2 >> 1) == (lo, hi)


def test_moments_from_hand_made_sums():
    counts = torch.tensor([4, 0, 10, 1 << 33])
    big = 3 * (1 << 66)
    sums = torch.from_numpy(pvc.words([[-8, 20, 52], [0, 0, 0], [5, 100, 97], [-(1 << 35), big, 3 * big]]))
    scale = 3.0
    step = scale / Q
    res = statistics.pairwise_velocity_moments(counts, sums, scale, [0.0, 1.0, 2.0, 3.0, 4.0])
    assert sorted(res) == ["counts", "mean_square_par", "r_hi", "r_lo", "sigma_par", "sigma_perp", "v12"]
    assert torch.equal(res["counts"], counts) and res["r_lo"].tolist() == [0, 1, 2, 3] and res["r_hi"].tolist() == [1, 2, 3, 4]
    for key in ("v12", "sigma_par", "sigma_perp", "mean_square_par"):
        assert res[key].dtype == torch.float64 and res[key].shape == (4,)
        assert bool(torch.isnan(res[key][1])) and not bool(torch.isnan(res[key][[0, 2, 3]]).any())     # the empty bin
    np.testing.assert_allclose(res["v12"][[0, 2, 3]].numpy(), [step * -2.0, step * 0.5, step * -4.0], rtol=1e-15)
    np.testing.assert_allclose(res["sigma_par"][[0, 2]].numpy(), [step * 1.0, step * np.sqrt(10 - 0.25)], rtol=1e-15)
    np.testing.assert_allclose(res["sigma_perp"][0].item(), step * 2.0, rtol=1e-15)       # (52 - 20) / 8
    assert float(res["sigma_perp"][2]) == 0.0                       # T2 < R2 by three units: clipped
    np.testing.assert_allclose(res["mean_square_par"][[0, 2]].numpy(), [step ** 2 * 5.0, step ** 2 * 10.0], rtol=1e-15)
    # past int64: R2 / c = 3 * 2^33, T2 - R2 = 2 R2
    np.testing.assert_allclose(res["sigma_par"][3].item(), step * np.sqrt(3.0 * 2 ** 33 - 16.0), rtol=1e-14)
    np.testing.assert_allclose(res["sigma_perp"][3].item(), step * np.sqrt(3.0 * 2 ** 33), rtol=1e-14)
    want = pvc.moments([4, 0, 10, 1 << 33], pvc.totals(sums.numpy()), scale)
    for row, key in enumerate(("v12", "sigma_par", "sigma_perp")):
        np.testing.assert_allclose(res[key].numpy(), want[row], rtol=1e-14)
    # frames, a tensor scale, no edges
    two = statistics.pairwise_velocity_moments(torch.stack([counts, counts]), torch.stack([sums, sums]),
                                               torch.tensor(scale, dtype=torch.float64))
    assert sorted(two) == ["counts", "mean_square_par", "sigma_par", "sigma_perp", "v12"]
    assert two["v12"].shape == (2, 4) and torch.equal(two["v12"][1].view(torch.int64), res["v12"].view(torch.int64))
    for bad in (dict(sums=sums[:3]), dict(sums=sums.to(torch.float64)), dict(value_scale=0.0), dict(value_scale=-1.0),
                dict(value_scale=float("nan")), dict(value_scale=True), dict(edges=[0.0, 1.0])):
        kw = dict(counts=counts, sums=sums, value_scale=scale)
        kw.update(bad)
        with pytest.raises(ValueError):
            statistics.pairwise_velocity_moments(**kw)


def test_rigid_rotation_has_no_radial_velocity_beyond_three_steps():
    """The cap the GPU test relies on, confirmed on the restatement: quantisation moves each dq_c by at most one step
    (the radial part by at most sqrt(3)), the float32 roundings of w / r by under one more: |iu| <= 3 for every pair."""
    x = pvc.ball_points(600, seed=41, box_size=BOX)
    v = pvc.rotation_field(x, BOX)
    q = pvc.quantize(v, np.abs(v).max())
    assert np.abs(q).max() == Q
    _, iu, t2, _ = pvc.pair_terms(x, q, x, q, BOX)
    assert np.abs(iu).max() <= 3 and t2.max() > (Q // 2) ** 2
    counts, sums = pvc.auto_sums(x, q, BOX, EDGES)
    assert all(abs(s1) <= 3 * c and r2 <= 9 * c and t2 > 100 * r2 for c, (s1, r2, t2) in zip(counts, sums) if c)


def test_pair_velocity_sums_refuses_on_the_host():
    pos = torch.rand(10, 3)                             # a host tensor: refused later, were the arguments right
    q = torch.zeros(10, 3, dtype=torch.int32)
    ok = [0.0, 0.2]
    for kw in (dict(edges=np.linspace(0, 0.5, 66)),                    # 65 bins
               dict(edges=[0.0, 0.6]), dict(edges=[0.2, 0.1]), dict(edges=[0.1]), dict(edges=[0.0, float("nan")]),
               dict(box_size=0.0),
               dict(q_a=None), dict(q_a=q.long()), dict(q_a=q.float()), dict(q_a=q[:9]), dict(q_a=q.view(1, 10, 3)),
               dict(q_a=q.numpy()),
               dict(pos_b=pos), dict(q_b=q),                           # one without the other
               dict(pos_b=pos, q_b=q.long()), dict(pos_b=pos[:5], q_b=q)):
        args = dict(pos_a=pos, q_a=q, box_size=1.0, edges=ok)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.pair_velocity_sums(**args)
    for edges in (ok, np.linspace(0, 0.5, 65), [0.25, 0.5]):           # the limits pass; the host tensor does not
        with pytest.raises(_lib.CgnnError):
            ops.pair_velocity_sums(pos, q, 1.0, edges)
        with pytest.raises(_lib.CgnnError):
            ops.pair_velocity_sums(pos, q, 1.0, edges, pos, q)


def test_the_statistics_refuse_on_the_host():
    pos, vel = torch.rand(10, 3), torch.randn(10, 3)
    ok = [0.0, 0.2]
    pv = statistics.pairwise_velocities
    for kw in (dict(), dict(vel=vel, pos_prev=pos, dt=0.1),            # none, or both forms
               dict(pos_prev=pos), dict(pos_prev=pos, dt=0.0), dict(pos_prev=pos, dt=float("inf")),
               dict(pos_prev=pos, dt=True), dict(vel=vel, dt=0.1),
               dict(vel=vel[:9]), dict(pos_prev=pos[:9], dt=0.1),
               dict(vel=vel, vel_b=vel), dict(vel=vel, pos_b_prev=pos),            # no pos_b
               dict(vel=vel, pos_b=pos), dict(vel=vel, pos_b=pos, pos_b_prev=pos),
               dict(pos_prev=pos, dt=0.1, pos_b=pos, vel_b=vel), dict(pos_prev=pos, dt=0.1, pos_b=pos),
               dict(vel=vel, pos_b=pos, vel_b=vel[:9]), dict(vel=vel, pos_b=pos.view(1, 10, 3), vel_b=vel.view(1, 10, 3)),
               dict(vel=vel, value_scale=0.0), dict(vel=vel, value_scale=-2.0), dict(vel=vel, value_scale=torch.ones(2)),
               dict(vel=vel, edges=np.linspace(0, 0.5, 66)), dict(vel=vel, edges=[0.0, 0.6]), dict(vel=vel, box_size=-1.0)):
        args = dict(pos=pos, box_size=1.0, edges=ok)
        args.update(kw)
        with pytest.raises(ValueError):
            pv(**args)
    with pytest.raises(_lib.CgnnError):                 # the arguments pass; there is no CPU path
        pv(pos, 1.0, ok, vel=vel)
    frames = {"Coordinates": pos.view(1, 10, 3).repeat(3, 1, 1)}
    rp = statistics.rollout_pairwise_velocities
    for kw in (dict(edges=np.linspace(0, 0.5, 66)), dict(edges=[0.0, 0.6]), dict(dt=0.0), dict(dt=None),
               dict(value_scale=0.0), dict(frames=[0]), dict(frames=[3]), dict(frames=[])):
        args = dict(rollout_data=frames, ground_truth=frames, box_size=1.0, edges=ok, dt=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            rp(**args)
    with pytest.raises(_lib.CgnnError):
        rp(frames, frames, 1.0, ok, 0.1)


def test_new_entries_are_declared_exported_built_and_documented():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert name + "(" in header and name in notes
    assert "hi * 2^32 + lo" in header and "1 <= num_bins <= 64" in header and "iu = rint(u)" in header
    assert callable(ops.pair_velocity_sums)
    for fn in ("pairwise_velocity_moments", "pairwise_velocities", "rollout_pairwise_velocities"):
        assert callable(getattr(statistics, fn))
    makefile = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "Makefile")).read()
    assert "pair_velocities.hip" in makefile
    assert "FLAGS_pair_velocities := -ffp-contract=off -DCGNN_PAIR_CONTRACT_OFF\n" in makefile
    assert makefile.count("$(BUILD)/pair_velocities.o") == 2          # cell_grid.hpp and pair_walk.hpp
    for doc in ("README.md", "DESIGN.md"):
        assert "pair_velocity_sums" in open(os.path.join(ROOT, doc)).read()
    assert _lib.PAIR_VELOCITY_MAX_BINS == 64 and _lib.WEIGHT_BITS == 20


def test_workspace_size_and_the_host_refusals_of_the_c_entry():
    """The refusals come before any launch: no GPU is needed to meet them, and no pointer is dereferenced."""
    lib = _lib.load()
    wsb = lib.cgnn_pair_velocity_sums_workspace_bytes
    pcw = lib.cgnn_pair_counts_workspace_bytes
    assert wsb(0, 0, 8) == 256 and wsb(-1, 0, 8) == 256 and wsb(2 ** 31, 0, 8) == 256 and wsb(5, -1, 8) == 256

    def up(x):
        return (x + 255) // 256 * 256

    for n_a, n_b in ((4096, 0), (4096, 500), (500, 4096), (1, 0), (1000000, 0)):     # the pair job's plus an int4 each
        assert wsb(n_a, n_b, 8) == wsb(n_a, n_b, 64) == pcw(n_a, n_b, 8) + up(16 * n_a) + up(16 * n_b), (n_a, n_b)
    fake, odd = 1 << 20, (1 << 20) + 4                  # never dereferenced: every call below is refused on the host
    inv, unsup, short = -1, -2, -3                      # CGNN_ERR_INVALID_ARG, _UNSUPPORTED, _WORKSPACE
    half = float(np.float32(0.5))

    def arr(*v):
        return (C.c_float * len(v))(*v)

    def call(a=fake, qa=fake, n_a=100, b=None, qb=None, n_b=0, box=1.0, e=arr(0.0, 0.1, 0.2), nb=2, counts=fake,
             sums=fake, w=fake, wb=1 << 30):
        return lib.cgnn_pair_velocity_sums(a, qa, n_a, b, qb, n_b, box, e, nb, counts, sums, w, wb, None)

    for kw in (dict(a=None), dict(qa=None), dict(e=None), dict(counts=None), dict(sums=None), dict(w=None), dict(n_a=0),
               dict(n_a=-4), dict(b=fake, qb=fake, n_b=0), dict(box=0.0), dict(box=-1.0), dict(box=float("inf")),
               dict(box=float("nan"))):
        assert call(**kw) == inv, kw
    # q_b exactly when pos_b
    assert call(b=fake, n_b=50) == inv and "q_b" in lib.cgnn_last_error().decode()
    assert call(qb=fake) == inv and "q_b" in lib.cgnn_last_error().decode()
    # the bins
    assert call(nb=0) == inv and call(nb=-1) == inv
    assert call(e=arr(*np.linspace(0.0, 0.4, 66)), nb=65) == inv
    assert lib.cgnn_last_error().decode() == "cgnn_pair_velocity_sums: num_bins=65 outside [1, 64]"
    # edges as in cgnn_pair_counts
    for e in (arr(-0.1, 0.1, 0.2), arr(0.0, 0.2, 0.2), arr(0.0, 0.3, 0.2), arr(0.0, float("nan"), 0.2),
              arr(0.0, 0.1, float("inf")), arr(0.0, 0.1, float(np.nextafter(np.float32(half), np.float32(1))))):
        assert call(e=e) == inv
    assert "half the box" in lib.cgnn_last_error().decode()
    # too many particles; a misaligned workspace; a short one (the limits themselves pass up to there)
    assert call(n_a=2 ** 31) == unsup and call(b=fake, qb=fake, n_b=2 ** 31) == unsup
    assert call(w=odd) == inv and "aligned" in lib.cgnn_last_error().decode()
    assert call(e=arr(0.0, 0.1, half), wb=wsb(100, 0, 2) - 1) == short
    assert call(e=arr(*np.linspace(0.0, 0.5, 65)), nb=64, wb=0) == short
    assert call(b=fake, qb=fake, n_b=50, wb=wsb(100, 50, 2) - 1) == short
    assert call(wb=pcw(100, 0, 2)) == short             # the pair counter's workspace is not enough
    assert "workspace" in lib.cgnn_last_error().decode()
    # the checks this entry shares with the other pair walks, word for word
    for kw, code, text in (
            (dict(e=arr(0.0, 0.2, 0.2)), inv, "edges must be finite, non-negative and strictly ascending (edges[2])"),
            (dict(e=arr(0.0, 0.1, 0.6)), inv, "edges[num_bins]=0.6 exceeds half the box, 0.5"),
            (dict(w=odd), inv, "workspace must be 16-byte aligned"),
            (dict(wb=wsb(100, 0, 2) - 1), short, f"workspace {wsb(100, 0, 2) - 1} < required {wsb(100, 0, 2)} bytes")):
        assert call(**kw) == code and lib.cgnn_last_error().decode() == "cgnn_pair_velocity_sums: " + text, kw
