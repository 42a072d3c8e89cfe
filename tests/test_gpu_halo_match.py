"""GPU: ``ops.halo_match`` / ``ops.fof_group_sums`` (``cgnn_halo_match``, ``cgnn_fof_group_sums``) against the numpy
restatement of their contract (tests/halo_match_checks.py), and ``statistics.halo_matches`` /
``statistics.rollout_halo_matching`` built on them.  Integers throughout: every comparison of a kernel's output is
``torch.equal``.  N is at most 8192 (a table of 16384 slots, 32 workgroups of particles)."""
import functools

import numpy as np
import pytest
import torch

import fof_checks as fc
import halo_match_checks as hm
from cosmology_gnn_simulation_amd import _lib, ops, statistics, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOX = 25.0
# (n, groups of A, groups of B, minimum): few large groups (one key per wave), many small ones, as many groups as
# particles (mostly singletons: the table near its fullest), a single partly filled wave, a minimum that cuts groups
RANDOM_CASES = [(8192, 200, 150, 1), (8192, 2000, 1500, 3), (8192, 8192, 8192, 1), (300, 10, 7, 1), (4096, 64, 64, 60)]


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _want(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _edges(n):
    return [e for e in (1, 2, 3, 5, 9, 17, 33, 100, 1000) if e <= n] + [n + 1]


def _check(la, lb, min_a, min_b=None, sa=None, sb=None):
    """All four arrays and the summary equal the restatement's; returns the restatement's five."""
    la, lb = np.asarray(la, dtype=np.int32), np.asarray(lb, dtype=np.int32)
    sa = hm.sizes(la) if sa is None else sa
    sb = hm.sizes(lb) if sb is None else sb
    n = len(la)
    edges = _edges(n)
    want = hm.halo_match(la, sa, lb, sb, min_a, min_b, edges)
    got = ops.halo_match(_dev(la), _dev(sa), _dev(lb), _dev(sb), min_a, min_b, edges)
    for g, w, name in zip(got, want, ("match_ab", "shared_ab", "match_ba", "shared_ba", "summary")):
        assert g.dtype == (torch.int64 if name == "summary" else torch.int32), name
        assert g.shape == w.shape and torch.equal(g.cpu(), _want(w)), name
    none = ops.halo_match(_dev(la), _dev(sa), _dev(lb), _dev(sb), min_a, min_b)
    assert none[4] is None and all(torch.equal(a, b) for a, b in zip(none[:4], got[:4]))
    return want


@functools.lru_cache(maxsize=None)
def _random_case(n, g_a, g_b, seed):
    rng = np.random.default_rng(seed)
    return hm.labels_of_groups(rng.integers(0, g_a, n)), hm.labels_of_groups(rng.integers(0, g_b, n))


@pytest.mark.parametrize("n,g_a,g_b,minimum", RANDOM_CASES)
def test_random_labellings_equal_the_restatement(n, g_a, g_b, minimum):
    la, lb = _random_case(n, g_a, g_b, 7000 + g_a)
    sa, sb = hm.sizes(la), hm.sizes(lb)
    mab, sab, mba, sba, summary = _check(la, lb, minimum)
    # what the case is there for, from the restatement: ties, matches that are not mutual, groups below the minimum
    assert len(hm.ties(la, sa, lb, sb, minimum)) >= 3
    mutual = hm.mutual(mab, mba)
    assert mutual.sum() >= 5 and ((mab >= 0) & ~mutual).sum() >= 1
    if minimum > 1:
        assert ((sa > 0) & (sa < minimum)).sum() >= 1 and ((sb > 0) & (sb < minimum)).sum() >= 1
    assert len(hm.shared_pairs(la, sa, lb, sb, minimum, minimum)[0]) >= 70
    assert summary[:, 0].sum() == (sa >= minimum).sum() and summary[:, 2].sum() == mutual.sum()


def test_identity_labels_fill_the_table_to_its_fullest():
    n = 8192
    ident = np.arange(n, dtype=np.int32)
    mab, sab, mba, sba, summary = _check(ident, ident, 1)                       # n distinct keys in 2 n slots
    assert (mab == ident).all() and (sab == 1).all() and summary[0].tolist() == [n, n, n, n, n, n]
    for m in (4096, 4097, 5000):                                                # a table of exactly 2 n slots, and just above
        _check(np.arange(m), np.arange(m), 1)


def test_one_key_counted_n_times():
    n = 8192
    zeros = np.zeros(n, dtype=np.int32)
    mab, sab, mba, sba, _ = _check(zeros, zeros, 1)
    assert mab[0] == 0 and sab[0] == n and (mab[1:] == -1).all() and mba[0] == 0 and sba[0] == n
    _check(zeros, zeros, n)
    assert (_check(zeros, zeros, n, n + 1)[0] == -1).all()                      # nothing of B is listed: nobody counts


def test_n_ties_go_to_root_0_and_the_converse():
    n = 8192
    zeros, ident = np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32)
    mab, sab, mba, sba, _ = _check(zeros, ident, 1)                             # A: one group, B: n singletons
    assert mab[0] == 0 and sab[0] == 1 and (mba == 0).all() and (sba == 1).all()
    mab, sab, mba, sba, _ = _check(ident, zeros, 1)
    assert (mab == 0).all() and (sab == 1).all() and mba[0] == 0 and sba[0] == 1 and (mba[1:] == -1).all()


def test_a_single_particle():
    assert [a.tolist() for a in _check([0], [0], 1)[:4]] == [[0], [1], [0], [1]]
    assert [a.tolist() for a in _check([0], [0], 2)[:4]] == [[-1], [0], [-1], [0]]
    assert [a.tolist() for a in _check([-1], [0], 1)[:4]] == [[-1], [0], [-1], [0]]
    assert [a.tolist() for a in _check([0], [1], 1)[:4]] == [[-1], [0], [-1], [0]]


@pytest.mark.parametrize("min_a,min_b", [(60, 70), (70, 60), (1, 66), (64, 1)])
def test_different_minimums(min_a, min_b):
    la, lb = _random_case(4096, 64, 64, 7064)                                   # groups of 64 members, give or take 8
    sa, sb = hm.sizes(la), hm.sizes(lb)
    assert ((sa > 0) & (sa < min_a)).sum() + ((sb > 0) & (sb < min_b)).sum() >= 1 and (sa >= min_a).any() and (sb >= min_b).any()
    mab = _check(la, lb, min_a, min_b)[0]
    assert (mab >= 0).any() and (sb[mab[mab >= 0]] >= min_b).all()


def test_labels_outside_the_range_are_ignored():
    n = 8192
    la, lb = (a.copy() for a in _random_case(n, 200, 150, 7200))
    rng = np.random.default_rng(11)
    members_a, members_b = np.flatnonzero(la != np.arange(n)), np.flatnonzero(lb != np.arange(n))
    la[rng.choice(members_a, 300, replace=False)] = np.repeat(np.array([-1, n, -2 ** 31, 2 ** 31 - 1], dtype=np.int32), 75)
    lb[rng.choice(members_b, 300, replace=False)] = np.repeat(np.array([n, -1, n + 5, -7], dtype=np.int32), 75)
    sa, sb = hm.sizes(la), hm.sizes(lb)
    assert sa.sum() == n - 300 and sb.sum() == n - 300
    mab, sab, _, _, _ = _check(la, lb, 1, sa=sa, sb=sb)
    assert 0 < sab.sum() < n - 300                                              # some particles are out on one side only
    q = rng.integers(-2 ** 20, 2 ** 20 + 1, (n, 3)).astype(np.int32)
    sums, scale = ops.fof_group_sums(_dev(la), _dev(q))
    assert scale is None and torch.equal(sums.cpu(), _want(hm.group_sums(la, q)))


def test_frames_at_once_equal_separate_calls_and_a_second_call_gives_the_same_bits():
    cases = [_random_case(8192, g, g, 7300 + g) for g in (100, 1000, 8192)]
    la, lb = (_dev(np.stack([c[k] for c in cases])) for k in (0, 1))
    sa, sb = (_dev(np.stack([hm.sizes(c[k]) for c in cases])) for k in (0, 1))
    edges = _edges(8192)
    both = ops.halo_match(la, sa, lb, sb, 2, 3, edges)
    assert [tuple(t.shape) for t in both] == [(3, 8192)] * 4 + [(3, len(edges) - 1, 6)]
    for f in range(3):
        one = ops.halo_match(la[f], sa[f], lb[f], sb[f], 2, 3, edges)
        assert all(torch.equal(b[f], o) for b, o in zip(both, one))
        want = hm.halo_match(cases[f][0], hm.sizes(cases[f][0]), cases[f][1], hm.sizes(cases[f][1]), 2, 3, edges)
        assert all(torch.equal(o.cpu(), _want(w)) for o, w in zip(one, want))
    again = ops.halo_match(la, sa, lb, sb, 2, 3, edges)
    assert all(torch.equal(a, b) for a, b in zip(again, both))


def test_a_short_workspace_is_refused_and_nothing_is_written():
    n = 1000
    lib = _lib.load()
    la = _dev(np.zeros(n))
    size = _dev(hm.sizes(np.zeros(n)))
    out = torch.full((4, n), 7, dtype=torch.int32, device=DEV)
    need = lib.cgnn_halo_match_workspace_bytes(n)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(ws_bytes):
        return lib.cgnn_halo_match(la.data_ptr(), size.data_ptr(), la.data_ptr(), size.data_ptr(), n, 1, 1,
                                   out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None, 0,
                                   None, ws.data_ptr(), ws_bytes, _lib.stream_ptr(torch.device(DEV)))

    assert call(need - 1) == -3 and b"workspace" in lib.cgnn_last_error()     # CGNN_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert call(need) == 0
    assert out[:, 0].tolist() == [0, n, 0, n] and bool((out[0, 1:] == -1).all())


def test_no_host_synchronisation():
    la, lb = _random_case(8192, 2000, 1500, 9000)
    args = (_dev(la), _dev(hm.sizes(la)), _dev(lb), _dev(hm.sizes(lb)), 3, None, _edges(8192))
    values = torch.rand(8192, 2, device=DEV)
    warm = ops.halo_match(*args)
    warm_sums, warm_scale = ops.fof_group_sums(args[0], values)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = ops.halo_match(*args)
        sums, scale = ops.fof_group_sums(args[0], values)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(again, warm))
    assert torch.equal(sums, warm_sums) and torch.equal(scale, warm_scale)


# ---- from positions ----------------------------------------------------------------------------------------------------
def _wrapped(x, box=BOX):
    x = np.mod(x, np.float32(box)).astype(np.float32)
    return np.where(x >= np.float32(box), x - np.float32(box), x).astype(np.float32)


def _displaced(x, sigma, seed, box=BOX):
    noise = np.random.default_rng(seed).standard_normal(x.shape) * sigma
    return _wrapped(x.astype(np.float64) + noise, box)


def _catalogue(x, ll, box=BOX):
    pos = torch.from_numpy(x).to(DEV)
    labels = ops.fof_labels(pos, box, ll)
    size, disp, _ = ops.fof_catalogue(pos, labels, box)
    return labels, size, disp


def _match_frames(xa, xb, ll, minimum):
    la, sa, _ = _catalogue(xa, ll)
    lb, sb, _ = _catalogue(xb, ll)
    edges = statistics.default_size_edges(len(xa), minimum)
    got = ops.halo_match(la, sa, lb, sb, minimum, size_edges=edges)
    want = hm.halo_match(la.cpu().numpy(), sa.cpu().numpy(), lb.cpu().numpy(), sb.cpu().numpy(), minimum, None, edges)
    for g, w in zip(got, want):
        assert torch.equal(g.cpu(), _want(w))
    return sa.cpu().numpy(), sb.cpu().numpy(), want


def test_clustered_frame_against_itself_displaced_by_a_linking_length():
    n = 8192
    x = synthetic.make_clustered_positions(n, BOX, seed=3).numpy()
    ll = float(np.float32(0.2 * BOX / n ** (1 / 3)))
    sa, sb, (mab, sab, mba, sba, summary) = _match_frames(x, _displaced(x, 1.0 * ll, seed=21), ll, 5)
    mutual = hm.mutual(mab, mba)
    assert (sa >= 5).sum() >= 20 and 5 <= mutual.sum() < (sa >= 5).sum()
    big = int(np.argmax(sa))                                                    # the halo: whole waves of one key
    assert sa[big] >= 1500 and mutual[big] and sab[big] >= 1000 and sab[big] < sa[big]
    assert summary[:, 0].sum() == (sa >= 5).sum() and summary[:, 2].sum() == mutual.sum()


def test_uniform_frame_against_itself_displaced_by_a_quarter_of_a_linking_length():
    n = 8192
    x = np.random.default_rng(31).random((n, 3), dtype=np.float32) * np.float32(BOX)
    ll = float(np.float32(0.6 * BOX / n ** (1 / 3)))
    sa, sb, (mab, sab, mba, sba, summary) = _match_frames(x, _displaced(x, 0.25 * ll, seed=22), ll, 5)
    mutual = hm.mutual(mab, mba)
    assert (sa >= 5).sum() >= 100 and 50 <= mutual.sum() < (sa >= 5).sum()
    assert ((mab >= 0) & ~mutual).sum() >= 1 and ((sa >= 5) & (mab < 0)).sum() >= 1


# ---- cgnn_fof_group_sums -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("n", [1, 7, 8192])
def test_group_sums_equal_add_at(n, c):
    rng = np.random.default_rng(100 * n + c)
    labels = hm.labels_of_groups(rng.integers(0, max(1, n // 16), n))
    q = rng.integers(-2 ** 20, 2 ** 20 + 1, (n, c)).astype(np.int32)
    want = np.zeros((n, c), dtype=np.int64)
    np.add.at(want, labels, q.astype(np.int64))
    sums, scale = ops.fof_group_sums(_dev(labels), _dev(q))
    assert scale is None and sums.dtype == torch.int64 and sums.shape == (n, c)
    assert torch.equal(sums.cpu(), _want(want)) and (want == hm.group_sums(labels, q)).all()
    if c == 1:
        flat, _ = ops.fof_group_sums(_dev(labels), _dev(q[:, 0]))
        assert flat.shape == (n,) and torch.equal(flat.cpu(), _want(want[:, 0]))
    two, _ = ops.fof_group_sums(_dev(np.stack([labels, labels])), _dev(np.stack([q, -q])))
    assert two.shape == (2, n, c) and torch.equal(two[0].cpu(), _want(want)) and torch.equal(two[1].cpu(), _want(-want))


def test_group_sums_of_float_values_at_the_scale_and_cancelling_signs():
    n = 8192
    rng = np.random.default_rng(5)
    labels = hm.labels_of_groups(rng.integers(0, 40, n))
    values = rng.choice(np.array([-3.5, 0.0, 3.5]), (n, 2))                     # exactly -scale, 0 and +scale
    q = (values / 3.5 * 2 ** 20).astype(np.int64)
    for scale_in in (None, 3.5, torch.tensor(3.5, dtype=torch.float64, device=DEV)):
        sums, scale = ops.fof_group_sums(_dev(labels), _dev(values, torch.float32), scale_in)
        assert float(scale) == 3.5 and torch.equal(sums.cpu(), _want(hm.group_sums(labels, q)))
    # one group of all particles, alternating signs: the sum cancels exactly; one particle more and one weight is left
    signs = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    for m in (n, n - 1):
        sums, scale = ops.fof_group_sums(_dev(np.zeros(m)), _dev(2.25 * signs[:m], torch.float64))
        assert float(scale) == 2.25 and int(sums[0]) == (m % 2) * 2 ** 20 and bool((sums[1:] == 0).all())
    zeros, scale = ops.fof_group_sums(_dev(np.zeros(n)), torch.zeros(n, device=DEV))
    assert float(scale) == 1.0 and bool((zeros == 0).all())


# ---- the statistics functions ------------------------------------------------------------------------------------------
N_TRAJ, MIN_TRAJ = 4096, 5
LL_TRAJ = float(np.float32(0.65 * BOX / N_TRAJ ** (1 / 3)))


@functools.lru_cache(maxsize=None)
def _trajectory():
    """Three true frames (one halo of a quarter of the particles in a uniform field, jittered: at 0.65 mean spacings the
    field holds some sixty groups of five or more) and a prediction that wanders off: noise of 0, 0.15 and 0.4 linking
    lengths.  float32 [3, N, 3] twice, and a temperature per particle and frame [3, N]."""
    x0 = synthetic.make_clustered_positions(N_TRAJ, BOX, seed=8, blob_fraction=0.25, blob_sigma=0.03).numpy()
    truth = np.stack([_displaced(x0, 0.1 * LL_TRAJ * t, seed=40 + t) for t in range(3)])
    pred = np.stack([_displaced(truth[t], s * LL_TRAJ, seed=50 + t) for t, s in enumerate((0.0, 0.15, 0.4))])
    temp = (1.0 + np.random.default_rng(60).random((3, N_TRAJ)) * 4.0).astype(np.float32)
    return truth, pred, temp


def _restated_frame(xa, xb, minimum=MIN_TRAJ, ll=LL_TRAJ, edges=None):
    la, sa, da = (t.cpu().numpy() for t in _catalogue(xa, ll))
    lb, sb, db = (t.cpu().numpy() for t in _catalogue(xb, ll))
    return (la, sa, da), (lb, sb, db), hm.halo_match(la, sa, lb, sb, minimum, None, edges)


def _min_image_distance(a, b, box=BOX):
    d = b - a
    d -= np.float64(np.float32(box)) * np.round(d / np.float64(np.float32(box)))
    return np.sqrt((d * d).sum(axis=1))


def test_halo_matches_equals_the_restatement():
    truth, pred, temp = _trajectory()
    xa, xb = truth[2], pred[2]
    (la, sa, da), (lb, sb, db), (mab, sab, mba, sba, _) = _restated_frame(xa, xb)
    temp_b = (temp[2] * 1.5).astype(np.float32)
    got = statistics.halo_matches(torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV), BOX, LL_TRAJ, MIN_TRAJ,
                                  values_a=torch.from_numpy(temp[2]).to(DEV), values_b=torch.from_numpy(temp_b).to(DEV))
    assert all(not v.is_cuda for v in got.values())
    order = np.array(sorted(np.flatnonzero(sa >= MIN_TRAJ).tolist(), key=lambda r: (-int(sa[r]), r)))
    m = mab[order].astype(np.int64)
    mutual = hm.mutual(mab, mba)[order]
    assert len(order) >= 10 and 3 <= mutual.sum() and (m < 0).any() and ((m >= 0) & ~mutual).any()
    assert got["root"].tolist() == order.tolist() and got["size"].tolist() == sa[order].tolist()
    assert got["match_root"].tolist() == m.tolist() and got["shared"].tolist() == sab[order].tolist()
    assert got["match_size"].tolist() == np.where(m >= 0, sb[np.maximum(m, 0)], 0).tolist()
    assert got["mutual"].dtype == torch.bool and got["mutual"].tolist() == mutual.tolist()
    ca = fc.centres(xa, order, sa, da, BOX)
    np.testing.assert_allclose(got["centre"].numpy(), ca, rtol=0, atol=1e-12 * BOX)
    has = m >= 0
    off = got["centre_offset"].numpy()
    assert off.dtype == np.float64 and np.isnan(off[~has]).all()
    cb = fc.centres(xb, m[has], sb, db, BOX)
    np.testing.assert_allclose(off[has], _min_image_distance(ca[has], cb), rtol=0, atol=1e-11 * BOX)
    np.testing.assert_allclose(got["match_centre"].numpy()[has], cb, rtol=0, atol=1e-12 * BOX)
    # the means: each member's value is quantised to 2^-20 of the largest |value|, off by at most half a step
    for name, lab, roots, vals, rows in (("mean_value", la, order, temp[2], np.ones(len(order), dtype=bool)),
                                         ("match_mean_value", lb, m[has], temp_b, has)):
        want = np.array([vals[lab == r].astype(np.float64).mean() for r in roots])
        step = float(np.abs(vals).max()) / 2 ** 20
        assert got[name].shape == (len(order),) and got[name].dtype == torch.float64
        np.testing.assert_allclose(got[name].numpy()[rows], want, rtol=0, atol=0.5 * step * (1 + 1e-9))
    assert np.isnan(got["match_mean_value"].numpy()[~has]).all()
    # channels, int32 weights in units of their scale, and no values
    q = np.stack([np.full(N_TRAJ, 2 ** 19), np.arange(N_TRAJ) % 3 - 1], axis=1).astype(np.int32)
    two = statistics.halo_matches(torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV), BOX, LL_TRAJ, MIN_TRAJ,
                                  values_a=torch.from_numpy(q).to(DEV))
    want = hm.group_sums(la, q)[order] / sa[order][:, None] / 2 ** 20
    np.testing.assert_allclose(two["mean_value"].numpy(), want, rtol=1e-15, atol=0)
    assert (two["mean_value"][:, 0] == 0.5).all() and "match_mean_value" not in two
    assert torch.equal(two["match_root"], got["match_root"])


def test_rollout_halo_matching_equals_the_restatement():
    truth, pred, _ = _trajectory()
    edges = [MIN_TRAJ, 10, 20, 40, 200, N_TRAJ + 1]
    data, gt = {"Coordinates": torch.from_numpy(pred).to(DEV)}, {"Coordinates": torch.from_numpy(truth)}
    got = statistics.rollout_halo_matching(data, gt, BOX, LL_TRAJ, edges)
    assert got["frames"] == [0, 1, 2] and got["size_lo"].tolist() == edges[:-1] and got["size_hi"].tolist() == edges[1:]
    for t in range(3):
        (_, sa, _), (_, sb, _), (mab, sab, mba, sba, summary) = _restated_frame(truth[t], pred[t], edges=edges)
        mutual = hm.mutual(mab, mba)
        assert got["n_true"][t].tolist() == summary[:, 0].tolist() and got["n_matched"][t].tolist() == summary[:, 1].tolist()
        assert got["n_mutual"][t].tolist() == summary[:, 2].tolist()
        with np.errstate(invalid="ignore", divide="ignore"):
            for name, num, den in (("completeness", 2, 0), ("shared_fraction", 3, 4), ("size_ratio", 5, 4)):
                np.testing.assert_array_equal(got[name][t].numpy(), summary[:, num] / summary[:, den])
        assert int(got["n_groups_true"][t]) == (sa >= MIN_TRAJ).sum() == summary[:, 0].sum()
        assert int(got["n_groups_pred"][t]) == (sb >= MIN_TRAJ).sum()
        assert int(got["n_unmatched_pred"][t]) == (sb >= MIN_TRAJ).sum() - mutual.sum()
    assert got["n_true"].dtype == torch.int64 and got["completeness"].dtype == torch.float64
    # frame 0 is the truth itself; the last frame has lost groups
    assert (got["completeness"][0][got["n_true"][0] > 0] == 1).all() and int(got["n_unmatched_pred"][0]) == 0
    assert int(got["n_mutual"][2].sum()) < int(got["n_true"][2].sum()) and int(got["n_mutual"][2].sum()) >= 3
    assert torch.isnan(got["completeness"][got["n_true"] == 0]).all()
    # a selection of frames, another minimum, and the device part does not wait for the host
    some = statistics.rollout_halo_matching(data, gt, BOX, LL_TRAJ, edges, frames=[2, 0], min_members=8)
    assert some["frames"] == [2, 0] and torch.equal(some["n_true"][:, 1:], got["n_true"][[2, 0], 1:])
    assert int(some["n_true"][0, 0]) < int(got["n_true"][2, 0])
    e = ops.check_size_edges(edges, "test")
    frames = (torch.from_numpy(truth).to(DEV), torch.from_numpy(pred).to(DEV))
    warm = statistics.halo_matching_on_device(*frames, BOX, LL_TRAJ, e, MIN_TRAJ)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = statistics.halo_matching_on_device(*frames, BOX, LL_TRAJ, e, MIN_TRAJ)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again, warm) and again.shape == (3, 6 * 5 + 3)


def test_a_rollout_equal_to_the_truth_matches_itself():
    truth, _, _ = _trajectory()
    data = {"Coordinates": torch.from_numpy(truth).to(DEV)}
    got = statistics.rollout_halo_matching(data, data, BOX, LL_TRAJ, [MIN_TRAJ, 20, N_TRAJ + 1])
    assert (got["n_true"] > 0).all() and torch.equal(got["n_mutual"], got["n_true"])
    for name in ("completeness", "shared_fraction", "size_ratio"):
        assert (got[name] == 1).all(), name
    assert (got["n_unmatched_pred"] == 0).all() and torch.equal(got["n_groups_pred"], got["n_groups_true"])
    pos = torch.from_numpy(truth[1]).to(DEV)
    one = statistics.halo_matches(pos, pos, BOX, LL_TRAJ, MIN_TRAJ)
    assert len(one["root"]) == int(got["n_groups_true"][1]) and one["mutual"].all()
    assert torch.equal(one["match_root"], one["root"]) and torch.equal(one["shared"], one["size"])
    assert torch.equal(one["match_size"], one["size"]) and (one["centre_offset"] == 0).all()


def test_a_permutation_of_the_particles_permutes_the_roots_and_changes_no_count():
    truth, pred, _ = _trajectory()
    xa, xb = truth[2], pred[2]
    perm = np.random.default_rng(70).permutation(N_TRAJ)                         # new particle j is old particle perm[j]
    inv = np.argsort(perm)
    one = statistics.halo_matches(torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV), BOX, LL_TRAJ, MIN_TRAJ)
    two = statistics.halo_matches(torch.from_numpy(xa[perm]).to(DEV), torch.from_numpy(xb[perm]).to(DEV), BOX, LL_TRAJ,
                                  MIN_TRAJ)
    la = _catalogue(xa, LL_TRAJ)[0].cpu().numpy()
    lb = _catalogue(xb, LL_TRAJ)[0].cpu().numpy()
    new_a = {int(r): int(inv[la == r].min()) for r in one["root"].tolist()}
    new_b = {int(r): int(inv[lb == r].min()) for r in one["match_root"].tolist() if r >= 0}
    new_b[-1] = -1

    # a tie falls to the smaller root, and which root is smaller the permutation changes: no group of A is tied here,
    # and where a group of B is tied between groups of A, whether its partners' matches are mutual is left out
    assert len(hm.ties(la, hm.sizes(la), lb, hm.sizes(lb), MIN_TRAJ)) == 0
    tied_b = {new_b.get(int(r)) for r in hm.ties(lb, hm.sizes(lb), la, hm.sizes(la), MIN_TRAJ)} - {None}

    def rows(res, name_a=int, name_b=int):
        return sorted((-int(s), name_a(int(r)), name_b(int(m)), int(ms), int(sh), name_b(int(m)) in tied_b or bool(mu))
                      for r, s, m, ms, sh, mu in zip(res["root"], res["size"], res["match_root"], res["match_size"],
                                                     res["shared"], res["mutual"]))

    assert rows(one, new_a.get, new_b.get) == rows(two) and len(one["root"]) >= 10
    assert sum(1 for row in rows(two) if row[2] >= 0 and row[2] not in tied_b) >= 10
    # a centre is now measured from another member: every folded float32 displacement carries one rounding of at most
    # 2^-24 L, so a centre moves by less than 2^-23 L per axis and an offset of two of them by less than 2^-20 L
    np.testing.assert_allclose(np.sort(one["centre_offset"].numpy()), np.sort(two["centre_offset"].numpy()), rtol=0,
                               atol=BOX / 2 ** 20, equal_nan=True)


def test_the_centre_offset_of_a_group_across_a_box_face_is_under_the_minimum_image():
    rng = np.random.default_rng(80)
    d = rng.standard_normal((30, 3))
    d *= (0.1 * rng.random((30, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)      # a ball of radius 0.1
    blob = np.array([0.15, 12.0, 12.0]) + d                                     # just inside the face x = 0
    rest = rng.random((50, 3)) * BOX
    xa = _wrapped(np.concatenate([blob, rest]))
    xb = _wrapped(np.concatenate([blob - np.array([0.4, 0.0, 0.0]), rest]))     # the blob moves through the face
    assert (xa[:30, 0] < 0.3).all() and (xb[:30, 0] > BOX - 0.4).all()
    got = statistics.halo_matches(torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV), BOX, 0.5, 20)
    assert got["root"].tolist() == [0] and got["size"].tolist() == [30] and got["match_root"].tolist() == [0]
    assert got["shared"].tolist() == [30] and got["mutual"].tolist() == [True]
    assert abs(float(got["centre_offset"][0]) - 0.4) < 1e-5                     # not BOX - 0.4
    assert float(got["centre"][0, 0]) < 0.3 and float(got["match_centre"][0, 0]) > BOX - 0.4
    # and a minimum no group reaches: an empty list, the shapes kept
    none = statistics.halo_matches(torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV), BOX, 0.5, 31,
                                   values_a=torch.rand(80, 2, device=DEV), values_b=torch.rand(80, device=DEV))
    assert {k: tuple(v.shape) for k, v in none.items()} == {
        "root": (0,), "size": (0,), "centre": (0, 3), "match_root": (0,), "match_size": (0,), "shared": (0,),
        "mutual": (0,), "match_centre": (0, 3), "centre_offset": (0,), "mean_value": (0, 2), "match_mean_value": (0,)}
