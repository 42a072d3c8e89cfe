"""numpy restatement of the counting contract of ``cgnn_pair_counts_smu`` (include/cgnn.h), for the tests: a brute force
over all pairs in float32, one rounding per operation, chunked over rows.

    dx, dy, dz, d2   as in pair_count_checks: folded per axis, d2 = fl32(fl32(fl32(dx dx) + fl32(dy dy)) + fl32(dz dz))
    dl2 = fl32(dl dl)   dl the folded separation on axis los: the very product that enters d2
    s-bin  = searchsorted(e2, d2, side="right") - 1   with e2 = fl32(s_edges^2);  kept when 0 <= bin < ns
    mu-bin = #{ j' in 1 .. nmu - 1 : fl32(m2[j'] d2) <= dl2 }   with m2 = fl32(mu_edges^2)

numpy rounds every float32 ufunc once and fuses nothing, which is the contract.  The mu-bin is counted here literally,
threshold by threshold; the kernel's binary search gives the same number because the thresholds ascend
(``mu_thresholds`` lets a test see that).  Also: the closed-form integrals of L_0, L_2, L_4 over the mu-bins and the
pairs a uniform random set has per (s, mu) bin.
"""
import numpy as np

from pair_count_checks import _fold, squared_edges

CHUNK = 256


def mu_thresholds(mu_edges, d2):
    """fl32(m2[j'] d2) for j' = 1 .. nmu - 1 along a new last axis (float32)."""
    m2 = squared_edges(mu_edges)[1:-1]
    out = m2 * np.asarray(d2, dtype=np.float32)[..., None]
    assert out.dtype == np.float32
    return out


def _cross_ordered(a, b, box_size, s_edges, mu_edges, los, skip_diagonal):
    """Ordered pairs (a_i, b_j), int64 [ns, nmu]; skip_diagonal leaves out i == j (a is b then)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    box = np.float32(box_size)
    half = np.float32(0.5) * box
    e2 = squared_edges(s_edges)
    mu_edges = np.asarray(mu_edges, dtype=np.float32)
    assert mu_edges[0] == 0 and mu_edges[-1] == 1 and los in (0, 1, 2)
    ns, nmu = e2.size - 1, mu_edges.size - 1
    counts = np.zeros(ns * nmu, dtype=np.int64)
    for r0 in range(0, a.shape[0], CHUNK):
        rows = a[r0:r0 + CHUNK]
        d2 = dl2 = None
        for ax in (0, 1, 2):
            d = _fold(b[None, :, ax] - rows[:, None, ax], box, half)
            sq = d * d
            d2 = sq if d2 is None else d2 + sq
            if ax == los:
                dl2 = sq
        assert d2.dtype == np.float32 and dl2.dtype == np.float32
        idx = np.searchsorted(e2, d2, side="right") - 1
        keep = (idx >= 0) & (idx < ns)
        if skip_diagonal:
            i = np.arange(rows.shape[0])
            keep[i, r0 + i] = False
        d2k, dl2k = d2[keep], dl2[keep]
        j = (mu_thresholds(mu_edges, d2k) <= dl2k[:, None]).sum(axis=1) if nmu > 1 else np.zeros(d2k.size, dtype=np.int64)
        counts += np.bincount(idx[keep] * nmu + j, minlength=ns * nmu)
    return counts.reshape(ns, nmu)


def cross_counts(a, b, box_size, s_edges, mu_edges, los):
    """Every ordered pair (a in A, b in B) once."""
    return _cross_ordered(a, b, box_size, s_edges, mu_edges, los, False)


def auto_counts(x, box_size, s_edges, mu_edges, los):
    """Every unordered pair i < j once: the ordered pairs i != j, halved (the contract is symmetric)."""
    ordered = _cross_ordered(x, x, box_size, s_edges, mu_edges, los, True)
    assert (ordered % 2 == 0).all()
    return ordered // 2


def legendre_bin_integrals(mu_edges):
    """float64 [3, nmu]: the integrals of L_0, L_2, L_4 over each mu-bin, from the antiderivatives mu, (mu^3 - mu) / 2
    and (7 mu^5 - 10 mu^3 + 3 mu) / 8; the edges are the float32 values the kernel bins by."""
    mu = np.asarray(mu_edges, dtype=np.float32).astype(np.float64)
    prim = np.stack([mu, (mu ** 3 - mu) / 2.0, (7.0 * mu ** 5 - 10.0 * mu ** 3 + 3.0 * mu) / 8.0])
    return prim[:, 1:] - prim[:, :-1]


def expected_random_pairs(n, box_size, s_edges, mu_edges, n_b=None):
    """Pairs a uniform random set has per (s, mu) bin on average, float64 [ns, nmu]: N (N - 1) / 2 (or N N_b) times
    V_i / L^3 times the mu-bin's width (mu is |cos| folded into [0, 1]: a bin holds that fraction of a shell)."""
    s = np.asarray(s_edges, dtype=np.float32).astype(np.float64)
    mu = np.asarray(mu_edges, dtype=np.float32).astype(np.float64)
    shell = 4.0 * np.pi / 3.0 * (s[1:] ** 3 - s[:-1] ** 3) / float(box_size) ** 3
    pairs = n * (n - 1) / 2.0 if n_b is None else float(n) * float(n_b)
    return pairs * shell[:, None] * (mu[1:] - mu[:-1])[None, :]
