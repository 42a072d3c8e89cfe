"""numpy restatement of the contract of ``cgnn_triplet_moments`` (include/cgnn.h), for the tests.

Stage 1 (``moments``): a brute force over all ordered (primary, neighbour) pairs, every float32 operation a numpy float32
operation (one rounding each, nothing fused), chunked over rows.

    dx, dy, dz, d2   as in pair_count_checks: folded per axis, d2 = fl32(fl32(fl32(dx dx) + fl32(dy dy)) + fl32(dz dz))
    bin  = searchsorted(e2, d2, side="right") - 1   with e2 = fl32(edges^2);  kept when 0 <= bin < nb and d2 > 0,
           and in auto mode when the neighbour is not the primary itself
    r    = fl32(sqrt(d2)),  u_c = fl32(d_c / r)         numpy's float32 sqrt and / are correctly rounded
    p_c[0] = 1,  p_c[k] = fl32(p_c[k-1] u_c)
    monomial (a, b, c), degree >= 1:  q = rint(fl32(fl32(p_x[a] p_y[b]) p_z[c]) 2^unit_bits)     ties to even
    M[i, bin, alpha] += q;  M[i, bin, 0] += 1

with the monomials in the order of ``monomials``: degree n = 0 .. lmax, a = n .. 0, b = n - a .. 0, c = n - a - b.

Stage 2 (``power_sums``): T[n, b1, b2] = sum_i sum_{|alpha| = n} mult(alpha) M[i, b1, alpha] M[i, b2, alpha] in exact Python
integers, with the sum of the terms' absolute values and their number K beside it: a float64 sum of K terms, each the
product of three exactly converted factors with two roundings, differs from the exact sum by at most (K + 2) 2^-53
sum|terms| in any order ((K - 1) additions and 2 roundings per term, to first order, and the +1 left over covers the
higher orders for every K a device can hold).  Where sum|terms| < 2^53 no operation rounds at all and the float64 sum is
the exact integer (``exact_in_float64``).

The bound of stage 1 against float64 directions (``moment_bound``).  u* = d / |d| in float64 from the same float32
separations, v* the monomial of u* and M* the sum of v* over the same counted pairs (``float64_moments``).  Per pair,
|q - 2^ub v| <= 1/2 (the rint), and v differs from v* by the float32 roundings: d2 carries three (two products and
sums of non-negative terms in a row: relative 3 eps, eps = 2^-24), the square root halves them and adds its own, every
division adds one, and a monomial of degree n multiplies n such factors with at most n - 1 more roundings.  The issue
that introduced the entry sets the per-pair allowance to (n + 4) eps |v*| <= (n + 4) eps, which the tests assert as it
stands:

    |M - 2^ub M*| <= count (1/2 + (n + 4) 2^(ub - 24))      elementwise, degree n, count = M[i, bin, 0]

A worst-case first-order count of the roundings above gives (4.5 n - 1) eps per pair -- every rounding at its limit and
in the same direction, on an axis-aligned pair whose d2 is then exact -- which the allowance undercuts from n = 2 on;
summed over the neighbours of a primary the roundings are independent and stay far inside it.  From it the bound on the
power sums and on DDD_l (``ddd_bound``): with E the bound above and A* = 2^ub |M*|,
    |M1 M2 - 2^(2 ub) M1* M2*| <= E1 A2* + E2 A1* + E1 E2
per primary and monomial, times mult(alpha), summed, divided by 2^(2 ub) and weighted with |c[l, n]|.
"""
import math

import numpy as np

from pair_count_checks import _fold, squared_edges

CHUNK = 256
# P_l(x) = sum_n LEGENDRE[l][n] x^n
LEGENDRE = ((1.0,), (0.0, 1.0), (-0.5, 0.0, 1.5), (0.0, -1.5, 0.0, 2.5), (0.375, 0.0, -3.75, 0.0, 4.375))


def monomials(lmax):
    """[(a, b, c)] in the contract's order."""
    return [(a, b, n - a - b) for n in range(lmax + 1) for a in range(n, -1, -1) for b in range(n - a, -1, -1)]


def multinomials(lmax):
    return [math.factorial(a + b + c) // (math.factorial(a) * math.factorial(b) * math.factorial(c))
            for a, b, c in monomials(lmax)]


def degree_slices(lmax):
    """slice of the monomials of degree n, for n = 0 .. lmax."""
    off = [n * (n + 1) * (n + 2) // 6 for n in range(lmax + 2)]
    return [slice(off[n], off[n + 1]) for n in range(lmax + 1)]


def legendre_matrix(lmax):
    c = np.zeros((lmax + 1, lmax + 1))
    for l in range(lmax + 1):
        c[l, :l + 1] = LEGENDRE[l]
    return c


def _counted(a, b, box_size, edges, auto):
    """Yields per row chunk (rows, cols, bins, dx, dy, dz, d2) of the counted pairs, float32."""
    box = np.float32(box_size)
    half = np.float32(0.5) * box
    e2 = squared_edges(edges)
    nb = e2.size - 1
    chunk = max(1, min(CHUNK, (1 << 22) // max(1, b.shape[0])))
    for r0 in range(0, a.shape[0], chunk):
        rows = a[r0:r0 + chunk]
        d = [_fold(b[None, :, ax] - rows[:, None, ax], box, half) for ax in (0, 1, 2)]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        assert d2.dtype == np.float32
        idx = np.searchsorted(e2, d2, side="right") - 1
        keep = (idx >= 0) & (idx < nb) & (d2 > 0)
        if auto:
            i = np.arange(rows.shape[0])
            keep[i, r0 + i] = False
        ri, ci = np.nonzero(keep)
        yield ri + r0, ci, idx[ri, ci], d[0][ri, ci], d[1][ri, ci], d[2][ri, ci], d2[ri, ci]


def _sets(pos, pos_b):
    a = np.ascontiguousarray(pos, dtype=np.float32)
    return a, (a if pos_b is None else np.ascontiguousarray(pos_b, dtype=np.float32))


def moments(pos, box_size, edges, lmax, pos_b=None, unit_bits=20):
    """``(M int64 [n_a, nb, n_mono], pairs int64 [nb])`` of the contract; ``pos_b is None``: auto."""
    a, b = _sets(pos, pos_b)
    nb = len(edges) - 1
    mono = monomials(lmax)
    unit = np.float32(2.0 ** unit_bits)
    m = np.zeros((a.shape[0] * nb, len(mono)), dtype=np.int64)
    for ri, _, bins, dx, dy, dz, d2 in _counted(a, b, box_size, edges, pos_b is None):
        flat = ri * nb + bins
        r = np.sqrt(d2)
        u = [dx / r, dy / r, dz / r]
        assert r.dtype == np.float32 and u[0].dtype == np.float32
        p = [[np.ones_like(r)] for _ in range(3)]
        for k in range(1, lmax + 1):
            for c in range(3):
                p[c].append(p[c][k - 1] * u[c])
        for al, (ea, eb, ec) in enumerate(mono):
            if al == 0:
                q = np.ones(flat.shape, dtype=np.float64)
            else:
                v = (p[0][ea] * p[1][eb]) * p[2][ec]
                assert v.dtype == np.float32
                q = np.rint(v * unit).astype(np.float64)               # whole numbers of at most 2^20 + 1 in size
            # float64 bincount of whole numbers: exact while every partial sum stays below 2^53
            assert flat.size * (2.0 ** unit_bits + 1) < 2.0 ** 53
            m[:, al] += np.bincount(flat, weights=q, minlength=m.shape[0]).astype(np.int64)
    m = m.reshape(a.shape[0], nb, len(mono))
    return m, m[:, :, 0].sum(axis=0)


def float64_moments(pos, box_size, edges, lmax, pos_b=None):
    """M* float64 [n_a, nb, n_mono]: the monomials of the float64 unit vectors d / |d| of the SAME counted pairs (the
    float32 separations and the float32 bins of the contract), summed in float64."""
    a, b = _sets(pos, pos_b)
    nb = len(edges) - 1
    mono = monomials(lmax)
    m = np.zeros((a.shape[0] * nb, len(mono)))
    for ri, _, bins, dx, dy, dz, _ in _counted(a, b, box_size, edges, pos_b is None):
        flat = ri * nb + bins
        d = np.stack([dx, dy, dz]).astype(np.float64)
        u = d / np.sqrt((d * d).sum(axis=0))
        for al, (ea, eb, ec) in enumerate(mono):
            m[:, al] += np.bincount(flat, weights=u[0] ** ea * u[1] ** eb * u[2] ** ec, minlength=m.shape[0])
    return m.reshape(a.shape[0], nb, len(mono))


def moment_bound(m, lmax, unit_bits):
    """The elementwise bound on |M - 2^ub M*|: count (1/2 + (n + 4) 2^(ub - 24)) for degree n."""
    deg = np.array([sum(e) for e in monomials(lmax)], dtype=np.float64)
    return m[:, :, :1].astype(np.float64) * (0.5 + (deg + 4.0) * 2.0 ** (unit_bits - 24))


def power_sums(m, lmax):
    """``(T, abs_sum, terms)``: object arrays [lmax + 1, nb, nb] of Python integers -- the exact power sums and the sums
    of the terms' absolute values -- and the number of terms K of an entry of degree n, [lmax + 1]."""
    mo = np.asarray(m).astype(object)
    mult = np.array(multinomials(lmax), dtype=object)
    nb = mo.shape[1]
    t = np.zeros((lmax + 1, nb, nb), dtype=object)
    s = np.zeros((lmax + 1, nb, nb), dtype=object)
    for n, sl in enumerate(degree_slices(lmax)):
        terms = mo[:, :, None, sl] * mo[:, None, :, sl] * mult[sl]
        t[n] = terms.sum(axis=(0, 3))
        s[n] = np.abs(terms).sum(axis=(0, 3))
    return t, s, [mo.shape[0] * (sl.stop - sl.start) for sl in degree_slices(lmax)]


def exact_in_float64(abs_sum):
    """The precondition of the exact comparison: every sum of absolute terms stays below 2^53, so no float64 operation
    of the contraction rounds, in any order."""
    return all(int(v) < 2 ** 53 for v in np.asarray(abs_sum).reshape(-1))


def ddd_from_power_sums(t, unit_bits, pairs=None):
    """float64 DDD_l [lmax + 1, nb, nb] from power sums (Python integers or floats); with ``pairs`` the degenerate
    triangles j == k leave the diagonal."""
    t = np.asarray(t)
    lmax = t.shape[0] - 1
    s = np.array([[[float(v) for v in row] for row in tn] for tn in t])
    s[1:] /= 2.0 ** (2 * unit_bits)
    ddd = np.einsum("ln,nab->lab", legendre_matrix(lmax), s)
    if pairs is not None:
        ddd = ddd - np.diag(np.asarray(pairs, dtype=np.float64))[None]
    return ddd


def ddd_float64(pos, box_size, edges, lmax, pos_b=None):
    """The float64 brute force: DDD_l [lmax + 1, nb, nb] = sum over primaries and their counted neighbours j in b1, k in
    b2 (j == k included) of P_l(u_j . u_k), a triple loop per primary over its neighbour lists."""
    a, b = _sets(pos, pos_b)
    nb = len(edges) - 1
    out = np.zeros((lmax + 1, nb, nb))
    coef = legendre_matrix(lmax)
    for ri, _, bins, dx, dy, dz, _ in _counted(a, b, box_size, edges, pos_b is None):
        d = np.stack([dx, dy, dz], axis=1).astype(np.float64)
        u = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
        for i in np.unique(ri):
            sel = ri == i
            cos = u[sel] @ u[sel].T
            bi = bins[sel]
            for l in range(lmax + 1):
                p = np.polynomial.polynomial.polyval(cos, coef[l])
                np.add.at(out[l], (bi[:, None], bi[None, :]), p)
    return out


def ddd_bound(m, m_star, lmax, unit_bits):
    """The bound on |DDD_l - DDD_l*| [lmax + 1, nb, nb] that follows from ``moment_bound`` (the module docstring), plus
    the float64 roundings of both sides, (K + 2) 2^-53 sum|terms| each."""
    e = moment_bound(m, lmax, unit_bits)
    a = np.abs(m_star) * 2.0 ** unit_bits
    a[:, :, 0] = np.abs(m_star[:, :, 0])                               # the count is not scaled
    mult = np.array(multinomials(lmax), dtype=np.float64)
    coef = np.abs(legendre_matrix(lmax))
    nb = m.shape[1]
    ds = np.zeros((lmax + 1, nb, nb))
    size = np.zeros((lmax + 1, nb, nb))
    for n, sl in enumerate(degree_slices(lmax)):
        e1, a1 = e[:, :, None, sl], a[:, :, None, sl]
        e2, a2 = e[:, None, :, sl], a[:, None, :, sl]
        scale = 1.0 if n == 0 else 2.0 ** (-2 * unit_bits)
        ds[n] = ((e1 * a2 + e2 * a1 + e1 * e2) * mult[sl]).sum(axis=(0, 3)) * scale
        size[n] = ((a1 + e1) * (a2 + e2) * mult[sl]).sum(axis=(0, 3)) * scale
    ds[0] = 0.0                                                        # the counts are exact
    k = m.shape[0] * 15 + 2
    return np.einsum("ln,nab->lab", coef, ds + 2.0 * k * 2.0 ** -53 * size)


def zeta_on_host(t_data, pairs_data, t_queries, pairs_queries, n, n_queries, box_size, edges, unit_bits=20):
    """statistics.three_point_zeta restated: ``(zeta, zeta_full, triplet_queries, xi)`` float64."""
    r = np.asarray(edges, dtype=np.float32).astype(np.float64)
    vol = 4.0 * np.pi / 3.0 * (r[1:] ** 3 - r[:-1] ** 3)
    nbar = n / float(box_size) ** 3
    lmax = np.asarray(t_data).shape[0] - 1
    ell = (2.0 * np.arange(lmax + 1) + 1.0)[:, None, None]
    norm = nbar * nbar * vol[:, None] * vol[None, :]
    trip_d = ell * ddd_from_power_sums(t_data, unit_bits, pairs_data) / (n * norm)
    trip_q = ell * ddd_from_power_sums(t_queries, unit_bits, pairs_queries) / (n_queries * norm)
    xi = np.asarray(pairs_data, dtype=np.float64) / (n * nbar * vol) - 1.0
    zeta = trip_d - trip_q
    zeta[0] -= xi[:, None] + xi[None, :]
    full = trip_d.copy()
    full[0] -= 1.0
    return zeta, full, trip_q, xi


# ---- point sets with an answer known by hand ---------------------------------------------------------------------------
def cubic_lattice(m=6, a=1.0):
    """m^3 points of a simple-cubic lattice of side a filling a periodic box of side m a: ``(points float32, box)``."""
    g = np.arange(m, dtype=np.float32) * np.float32(a)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32), float(m * a)


def line_points(box_size, reach, per_line=12, seed=0):
    """Points on four straight segments of length 2.5 reach in generic directions, a tenth of a reach apart on
    average, the segments in different octants of the box and further apart than the reach: every triplet within the
    reach is collinear."""
    rng = np.random.default_rng(seed)
    centres = np.array([[0.25, 0.25, 0.25], [0.75, 0.75, 0.25], [0.25, 0.75, 0.75], [0.75, 0.25, 0.75]]) * box_size
    assert 0.5 * box_size >= 2.5 * reach + reach                       # segments stay inside their octants' reach
    pts = []
    for c in centres:
        v = rng.standard_normal(3)
        v /= np.linalg.norm(v)
        s = np.sort(rng.random(per_line) - 0.5) * 2.5 * reach
        pts.append(c[None, :] + s[:, None] * v[None, :])
    return np.concatenate(pts).astype(np.float32)
