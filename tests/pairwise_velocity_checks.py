"""numpy restatement of the contract of ``cgnn_pair_velocity_sums`` (include/cgnn.h), for the tests: a brute force over
all ordered pairs, every float32 operation a numpy float32 operation (one rounding each, nothing fused), chunked over
rows; the totals are Python integers.

    dx, dy, dz, d2   as in pair_count_checks: folded per axis, d2 = fl32(fl32(fl32(dx dx) + fl32(dy dy)) + fl32(dz dz))
    bin  = searchsorted(e2, d2, side="right") - 1   with e2 = fl32(edges^2);  kept when 0 <= bin < nb
    dq_c = q_b[c] - q_a[c]                     exact integers, |dq_c| <= 2^21
    t2   = dq_x^2 + dq_y^2 + dq_z^2            exact integers, < 2^44
    w    = fl32(fl32(fl32(f(dq_x) dx) + fl32(f(dq_y) dy)) + fl32(f(dq_z) dz))      f: int -> float32, exact below 2^24
    d2 > 0:  r = fl32(sqrt(d2)), u = fl32(w / r), iu = rint(u)      numpy's float32 sqrt and / are correctly rounded
    d2 == 0: iu = 0
    per bin: counts += 1, S1 += iu, R2 += iu^2, T2 += t2

Also the two-word form the device returns (``split_words`` / ``join_words``): a total v as (lo, hi) with v = hi 2^32 + lo
and 0 <= lo < 2^32.
"""
import numpy as np

from pair_count_checks import _fold, squared_edges

CHUNK = 256
Q_ONE = 1 << 20                 # one value scale (ops.quantize_weights, _lib.WEIGHT_BITS)
MOMENTS = ("S1", "R2", "T2")


def split_words(v):
    """A Python integer total -> (lo, hi) with v == hi * 2^32 + lo and 0 <= lo < 2^32 (hi negative for a negative v)."""
    v = int(v)
    return v & 0xffffffff, v >> 32


def join_words(lo, hi):
    return (int(hi) << 32) + int(lo)


def words(sums):
    """Python integer totals [nb][3] -> int64 [nb, 3, 2], what the device returns."""
    return np.array([[split_words(v) for v in row] for row in sums], dtype=np.int64).reshape(len(sums), 3, 2)


def totals(word_array):
    """int64 [..., 3, 2] -> nested lists of Python integers [...][3]."""
    w = np.asarray(word_array)
    if w.ndim == 1:
        return join_words(w[0], w[1])
    return [totals(x) for x in w]


def quantize(v, scale):
    """ops.quantize_weights in numpy: round(clamp(v / scale, -1, 1) * 2^20), ties to even, int32."""
    a = np.clip(np.asarray(v, dtype=np.float64) / float(scale), -1.0, 1.0)
    return np.rint(a * float(Q_ONE)).astype(np.int32)


def pair_terms(a, qa, b, qb, box_size):
    """Every ordered pair of the rows ``a`` with the rows ``b``: ``(d2 float32, iu int64, t2 int64, d float64)`` as
    [len(a), len(b)] arrays; ``d`` is the float64 length of the folded float32 separation (for the physics tests)."""
    box = np.float32(box_size)
    half = np.float32(0.5) * box
    dq = qb[None, :, :].astype(np.int64) - qa[:, None, :].astype(np.int64)
    assert np.abs(dq).max(initial=0) <= 2 * Q_ONE
    d = [_fold(b[None, :, ax] - a[:, None, ax], box, half) for ax in (0, 1, 2)]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    f = dq.astype(np.float32)
    w = (f[..., 0] * d[0] + f[..., 1] * d[1]) + f[..., 2] * d[2]
    assert d2.dtype == np.float32 and w.dtype == np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        u = w / np.sqrt(d2)
    assert u.dtype == np.float32
    iu = np.where(d2 > 0, np.rint(u), np.float32(0)).astype(np.int64)
    t2 = (dq * dq).sum(axis=-1)
    length = np.sqrt(sum(x.astype(np.float64) ** 2 for x in d))
    return d2, iu, t2, length


def _bin_sums(idx, values, nb):
    """Exact per-bin sums of non-negative int64 ``values`` < 2^44 as Python integers: the 22 low and the high bits go
    through float64 bincounts apart, which stay below 2^53 for a chunk of at most 2^22 pairs."""
    assert values.size <= 1 << 22
    lo = np.bincount(idx, weights=(values & 0x3fffff).astype(np.float64), minlength=nb)
    hi = np.bincount(idx, weights=(values >> 22).astype(np.float64), minlength=nb)
    assert lo.max(initial=0) < 2.0 ** 53 and hi.max(initial=0) < 2.0 ** 53
    return [int(l) + (int(h) << 22) for l, h in zip(lo, hi)]


def _cross_ordered(a, qa, b, qb, box_size, edges, skip_diagonal, with_lengths=False):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    qa, qb = np.asarray(qa), np.asarray(qb)
    assert qa.shape == a.shape and qb.shape == b.shape and qa.dtype == np.int32 and qb.dtype == np.int32
    assert np.abs(qa).max(initial=0) <= Q_ONE and np.abs(qb).max(initial=0) <= Q_ONE
    e2 = squared_edges(edges)
    nb = e2.size - 1
    counts = [0] * nb
    sums = [[0, 0, 0] for _ in range(nb)]
    lengths = np.zeros(nb, dtype=np.float64)
    chunk = max(1, min(CHUNK, (1 << 22) // max(1, b.shape[0])))
    for r0 in range(0, a.shape[0], chunk):
        rows = slice(r0, r0 + chunk)
        d2, iu, t2, length = pair_terms(a[rows], qa[rows], b, qb, box_size)
        idx = np.searchsorted(e2, d2, side="right") - 1
        keep = (idx >= 0) & (idx < nb)
        if skip_diagonal:
            i = np.arange(d2.shape[0])
            keep[i, r0 + i] = False
        idx, iu, t2 = idx[keep], iu[keep], t2[keep]
        pos, neg = _bin_sums(idx, np.maximum(iu, 0), nb), _bin_sums(idx, np.maximum(-iu, 0), nb)
        r2, tt = _bin_sums(idx, iu * iu, nb), _bin_sums(idx, t2, nb)
        n = np.bincount(idx, minlength=nb)
        lengths += np.bincount(idx, weights=length[keep], minlength=nb)
        for k in range(nb):
            counts[k] += int(n[k])
            sums[k][0] += pos[k] - neg[k]
            sums[k][1] += r2[k]
            sums[k][2] += tt[k]
    if with_lengths:
        return counts, sums, lengths
    return counts, sums


def cross_sums(a, qa, b, qb, box_size, edges):
    """Every ordered pair (a in A, b in B) once: ``(counts [nb], sums [nb][3])`` as Python integers."""
    return _cross_ordered(a, qa, b, qb, box_size, edges, False)


def auto_sums(x, q, box_size, edges, with_lengths=False):
    """Every unordered pair i < j once: the ordered pairs i != j, halved (the contract is symmetric, so every total is
    even).  ``with_lengths``: also the float64 sum of the counted pairs' separations per bin."""
    counts, sums, lengths = _cross_ordered(x, q, x, q, box_size, edges, True, True)
    assert all(c % 2 == 0 for c in counts) and all(v % 2 == 0 for row in sums for v in row)
    out = [c // 2 for c in counts], [[v // 2 for v in row] for row in sums]
    return out + (lengths / 2.0,) if with_lengths else out


# ---- velocity fields of the physics tests: points in a ball of radius L / 5 around the box centre, so no image wraps ----
def ball_points(n, seed, box_size):
    """n float32 points uniform in the ball of radius box_size / 5 around the centre of the box."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d *= (0.2 * box_size * rng.random((n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(d, axis=1, keepdims=True)
    return (0.5 * box_size + d).astype(np.float32)


def rotation_field(x, box_size, omega=(0.3, -0.5, 0.8)):
    """omega x (x - c) in float64: a rigid rotation about the box centre; no relative velocity has a radial part."""
    return np.cross(np.asarray(omega, dtype=np.float64), x.astype(np.float64) - 0.5 * box_size)


def expansion_field(x, box_size, hubble):
    """H (x - c) in float64: every relative velocity is H times the separation, along it."""
    return hubble * (x.astype(np.float64) - 0.5 * box_size)


def moments(counts, sums, scale):
    """float64 (v12, sigma_par, sigma_perp) per bin from Python integer totals: statistics.pairwise_velocity_moments."""
    step = float(scale) / Q_ONE
    out = []
    for c, (s1, r2, t2) in zip(counts, sums):
        if c == 0:
            out.append((np.nan, np.nan, np.nan))
            continue
        mean = s1 / c
        out.append((step * mean, step * np.sqrt(max(r2 / c - mean * mean, 0.0)),
                    step * np.sqrt(max(t2 - r2, 0) / (2.0 * c))))
    return np.array(out, dtype=np.float64).T


def gaussian_deviations(v12, sigma_par, sigma_perp, sigma_v):
    """Isotropic Gaussian velocities of width sigma_v have v12 = 0 and sigma_par = sigma_perp = sqrt(2) sigma_v: the
    largest deviations over the bins, |v12| / sigma_v and |sigma / (sqrt(2) sigma_v) - 1| for the two dispersions."""
    root = np.sqrt(2.0) * sigma_v
    return {"v12": float(np.abs(v12).max() / sigma_v), "sigma_par": float(np.abs(np.asarray(sigma_par) / root - 1.0).max()),
            "sigma_perp": float(np.abs(np.asarray(sigma_perp) / root - 1.0).max())}
