"""numpy restatement of the counting contract of ``cgnn_pair_counts`` (include/cgnn.h), for the tests: a brute force over
all pairs in float32, one rounding per operation, chunked over rows.

    d  = fl32(b - a) per axis;  half = fl32(0.5 * L);  d > half: fl32(d - L);  d < -half: fl32(d + L)
    d2 = fl32(fl32(fl32(dx dx) + fl32(dy dy)) + fl32(dz dz))
    bin = searchsorted(e2, d2, side="right") - 1   with e2 = fl32(edges * edges);  kept when 0 <= bin < nb

numpy rounds every float32 ufunc once and fuses nothing, which is the contract.
"""
import numpy as np

CHUNK = 512

# 8^3 points at integer coordinates in a box of side 8, edges 0, 0.5, ..., 4: lattice vectors of squared norm 1, 2, 3,
# 4, ... come 6, 12, 8, 6, 24, 24, 0, 12, 30, 24, 24, 8, 24, 48, 0 times (norms 1 .. 15; 16 is outside), each seen from
# N / 2 = 256 ordered starting points per unordered pair.  d2 = 1, 4, 9 sit on an edge and fall in the UPPER bin.
LATTICE_EDGES = np.arange(9, dtype=np.float32) * np.float32(0.5)
LATTICE_COUNTS = [0, 0, 4608, 2048, 13824, 3072, 22016, 18432]


def lattice_points(shift=0.0):
    g = np.arange(8, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return (pts + np.float32(shift)).astype(np.float32)


def _fold(d, box, half):
    return np.where(d > half, d - box, np.where(d < -half, d + box, d)).astype(np.float32)


def squared_edges(edges):
    e = np.asarray(edges, dtype=np.float32)
    return e * e


def _cross_ordered(a, b, box_size, edges, skip_diagonal):
    """Ordered pairs (a_i, b_j), int64 [nb]; skip_diagonal leaves out i == j (a is b then)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    box = np.float32(box_size)
    half = np.float32(0.5) * box
    e2 = squared_edges(edges)
    nb = e2.size - 1
    counts = np.zeros(nb, dtype=np.int64)
    for r0 in range(0, a.shape[0], CHUNK):
        rows = a[r0:r0 + CHUNK]
        d2 = None
        for ax in (0, 1, 2):
            d = _fold(b[None, :, ax] - rows[:, None, ax], box, half)
            sq = d * d
            d2 = sq if d2 is None else d2 + sq
        assert d2.dtype == np.float32
        idx = np.searchsorted(e2, d2, side="right") - 1
        keep = (idx >= 0) & (idx < nb)
        if skip_diagonal:
            i = np.arange(rows.shape[0])
            keep[i, r0 + i] = False
        counts += np.bincount(idx[keep], minlength=nb)[:nb]
    return counts


def cross_counts(a, b, box_size, edges):
    """Every ordered pair (a in A, b in B) once."""
    return _cross_ordered(a, b, box_size, edges, False)


def auto_counts(a, box_size, edges):
    """Every unordered pair i < j once: the ordered pairs i != j, halved (the contract is symmetric)."""
    ordered = _cross_ordered(a, a, box_size, edges, True)
    assert (ordered % 2 == 0).all()
    return ordered // 2


def expected_random_pairs(n, box_size, edges):
    """Pairs a uniform random set of n points has per bin on average: N (N - 1) / 2 * V_b / L^3, float64."""
    r = np.asarray(edges, dtype=np.float32).astype(np.float64)
    shell = 4.0 * np.pi / 3.0 * (r[1:] ** 3 - r[:-1] ** 3)
    return n * (n - 1) / 2.0 * shell / float(box_size) ** 3
