"""The contracts of ``cgnn_knn_distances`` and ``cgnn_knn_cdf_counts`` (include/cgnn.h) restated in numpy, and the query
lattice of ``statistics.query_lattice``: what the CPU and GPU tests compare against.

Distances: a brute force over the 27 n periodic images the graph builder ranks, every float32 operation rounded once
(``.astype(np.float32)`` after each; numpy's elementwise float32 operations do not fuse), then a sort per query and the
ranks picked.  Only values are kept, so ties need no rule.  Counts: ``v < fl32(r r)``, strict."""
import math

import numpy as np

F = np.float32
CHUNK = 1 << 25          # image distances formed at a time (128 MiB of float32)


def image_d2(pos, queries, box_size):
    """float32 ``[nq, 27 n]``: the squared distance from every query to every image, by the contract:
    ``e = fl32(pos + fl32(s box))``, ``d = fl32(e - q)``, ``d2 = fl32(fl32(fl32(dx dx) + fl32(dy dy)) + fl32(dz dz))``."""
    pos = np.ascontiguousarray(pos, dtype=F)
    q = np.ascontiguousarray(queries, dtype=F)
    shift = (np.array([-1.0, 0.0, 1.0], dtype=F) * F(box_size)).astype(F)
    sq = []
    for axis in range(3):
        e = (pos[None, :, axis] + shift[:, None]).astype(F)                  # [3, n]
        d = (e[None, :, :] - q[:, None, None, axis]).astype(F)               # [nq, 3, n]
        sq.append((d * d).astype(F))
    xy = (sq[0][:, :, None, :] + sq[1][:, None, :, :]).astype(F)             # [nq, 3, 3, n]
    d2 = (xy[:, :, :, None, :] + sq[2][:, None, None, :, :]).astype(F)       # [nq, 3, 3, 3, n]
    return d2.reshape(q.shape[0], -1)


def knn_table(pos, queries, box_size, kmax):
    """float32 ``[nq, kmax]``: the ``kmax`` smallest image distances of every query, ascending."""
    pos = np.asarray(pos, dtype=F)
    queries = np.asarray(queries, dtype=F)
    n, nq = pos.shape[0], queries.shape[0]
    assert 1 <= kmax <= 27 * n
    out = np.empty((nq, kmax), dtype=F)
    step = max(1, CHUNK // (27 * n))
    for a in range(0, nq, step):
        d2 = image_d2(pos, queries[a:a + step], box_size)
        if kmax < d2.shape[1]:
            d2 = np.partition(d2, kmax - 1, axis=1)[:, :kmax]
        out[a:a + step] = np.sort(d2, axis=1)
    return out


def knn_distances(pos, queries, box_size, ks):
    """float32 ``[nq, nk]``: ``d2[q, j]`` is the ``ks[j]``-th smallest image distance of query ``q``."""
    ks = [int(k) for k in ks]
    assert ks[0] >= 1 and all(b > a for a, b in zip(ks, ks[1:]))
    return knn_table(pos, queries, box_size, ks[-1])[:, [k - 1 for k in ks]]


def cdf_counts(d2_a, radii, d2_b=None):
    """int64 ``[nk, nr]``: ``below[j, b] = #{q : v[q, j] < fl32(r_b r_b)}``, ``v = d2_a`` or ``max(d2_a, d2_b)``."""
    v = np.asarray(d2_a, dtype=F)
    if d2_b is not None:
        v = np.maximum(v, np.asarray(d2_b, dtype=F))
    r = np.asarray(radii, dtype=F).reshape(-1)
    e2 = (r * r).astype(F)
    return (v[:, :, None] < e2[None, None, :]).sum(axis=0).astype(np.int64)


def query_lattice(m, box_size):
    """float32 ``[m^3, 3]``: the cell centres ``fl32((i + 0.5) box / m)``, x slowest."""
    c = ((np.arange(m, dtype=np.float64) + 0.5) * float(box_size) / m).astype(F)
    g = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1)
    return np.ascontiguousarray(g.reshape(m ** 3, 3))


def binomial_tail(n, p, k):
    """``P(Binomial(n, p) >= k)`` in float64, for small ``k``."""
    return 1.0 - sum(math.comb(n, i) * p ** i * (1.0 - p) ** (n - i) for i in range(k))


def expected_below(n, nq, box_size, radii, ks):
    """For ``n`` uniform points and ``nq`` queries whose spheres do not overlap: the expectation of ``below[j, b]``,
    ``nq P(Binomial(n, (4/3) pi r^3 / box^3) >= k)`` -- exact for a fixed-``n`` uniform sample -- and its standard
    deviation ``sqrt(nq p (1 - p))``.  Both float64 ``[nk, nr]``."""
    mean = np.empty((len(ks), len(radii)))
    for b, r in enumerate(radii):
        vol = 4.0 / 3.0 * math.pi * float(r) ** 3 / float(box_size) ** 3
        for j, k in enumerate(ks):
            mean[j, b] = binomial_tail(n, vol, int(k))
    return nq * mean, np.sqrt(nq * mean * (1.0 - mean))


def min_image_d2_f64(pos, queries, box_size):
    """float64 ``[nq, n]``: the minimum-image squared distance, for the dyadic inputs on which float32 is exact."""
    d = np.asarray(pos, dtype=np.float64)[None, :, :] - np.asarray(queries, dtype=np.float64)[:, None, :]
    d -= float(box_size) * np.round(d / float(box_size))
    return (d * d).sum(axis=-1)
