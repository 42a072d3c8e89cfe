"""numpy restatements for the halo-profile tests: the counting contract of ``cgnn_halo_profiles`` (include/cgnn.h) as a
brute force over all (centre, particle) pairs, the spherical-overdensity rule of ``statistics.so_masses``, and the
stacking of ``statistics.rollout_halo_profiles``.

    d  = fl32(p - c) per axis;  half = fl32(0.5 * L);  d > half: fl32(d - L);  d < -half: fl32(d + L)
    d2 = fl32(fl32(fl32(dx dx) + fl32(dy dy)) + fl32(dz dz))
    bin = searchsorted(e2, d2, side="right") - 1   with e2 = fl32(edges * edges);  kept when 0 <= bin < nb

numpy rounds every float32 ufunc once and fuses nothing, which is the contract (``pair_count_checks`` computes the same
d2; the two are compared in test_halo_profiles_cpu.py).  Nothing is excluded: a centre is no particle.
"""
import numpy as np

from pair_count_checks import _fold, squared_edges

CHUNK = 64


def profiles(pos, centres, box_size, edges, q=None):
    """counts int64 [H, nb], and with q (int [N] or [N, C]) the sums int64 [H, nb(, C)]."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    centres = np.ascontiguousarray(centres, dtype=np.float32)
    box = np.float32(box_size)
    half = np.float32(0.5) * box
    e2 = squared_edges(edges)
    nb = e2.size - 1
    h = centres.shape[0]
    counts = np.zeros((h, nb), dtype=np.int64)
    qq = None
    if q is not None:
        qq = np.asarray(q).astype(np.int64).reshape(pos.shape[0], -1)
        sums = np.zeros((h, nb, qq.shape[1]), dtype=np.int64)
    for r0 in range(0, h, CHUNK):
        rows = centres[r0:r0 + CHUNK]
        d2 = None
        for ax in (0, 1, 2):
            d = _fold(pos[None, :, ax] - rows[:, None, ax], box, half)
            sq = d * d
            d2 = sq if d2 is None else d2 + sq
        assert d2.dtype == np.float32
        idx = np.searchsorted(e2, d2, side="right") - 1
        keep = (idx >= 0) & (idx < nb)
        for i in range(rows.shape[0]):
            k = keep[i]
            counts[r0 + i] = np.bincount(idx[i][k], minlength=nb)[:nb]
            if qq is not None:
                np.add.at(sums[r0 + i], idx[i][k], qq[k])
    if q is None:
        return counts
    return counts, (sums[..., 0] if np.asarray(q).ndim == 1 else sums)


def so_masses(counts, n, box_size, edges, delta=200.0):
    """(r_delta, m_delta) float64 [H] by the rule of statistics.so_masses, one halo at a time with plain loops."""
    r = np.asarray(edges, dtype=np.float32).astype(np.float64)
    assert r[0] == 0.0
    counts = np.asarray(counts, dtype=np.float64).reshape(-1, r.size - 1)
    rho = float(n) / float(box_size) ** 3
    r_delta = np.full(counts.shape[0], np.nan)
    for hh, row in enumerate(counts):
        inside = np.cumsum(row)                                        # N_i at edge i + 1
        dens = inside / (rho * (4.0 / 3.0 * np.pi) * r[1:] ** 3)           # D_i, i = 1 .. nb, at column i - 1
        first = next((j for j in range(dens.size) if dens[j] >= delta), None)
        if first is None:
            continue
        k = next((j for j in range(first + 1, dens.size) if dens[j] < delta), None)
        if k is None:
            continue
        l0, l1 = np.log(r[k]), np.log(r[k + 1])                            # edges k and k + 1 hold columns k - 1 and k
        d0, d1 = np.log(dens[k - 1]), np.log(dens[k])
        r_delta[hh] = np.exp(l0 + (np.log(delta) - d0) / (d1 - d0) * (l1 - l0))
    return r_delta, delta * rho * (4.0 / 3.0 * np.pi) * r_delta ** 3


def largest_groups(size, min_members, max_halos):
    """The roots of the max_halos largest groups with at least min_members members (size [N]: members at root slots,
    0 elsewhere), size descending, ties to the smaller root; and how many listed groups are left out."""
    size = np.asarray(size, dtype=np.int64)
    roots = [int(r) for r in np.nonzero(size >= min_members)[0]]
    roots.sort(key=lambda r: (-int(size[r]), r))
    return roots[:max_halos], max(len(roots) - max_halos, 0)


def stack(counts, sizes, size_edges):
    """Per-halo rows counts [H, ...] summed over the halos of each size bin: ([sb, ...], halos per bin [sb])."""
    counts = np.asarray(counts)
    se = np.asarray(size_edges, dtype=np.int64)
    out = np.zeros((se.size - 1,) + counts.shape[1:], dtype=counts.dtype)
    num = np.zeros(se.size - 1, dtype=np.int64)
    for row, s in zip(counts, sizes):
        b = int(np.searchsorted(se, int(s), side="right")) - 1
        if 0 <= b < se.size - 1:
            out[b] += row
            num[b] += 1
    return out, num
