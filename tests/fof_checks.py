"""numpy restatement of the linking contract of ``cgnn_fof_labels`` and of the sums of ``cgnn_fof_catalogue``
(include/cgnn.h), for the tests: a brute-force float32 link matrix in row chunks, the squared distance of
``pair_count_checks`` (one rounding per operation), a small host union-find, and the catalogue in integers.

    linked(i, j)  iff  i != j  and  d2(i, j) < fl32(l * l)
    labels[i]     =    the smallest index of i's connected component
    q             =    rint(float64(fold(fl32(pos[i] - pos[root]))) * (2^30 / float64(fl32(L))))    summed per root
"""
import numpy as np

from pair_count_checks import CHUNK, _fold


def link_pairs(x, box_size, linking_length, with_d2=False):
    """The linked pairs (i, j) with i < j, int64 [P, 2], in row-major order; with_d2: their float32 d2 as well (the pairs
    of a shorter linking length l are then those with d2 < fl32(l * l): one brute force serves several lengths)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    box = np.float32(box_size)
    half = np.float32(0.5) * box
    ll = np.float32(linking_length)
    l2 = ll * ll
    assert l2.dtype == np.float32
    out, out_d2 = [], []
    for r0 in range(0, x.shape[0], CHUNK):
        rows = x[r0:r0 + CHUNK]
        d2 = None
        for ax in (0, 1, 2):
            d = _fold(x[None, :, ax] - rows[:, None, ax], box, half)
            sq = d * d
            d2 = sq if d2 is None else d2 + sq
        assert d2.dtype == np.float32
        link = d2 < l2
        i, j = np.nonzero(link)
        i = i + r0
        keep = i < j                        # the diagonal is excluded; the contract is symmetric
        out.append(np.stack([i[keep], j[keep]], axis=1))
        out_d2.append(d2[i[keep] - r0, j[keep]])
    pairs = np.concatenate(out).astype(np.int64)
    return (pairs, np.concatenate(out_d2)) if with_d2 else pairs


def labels_from_pairs(n, pairs):
    """Connected components by a host union-find that hooks the larger root under the smaller: int32 [n], every
    particle labelled by the smallest index of its component."""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j in pairs.tolist():
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int32)


def fof_labels(x, box_size, linking_length):
    return labels_from_pairs(len(x), link_pairs(x, box_size, linking_length))


def catalogue(x, labels, box_size, size_edges=None):
    """size int32 [n], disp int64 [n, 3], hist int64 [nb] (None without size_edges), as cgnn_fof_catalogue defines them."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    n = len(x)
    box = np.float32(box_size)
    half = np.float32(0.5) * box
    size = np.bincount(labels, minlength=n).astype(np.int32)
    d = _fold(x - x[labels], box, half)
    assert d.dtype == np.float32
    q = np.rint(d.astype(np.float64) * (2 ** 30 / np.float64(box))).astype(np.int64)
    disp = np.zeros((n, 3), dtype=np.int64)
    np.add.at(disp, labels, q)
    hist = None
    if size_edges is not None:
        e = np.asarray(size_edges, dtype=np.int64)
        idx = np.searchsorted(e, size[size > 0], side="right") - 1
        keep = (idx >= 0) & (idx < e.size - 1)
        hist = np.bincount(idx[keep], minlength=e.size - 1)[:e.size - 1].astype(np.int64)
    return size, disp, hist


def centres(x, root, size, disp, box_size):
    """(pos[root] + disp / size * L / 2^30) mod L in float64, L the float32 box."""
    box = np.float64(np.float32(box_size))
    c = x[root].astype(np.float64) + disp[root].astype(np.float64) / size[root].astype(np.float64)[:, None] * (box / 2 ** 30)
    return np.mod(c, box)
