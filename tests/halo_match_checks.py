"""numpy restatement of the contract of ``cgnn_halo_match`` and ``cgnn_fof_group_sums`` (include/cgnn.h), for the tests.

    listed(side, r)   iff  size_side[r] >= min_side
    counts(i)         iff  labels_a[i], labels_b[i] in [0, n)  and  listed(a, labels_a[i])  and  listed(b, labels_b[i])
    shared(ra, rb)    =    #{i : counts(i), labels_a[i] == ra, labels_b[i] == rb}
    match_ab[ra]      =    the rb with the largest shared(ra, rb), ties to the smallest rb;  shared_ab[ra] that count;
                           -1 and 0 at every slot without a counting member
    summary[b]        =    over the listed r of A with e[b] <= size_a[r] < e[b + 1]: the groups, those with a match, the
                           mutual ones (match_ba[match_ab[r]] == r), and over the mutual ones the sums of shared_ab[r],
                           size_a[r] and size_b[match_ab[r]]
"""
import numpy as np


def labels_of_groups(group):
    """A labelling in the sense of cgnn_fof_labels from arbitrary group numbers: every particle is labelled by the smallest
    index among the particles of its group.  int32 [n]."""
    group = np.asarray(group, dtype=np.int64)
    first = np.full(int(group.max()) + 1, len(group), dtype=np.int64)
    np.minimum.at(first, group, np.arange(len(group)))
    return first[group].astype(np.int32)


def sizes(labels):
    """size as cgnn_fof_catalogue writes it: the members at each root slot, labels outside [0, n) skipped.  int32 [n]."""
    labels = np.asarray(labels, dtype=np.int64)
    n = len(labels)
    ok = (labels >= 0) & (labels < n)
    return np.bincount(labels[ok], minlength=n).astype(np.int32)


def shared_pairs(labels_a, size_a, labels_b, size_b, min_a, min_b):
    """The distinct (ra, rb) of the counting particles and their counts: int64 [K], [K], [K], sorted by (ra, rb)."""
    la, lb = np.asarray(labels_a, dtype=np.int64), np.asarray(labels_b, dtype=np.int64)
    sa, sb = np.asarray(size_a, dtype=np.int64), np.asarray(size_b, dtype=np.int64)
    n = len(la)
    ok = (la >= 0) & (la < n) & (lb >= 0) & (lb < n)
    ok[ok] = (sa[la[ok]] >= min_a) & (sb[lb[ok]] >= min_b)
    keys, counts = np.unique(la[ok] * n + lb[ok], return_counts=True)
    return keys // n, keys % n, counts.astype(np.int64)


def _best(n, own, other, counts):
    match, shared = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    order = np.lexsort((other, -counts, own))           # by own root, then the larger count, then the smaller partner
    own, other, counts = own[order], other[order], counts[order]
    first = np.ones(len(own), dtype=bool)
    first[1:] = own[1:] != own[:-1]
    match[own[first]] = other[first]
    shared[own[first]] = counts[first]
    return match, shared


def halo_match(labels_a, size_a, labels_b, size_b, min_a, min_b=None, size_edges=None):
    """(match_ab, shared_ab, match_ba, shared_ba, summary): int32 [n] four times and int64 [nb, 6] (None without edges)."""
    min_b = min_a if min_b is None else min_b
    n = len(labels_a)
    ra, rb, counts = shared_pairs(labels_a, size_a, labels_b, size_b, min_a, min_b)
    match_ab, shared_ab = _best(n, ra, rb, counts)
    match_ba, shared_ba = _best(n, rb, ra, counts)
    summary = None
    if size_edges is not None:
        e = np.asarray(size_edges, dtype=np.int64)
        sa, sb = np.asarray(size_a, dtype=np.int64), np.asarray(size_b, dtype=np.int64)
        summary = np.zeros((len(e) - 1, 6), dtype=np.int64)
        for r in np.flatnonzero(sa >= min_a):
            b = int(np.searchsorted(e, sa[r], side="right")) - 1
            if b < 0 or b >= len(e) - 1:
                continue
            summary[b, 0] += 1
            m = int(match_ab[r])
            if m < 0:
                continue
            summary[b, 1] += 1
            if match_ba[m] == r:
                summary[b, 2:] += (1, shared_ab[r], sa[r], sb[m])
    return match_ab, shared_ab, match_ba, shared_ba, summary


def mutual(match_ab, match_ba):
    """bool [n]: the slots r of A with a match whose match has r as its match."""
    m = np.asarray(match_ab, dtype=np.int64)
    return (m >= 0) & (np.asarray(match_ba, dtype=np.int64)[np.maximum(m, 0)] == np.arange(len(m)))


def ties(labels_a, size_a, labels_b, size_b, min_a, min_b=None):
    """The A roots whose largest shared count is reached by more than one B root."""
    ra, rb, counts = shared_pairs(labels_a, size_a, labels_b, size_b, min_a, min_a if min_b is None else min_b)
    best = np.zeros(len(labels_a), dtype=np.int64)
    np.maximum.at(best, ra, counts)
    at_best = np.bincount(ra[counts == best[ra]], minlength=len(labels_a))
    return np.flatnonzero(at_best > 1)


def group_sums(labels, q):
    """int64 [n, C]: at a root slot the sum of its members' q [n, C]; labels outside [0, n) skipped."""
    labels = np.asarray(labels, dtype=np.int64)
    q = np.asarray(q, dtype=np.int64).reshape(len(labels), -1)
    ok = (labels >= 0) & (labels < len(labels))
    out = np.zeros(q.shape, dtype=np.int64)
    np.add.at(out, labels[ok], q[ok])
    return out
