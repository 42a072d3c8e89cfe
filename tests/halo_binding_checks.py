"""numpy restatement of the contract of ``cgnn_halo_potentials`` (include/cgnn.h), of the member ordering of
``ops.halo_member_order`` and of the unbinding passes of ``statistics.halo_binding``, for the tests: a brute force per
group in float32 with one rounding per operation and int64 sums.

    d2   = the folded minimum-image squared distance of pair_count_checks (fl32, one rounding per operation)
    eps2 = fl32(eps eps);  s = fl32(d2 + eps2);  w = fl32(1 / fl32(sqrt(s)));  iw = rint(w 2^S)
    S    : w_max 2^S in [2^29, 2^30) for w_max = fl32(1 / fl32(sqrt(eps2)))
    P_i  = sum over j != i, j in i's group and active, of iw_ij     for i active in a listed group; 0 elsewhere

numpy rounds every float32 ufunc once (its sqrt and division are correctly rounded) and fuses nothing, which is the
contract.  The generators place compact blobs more than a linking length apart, so that the friends-of-friends groups of
a frame are the blobs, whatever the order of the particles.
"""
import math

import numpy as np

from pair_count_checks import _fold

MIN_SOFTENING_BITS = 16
BOX = 16.0              # a power of two: dyadic coordinates stay exact under translation and wrapping
LINKING = 1.0           # with blobs in cubes of side 0.5 (diagonal 0.87 < 1) every pair of a blob is linked
BLOB_SIDE = 0.5


def shift_of(eps, box_size):
    """(eps as float32, eps2, w_max, S), or ValueError for a softening outside the contract."""
    eps, box = np.float32(eps), np.float32(box_size)
    if not (np.isfinite(eps) and eps > 0) or eps < box * np.float32(2.0 ** -MIN_SOFTENING_BITS):
        raise ValueError("softening outside the contract")
    eps2 = eps * eps
    if not 2.0 ** -100 <= float(eps2) <= 2.0 ** 100:
        raise ValueError("softening outside the contract")
    w_max = np.float32(1) / np.sqrt(eps2)
    assert eps2.dtype == np.float32 and w_max.dtype == np.float32
    return eps, eps2, w_max, 30 - math.frexp(float(w_max))[1]


def listed_mask(labels, size, min_members):
    labels = np.asarray(labels, dtype=np.int64)
    n = labels.size
    inside = (labels >= 0) & (labels < n)
    return inside & (np.asarray(size, dtype=np.int64)[np.clip(labels, 0, n - 1)] >= min_members)


def member_order(labels, size, min_members):
    """(order, start, count) int32 [N]: the stable sort of the indices by (listed ? root : N), and per root slot the
    number of listed members and their exclusive prefix sum."""
    labels = np.asarray(labels, dtype=np.int64)
    n = labels.size
    key = np.where(listed_mask(labels, size, min_members), labels, n)
    order = np.argsort(key, kind="stable")
    count = np.bincount(key, minlength=n + 1)[:n]
    return order.astype(np.int32), (np.cumsum(count) - count).astype(np.int32), count.astype(np.int32)


def pair_terms(x, box_size, eps):
    """iw [M, M] int64 of all ordered pairs of the float32 positions x [M, 3], the diagonal included, and S."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    box = np.float32(box_size)
    half = np.float32(0.5) * box
    _, eps2, _, shift = shift_of(eps, box_size)
    d2 = None
    for ax in (0, 1, 2):
        d = _fold(x[None, :, ax] - x[:, None, ax], box, half)
        sq = d * d
        d2 = sq if d2 is None else d2 + sq
    w = np.float32(1) / np.sqrt(d2 + eps2)
    assert w.dtype == np.float32
    scaled = w * np.float32(2.0 ** shift)          # a power of two: exact
    assert scaled.dtype == np.float32
    return np.rint(scaled).astype(np.int64), shift


def potentials(pos, labels, size, box_size, eps, min_members=20, active=None):
    """(P int64 [N], S) as the contract defines them."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    n = labels.size
    act = np.ones(n, dtype=bool) if active is None else np.asarray(active).astype(bool)
    listed = listed_mask(labels, size, min_members)
    shift = shift_of(eps, box_size)[3]
    out = np.zeros(n, dtype=np.int64)
    for root in np.unique(labels[listed]):
        idx = np.nonzero(listed & (labels == root) & act)[0]
        if idx.size == 0:
            continue
        iw, _ = pair_terms(pos[idx], box_size, eps)
        np.fill_diagonal(iw, 0)
        out[idx] = iw.sum(axis=1)
    return out, shift


def exact_sums(pos, labels, size, box_size, eps, min_members=20):
    """sum over the other members of 1 / sqrt(r^2 + eps^2) in float64, from the float32 positions and the float32 eps
    under the exact minimum image; and the number of terms per particle."""
    pos64 = np.ascontiguousarray(pos, dtype=np.float32).astype(np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    box = float(np.float32(box_size))
    e = float(np.float32(eps))
    listed = listed_mask(labels, size, min_members)
    out, terms = np.zeros(labels.size), np.zeros(labels.size, dtype=np.int64)
    for root in np.unique(labels[listed]):
        idx = np.nonzero(listed & (labels == root))[0]
        d = pos64[idx][None, :, :] - pos64[idx][:, None, :]
        d -= box * np.round(d / box)
        w = 1.0 / np.sqrt((d * d).sum(-1) + e * e)
        np.fill_diagonal(w, 0.0)
        out[idx], terms[idx] = w.sum(1), idx.size - 1
    return out, terms


def unbind(pos, vel, labels, size, box_size, gm, eps, min_members=20, hubble=0.0, centres=None, internal_energy=None,
           iterations=3):
    """The unbinding passes in float64 on the restated integer potentials: every pass takes v_bulk and P from the
    members still active and drops those with e >= 0, all at once; a last evaluation over the members that stayed.
    ``centres``: float64 [N, 3] per root slot (with hubble).  Returns a dict per root slot (arrays [N]) and ``bound``."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    vel = np.asarray(vel, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    n = labels.size
    box = float(np.float32(box_size))
    active = listed_mask(labels, size, min_members)
    roots = np.unique(labels[active])
    dx = np.zeros((n, 3))
    if hubble != 0.0:
        d = pos.astype(np.float64) - centres[labels]
        dx = d - box * np.round(d / box)
    u = np.zeros(n) if internal_energy is None else np.asarray(internal_energy, dtype=np.float64)
    removed_last = np.zeros(n, dtype=np.int64)

    def evaluate(active):
        p, shift = potentials(pos, labels, size, box_size, eps, min_members, active)
        phi = -gm * p.astype(np.float64) * 2.0 ** -shift
        pec = np.zeros((n, 3))
        for r in roots:
            m = active & (labels == r)
            if m.any():
                pec[m] = vel[m] - vel[m].mean(axis=0)
        w = pec + hubble * dx
        return 0.5 * (w * w).sum(1) + u, phi, (pec * pec).sum(1)

    for _ in range(iterations):
        k, phi, _ = evaluate(active)
        keep = active & (k + phi < 0)
        removed_last = np.bincount(labels[active & ~keep], minlength=n)
        active = keep
    k, phi, pec2 = evaluate(active)
    res = {"bound": active, "removed_last": removed_last, "n_bound": np.bincount(labels[active], minlength=n)}
    res["kinetic"] = np.bincount(labels[active], weights=k[active], minlength=n)
    res["potential"] = 0.5 * np.bincount(labels[active], weights=phi[active], minlength=n)
    res["peculiar2"] = np.bincount(labels[active], weights=pec2[active], minlength=n)
    return res


# ---- generators ------------------------------------------------------------------------------------------------------

def _cell_centres(count, cells, box):
    g = (np.arange(cells) + 0.5) * (box / cells)
    c = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    assert count <= len(c)
    return c[:count]


def blobs(sizes, seed, cells=4, box=BOX, side=BLOB_SIDE, dyadic_bits=None, shuffle=True):
    """Compact blobs of the given sizes, blob b uniform in a cube of side ``side`` around the centre of cell b of a lattice
    of ``cells`` per axis: any two members are closer than LINKING and two blobs at least box / cells - side apart.
    ``dyadic_bits``: coordinates are whole multiples of 2^-bits.  Returns float32 pos [N, 3], labels (the smallest index
    of the blob, as fof_labels names a group) and size (at the root slot the members, elsewhere 0), the particles in a
    random order when ``shuffle``."""
    assert box / cells - side > LINKING and side * math.sqrt(3.0) < LINKING
    rng = np.random.default_rng(seed)
    centres = _cell_centres(len(sizes), cells, box)
    pts, blob = [], []
    for b, m in enumerate(sizes):
        off = (rng.random((m, 3)) - 0.5) * side
        pts.append(centres[b] + off)
        blob.append(np.full(m, b))
    x, blob = np.concatenate(pts), np.concatenate(blob)
    if dyadic_bits is not None:
        x = np.round(x * 2.0 ** dyadic_bits) / 2.0 ** dyadic_bits
    if shuffle:
        perm = rng.permutation(len(x))
        x, blob = x[perm], blob[perm]
    x = x.astype(np.float32)
    labels, size = labels_of(blob)
    return x, labels, size


def labels_of(blob):
    """labels int32 [N] (the smallest index of each blob) and size int32 [N] from blob numbers."""
    blob = np.asarray(blob)
    n = blob.size
    first = np.full(blob.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, blob, np.arange(n))
    labels = first[blob].astype(np.int32)
    return labels, np.bincount(labels, minlength=n).astype(np.int32)


def blob_with_interlopers(n_core, n_fast, seed, box=BOX):
    """One blob of n_core members in the cube of side BLOB_SIDE around the box centre and n_fast (even) interlopers on
    a sphere of radius 0.7 around it: each is within LINKING of core members, so all are one friends-of-friends group.
    Returns pos float32 [n_core + n_fast, 3] and the interlopers' mask."""
    assert n_fast % 2 == 0
    rng = np.random.default_rng(seed)
    core = box / 2 + (rng.random((n_core, 3)) - 0.5) * BLOB_SIDE
    dirs = rng.normal(size=(n_fast, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    x = np.concatenate([core, box / 2 + 0.7 * dirs]).astype(np.float32)
    fast = np.arange(len(x)) >= n_core
    return x, fast


def translated(x, shift, box=BOX):
    """(x + shift) mod box in float64, back to float32: exact for dyadic coordinates and shifts."""
    return np.mod(x.astype(np.float64) + np.asarray(shift, dtype=np.float64), box).astype(np.float32)
