"""Helpers of the Minkowski-functional tests (not collected): the numpy restatement of ``cgnn_excursion_counts``
(``include/cgnn.h``), the field families, the exact shapes on mesh 8 with their counts, and the guarded buffers of the GPU
tests."""
import numpy as np

SHAPE_MESH = 8
SHAPE_THRESHOLD = 0.5


# ---- the restatement ------------------------------------------------------------------------------------------------------
def indices(field, nu):
    """idx(v) = #{t : nu[t] <= field(v)}: a value equal to a threshold is in; NaN -> 0 (numpy sorts it past every
    threshold), -inf -> 0, +inf -> nt"""
    nu = np.asarray(nu, dtype=np.float64)
    field = np.asarray(field, dtype=np.float64)
    idx = np.searchsorted(nu, field, side="right").astype(np.int64)
    idx[np.isnan(field)] = 0
    return idx


def element_indices(idx):
    """The indices of the elements of the cubical complex of idx [M, M, M], by dimension: vertices [M^3], edges [3 M^3],
    faces [3 M^3], cubes [M^3].  An element belongs to the lower corner of its voxel and takes the largest index among the
    voxels at offsets {0, -1} along the axes it does not extend in; np.roll(., 1, axis) is the neighbour at -1, modulo M."""
    def low(a, axis):
        return np.maximum(a, np.roll(a, 1, axis=axis))

    faces = [low(idx, a) for a in range(3)]                                             # normal to a
    edges = [low(low(idx, (a + 1) % 3), (a + 2) % 3) for a in range(3)]                 # along a
    vertices = low(low(low(idx, 0), 1), 2)
    return [vertices.ravel(), np.concatenate([e.ravel() for e in edges]), np.concatenate([f.ravel() for f in faces]),
            idx.ravel()]


def excursion_counts(field, nu):
    """counts [4, nt] int64 of a field [M, M, M] (or [F, 4, nt] of [F, M, M, M]): counts[d, t] = the number of elements of
    dimension d with an index above t"""
    field = np.asarray(field, dtype=np.float64)
    if field.ndim == 4:
        return np.stack([excursion_counts(f, nu) for f in field])
    nt = len(nu)
    out = np.zeros((4, nt), dtype=np.int64)
    for d, e in enumerate(element_indices(indices(field, nu))):
        hist = np.bincount(e, minlength=nt + 1).astype(np.int64)
        out[d] = np.cumsum(hist[:0:-1])[::-1]                  # suffix sums of hist[1 .. nt]
    return out


def from_counts(counts, mesh, box_size):
    """v0 .. v3 and the Euler characteristic of statistics.minkowski_from_counts, in float64 numpy"""
    c = np.asarray(counts, dtype=np.int64)
    n0, n1, n2, n3 = (c[..., d, :] for d in range(4))
    a, cells = float(box_size) / mesh, float(mesh) ** 3
    euler = n0 - n1 + n2 - n3
    return {"v0": n3 / cells, "v1": 2.0 * (n2 - 3 * n3) / (9.0 * a * cells),
            "v2": 2.0 * (n1 - 2 * n2 + 3 * n3) / (9.0 * a * a * cells), "v3": euler / (a ** 3 * cells), "euler": euler}


# ---- thresholds and fields ----------------------------------------------------------------------------------------------
def thresholds(nt):
    """nt = 1: the shapes' 0.5; 2: 0 and 1; else nt equal steps from -3 to 3 (25: steps of exactly 1/4, so that the small
    integers of integer_field sit on thresholds)"""
    if nt == 1:
        return np.array([SHAPE_THRESHOLD])
    if nt == 2:
        return np.array([0.0, 1.0])
    return np.linspace(-3.0, 3.0, nt)


def integer_field(mesh, seed):
    """small random integers -4 .. 4: most values sit exactly on a threshold of thresholds(25), some lie outside all"""
    return np.random.default_rng(seed).integers(-4, 5, size=(mesh,) * 3).astype(np.float64)


def smooth_field(mesh, seed):
    """a few long waves of unit variance or so: long runs of equal index along z"""
    rng = np.random.default_rng(seed)
    x = np.arange(mesh) / mesh
    out = np.zeros((mesh,) * 3)
    for _ in range(4):
        k = rng.integers(-2, 3, size=3)
        phase = rng.uniform(0, 2 * np.pi)
        out += rng.uniform(0.5, 1.0) * np.cos(2 * np.pi * (k[0] * x[:, None, None] + k[1] * x[None, :, None] +
                                                           k[2] * x[None, None, :]) + phase)
    return out


def white_field(mesh, seed):
    return np.random.default_rng(seed).standard_normal((mesh,) * 3)


def checkerboard(mesh):
    i = np.arange(mesh)
    return ((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2).astype(np.float64)


def constant_field(mesh, value):
    return np.full((mesh,) * 3, float(value))


def planted(field, tile=(8, 8, 64)):
    """field with NaN, +inf and -inf at (0, 0, 0), (M-1, M-1, M-1) and in the middle of the first tile"""
    out = np.array(field, dtype=np.float64)
    m = out.shape[0]
    mid = tuple(min(t, m) // 2 for t in tile)
    for n, v in enumerate((np.nan, np.inf, -np.inf)):
        for p in ((0, 0, 0), (m - 1,) * 3, mid):
            out[(p[0] + n) % m, p[1], (p[2] + 2 * n) % m] = v
    return out


def smoothed_white_noise(mesh, cells, seed):
    """White noise smoothed with a Gaussian of `cells` cells (box 1), divided by its standard deviation ->
    (field, sigma0 = 1, sigma1 of the normalised field from its spectrum with the Hermitian weights)"""
    w = np.random.default_rng(seed).standard_normal((mesh,) * 3)
    n = np.fft.fftfreq(mesh, 1.0 / mesh)
    nz = np.fft.rfftfreq(mesh, 1.0 / mesh)
    k2 = (2 * np.pi) ** 2 * (n[:, None, None] ** 2 + n[None, :, None] ** 2 + nz[None, None, :] ** 2)
    modes = np.fft.rfftn(w) * np.exp(-0.5 * k2 * (cells / mesh) ** 2)
    u = np.fft.irfftn(modes, s=(mesh,) * 3, axes=(0, 1, 2))
    s0 = np.sqrt((u * u).mean())
    herm = np.full(mesh // 2 + 1, 2.0)
    herm[0] = 1.0
    if mesh % 2 == 0:
        herm[-1] = 1.0
    s1 = np.sqrt((k2 * herm * np.abs(modes) ** 2).sum()) / mesh ** 3
    return u / s0, 1.0, s1 / s0


# ---- the exact shapes: 0/1 fields on mesh 8 at threshold 0.5 -> (n0, n1, n2, n3), Euler characteristic ------------------------
def _shape(*slices):
    f = np.zeros((SHAPE_MESH,) * 3)
    for s in slices:
        f[s] = 1.0
    return f


def shapes():
    hollow = _shape(np.s_[2:5, 2:5, 2:5])
    hollow[3, 3, 3] = 0.0
    ring = _shape(np.s_[2:5, 2:5, 4])
    ring[3, 3, 4] = 0.0
    return {
        "one voxel": (_shape(np.s_[2, 3, 4]), (8, 12, 6, 1), 1),
        "two face neighbours": (_shape(np.s_[2, 3, 4], np.s_[3, 3, 4]), (12, 20, 11, 2), 1),
        "two voxels touching at a corner": (_shape(np.s_[2, 3, 4], np.s_[3, 4, 5]), (15, 24, 12, 2), 1),
        "a tube wrapping the box": (_shape(np.s_[:, 3, 4]), (32, 64, 40, 8), 0),
        "a slab wrapping two axes": (_shape(np.s_[:, :, 4]), (128, 320, 256, 64), 0),
        "a 3x3x3 block without its centre": (hollow, (64, 144, 108, 26), 2),
        "a flat 3x3 ring": (ring, (32, 64, 40, 8), 0),
        "the full box": (np.ones((SHAPE_MESH,) * 3), (512, 1536, 1536, 512), 0),
    }


# translations that carry a shape at 2 .. 4 across the box face of each axis, and of all three at once
SHIFTS = ((5, 0, 0), (0, 5, 0), (0, 0, 5), (6, 5, 4), (-3, 0, 0), (0, -3, -3))


def translated(field, shift):
    return np.roll(field, shift, axis=(0, 1, 2))


# ---- guarded device buffers ---------------------------------------------------------------------------------------------
PAD = 4096                                      # guard values on either side of a buffer
CANARY = -0x5A5A5A5A5A5A5A5A                    # in the int64 counts and around them before the call


def guarded(x, fill, device):
    """x on the device with PAD guard values before and behind it in one allocation -> (view, whole buffer)"""
    import torch
    x = torch.as_tensor(x)
    buf = torch.full((x.numel() + 2 * PAD,), fill, dtype=x.dtype, device=device)
    view = buf[PAD:PAD + x.numel()].view(x.shape)
    view.copy_(x)
    return view, buf


def guards_intact(buf, fill):
    import torch
    ends = torch.cat([buf[:PAD], buf[-PAD:]])
    return bool(torch.isnan(ends).all()) if fill != fill else bool((ends == fill).all())
