"""numpy restatement of the contracts of ``cgnn_mass_assign``, ``cgnn_power_bin_ids`` and ``cgnn_power_bins``
(include/cgnn.h), for the tests, and a brute-force binning over the FULL ``np.fft.fftn`` cube that knows nothing of
Hermitian weights.

Deposit: s = fl32(fl32(M) / fl32(L)); per axis u = fl32(p s); integer weights that sum to Q = 2^13:
    NGP  j = floor(fl32(u + 0.5)):  Q on j
    CIC  i = floor(u), f = fl32(u - i), a1 = rint(f Q):  Q - a1 on i, a1 on i + 1
    TSC  j = floor(fl32(u + 0.5)), d = fl32(u - j), tm = fl32(0.5 - d), tp = fl32(0.5 + d),
         am = rint(fl32(fl32(tm tm) 0.5) Q), ap likewise:  am on j - 1, Q - am - ap on j, ap on j + 1
cells wrapped with a true modulo; a particle adds the product of its three axis weights to each of its order^3 cells.
numpy rounds every float32 ufunc once and fuses nothing, and np.rint rounds ties to even: the contract.

Binning: n2 = nx^2 + ny^2 + nz^2 of the signed integer frequencies; bin = searchsorted(e2, fl32(n2), side="right") - 1
with e2 = fl32(k_edges^2), kept when 0 <= bin < nb and n2 != 0; W2 = (sinc sinc sinc)^(2 order) in float64.
"""
import numpy as np

Q = 8192
F32 = np.float32


def _axis(u, order):
    """cells [order, N] (not yet wrapped) and integer weights [order, N] of one axis, from u float32 [N]"""
    assert u.dtype == np.float32
    if order == 1:
        j = np.floor(u + F32(0.5)).astype(np.int64)
        return np.stack([j]), np.stack([np.full(j.shape, Q, dtype=np.int64)])
    if order == 2:
        fi = np.floor(u)
        f = u - fi
        assert f.dtype == np.float32
        a1 = np.rint(f * F32(Q)).astype(np.int64)
        i = fi.astype(np.int64)
        return np.stack([i, i + 1]), np.stack([Q - a1, a1])
    if order == 3:
        fj = np.floor(u + F32(0.5))
        d = u - fj
        tm, tp = F32(0.5) - d, F32(0.5) + d
        assert tm.dtype == np.float32 and tp.dtype == np.float32
        am = np.rint((tm * tm) * F32(0.5) * F32(Q)).astype(np.int64)
        ap = np.rint((tp * tp) * F32(0.5) * F32(Q)).astype(np.int64)
        j = fj.astype(np.int64)
        return np.stack([j - 1, j, j + 1]), np.stack([am, Q - am - ap, ap])
    raise ValueError(order)


def mass_assign(pos, box_size, mesh, order):
    """int64 [M, M, M] for pos [N, 3], [T, M, M, M] for [T, N, 3]"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    if pos.ndim == 3:
        return np.stack([mass_assign(p, box_size, mesh, order) for p in pos])
    s = F32(mesh) / F32(box_size)
    assert s.dtype == np.float32
    cells, weights = zip(*(_axis(pos[:, ax] * s, order) for ax in range(3)))
    grid = np.zeros(mesh ** 3, dtype=np.int64)
    for a in range(order):
        for b in range(order):
            for c in range(order):
                at = ((cells[0][a] % mesh) * mesh + cells[1][b] % mesh) * mesh + cells[2][c] % mesh   # % of numpy: true modulo
                np.add.at(grid, at, weights[0][a] * weights[1][b] * weights[2][c])
    return grid.reshape(mesh, mesh, mesh)


def density_contrast(grid, n):
    """delta = grid (M^3 / (N Q^3)) - 1 in float64, the expression of ops.grid_contrast"""
    mesh = grid.shape[-1]
    return grid.astype(np.float64) * (mesh ** 3 / (n * Q ** 3)) - 1.0


def signed_frequencies(mesh):
    """n in (-M/2, M/2] for the indices 0 .. M - 1"""
    i = np.arange(mesh)
    return np.where(i <= mesh // 2, i, i - mesh)


def _bins_of(n2, k_edges):
    e = np.asarray(k_edges, dtype=np.float32)
    e2 = e * e
    idx = np.searchsorted(e2, n2.astype(np.float32), side="right") - 1
    return np.where((idx >= 0) & (idx < e.size - 1) & (n2 != 0), idx, -1).astype(np.int32)


def _window2(nx, ny, nz, mesh, order):
    w = np.sinc(nx / mesh) * np.sinc(ny / mesh) * np.sinc(nz / mesh)       # np.sinc(x) = sin(pi x) / (pi x)
    return w ** (2 * order) if order else np.ones_like(w)


def _half_grid(mesh):
    n = signed_frequencies(mesh)
    return np.meshgrid(n, n, np.arange(mesh // 2 + 1), indexing="ij")


def bin_ids(mesh, k_edges):
    """int32 [M, M, M/2 + 1]: the bin of every mode of the rfft array, -1 where it is not counted"""
    nx, ny, nz = _half_grid(mesh)
    return _bins_of(nx * nx + ny * ny + nz * nz, k_edges)


def _sums(a, b, ids, h, w2, n2, nb):
    keep = ids >= 0
    modes = np.bincount(ids[keep], weights=h[keep], minlength=nb)[:nb].astype(np.int64)
    sums = np.full((4, nb), np.nan)

    def re_conj(x, y):                                   # Re(x conj y), as the kernel forms it
        return x.real * y.real + x.imag * y.imag

    terms = [re_conj(a, a) / w2, None if b is None else re_conj(b, b) / w2,
             None if b is None else re_conj(a, b) / w2, np.sqrt(n2.astype(np.float64))]
    for row, t in enumerate(terms):
        if t is not None:
            sums[row] = np.bincount(ids[keep], weights=(h * t)[keep], minlength=nb)[:nb]
    return modes, sums


def power_bins(a, b, mesh, order, k_edges):
    """(modes int64 [nb], sums float64 [4, nb]) of the rfft arrays a, b [M, M, M/2 + 1] (b may be None: rows 1, 2 nan),
    with the Hermitian weights of the half array"""
    nx, ny, nz = _half_grid(mesh)
    n2 = nx * nx + ny * ny + nz * nz
    own_conjugate = (nz == 0) | ((mesh % 2 == 0) & (nz == mesh // 2))
    h = np.where(own_conjugate, 1.0, 2.0)
    return _sums(a, b, _bins_of(n2, k_edges), h, _window2(nx, ny, nz, mesh, order), n2, len(k_edges) - 1)


def power_bins_full(a_full, b_full, mesh, order, k_edges):
    """The same sums by brute force over the full fftn cubes [M, M, M]: every mode once, no Hermitian weights"""
    n = signed_frequencies(mesh)
    nx, ny, nz = np.meshgrid(n, n, n, indexing="ij")
    n2 = nx * nx + ny * ny + nz * nz
    return _sums(a_full, b_full, _bins_of(n2, k_edges), np.ones(n2.shape), _window2(nx, ny, nz, mesh, order), n2,
                 len(k_edges) - 1)


def spectra(modes, sums, n_a, n_b, box_size, mesh, subtract_shot_noise=True):
    """P, cross, r and T from the shell sums, written out from their definitions in numpy float64 (nothing of the
    package): P = L^3 S / modes / M^6; the shot noise L^3 / N leaves the auto spectra only; r from the spectra before
    the subtraction, T = sqrt(P_a / P_b) from the spectra after it (nan where that ratio is negative); an empty bin nan."""
    with np.errstate(divide="ignore", invalid="ignore"):
        count = np.where(modes > 0, modes, np.nan).astype(np.float64)
        vol = float(box_size) ** 3
        raw_a, raw_b, cross = (vol * sums[..., row, :] / count / float(mesh) ** 6 for row in (0, 1, 2))
        shot_a, shot_b = (vol / n if subtract_shot_noise else 0.0 for n in (n_a, n_b))
        return {"power": raw_a - shot_a, "power_b": raw_b - shot_b, "cross": cross,
                "r": cross / np.sqrt(raw_a * raw_b), "transfer": np.sqrt((raw_a - shot_a) / (raw_b - shot_b)),
                "k_mean": sums[..., 3, :] / count * (2.0 * np.pi / float(box_size))}


def default_k_edges(mesh):
    return 0.5 + np.arange(0, mesh // 2 + 1, dtype=np.float64)


def uniform(n, seed, box):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32) * np.float32(box)


def with_special_positions(x, box):
    """x with its first rows put on 0, on L and on mixtures of the two"""
    x = x.copy()
    box = np.float32(box)
    for row, p in enumerate([(0, 0, 0), (box, box, box), (0, box, 0), (box, 0, box)][:max(0, x.shape[0] - 1)]):
        x[row] = p
    return x
