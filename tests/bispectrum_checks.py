"""numpy restatement of the contracts of ``cgnn_bispectrum_shells`` and ``cgnn_bispectrum_sums`` (include/cgnn.h), of the
FFT estimator built on them and of the host arithmetic of ``statistics.bispectrum_from_sums``, for the tests; and a
brute force over all pairs of shell modes of the FULL ``np.fft.fftn`` cube with true closure ``k1 + k2 + k3 = 0`` (no
modulo), which knows nothing of shell fields.

Filter: the bin of every mode is the restated ``cgnn_power_bin_ids`` (tests/power_spectrum_checks.py); a mode of shell i
goes to ``out[i]`` times ``invw = (t[|nx|] t[|ny|]) t[nz]``, ``t[n] = 1 / sinc(pi n / M)^order`` -- the window's AMPLITUDE
-- and every other element is exactly 0.  ``delta_k=None``: 1 on the shell's modes.

Estimator: ``D_i = irfftn(out[i], norm="forward")`` (no 1 / M^3); ``S_ijl = sum_x D_i D_j D_l / M^3`` is the sum of
``delta_k1 delta_k2 delta_k3`` over all closed triangles with k1 in i, k2 in j, k3 in l, and with 1 for delta their number.
"""
import math

import numpy as np

import power_spectrum_checks as pc

MAX_SHELLS, MAX_TRIANGLES = 32, 5984


def window_table(mesh, order):
    """t[n] = 1 / sinc(pi n / M)^order for n in [0, M/2], float64"""
    n = np.arange(mesh // 2 + 1)
    return 1.0 / np.sinc(n / mesh) ** order if order else np.ones(n.size)


def shell_filter(delta_k, mesh, order, k_edges):
    """complex128 [nb, M, M, M/2 + 1] from delta_k [M, M, M/2 + 1] (None: ones on the shells, no window)"""
    ids = pc.bin_ids(mesh, k_edges)
    nb = len(k_edges) - 1
    if delta_k is None:
        value = np.ones(ids.shape, dtype=np.complex128)
    else:
        nx, ny, nz = pc._half_grid(mesh)
        t = window_table(mesh, order)
        value = delta_k * ((t[np.abs(nx)] * t[np.abs(ny)]) * t[nz])
    out = np.zeros((nb,) + ids.shape, dtype=np.complex128)
    for i in range(nb):
        out[i][ids == i] = value[ids == i]
    return out


def shell_fields(filtered, mesh):
    """float64 [..., M, M, M]: the inverse real transform without its 1 / M^3"""
    return np.fft.irfftn(filtered, s=(mesh, mesh, mesh), axes=(-3, -2, -1), norm="forward")


def triangles(k_edges):
    """int32 [nt, 3]: every i <= j <= l with e[l] < e[i + 1] + e[j + 1], e the float32 edges"""
    e = np.asarray(k_edges, dtype=np.float32).astype(np.float64)
    nb = e.size - 1
    rows = [(i, j, l) for i in range(nb) for j in range(i, nb) for l in range(j, nb) if e[l] < e[i + 1] + e[j + 1]]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)


def all_triples(nb):
    return np.asarray([(i, j, l) for i in range(nb) for j in range(i, nb) for l in range(j, nb)], dtype=np.int32)


def triple_terms(fields, tri):
    """float64 [nt, cells]: (D_i D_j) D_l, two single-rounded products as the kernel forms them"""
    f = np.asarray(fields, dtype=np.float64).reshape(fields.shape[0], -1)
    return (f[tri[:, 0]] * f[tri[:, 1]]) * f[tri[:, 2]]


def triple_sums(fields, tri):
    """(sums [nt], absolute sums [nt]) with math.fsum: the correctly rounded sum of the rounded terms"""
    terms = triple_terms(fields, tri)
    return (np.asarray([math.fsum(t.tolist()) for t in terms]), np.asarray([math.fsum(np.abs(t).tolist()) for t in terms]))


def summation_bound(cells, abs_sums):
    """|any-order float64 sum of single-rounded products - exact| <= (cells + 2) 2^-53 sum |terms|"""
    return (cells + 2) * 2.0 ** -53 * np.asarray(abs_sums)


def fft_estimator(delta_k, mesh, order, k_edges, tri):
    """(S [nt], N_raw [nt]): sum_x D_i D_j D_l / M^3 and the same for the fields of ones"""
    d = shell_fields(shell_filter(delta_k, mesh, order, k_edges), mesh)
    ones = shell_fields(shell_filter(None, mesh, 0, k_edges), mesh)
    return triple_sums(d, tri)[0] / mesh ** 3, triple_sums(ones, tri)[0] / mesh ** 3


def brute_force(delta_full, mesh, order, k_edges):
    """{(i, j, l): (count, sum)} for EVERY i <= j <= l, from the full fftn cube [M, M, M]: all k1 in shell i and k2 in
    shell j, k3 = -(k1 + k2) as integers; the triple counts iff k3 is a frequency of the mesh, (-M/2, M/2] per axis, and
    lies in shell l.  No modulo anywhere but in the array index of a k3 that passed."""
    n = pc.signed_frequencies(mesh)
    nx, ny, nz = np.meshgrid(n, n, n, indexing="ij")
    ids = pc._bins_of(nx * nx + ny * ny + nz * nz, k_edges)
    w = np.sinc(nx / mesh) * np.sinc(ny / mesh) * np.sinc(nz / mesh)
    value = delta_full / (w ** order if order else 1.0)
    nb = len(k_edges) - 1
    k = [np.stack([nx[ids == i], ny[ids == i], nz[ids == i]], axis=1) for i in range(nb)]
    v = [value[ids == i] for i in range(nb)]
    out = {}
    for i in range(nb):
        for j in range(i, nb):
            k3 = -(k[i][:, None, :] + k[j][None, :, :])
            inside = ((k3 > -mesh / 2) & (k3 <= mesh / 2)).all(axis=-1)
            at = tuple(k3[..., ax] % mesh for ax in range(3))
            shell = np.where(inside, ids[at], -1)
            prod = v[i][:, None] * v[j][None, :] * value[at]
            for l in range(j, nb):
                hit = shell == l
                out[(i, j, l)] = (int(hit.sum()), complex(prod[hit].sum()))
    return out


def bispectrum(counts, triangle_sums, tri, modes, sums, n, box_size, mesh, subtract_shot_noise=True):
    """The formulas of the issue, written out: triangle_sums = sum_x D D D (not yet over M^3); modes, sums [4, nb] of
    the power bins on the same edges.  Returns bispectrum, reduced_bispectrum, power, gaussian_sigma."""
    with np.errstate(divide="ignore", invalid="ignore"):
        L, M = float(box_size), float(mesh)
        shell_count = np.where(modes > 0, modes, np.nan).astype(np.float64)
        p_hat = L ** 3 * sums[..., 0, :] / shell_count / M ** 6
        nbar = n / L ** 3
        i, j, l = tri[:, 0], tri[:, 1], tri[:, 2]
        num = np.where(counts > 0, counts, np.nan).astype(np.float64)
        s = np.asarray(triangle_sums) / M ** 3
        b = L ** 6 / M ** 9 * s / num
        power = p_hat
        if subtract_shot_noise:
            b = b - (p_hat[..., i] + p_hat[..., j] + p_hat[..., l]) / nbar + 2.0 / nbar ** 2
            power = p_hat - 1.0 / nbar
        q = b / (power[..., i] * power[..., j] + power[..., j] * power[..., l] + power[..., l] * power[..., i])
        sym = np.where((i == j) & (j == l), 6.0, np.where((i == j) | (j == l), 2.0, 1.0))
        sigma = np.sqrt(sym * L ** 3 * p_hat[..., i] * p_hat[..., j] * p_hat[..., l] / num)
        return {"bispectrum": b, "reduced_bispectrum": q, "power": power, "gaussian_sigma": sigma}


def bispectrum_of_mesh(grid, n, box_size, mesh, order, k_edges, subtract_shot_noise=True):
    """The whole chain in numpy from an integer mesh of the deposit: contrast, rfftn, power bins, filter, fields, fsum
    triple sums, formulas.  Returns the dict of :func:`bispectrum` plus ``count``, ``triangles``, ``abs_sums`` (sum |D D
    D|) and ``triangle_sums``."""
    delta_k = np.fft.rfftn(pc.density_contrast(grid, n))
    modes, sums = pc.power_bins(delta_k, None, mesh, order, k_edges)
    tri = triangles(k_edges)
    d = shell_fields(shell_filter(delta_k, mesh, order, k_edges), mesh)
    ones = shell_fields(shell_filter(None, mesh, 0, k_edges), mesh)
    ts, abs_sums = triple_sums(d, tri)
    counts = np.rint(triple_sums(ones, tri)[0] / mesh ** 3).astype(np.int64)
    out = bispectrum(counts, ts, tri, modes, sums, n, box_size, mesh, subtract_shot_noise)
    out.update(count=counts, triangles=tri, abs_sums=abs_sums, triangle_sums=ts)
    return out


def gaussian_field(mesh, seed):
    """A real white Gaussian field [M, M, M] without a mean"""
    x = np.random.default_rng(seed).standard_normal((mesh, mesh, mesh))
    return x - x.mean()


def integer_fields(nb, cells, seed, frames=None):
    """Small integers in [-8, 8] as float64: every product and every sum of up to 2^40 of them is exact"""
    shape = (nb, cells) if frames is None else (frames, nb, cells)
    return np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float64)


def integer_sums(fields, tri):
    """int64 [..., nt]: the exact triple sums of integer-valued fields"""
    f = np.asarray(fields).astype(np.int64)
    parts = [(f[..., t[:, 0], :] * f[..., t[:, 1], :] * f[..., t[:, 2], :]).sum(axis=-1)
             for t in np.array_split(tri, max(1, len(tri) // 256))]
    return np.concatenate(parts, axis=-1)


def sums_layout(cells, chunk, max_parts):
    """(chunks per slice, slices) of cgnn_bispectrum_sums, from cells alone"""
    chunks = -(-cells // chunk)
    per = -(-chunks // max_parts)
    return per, -(-chunks // per)
