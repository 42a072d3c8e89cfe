"""numpy restatement of the contracts of ``cgnn_redshift_positions`` and ``cgnn_power_multipoles`` (include/cgnn.h) and of
``ops.interlace_shift``, for the tests, a brute-force sum over the FULL ``np.fft.fftn`` cube that knows nothing of
Hermitian weights, and the multipoles written out from their definitions.

Redshift positions, L = fl32(box), p and q the line-of-sight coordinates of pos and pos_prev, float32 throughout:
    d = p - q;  d = d - L rint(d / L);  s = p + shift d;  s = s - L floor(s / L)
    s < 0: 0;  else s >= L: s - L;  then anything outside [0, L] (nan): 0
numpy rounds every float32 ufunc once and fuses nothing, np.rint rounds ties to even: the contract.

Shell sums: the bins, h and W2 of power_spectrum_checks; mu2 = n_los^2 / n2, L2 = 1.5 mu2 - 0.5, L4 = (4.375 mu2 - 3.75)
mu2 + 0.375; with a second transform a2 of the particles displaced by half a cell, x = (a + a2 e^{i pi (nx+ny+nz)/M}) / 2
over the signed frequencies (an index of M/2 read as +M/2)."""
import numpy as np

import power_spectrum_checks as psc

F32 = np.float32
ROWS = 12


def redshift_positions(pos, pos_prev, box_size, los, shift):
    """pos with its `los` coordinate displaced; float32, bit for bit the kernel's sequence.  shift: any float, rounded to
    float32 once (the caller's fl32(velocity_scale / dt))."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    prev = np.ascontiguousarray(pos_prev, dtype=np.float32)
    box, shift = F32(box_size), F32(shift)
    p, q = pos[..., los], prev[..., los]
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - q
        d = d - box * np.rint(d / box)
        s = p + shift * d
        s = s - box * np.floor(s / box)
        assert s.dtype == np.float32
        s = np.where(s < 0, F32(0), np.where(s >= box, s - box, s))
        s = np.where((s >= 0) & (s <= box), s, F32(0)).astype(np.float32)
    out = pos.copy()
    out[..., los] = s
    return out


def redshift_shift(dt, velocity_scale):
    return F32(float(velocity_scale) / float(dt))


def interlace_shift(pos, box_size, mesh):
    """p + fl32(L / (2 M)) wrapped into [0, L), float32"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = F32(box_size)
    half = F32(float(box) / (2 * mesh))
    s = pos + half
    assert s.dtype == np.float32
    return np.where(s >= box, s - box, s).astype(np.float32)


def legendre(mu2):
    return 1.5 * mu2 - 0.5, (4.375 * mu2 - 3.75) * mu2 + 0.375


def _sums(x, y, ids, h, w2, n, los, nb):
    n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        mu2 = np.where(n2 != 0, (n[los] * n[los]).astype(np.float64) / n2.astype(np.float64), 0.0)
    l2, l4 = legendre(mu2)
    keep = ids >= 0
    modes = np.bincount(ids[keep], weights=h[keep], minlength=nb)[:nb].astype(np.int64)
    sums = np.full((ROWS, nb), np.nan)

    def re_conj(u, v):
        return u.real * v.real + u.imag * v.imag

    def put(row, t):
        sums[row] = np.bincount(ids[keep], weights=t[keep], minlength=nb)[:nb]

    sets = [(0, x, x)] if y is None else [(0, x, x), (3, y, y), (6, x, y)]
    for row, u, v in sets:
        p = h * re_conj(u, v) / w2
        for i, leg in enumerate((np.ones_like(l2), l2, l4)):
            put(row + i, p * leg)
    put(9, h * np.sqrt(n2.astype(np.float64)))
    put(10, h * l2)
    put(11, h * l4)
    return modes, sums


def _combine(a, a2, n, mesh):
    if a2 is None:
        return a
    return 0.5 * (a + a2 * np.exp(1j * np.pi * (n[0] + n[1] + n[2]) / mesh))


def power_multipoles(a, b, mesh, order, los, k_edges, a2=None, b2=None):
    """(modes int64 [nb], sums float64 [12, nb]) of the rfft arrays [M, M, M/2 + 1]; b None: rows 3-8 nan"""
    n = psc._half_grid(mesh)
    n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
    own_conjugate = (n[2] == 0) | ((mesh % 2 == 0) & (n[2] == mesh // 2))
    h = np.where(own_conjugate, 1.0, 2.0)
    x = _combine(a, a2, n, mesh)
    y = None if b is None else _combine(b, b2, n, mesh)
    return _sums(x, y, psc._bins_of(n2, k_edges), h, psc._window2(*n, mesh, order), n, los, len(k_edges) - 1)


def power_multipoles_full(a_full, b_full, mesh, order, los, k_edges, a2_full=None, b2_full=None):
    """The same sums by brute force over the full fftn cubes [M, M, M]: every mode once, no Hermitian weights"""
    f = psc.signed_frequencies(mesh)
    n = np.meshgrid(f, f, f, indexing="ij")
    n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
    x = _combine(a_full, a2_full, n, mesh)
    y = None if b_full is None else _combine(b_full, b2_full, n, mesh)
    return _sums(x, y, psc._bins_of(n2, k_edges), np.ones(n2.shape), psc._window2(*n, mesh, order), n, los,
                 len(k_edges) - 1)


def multipoles(modes, sums, n_a, n_b, box_size, mesh, subtract_shot_noise=True):
    """P_l = (2 l + 1) L^3 S_l / modes / M^6 written out in numpy float64 (nothing of the package); the shot noise L^3 / N
    leaves l = 0 of the auto spectra only; an empty bin nan"""
    with np.errstate(divide="ignore", invalid="ignore"):
        count = np.where(modes > 0, modes, np.nan).astype(np.float64)
        vol = float(box_size) ** 3
        out = {"legendre_mean_2": sums[..., 10, :] / count, "legendre_mean_4": sums[..., 11, :] / count,
               "k_mean": sums[..., 9, :] / count * (2.0 * np.pi / float(box_size))}
        for name, row, n in (("power_", 0, n_a), ("power_b_", 3, n_b), ("cross_", 6, None)):
            for i, ell in enumerate((0, 2, 4)):
                p = (2 * ell + 1) * vol * sums[..., row + i, :] / count / float(mesh) ** 6
                if ell == 0 and n is not None and subtract_shot_noise:
                    p = p - vol / n
                out[f"{name}{ell}"] = p
        raw = [vol * sums[..., row, :] / count / float(mesh) ** 6 for row in (0, 3, 6)]
        out["r"] = raw[2] / np.sqrt(raw[0] * raw[1])
        out["transfer"] = np.sqrt(out["power_0"] / out["power_b_0"])
        return out


def contrast_modes(pos, box_size, mesh, order):
    """rfftn of the density contrast of pos [N, 3]"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    return np.fft.rfftn(psc.density_contrast(psc.mass_assign(pos, box_size, mesh, order), pos.shape[0]))


def frame_sums(pos, box_size, mesh, order, los, k_edges, pos_b=None, interlace=True):
    """(modes, sums) of one frame (and a second set), deposit to shell sums"""
    def pair(p):
        if p is None:
            return None, None
        return contrast_modes(p, box_size, mesh, order), \
            contrast_modes(interlace_shift(p, box_size, mesh), box_size, mesh, order) if interlace else None
    a, a2 = pair(pos)
    b, b2 = pair(pos_b)
    return power_multipoles(a, b, mesh, order, los, k_edges, a2, b2)


def white_noise(n, seed, box):
    """n uniform points: default_rng(seed).random((n, 3)) in float64, times the box, rounded to float32 once (and a
    value that rounds up to the box put on 0)"""
    x = (np.random.default_rng(seed).random((n, 3)) * box).astype(np.float32)
    return np.where(x >= np.float32(box), np.float32(0), x)


def real_field_modes(mesh, seed, full=False):
    """the transform of a random real field: a Hermitian array, so the half array and the full cube agree"""
    field = np.random.default_rng(seed).standard_normal((mesh, mesh, mesh))
    return np.fft.fftn(field) if full else np.fft.rfftn(field)


def trajectory(n, frames, seed, box):
    """a synthetic trajectory [frames, n, 3] in [0, box): uniform points drifting with per-particle velocities, with the
    first rows of frame 1 put on 0 and on the box faces"""
    rng = np.random.default_rng(seed)
    x0 = rng.random((n, 3)) * box
    v = rng.standard_normal((n, 3)) * (0.01 * box)
    out = np.stack([np.mod(x0 + t * v + 0.002 * box * np.sin(t + x0), box) for t in range(frames)]).astype(np.float32)
    out = np.where(out >= np.float32(box), np.float32(0), out)
    return out
