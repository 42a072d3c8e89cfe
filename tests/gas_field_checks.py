"""numpy restatement of the contracts of ``cgnn_mass_assign_weighted`` and ``cgnn_mass_assign_weighted_backward``
(include/cgnn.h), built on the restated deposit (tests/power_spectrum_checks.py) and its restated transpose
(tests/density_loss_checks.py), and the float64 definitions of what stands on them: the unquantised weighted deposit for
finite differences and bounds, ``ops.weighted_field``, ``losses.thermal_field_loss`` and the shot noise of a weighted field.

Deposit: u (with the guard: NaN or |u| >= 1e9 reads as 0), the cells and the integer axis weights are the plain
deposit's (``psc._axis``); with v the product of the three axis weights of a cell and qc = clip(q, -2^20, 2^20),
channel c receives (v qc + 2^19) >> 20 in int64 (numpy's >> on int64 is arithmetic).

Transpose: per channel, D, wv, dw of ``dlc._gathered``;
    val = sum over a (outer), b, c (inner) of ((wv_x[a] wv_y[b]) wv_z[c]) D[a][b][c],  d_val = fl32(val scale_val)
    g = the acc of ``dlc.mass_assign_backward``;  chan += a_c g over the channels in ascending order, a_c = qc 2^-20
    d_pos = fl32((chan fl64(s)) scale_pos)
numpy rounds every float64 ufunc once and fuses nothing: the contract.
"""
import numpy as np

import density_loss_checks as dlc
import power_spectrum_checks as psc

Q = psc.Q
F32 = np.float32
BITS = 20
ONE = 1 << BITS


def quantize(values, scale):
    """int64 in the shape of values: rint(clip(float64(values) / scale, -1, 1) 2^20), ties to even"""
    a = np.clip(np.asarray(values).astype(np.float64) / np.float64(scale), -1.0, 1.0)
    return np.rint(a * float(ONE)).astype(np.int64)


def _guarded_axis(p, s, order):
    with np.errstate(invalid="ignore", over="ignore"):
        u = p * s
        ok = np.abs(u) < F32(1.0e9)
    assert u.dtype == np.float32
    return psc._axis(np.where(ok, u, F32(0.0)).astype(np.float32), order)


def mass_assign_weighted(pos, q, box_size, mesh, order):
    """int64 [C, M, M, M] for pos [N, 3] and q [N, C] (or [N]: C = 1); [T, C, M, M, M] for [T, N, 3] and [T, N(, C)]"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    q = np.asarray(q)
    if q.ndim == pos.ndim - 1:
        q = q[..., None]
    if pos.ndim == 3:
        return np.stack([mass_assign_weighted(p, w, box_size, mesh, order) for p, w in zip(pos, q)])
    qc = np.clip(q.astype(np.int64), -ONE, ONE)
    s = F32(mesh) / F32(box_size)
    assert s.dtype == np.float32
    cells, weights = zip(*(_guarded_axis(pos[:, ax], s, order) for ax in range(3)))
    grid = np.zeros((qc.shape[1], mesh ** 3), dtype=np.int64)
    for a in range(order):
        for b in range(order):
            for c in range(order):
                at = ((cells[0][a] % mesh) * mesh + cells[1][b] % mesh) * mesh + cells[2][c] % mesh
                v = weights[0][a] * weights[1][b] * weights[2][c]
                for ch in range(qc.shape[1]):
                    np.add.at(grid[ch], at, (v * qc[:, ch] + (1 << (BITS - 1))) >> BITS)
    return grid.reshape(-1, mesh, mesh, mesh)


def mass_assign_weighted_backward(pos, q, d_field, box_size, mesh, order, scale_pos=1.0, scale_val=1.0):
    """-> (d_pos float32 [N, 3], d_val float32 [N, C]) for pos [N, 3], q [N, C] and d_field float64 [C, M, M, M]; with a
    leading T on all three, per frame"""
    pos = np.asarray(pos)
    q = np.asarray(q)
    if q.ndim == pos.ndim - 1:
        q = q[..., None]
    if pos.ndim == 3:
        parts = [mass_assign_weighted_backward(p, w, d, box_size, mesh, order, scale_pos, scale_val)
                 for p, w, d in zip(pos, q, d_field)]
        return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    qc = np.clip(q.astype(np.int64), -ONE, ONE)
    n, channels = qc.shape
    chan = np.zeros((3, n))
    d_val = np.empty((n, channels), dtype=np.float32)
    for ch in range(channels):
        s, D, wv, dw = dlc._gathered(pos, d_field[ch], box_size, mesh, order)
        val = np.zeros(n)
        for a in range(order):
            for b in range(order):
                for c in range(order):
                    val = val + ((wv[0][a] * wv[1][b]) * wv[2][c]) * D[a, b, c]
        with np.errstate(over="ignore"):
            d_val[:, ch] = (val * np.float64(scale_val)).astype(np.float32)
        acc = np.zeros((3, n))
        for p in range(order):
            for r in range(order):
                acc[0] = acc[0] + (dlc._diff(D[:, p, r], dw[0]) * wv[1][p]) * wv[2][r]
                acc[1] = acc[1] + (dlc._diff(D[p, :, r], dw[1]) * wv[0][p]) * wv[2][r]
                acc[2] = acc[2] + (dlc._diff(D[p, r, :], dw[2]) * wv[0][p]) * wv[1][r]
        a_ch = qc[:, ch].astype(np.float64) * (1.0 / ONE)
        chan = chan + a_ch * acc
    with np.errstate(over="ignore"):
        d_pos = ((chan * np.float64(s)) * np.float64(scale_pos)).astype(np.float32).T.copy()
    return d_pos, d_val


def weighted_field(grid, n, scale):
    """float64: grid (scale (M^3 / (N Q^3))), the expression of ``ops.weighted_field``"""
    mesh = grid.shape[-1]
    return grid.astype(np.float64) * (np.float64(scale) * (mesh ** 3 / (n * Q ** 3)))


# ---- the unquantised weighted deposit in float64 ----------------------------------------------------------------------

def field_unquantised(pos64, values, box_size, mesh, order):
    """float64 [C, M, M, M]: A_c[cell] = sum_i W_i(cell) values[i, c] with the unquantised CIC / TSC weights (mass in
    particles per cell), for pos64 float64 [N, 3] and values float64 [N, C]; the cell scale is the contract's float32 s"""
    s = np.float64(F32(mesh) / F32(box_size))
    cells, w = zip(*(dlc._axis_exact(pos64[:, ax] * s, order) for ax in range(3)))
    out = np.zeros((values.shape[1], mesh ** 3))
    for a in range(order):
        for b in range(order):
            for c in range(order):
                at = ((cells[0][a] % mesh) * mesh + cells[1][b] % mesh) * mesh + cells[2][c] % mesh
                for ch in range(values.shape[1]):
                    np.add.at(out[ch], at, w[0][a] * w[1][b] * w[2][c] * values[:, ch])
    return out.reshape(-1, mesh, mesh, mesh)


def contraction_unquantised(pos64, values, d_field, box_size, mesh, order):
    """the scalar sum_c sum_cells d_field_c A_c whose gradients the transpose states"""
    return float((d_field * field_unquantised(pos64, values, box_size, mesh, order)).sum())


def gradients_unquantised(pos64, values, d_field, box_size, mesh, order):
    """-> (d / d pos64 float64 [N, 3], d / d values float64 [N, C]) of :func:`contraction_unquantised`, analytically: the
    gradient in pos is the sum over the channels of values_c times ``dlc.gradient_unquantised`` on d_field_c, the one in
    values the per-particle contraction ``dlc.contraction_unquantised`` on d_field_c"""
    d_pos = np.zeros(pos64.shape)
    d_val = np.empty(values.shape)
    for ch in range(values.shape[1]):
        d_pos += values[:, ch:ch + 1] * dlc.gradient_unquantised(pos64, d_field[ch], box_size, mesh, order)
        d_val[:, ch] = dlc.contraction_unquantised(pos64, d_field[ch], box_size, mesh, order)
    return d_pos, d_val


def touch_count(pos, box_size, mesh, order):
    """int64 [M, M, M]: an upper count of the particles whose deposit can differ in a cell between the integer and the
    unquantised form: every cell of the integer stencil plus every cell of the float64 stencil (the two differ only
    where fl32(p s) and the float64 product fall on different sides of a cell boundary)"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    s = F32(mesh) / F32(box_size)
    grid = np.zeros(mesh ** 3, dtype=np.int64)
    quantised = [_guarded_axis(pos[:, ax], s, order)[0] for ax in range(3)]
    exact = [dlc._axis_exact(pos[:, ax].astype(np.float64) * np.float64(s), order)[0] for ax in range(3)]
    for cells in (quantised, exact):
        for a in range(order):
            for b in range(order):
                for c in range(order):
                    np.add.at(grid, ((cells[0][a] % mesh) * mesh + cells[1][b] % mesh) * mesh + cells[2][c] % mesh, 1)
    return grid.reshape(mesh, mesh, mesh)


# ---- the thermal loss in numpy float64 --------------------------------------------------------------------------------

def thermal_scale(temp_true):
    """2 max|temp_true| as ``losses.thermal_field_loss`` forms it: the float32 maximum widened, times 2.0"""
    return 2.0 * np.float64(np.abs(np.asarray(temp_true, dtype=np.float32)).max())


def _thermal_field(pos, temp, scale, box_size, mesh, order):
    temp = np.asarray(temp, dtype=np.float32).reshape(np.asarray(pos).shape[:-1])
    grid = mass_assign_weighted(pos, quantize(temp, scale), box_size, mesh, order)
    return weighted_field(grid, np.asarray(pos).shape[-2], scale)


def thermal_field_loss(pos_pred, temp_pred, pos_true, temp_true, box_size, mesh, order, smoothing=0.0):
    """-> (loss float64, d loss / d F_pred float64 [(T,) 1, M, M, M]) from the definitions, on the full FFT cube"""
    scale = thermal_scale(temp_true)
    diff = (_thermal_field(pos_pred, temp_pred, scale, box_size, mesh, order)
            - _thermal_field(pos_true, temp_true, scale, box_size, mesh, order))
    norm = np.asarray(temp_true, dtype=np.float32).astype(np.float64).mean() ** 2
    if smoothing > 0:
        g = dlc.gaussian_filter(mesh, box_size, smoothing)
        axes = (-3, -2, -1)
        diff = np.fft.ifftn(np.fft.fftn(diff, axes=axes) * g, axes=axes).real
        grad = np.fft.ifftn(np.fft.fftn(2.0 * diff / diff.size, axes=axes) * g, axes=axes).real
    else:
        grad = 2.0 * diff / diff.size
    return np.mean(diff * diff) / norm, grad / norm


def thermal_field_loss_gradients(pos_pred, temp_pred, pos_true, temp_true, box_size, mesh, order, smoothing=0.0):
    """-> (d / d pos_pred float32, d / d temp_pred float32 [(T,) N, 1]): the analytic mesh gradient through the restated
    transpose with the field's scales, scale_pos = value_scale M^3 / N and scale_val = M^3 / N"""
    _, grad = thermal_field_loss(pos_pred, temp_pred, pos_true, temp_true, box_size, mesh, order, smoothing)
    scale = thermal_scale(temp_true)
    n = np.asarray(pos_pred).shape[-2]
    temp = np.asarray(temp_pred, dtype=np.float32).reshape(np.asarray(pos_pred).shape[:-1])
    return mass_assign_weighted_backward(pos_pred, quantize(temp, scale), grad, box_size, mesh, order,
                                         scale_pos=scale * (mesh ** 3 / n), scale_val=mesh ** 3 / n)


# ---- shot noise of a weighted field -----------------------------------------------------------------------------------

def shot_noise(values, box_size, normalise):
    """"mean": L^3 sum a^2 / (sum a)^2;  "none": L^3 sum a^2 / N^2 (float64, per frame over the last axis)"""
    a = np.asarray(values, dtype=np.float64)
    s2 = (a * a).sum(axis=-1)
    return float(box_size) ** 3 * s2 / (a.sum(axis=-1) ** 2 if normalise == "mean" else a.shape[-1] ** 2)
