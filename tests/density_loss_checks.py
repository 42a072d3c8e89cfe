"""numpy restatement of the contract of ``cgnn_mass_assign_backward`` (include/cgnn.h), built on the restated deposit
(tests/power_spectrum_checks.py), and a float64 unquantised deposit for finite differences.

Per axis, u, the cells and the integer weights are the forward's (``psc._axis``); wv = weight / Q in float64.  The
derivative of the axis' weights with respect to u, (-1, +1) for CIC and (-tm, tm - tp, +tp) for TSC, is applied in
difference form along the axis:
    CIC  diff(v) = 1.0 * (v[1] - v[0])
    TSC  diff(v) = tm * (v[1] - v[0]) + tp * (v[2] - v[1])           (tm, tp the forward's float32 values, widened)
and with D[a][b][c] the mesh gradient in the particle's cells
    acc_x = sum over b (outer), c (inner) of (diff_x(D[.][b][c]) * wv_y[b]) * wv_z[c]
    acc_y = sum over a (outer), c (inner) of (diff_y(D[a][.][c]) * wv_x[a]) * wv_z[c]
    acc_z = sum over a (outer), b (inner) of (diff_z(D[a][b][.]) * wv_x[a]) * wv_y[b]
each from 0.0 in loop order; d_pos = fl32((acc * fl64(s)) * scale).  An axis the forward reads as u = 0 (NaN, |u| >=
1e9) has tm = tp = 0 (CIC: 0.0 for the 1.0).  numpy rounds every float64 ufunc once and fuses nothing: the contract.
"""
import numpy as np

import power_spectrum_checks as psc

Q = psc.Q
F32 = np.float32


def _axis_grad(p, s, order):
    """cells [order, N] (unwrapped), wv float64 [order, N], dw float64 [order - 1, N] of one axis from p float32 [N]"""
    with np.errstate(invalid="ignore", over="ignore"):
        u = p * s
        ok = np.abs(u) < F32(1.0e9)
    assert u.dtype == np.float32
    u = np.where(ok, u, F32(0.0)).astype(np.float32)
    cells, w = psc._axis(u, order)
    wv = w.astype(np.float64) * (1.0 / Q)
    if order == 2:
        dw = np.stack([np.where(ok, 1.0, 0.0)])
    else:
        d = u - np.floor(u + F32(0.5))
        tm, tp = F32(0.5) - d, F32(0.5) + d
        assert tm.dtype == np.float32 and tp.dtype == np.float32
        dw = np.stack([np.where(ok, tm.astype(np.float64), 0.0), np.where(ok, tp.astype(np.float64), 0.0)])
    return cells, wv, dw


def _diff(line, dw):
    """sum_t dw[t] (line[t + 1] - line[t]), left to right"""
    out = dw[0] * (line[1] - line[0])
    for t in range(1, len(dw)):
        out = out + dw[t] * (line[t + 1] - line[t])
    return out


def _gathered(pos, d_mesh, box_size, mesh, order):
    """-> (s, D [order, order, order, N], wv [3][order, N], dw [3][order - 1, N]) of one frame"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    d_mesh = np.ascontiguousarray(d_mesh, dtype=np.float64)
    assert order in (2, 3) and d_mesh.shape == (mesh, mesh, mesh)
    s = F32(mesh) / F32(box_size)
    assert s.dtype == np.float32
    cells, wv, dw = zip(*(_axis_grad(pos[:, ax], s, order) for ax in range(3)))
    wrapped = [c % mesh for c in cells]                               # % of numpy: true modulo
    n = pos.shape[0]
    D = np.empty((order, order, order, n))
    for a in range(order):
        for b in range(order):
            for c in range(order):
                D[a, b, c] = d_mesh[wrapped[0][a], wrapped[1][b], wrapped[2][c]]
    return s, D, wv, dw


def mass_assign_backward(pos, d_mesh, box_size, mesh, order, scale=1.0):
    """float32 [N, 3] for pos [N, 3] and d_mesh float64 [M, M, M]; [T, N, 3] for [T, N, 3] and [T, M, M, M]"""
    pos = np.asarray(pos)
    if pos.ndim == 3:
        return np.stack([mass_assign_backward(p, d, box_size, mesh, order, scale) for p, d in zip(pos, d_mesh)])
    s, D, wv, dw = _gathered(pos, d_mesh, box_size, mesh, order)
    acc = np.zeros((3, pos.shape[0]))
    for p in range(order):
        for q in range(order):
            acc[0] = acc[0] + (_diff(D[:, p, q], dw[0]) * wv[1][p]) * wv[2][q]
            acc[1] = acc[1] + (_diff(D[p, :, q], dw[1]) * wv[0][p]) * wv[2][q]
            acc[2] = acc[2] + (_diff(D[p, q, :], dw[2]) * wv[0][p]) * wv[1][q]
    with np.errstate(over="ignore"):
        return ((acc * np.float64(s)) * np.float64(scale)).astype(np.float32).T.copy()


def abs_sum_over_cells(pos, d_mesh, box_size, mesh, order):
    """float64 [N]: sum of |d_mesh| over the particle's order^3 cells (the scale of the quantisation bound)"""
    return np.abs(_gathered(pos, d_mesh, box_size, mesh, order)[1]).sum(axis=(0, 1, 2))


# ---- the unquantised assignment function in float64 -------------------------------------------------------------------

def _axis_exact(u, order):
    """cells [order, N] and float64 weights [order, N] of the unquantised CIC / TSC kernel at u float64 [N]"""
    if order == 2:
        i = np.floor(u)
        f = u - i
        i = i.astype(np.int64)
        return np.stack([i, i + 1]), np.stack([1.0 - f, f])
    j = np.floor(u + 0.5)
    d = u - j
    j = j.astype(np.int64)
    return np.stack([j - 1, j, j + 1]), np.stack([0.5 * (0.5 - d) ** 2, 0.75 - d * d, 0.5 * (0.5 + d) ** 2])


def _axis_exact_grad(u, order):
    """d weights / du, float64 [order, N]"""
    if order == 2:
        return np.stack([-np.ones_like(u), np.ones_like(u)])
    d = u - np.floor(u + 0.5)
    return np.stack([-(0.5 - d), -2.0 * d, 0.5 + d])


def contraction_unquantised(pos64, d_mesh, box_size, mesh, order):
    """float64 [N]: per particle, the sum over cells of d_mesh * (its unquantised deposit, mass in particles per cell),
    for pos64 float64 [N, 3]; the scalar whose gradient the backward states is the sum of these.  The cell scale is the
    contract's float32 s widened, so that the two sides differentiate the same function of pos"""
    s = np.float64(F32(mesh) / F32(box_size))
    cells, w = zip(*(_axis_exact(pos64[:, ax] * s, order) for ax in range(3)))
    total = np.zeros(pos64.shape[0])
    for a in range(order):
        for b in range(order):
            for c in range(order):
                total += d_mesh[cells[0][a] % mesh, cells[1][b] % mesh, cells[2][c] % mesh] * w[0][a] * w[1][b] * w[2][c]
    return total


def gradient_unquantised(pos64, d_mesh, box_size, mesh, order, scale=1.0):
    """float64 [N, 3]: the analytic gradient of ``scale * contraction_unquantised`` with respect to pos64"""
    s = np.float64(F32(mesh) / F32(box_size))
    u = [pos64[:, ax] * s for ax in range(3)]
    cells, w = zip(*(_axis_exact(x, order) for x in u))
    dw = [_axis_exact_grad(x, order) for x in u]
    out = np.zeros(pos64.shape)
    for a in range(order):
        for b in range(order):
            for c in range(order):
                d = d_mesh[cells[0][a] % mesh, cells[1][b] % mesh, cells[2][c] % mesh]
                out[:, 0] += d * dw[0][a] * w[1][b] * w[2][c]
                out[:, 1] += d * w[0][a] * dw[1][b] * w[2][c]
                out[:, 2] += d * w[0][a] * w[1][b] * dw[2][c]
    return out * s * scale


# ---- the loss in numpy float64 ----------------------------------------------------------------------------------------

def gaussian_filter(mesh, box_size, smoothing):
    """exp(-|k|^2 R^2 / 2) on the full cube [M, M, M], k = 2 pi n / L over the signed integer frequencies"""
    n = psc.signed_frequencies(mesh).astype(np.float64)
    n2 = (n * n)[:, None, None] + (n * n)[None, :, None] + (n * n)[None, None, :]
    return np.exp(-0.5 * n2 * (2.0 * np.pi * smoothing / box_size) ** 2)


def _contrast(pos, box_size, mesh, order):
    return psc.density_contrast(psc.mass_assign(pos, box_size, mesh, order), np.asarray(pos).shape[-2])


def density_field_loss(pos_pred, pos_true, box_size, mesh, order, smoothing=0.0):
    """-> (loss float64, d loss / d delta_pred float64 [(T,) M, M, M]) from the definitions, on the full FFT cube"""
    diff = _contrast(pos_pred, box_size, mesh, order) - _contrast(pos_true, box_size, mesh, order)
    if smoothing > 0:
        g = gaussian_filter(mesh, box_size, smoothing)
        axes = (-3, -2, -1)
        diff = np.fft.ifftn(np.fft.fftn(diff, axes=axes) * g, axes=axes).real
        grad = np.fft.ifftn(np.fft.fftn(2.0 * diff / diff.size, axes=axes) * g, axes=axes).real   # the filter is symmetric
    else:
        grad = 2.0 * diff / diff.size
    return np.mean(diff * diff), grad


def density_field_loss_gradient(pos_pred, pos_true, box_size, mesh, order, smoothing=0.0):
    """float32 in the shape of pos_pred: the analytic mesh gradient through the restated backward, scale = M^3 / N"""
    _, grad = density_field_loss(pos_pred, pos_true, box_size, mesh, order, smoothing)
    return mass_assign_backward(pos_pred, grad, box_size, mesh, order, scale=mesh ** 3 / np.asarray(pos_pred).shape[-2])
