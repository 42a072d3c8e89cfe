"""Loss terms of the reference's training loop that sit on the hot path."""
from __future__ import annotations

import math

import torch

from . import ops


class _SegmentColsum(torch.autograd.Function):
    """``sums[g] = sum_{n in graph g} acc[n]`` in float64 (``cgnn_segment_colsum``); the backward broadcasts each
    graph's gradient row back to its particles."""

    @staticmethod
    def forward(ctx, acc, batch, num_graphs):
        ctx.batch, ctx.n = batch, acc.shape[0]
        return ops.segment_colsum(acc, batch, num_graphs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_sums):
        d = d_sums.to(torch.float32)
        if ctx.batch is None:
            return d[0].expand(ctx.n, -1).contiguous(), None, None
        return d[ctx.batch.long()], None, None


def momentum_conservation_loss(accelerations: torch.Tensor, batch_graph, dt: float, momentum_weight: float):
    """``w / B * sum_g || sum_{n in g} acc[n] * dt ||^2`` (reference train.py:107-118,
    duplicated at validation.py:5-16).  The per-graph column sums run in one
    segmented float64 reduction on the device instead of a Python loop over
    boolean masks.  Returns a 0-d float32 tensor on the accelerations' device; differentiable with respect to
    ``accelerations``."""
    num_graphs = int(getattr(batch_graph, "num_graphs", 1) or 1)
    batch = getattr(batch_graph, "batch", None)
    sums = _SegmentColsum.apply(accelerations, batch, num_graphs)                 # [B, 3] float64
    total = torch.sum((sums * float(dt)) ** 2)
    return (momentum_weight * total / num_graphs).to(torch.float32)


def check_density_loss(who: str, mesh, order, smoothing) -> int:
    """The checks of :func:`density_field_loss` that need no device (``ValueError``) -> ``mesh`` as an int."""
    mesh = ops.check_mesh(mesh, who)
    if isinstance(order, bool) or order not in (2, 3):
        raise ValueError(f"{who}: order must be 2 (CIC) or 3 (TSC), got {order!r} (NGP has no gradient)")
    if isinstance(smoothing, bool) or not math.isfinite(smoothing) or smoothing < 0:
        raise ValueError(f"{who}: smoothing must be a finite length >= 0, got {smoothing!r}")
    return mesh


def gaussian_filter(mesh: int, box_size: float, smoothing: float, device) -> torch.Tensor:
    """``exp(-|k|^2 R^2 / 2)`` on the modes of ``torch.fft.rfftn`` of a ``mesh^3`` grid (float64 ``[M, M, M/2 + 1]``),
    ``k = 2 pi n / box_size`` over the signed integer frequencies ``n``."""
    n = torch.fft.fftfreq(mesh, 1.0 / mesh, dtype=torch.float64, device=device)
    nz = torch.fft.rfftfreq(mesh, 1.0 / mesh, dtype=torch.float64, device=device)
    n2 = (n * n)[:, None, None] + (n * n)[None, :, None] + (nz * nz)[None, None, :]
    return torch.exp(n2 * (-0.5 * (2.0 * math.pi * float(smoothing) / float(box_size)) ** 2))


def _mean_square(diff: torch.Tensor, kernel) -> torch.Tensor:
    """``mean(diff^2)`` of a real field ``[..., M, M, M]``, filtered first by ``kernel`` (``[M, M, M/2 + 1]`` on the modes
    of its real FFT) unless that is ``None``."""
    if kernel is not None:
        diff = torch.fft.irfftn(torch.fft.rfftn(diff, dim=(-3, -2, -1)) * kernel, s=diff.shape[-3:], dim=(-3, -2, -1))
    return (diff * diff).mean()


def density_field_loss(pos_pred: torch.Tensor, pos_true: torch.Tensor, box_size: float, mesh: int, order: int = 2,
                       smoothing: float = 0.0) -> torch.Tensor:
    """The field-level loss of a predicted frame: ``mean((delta_pred - delta_true)^2)`` over the ``mesh^3`` cells, the two
    density contrasts from ``ops.density_contrast`` (exact integer CIC / TSC deposits, ``order`` 2 / 3).  0-d float64,
    differentiable in ``pos_pred`` (``cgnn_mass_assign_backward``); ``pos_true`` is deposited without autograd.
    ``[N, 3]``, or ``[T, N, 3]`` for the mean over T frames as well.

    ``smoothing = R > 0`` (a length in the units of ``box_size``) first filters the difference with the Gaussian
    ``exp(-|k|^2 R^2 / 2)`` in Fourier space (``torch.fft.rfftn`` / ``irfftn`` in float64, whose own autograd carries
    that part of the gradient): scales below ``R``, where the trajectories of a rollout have long diverged, stop
    counting.  ``smoothing=0`` takes no FFT.

    ``ValueError`` before any device work: ``smoothing`` negative or not finite, ``order`` 1 (NGP has no gradient),
    ``mesh`` outside ``ops.check_mesh``.  One box, one GPU."""
    who = "density_field_loss"
    mesh = check_density_loss(who, mesh, order, smoothing)
    if pos_pred.shape != pos_true.shape:
        raise ValueError(f"{who}: pos_pred {tuple(pos_pred.shape)} and pos_true {tuple(pos_true.shape)} differ in shape")
    delta_pred = ops.density_contrast(pos_pred, box_size, mesh, order)
    with torch.no_grad():
        delta_true = ops.density_contrast(pos_true, box_size, mesh, order)
    kernel = gaussian_filter(mesh, box_size, smoothing, delta_pred.device) if smoothing > 0 else None
    return _mean_square(delta_pred - delta_true, kernel)


def thermal_field_loss(pos_pred: torch.Tensor, temp_pred: torch.Tensor, pos_true: torch.Tensor, temp_true: torch.Tensor,
                       box_size: float, mesh: int, order: int = 2, smoothing: float = 0.0) -> torch.Tensor:
    """The field-level loss of a predicted frame's internal energy: ``mean((F_pred - F_true)^2) / mean(temp_true)^2`` over
    the ``mesh^3`` cells, ``F = ops.weighted_field(pos, temp)`` the internal-energy-weighted field (exact integer CIC /
    TSC deposits of the quantised temperatures, ``order`` 2 / 3; its mean over the cells is the mean temperature).  Both
    deposits share ``value_scale = 2 max|temp_true|`` (a detached 0-d device tensor: a prediction up to twice the
    largest true value is not clamped).  0-d float64, differentiable in ``pos_pred`` and ``temp_pred``
    (``cgnn_mass_assign_weighted_backward``); the true frame is deposited without autograd.  ``[N, 3]`` with ``[N]`` or
    ``[N, 1]``, or with a leading ``T`` for the mean over T frames as well.  ``smoothing``: as in
    :func:`density_field_loss`.  A true frame whose temperatures are all zero has no scale: the result is ``nan``.

    ``ValueError`` before any device work: the refusals of :func:`density_field_loss`, temperatures that do not go with
    the positions.  One box, one GPU; no host synchronisation."""
    who = "thermal_field_loss"
    mesh = check_density_loss(who, mesh, order, smoothing)
    if pos_pred.shape != pos_true.shape:
        raise ValueError(f"{who}: pos_pred {tuple(pos_pred.shape)} and pos_true {tuple(pos_true.shape)} differ in shape")
    lead = tuple(pos_pred.shape[:-1])
    for name, t in (("temp_pred", temp_pred), ("temp_true", temp_true)):
        if tuple(t.shape) not in (lead, lead + (1,)):
            raise ValueError(f"{who}: {name} must be {list(lead)} or {list(lead) + [1]}, got {tuple(t.shape)}")
    temp_true = temp_true.detach()
    scale = 2.0 * temp_true.abs().max().to(torch.float64)
    f_pred = ops.weighted_field(pos_pred, temp_pred.reshape(lead), box_size, mesh, order, scale)
    with torch.no_grad():
        f_true = ops.weighted_field(pos_true, temp_true.reshape(lead), box_size, mesh, order, scale)
    kernel = gaussian_filter(mesh, box_size, smoothing, f_pred.device) if smoothing > 0 else None
    return _mean_square(f_pred - f_true, kernel) / temp_true.to(torch.float64).mean() ** 2
