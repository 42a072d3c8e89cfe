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
