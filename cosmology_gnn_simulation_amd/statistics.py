"""Judging a rollout on the device: the two-point correlation function xi(r) of a frame from exact periodic pair counts
(``ops.pair_counts``), the cross-correlation of a predicted frame with the true one, and per-frame errors under the
minimum image (``ops.frame_errors``).

Per-particle errors stop meaning much a few steps into an N-body rollout, because trajectories diverge; whether the
clustering is right is what xi(r) of the predicted frame against the true one, and their cross-correlation, tell.
``rollout.calculate_errors`` (the reference's function) stays as it is: one host synchronisation per frame, and a
particle that crossed a box face scored as wrong by a whole box length.

One box per call.  Batches of simulations (``offsets``) and counting across spatial shards are out of scope: an
owned-storage rollout (``dist.sharded_rollout(storage="owned")``) goes through ``dist.assemble_frames`` first.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

from . import ops


def _radii(edges, box_size: float, who: str) -> torch.Tensor:
    """The radii the kernel bins by (float32 values), as float64."""
    return torch.tensor(ops.check_pair_count_edges(edges, box_size, who), dtype=torch.float64)


def correlation_from_counts(counts, n_a: int, n_b: Optional[int], box_size: float, edges, auto: bool) -> torch.Tensor:
    """The natural estimator ``xi = DD / RR - 1`` with the analytic random term of a periodic box, on the host in
    float64 from the ``nb`` integers (``counts [nb]`` or ``[T, nb]``; returns the same shape, float64, on the CPU):

    * auto:  ``xi_b = DD_b / (N (N - 1) / 2 * V_b / L^3) - 1``  (``N = n_a``; ``n_b`` is ignored)
    * cross: ``xi_b = D1D2_b / (N_a N_b V_b / L^3) - 1``

    with ``V_b = 4 pi / 3 (r_{b+1}^3 - r_b^3)``.  A shell inside half the box never meets its own periodic image, so
    the random term needs no random catalogue.  A bin that expects no pair at all (``N < 2``) gives ``nan``."""
    r = _radii(edges, box_size, "correlation_from_counts")
    c = torch.as_tensor(counts).detach().to(device="cpu", dtype=torch.float64)
    if c.shape[-1] != r.numel() - 1:
        raise ValueError(f"correlation_from_counts: {c.shape[-1]} counts for {r.numel() - 1} bins")
    shell = 4.0 * math.pi / 3.0 * (r[1:] ** 3 - r[:-1] ** 3) / float(box_size) ** 3
    pairs = n_a * (n_a - 1) / 2.0 if auto else float(n_a) * float(n_b)
    return c / (pairs * shell) - 1.0


def correlation_function(pos: torch.Tensor, box_size: float, edges, pos_b: Optional[torch.Tensor] = None) -> Dict:
    """xi(r) of ``pos [N, 3]`` (or of every frame of ``[T, N, 3]``), or with ``pos_b`` the cross-correlation of the two
    sets.  Returns ``{"r_lo", "r_hi", "counts", "xi"}`` on the CPU: bin radii (float64 ``[nb]``), the exact pair counts
    (int64) and the estimator of :func:`correlation_from_counts` (float64).  The counts come back in one transfer."""
    r = _radii(edges, box_size, "correlation_function")
    counts = ops.pair_counts(pos, box_size, edges, pos_b).cpu()
    n_a = pos.shape[-2]
    n_b = None if pos_b is None else pos_b.shape[-2]
    return {"r_lo": r[:-1].clone(), "r_hi": r[1:].clone(), "counts": counts,
            "xi": correlation_from_counts(counts, n_a, n_b, box_size, edges, pos_b is None)}


def rollout_statistics(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], box_size: float,
                       edges, frames: Optional[Sequence[int]] = None) -> Dict:
    """Statistics of a rollout against the truth, for the dicts ``rollout.rollout`` returns and
    ``rollout.calculate_errors`` takes (``Coordinates [T, N, 3]``, ``InternalEnergy [T, N(, 1)]``).  ``frames``: the frame
    numbers to judge (default: every frame both hold).  Per selected frame:

    * ``position_mse``, ``temperature_mse``: ``ops.frame_errors`` (positions under the minimum image);
    * ``xi_pred``, ``xi_true``: the correlation function of the predicted and of the true frame;
    * ``xi_cross``: the cross-correlation predicted x true;
    * ``counts_pred``, ``counts_true``, ``counts_cross``: the pair counts behind them,

    plus ``frames``, ``r_lo`` and ``r_hi``.  Everything is computed on the device of the rollout without a host
    synchronisation, and the results come back in one transfer at the end (CPU tensors, float64 / int64)."""
    what = "rollout_statistics"
    r = _radii(edges, box_size, what)
    pc = rollout_data["Coordinates"]
    dev = pc.device
    tc = ground_truth["Coordinates"].to(dev)
    pt, tt = rollout_data["InternalEnergy"], ground_truth["InternalEnergy"].to(dev)
    avail = min(len(pc), len(tc), len(pt), len(tt))
    sel = list(range(avail)) if frames is None else [int(f) for f in frames]
    if not sel or min(sel) < 0 or max(sel) >= avail:
        raise ValueError(f"{what}: frames must be numbers in [0, {avail}), got {sel}")
    if pc.shape[1:] != tc.shape[1:]:
        raise ValueError(f"{what}: predicted frames are {tuple(pc.shape[1:])}, true frames {tuple(tc.shape[1:])}")
    n = pc.shape[1]
    idx = torch.tensor(sel, dtype=torch.int64).to(dev)
    pc, tc = pc.index_select(0, idx), tc.index_select(0, idx)
    pt, tt = pt.index_select(0, idx).reshape(len(sel), -1), tt.index_select(0, idx).reshape(len(sel), -1)
    errs = ops.frame_errors(pc, tc, pt, tt, box_size)                                   # [F, 2] float64
    counts = torch.stack([ops.pair_counts(pc, box_size, edges), ops.pair_counts(tc, box_size, edges),
                          ops.pair_counts(pc, box_size, edges, tc)])                    # [3, F, nb] int64
    # one transfer: the float64 errors travel as their bits among the integers
    packed = torch.cat([errs.view(torch.int64).reshape(-1), counts.reshape(-1)]).cpu()
    errs = packed[:2 * len(sel)].view(torch.float64).reshape(len(sel), 2)
    counts = packed[2 * len(sel):].reshape(3, len(sel), -1)
    return {"frames": sel, "r_lo": r[:-1].clone(), "r_hi": r[1:].clone(),
            "position_mse": errs[:, 0].clone(), "temperature_mse": errs[:, 1].clone(),
            "counts_pred": counts[0], "counts_true": counts[1], "counts_cross": counts[2],
            "xi_pred": correlation_from_counts(counts[0], n, None, box_size, edges, True),
            "xi_true": correlation_from_counts(counts[1], n, None, box_size, edges, True),
            "xi_cross": correlation_from_counts(counts[2], n, n, box_size, edges, False)}
