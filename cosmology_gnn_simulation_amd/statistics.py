"""Judging a rollout on the device: the two-point correlation function xi(r) of a frame from exact periodic pair counts
(``ops.pair_counts``), the cross-correlation of a predicted frame with the true one, and per-frame errors under the
minimum image (``ops.frame_errors``).

Per-particle errors stop meaning much a few steps into an N-body rollout, because trajectories diverge; whether the
clustering is right is what xi(r) of the predicted frame against the true one, and their cross-correlation, tell.
``rollout.calculate_errors`` (the reference's function) stays as it is: one host synchronisation per frame, and a
particle that crossed a box face scored as wrong by a whole box length.

In Fourier space (what a learned cosmological simulator is normally judged by, and what reaches scales far beyond
the few interparticle spacings pair counting can afford): ``power_spectrum`` gives the matter power spectrum P(k) of
a frame -- an exact integer mass assignment (``ops.mass_assign``), one ``torch.fft.rfftn`` in complex128 and shell sums
in a fixed order (``ops.power_bins``) -- and, with a second set, the cross spectrum, the cross-correlation coefficient
r(k) = P_ab / sqrt(P_aa P_bb) and the transfer function T(k) = sqrt(P_aa / P_bb); ``rollout_power_spectra`` does that
for every selected frame of a rollout against the truth; ``spectra_from_sums`` is the host arithmetic behind both
and ``default_k_edges`` the unit-wide bins centred on the integer frequencies.

Halos (what neither two-point statistic can tell: a rollout may match P(k) to a few per cent and still smear every
halo into a puff): friends-of-friends groups, the connected components of "closer than the linking length" (0.2 mean
interparticle spacings by convention, ``default_linking_length``), labelled by a lock-free union-find on the device
(``ops.fof_labels``) and reduced in exact integers (``ops.fof_catalogue``).  ``halo_catalogue`` lists the groups of a
frame with their sizes and centres, ``halo_mass_function`` counts them by size (``default_size_edges``: doubling bins
from 20 members) and ``rollout_halo_statistics`` does that for every selected frame of a rollout against the truth.
The mass function tells whether a frame has the right number of groups of each size, not whether they are the same
groups: the predicted and the true frame hold the same particles under the same indices, so ``halo_matches`` pairs
the groups of two frames by the members they share (``ops.halo_match``; a pair is mutual when each is the other's
best partner), with sizes, centre offsets and, given per-particle values such as the temperature, each group's mean
(``ops.fof_group_sums``), and ``rollout_halo_matching`` gives per frame and per size bin of the true groups the
completeness, the shared fraction and the size ratio.  What is inside a halo, which neither tells (an emulator gets the
number and the membership of its halos about right and smears their interiors): ``halo_profiles`` gives per group the
radial density profile around its centre (``ops.halo_profiles``, one histogram per centre), with per-particle values the
mean value per shell, and from the profile the spherical-overdensity radius and mass (``so_masses``);
``rollout_halo_profiles`` stacks the profiles of the largest groups by size for every frame of a rollout and of the
truth.  Unbinding, velocities and merger trees over more than two frames are out of scope.

Redshift space (whether the velocities are right where they matter: coherent infall and the virial motions inside halos
show in the quadrupole, not in P(k)): ``power_multipoles`` gives P_0, P_2 and P_4 about a box axis, of a frame displaced
along it by its velocities (``ops.redshift_positions``), from Legendre-weighted shell sums of an interlaced pair of
meshes (``ops.power_multipoles``); ``rollout_redshift_spectra`` does that for every frame of a rollout against the
truth; ``multipoles_from_sums`` is the host arithmetic.  ``power_spectrum(interlace=True)`` uses the same reduction.
Below a few mean interparticle spacings a mesh cannot follow the field, and that is where the virial motions stretch
structures along the line of sight (the fingers of god): ``correlation_multipoles`` gives xi(s, mu) and xi_0, xi_2,
xi_4 of the displaced frame from exact pair counts by separation and by mu = |cos| of the angle to the line of sight
(``ops.pair_counts_smu``), down to zero separation, in integers and with the same bits on every run;
``rollout_redshift_correlation`` does that for every frame of a rollout against the truth;
``correlation_multipoles_from_counts`` is the host arithmetic and ``default_mu_edges`` the 20 equal mu-bins.

Beyond two points (two frames can agree in everything above and differ in how empty their voids are): ``knn_cdfs`` gives
the k-nearest-neighbour distance distributions of a frame seen from a lattice of query points (``ops.knn_distances``,
``ops.knn_cdf_counts``; ``query_lattice``, ``default_knn_radii``), with the void probability function, the
counts-in-spheres distribution and, for two sets, the joint CDF and its excess over independence;
``rollout_knn_cdfs`` does that for every frame of a rollout against the truth and ``knn_cdfs_from_counts`` is the host
arithmetic.  At which scales and in which configurations the non-Gaussianity sits, which the kNN-CDFs do not say:
``bispectrum`` gives B(k1, k2, k3) and the reduced Q of a frame by the FFT estimator -- the modes filtered into shells
(``ops.bispectrum_shells``), every shell back in real space, the products of three shell fields summed over the mesh
(``ops.bispectrum_sums``) -- ``rollout_bispectra`` does that for every frame of a rollout against the truth,
``bispectrum_from_sums`` is the host arithmetic and ``default_bispectrum_edges`` the shells up to a third of the mesh.
Its partner below the mesh, where filaments and halo outskirts live: ``three_point_correlation`` gives the Legendre
multipoles zeta_l(r1, r2) of the connected three-point function from exact pair walks -- per primary and radial bin the
integer sums of the monomials of the directions to its neighbours, contracted over two bins in float64
(``ops.triplet_moments``), once around the particles and once around a lattice of query points;
``rollout_three_point`` does that for every frame of a rollout against the truth, ``three_point_from_sums`` and
``three_point_zeta`` are the host arithmetic and ``default_three_point_edges`` the 8 bins from 0.5 to 4.5 spacings.

Morphology, which no N-point function of fixed order says: ``minkowski_functionals`` gives the four Minkowski functionals
V0 .. V3 (volume, surface, mean curvature, Euler characteristic) of the excursion sets of the smoothed density field as
functions of the threshold, from exact integer counts of the cubes, faces, edges and vertices of the sets on the mesh
(``ops.excursion_counts``), next to the curves of a Gaussian field (``gaussian_minkowski``); ``rollout_minkowski`` does
that for every frame of a rollout against the truth, ``minkowski_from_counts`` is the host arithmetic and
``default_minkowski_thresholds`` the 25 thresholds from -3 to 3 standard deviations.

Whether the halos are gravitationally bound, which nothing above says (a friends-of-friends group is a set of particles
that are close together): ``halo_binding`` unbinds the groups of one frame -- per member the softened potential of the
other members in exact integers (``ops.halo_potentials``), the specific energies (``binding_energies``), a fixed number
of passes that drop the members with ``e >= 0`` -- and lists bound masses, virial ratios and velocity dispersions;
``rollout_halo_binding`` does that for every frame of a rollout from 1 on against the truth, ``binding_from_sums`` and
``binding_size_bins`` are the host arithmetic.

One box per call.  Batches of simulations (``offsets``) and counting across spatial shards are out of scope: an
owned-storage rollout (``dist.sharded_rollout(storage="owned")``) goes through ``dist.assemble_frames`` first.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

from . import _lib, ops


def _radii(edges, box_size: float, who: str) -> torch.Tensor:
    """The radii the kernel bins by (float32 values), as float64."""
    return torch.tensor(ops.check_pair_count_edges(edges, box_size, who), dtype=torch.float64)


def _shell_volumes(r: torch.Tensor) -> torch.Tensor:
    """The volumes of the shells between consecutive radii ``r`` (float64)."""
    return 4.0 * math.pi / 3.0 * (r[1:] ** 3 - r[:-1] ** 3)


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
    shell = _shell_volumes(r) / float(box_size) ** 3
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


def default_k_edges(mesh: int) -> torch.Tensor:
    """``0.5 + arange(0, mesh // 2 + 1)``: unit-wide bins centred on the frequencies n = 1 .. mesh // 2, in units of the
    fundamental frequency ``2 pi / L`` (float64)."""
    mesh = ops.check_mesh(mesh, "default_k_edges")
    return 0.5 + torch.arange(0, mesh // 2 + 1, dtype=torch.float64)


def _sums_on_host(what: str, modes, sums, rows: int, box_size: float, mesh: int, k_edges):
    """The opening of :func:`spectra_from_sums` and :func:`multipoles_from_sums`: the checked arguments as ``(box, k,
    modes, sums, count, norm)``: ``k`` the edges times ``2 pi / L``, ``modes [..., nb]`` and ``sums [..., rows, nb]`` on the
    CPU, ``count`` the modes in float64 with ``nan`` for an empty bin, ``norm = L^3 / M^6``."""
    mesh = ops.check_mesh(mesh, what)
    box = float(box_size)
    if not (box > 0.0 and math.isfinite(box)):
        raise ValueError(f"{what}: box_size must be positive and finite, got {box_size!r}")
    k = torch.tensor(ops.check_power_edges(k_edges, what), dtype=torch.float64) * (2.0 * math.pi / box)
    modes = torch.as_tensor(modes).detach().to(device="cpu", dtype=torch.int64)
    sums = torch.as_tensor(sums).detach().to(device="cpu", dtype=torch.float64)
    nb = k.numel() - 1
    if modes.shape[-1] != nb or sums.shape[-2:] != (rows, nb) or sums.shape[:-2] != modes.shape[:-1]:
        raise ValueError(f"{what}: modes {tuple(modes.shape)} and sums {tuple(sums.shape)} do not fit {nb} bins")
    count = modes.to(torch.float64)
    count = torch.where(modes > 0, count, torch.full_like(count, float("nan")))
    return box, k, modes, sums, count, box ** 3 / float(mesh) ** 6


def spectra_from_sums(modes, sums, n_a: int, n_b: Optional[int], box_size: float, mesh: int, k_edges,
                      subtract_shot_noise: bool = True) -> Dict:
    """Spectra from the shell sums of ``ops.power_bins``, on the host in float64 (``modes [..., nb]`` int64, ``sums
    [..., 4, nb]``; the results have the shape of ``modes``, on the CPU).  With ``L = box_size``, ``M = mesh``:

    * ``k_lo``, ``k_hi`` ``[nb]``: the bin edges (the float32 values the kernel bins by) times ``2 pi / L``;
      ``k_mean``: the mean ``|k|`` over the modes of each bin;
    * ``power``: ``P = L^3 S_aa / modes / M^6``, minus the shot noise ``L^3 / n_a`` when ``subtract_shot_noise``;

    and with a second set (``n_b`` is not None)

    * ``power_b``: likewise from ``S_bb`` and ``n_b``;   ``cross``: ``L^3 S_ab / modes / M^6`` (no shot noise);
    * ``r = cross / sqrt(P_aa P_bb)`` from the spectra BEFORE the shot-noise subtraction, so ``|r| <= 1`` by
      Cauchy-Schwarz up to rounding;
    * ``transfer = sqrt(power / power_b)`` from the spectra AFTER it: ``nan`` where the subtraction leaves a spectrum
      negative (shot-noise dominated bins) or ``power_b`` zero.

    A bin without modes gives ``nan`` everywhere."""
    box, k, modes, sums, count, norm = _sums_on_host("spectra_from_sums", modes, sums, 4, box_size, mesh, k_edges)

    def spectrum(row):
        return norm * sums[..., row, :] / count

    p_a = spectrum(0)
    out = {"k_lo": k[:-1].clone(), "k_hi": k[1:].clone(), "k_mean": sums[..., 3, :] / count * (2.0 * math.pi / box),
           "modes": modes, "power": p_a - box ** 3 / n_a if subtract_shot_noise else p_a}
    if n_b is not None:
        p_b, p_ab = spectrum(1), spectrum(2)
        out["power_b"] = p_b - box ** 3 / n_b if subtract_shot_noise else p_b
        out["cross"] = p_ab
        out["r"] = p_ab / torch.sqrt(p_a * p_b)
        out["transfer"] = torch.sqrt(out["power"] / out["power_b"])
    return out


def _frames3(pos: torch.Tensor, name: str, what: str) -> torch.Tensor:
    if pos.dim() not in (2, 3) or pos.shape[-1] != 3 or pos.shape[-2] < 1 or pos.shape[0] < 1:
        raise ValueError(f"{what}: {name} must be [N, 3] or [T, N, 3] with N >= 1, got {tuple(pos.shape)}")
    return pos if pos.dim() == 3 else pos.unsqueeze(0)


def _check_spectrum_arguments(what: str, box_size, mesh, k_edges, order):
    mesh = ops.check_mesh(mesh, what)
    k_edges = ops.check_power_edges(default_k_edges(mesh) if k_edges is None else k_edges, what)
    if isinstance(order, bool) or order not in (1, 2, 3):
        raise ValueError(f"{what}: order must be 1 (NGP), 2 (CIC) or 3 (TSC), got {order!r}")
    if not (float(box_size) > 0.0 and math.isfinite(float(box_size))):
        raise ValueError(f"{what}: box_size must be positive and finite, got {box_size!r}")
    return mesh, k_edges


def _rollout_frames(rollout_data, ground_truth, frames, what: str, also=()):
    """The selected predicted and true frames ``[F, N, 3]`` on the rollout's device, and their numbers.  ``also``: further
    tensors on that device with one entry per frame; they bound the frames there are, and their selected entries
    follow."""
    pc = rollout_data["Coordinates"]
    dev = pc.device
    tc = ground_truth["Coordinates"].to(dev)
    avail = min(len(pc), len(tc), *(len(x) for x in also))
    sel = list(range(avail)) if frames is None else [int(f) for f in frames]
    if not sel or min(sel) < 0 or max(sel) >= avail:
        raise ValueError(f"{what}: frames must be numbers in [0, {avail}), got {sel}")
    if pc.shape[1:] != tc.shape[1:]:
        raise ValueError(f"{what}: predicted frames are {tuple(pc.shape[1:])}, true frames {tuple(tc.shape[1:])}")
    idx = torch.tensor(sel, dtype=torch.int64).to(dev)
    pc, tc = pc.index_select(0, idx), tc.index_select(0, idx)
    _frames3(pc, "Coordinates", what)
    return (pc, tc, sel) + tuple(x.index_select(0, idx) for x in also)


def _contrast_modes(pos: torch.Tensor, box_size: float, mesh: int, order: int) -> torch.Tensor:
    """``rfftn`` of the density contrast of every frame of ``pos [F, N, 3]``: complex128 ``[F, M, M, M/2 + 1]``."""
    grid = ops.mass_assign(pos, box_size, mesh, order)
    delta = ops.grid_contrast(grid, pos.shape[1])
    del grid                    # the int64 mesh goes before the transform takes its memory
    return torch.fft.rfftn(delta, dim=(-3, -2, -1))


def _shell_sums(pos_a: torch.Tensor, pos_b: Optional[torch.Tensor], box_size: float, mesh: int, k_edges, order: int,
                los: Optional[int] = None, interlace: bool = False):
    """The shell sums of the density contrast of every frame of ``pos_a [F, N, 3]`` (and ``pos_b [F, N_b, 3]``) as device
    tensors ``modes [F, nb]``, ``sums [F, rows, nb]``: ``ops.power_bins`` (4 rows) when ``los`` is None, else
    ``ops.power_multipoles`` (12 rows) about ``los``, from an interlaced pair of meshes with ``interlace``.  Frames go
    through in chunks whose meshes fit the free device memory: per frame, set and mesh of the interlaced pair ``8 M^3``
    (the contrast) + ``16 M^2 (M/2 + 1)`` (its transform) + ``8 M^3`` (the int64 mesh) bytes and as much again for the
    FFT's own scratch, and per frame the workspace (``nb * 64`` slices of ``rows`` float64 sums and a count) and the
    outputs (``(rows + 1) nb`` values).  The int64 mesh and the contrast of one transform are gone before the next is
    made, and the transforms of a chunk before the next chunk."""
    from .training import free_device_bytes
    assert los is not None or not interlace       # no four-row interlaced entry: _interlaced_shell_sums selects the rows
    n_frames, nb = pos_a.shape[0], len(k_edges) - 1
    values = 5 if los is None else _lib.POWER_MULTIPOLE_SUMS + 1
    meshes = (1 if pos_b is None else 2) * (2 if interlace else 1)
    per_frame = (16 * mesh ** 3 + 16 * mesh * mesh * (mesh // 2 + 1)) * meshes * 2 + nb * 64 * values * 8 + nb * values * 8
    chunk = max(1, min(n_frames, free_device_bytes(pos_a.device) // per_frame))
    plan = ops.PowerPlan.of(mesh, k_edges, pos_a.device)

    def transforms(pos):
        if pos is None:
            return None, None
        first = _contrast_modes(pos, box_size, mesh, order)
        if not interlace:
            return first, None
        return first, _contrast_modes(ops.interlace_shift(pos, box_size, mesh), box_size, mesh, order)

    modes, sums = [], []
    for f0 in range(0, n_frames, chunk):
        a, a2 = transforms(pos_a[f0:f0 + chunk])
        b, b2 = transforms(None if pos_b is None else pos_b[f0:f0 + chunk])
        if los is None:
            m, s = ops.power_bins(a, mesh, order, k_edges, b, plan)
        else:
            m, s = ops.power_multipoles(a, mesh, order, k_edges, los, b, a2, b2, plan)
        del a, a2, b, b2
        modes.append(m)
        sums.append(s)
    return (modes[0], sums[0]) if len(modes) == 1 else (torch.cat(modes), torch.cat(sums))


def _to_host(modes: torch.Tensor, sums: torch.Tensor, *extra: Optional[torch.Tensor]):
    """One transfer: the float64 sums, and every float64 or int64 ``extra`` that is not None, travel as their bits among
    the integers -> ``(modes, sums, *extra)`` on the CPU."""
    parts = [modes, sums] + [x.contiguous() for x in extra if x is not None]
    packed = torch.cat([p.view(torch.int64).reshape(-1) for p in parts]).cpu()
    host = packed.split([p.numel() for p in parts])
    return tuple(h.view(p.dtype).reshape(p.shape) for h, p in zip(host, parts))


def _interlaced_shell_sums(pos_a, pos_b, box_size: float, mesh: int, k_edges, order: int):
    """:func:`_shell_sums` from an interlaced pair of meshes: rows 0, 3, 6 and 9 of ``ops.power_multipoles``."""
    modes, sums = _shell_sums(pos_a, pos_b, box_size, mesh, k_edges, order, 2, True)
    return modes, torch.stack([sums[:, row] for row in (0, 3, 6, 9)], dim=1)


def power_spectrum(pos: torch.Tensor, box_size: float, mesh: int, k_edges=None, pos_b: Optional[torch.Tensor] = None,
                   order: int = 2, subtract_shot_noise: bool = True, interlace: bool = False) -> Dict:
    """The matter power spectrum of ``pos [N, 3]`` (or of every frame of ``[T, N, 3]``) on a ``mesh^3`` grid, deposited
    with ``order`` (1 = NGP, 2 = CIC, 3 = TSC) and deconvolved by that window; with ``pos_b`` (``[N_b, 3]`` or ``[T, N_b,
    3]``) also its spectrum and the cross spectrum of the two.  ``k_edges``: ``nb + 1`` bin edges in units of ``2 pi / L``
    (default :func:`default_k_edges`).  Returns the dict of :func:`spectra_from_sums` (CPU, float64 / int64; ``[nb]`` or
    ``[T, nb]``): ``k_lo``, ``k_hi``, ``k_mean``, ``modes``, ``power`` and with ``pos_b`` also ``power_b``, ``cross``,
    ``r``, ``transfer``.  ``transfer`` may be ``nan`` (see there); an empty bin is ``nan``.  Without ``interlace``
    aliasing is not corrected beyond the window deconvolution: bins past half the Nyquist frequency are lifted by it.
    ``interlace=True`` deposits every set a second time, displaced by half a cell (``ops.interlace_shift``), and combines
    the two transforms inside the reduction (``ops.power_multipoles``): the odd aliases cancel and the bins up to the
    Nyquist frequency are usable, for twice the meshes and transforms.  Everything is computed on the device of ``pos``
    without a host synchronisation and comes back in one transfer."""
    what = "power_spectrum"
    mesh, k_edges = _check_spectrum_arguments(what, box_size, mesh, k_edges, order)
    frames_a = _frames3(pos, "pos", what)
    frames_b = None if pos_b is None else _frames3(pos_b, "pos_b", what)
    if frames_b is not None and (pos_b.dim() != pos.dim() or frames_b.shape[0] != frames_a.shape[0]):
        raise ValueError(f"{what}: pos_b {tuple(pos_b.shape)} does not go with pos {tuple(pos.shape)}")
    shell_sums = _interlaced_shell_sums if interlace else _shell_sums
    modes, sums = _to_host(*shell_sums(frames_a, frames_b, box_size, mesh, k_edges, order))
    if pos.dim() == 2:
        modes, sums = modes[0], sums[0]
    return spectra_from_sums(modes, sums, frames_a.shape[1], None if frames_b is None else frames_b.shape[1], box_size,
                             mesh, k_edges, subtract_shot_noise)


def rollout_power_spectra(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], box_size: float,
                          mesh: int, k_edges=None, frames: Optional[Sequence[int]] = None, order: int = 2,
                          interlace: bool = False) -> Dict:
    """Fourier-space statistics of a rollout against the truth, for the dicts ``rollout.rollout`` returns
    (``Coordinates [T, N, 3]``).  ``frames``: the frame numbers to judge (default: every frame both hold).  Per selected
    frame (``[F, nb]``, CPU, float64):

    * ``power_pred``, ``power_true``: the shot-noise-subtracted power spectra of the predicted and the true frame;
    * ``cross``: their cross spectrum;  ``r``: the cross-correlation coefficient (``|r| <= 1``);
    * ``transfer``: ``sqrt(power_pred / power_true)``, ``nan`` where a subtracted spectrum is negative,

    plus ``frames``, ``k_lo``, ``k_hi``, ``k_mean`` (``[nb]``) and ``modes`` (``[nb]``, int64).  ``interlace``: as in
    :func:`power_spectrum`.  Everything is computed on the device of the rollout without a host synchronisation per
    frame; the results come back in one transfer."""
    what = "rollout_power_spectra"
    mesh, k_edges = _check_spectrum_arguments(what, box_size, mesh, k_edges, order)
    pc, tc, sel = _rollout_frames(rollout_data, ground_truth, frames, what)
    n = pc.shape[1]
    shell_sums = _interlaced_shell_sums if interlace else _shell_sums
    modes, sums = _to_host(*shell_sums(pc, tc, box_size, mesh, k_edges, order))
    sp = spectra_from_sums(modes, sums, n, n, box_size, mesh, k_edges, True)
    return {"frames": sel, "k_lo": sp["k_lo"], "k_hi": sp["k_hi"], "k_mean": sp["k_mean"][0].clone(),
            "modes": sp["modes"][0].clone(), "power_pred": sp["power"], "power_true": sp["power_b"],
            "cross": sp["cross"], "r": sp["r"], "transfer": sp["transfer"]}


# ---- redshift space: the multipoles of the power spectrum, interlaced -------------------------------------------------
#
# ``ops.redshift_positions`` displaces every particle along a box axis by its velocity (plane-parallel line of sight),
# ``ops.power_multipoles`` sums the modes of the displaced frame's mesh with Legendre weights about that axis and combines
# an interlaced pair of meshes inside the reduction.  Per-particle or wide-angle lines of sight, sharded, batched and
# owned-storage variants, a multipole loss and interlaced momentum and thermal spectra are not built (xi(s, mu) pair
# counts: the section after this one).

MULTIPOLES = (0, 2, 4)


def multipoles_from_sums(modes, sums, n_a: int, n_b: Optional[int], box_size: float, mesh: int, k_edges,
                         subtract_shot_noise: bool = True) -> Dict:
    """Multipoles from the shell sums of ``ops.power_multipoles``, on the host in float64 (``modes [..., nb]`` int64,
    ``sums [..., 12, nb]``; the results have the shape of ``modes``, on the CPU).  With ``L = box_size``, ``M = mesh`` and
    ``S_l`` the row of the Legendre polynomial ``L_l``:

    * ``k_lo``, ``k_hi``, ``k_mean``, ``modes``: as in :func:`spectra_from_sums`;
    * ``power_0``, ``power_2``, ``power_4``: ``P_l = (2 l + 1) L^3 S_l / modes / M^6``; the shot noise ``L^3 / n_a`` is
      isotropic and leaves ``l = 0`` only (when ``subtract_shot_noise``);
    * ``legendre_mean_2``, ``legendre_mean_4``: the mean of ``L_2``, ``L_4`` over the modes of the bin.  A discrete
      shell is not a sphere: an isotropic spectrum ``P`` shows ``(2 l + 1) P legendre_mean_l`` in ``power_l``;

    and with a second set (``n_b`` is not None) ``power_b_0/2/4`` (shot noise ``L^3 / n_b``), ``cross_0/2/4`` (no shot
    noise) and the monopole's ``r`` and ``transfer``, defined as in :func:`spectra_from_sums`.  A bin without modes gives
    ``nan`` everywhere."""
    box, k, modes, sums, count, norm = _sums_on_host("multipoles_from_sums", modes, sums, _lib.POWER_MULTIPOLE_SUMS,
                                                     box_size, mesh, k_edges)

    def multipole(first_row, i):
        p = norm * sums[..., first_row + i, :] / count
        return p if i == 0 else (2 * MULTIPOLES[i] + 1) * p

    out = {"k_lo": k[:-1].clone(), "k_hi": k[1:].clone(), "k_mean": sums[..., 9, :] / count * (2.0 * math.pi / box),
           "modes": modes, "legendre_mean_2": sums[..., 10, :] / count, "legendre_mean_4": sums[..., 11, :] / count}
    sets = (("power_", 0, n_a),) if n_b is None else (("power_", 0, n_a), ("power_b_", 3, n_b), ("cross_", 6, None))
    for name, first_row, n in sets:
        for i, ell in enumerate(MULTIPOLES):
            p = multipole(first_row, i)
            out[f"{name}{ell}"] = p - box ** 3 / n if (ell == 0 and n is not None and subtract_shot_noise) else p
    if n_b is not None:
        out["r"] = out["cross_0"] / torch.sqrt(multipole(0, 0) * multipole(3, 0))
        out["transfer"] = torch.sqrt(out["power_0"] / out["power_b_0"])
    return out


def _check_multipole_arguments(what: str, box_size, mesh, k_edges, order, los, dt, velocity_scale, moving: bool):
    mesh, k_edges = _check_spectrum_arguments(what, box_size, mesh, k_edges, order)
    los = ops.check_los(los, what)
    if moving:
        ops.redshift_shift(dt, velocity_scale, what)
    return mesh, k_edges, los


def _f32_frames(pos: torch.Tensor, name: str, what: str) -> torch.Tensor:
    frames = _frames3(pos, name, what)
    return frames if frames.dtype == torch.float32 else frames.float()


def power_multipoles(pos: torch.Tensor, box_size: float, mesh: int, pos_prev: Optional[torch.Tensor] = None,
                     dt: Optional[float] = None, velocity_scale: float = 1.0, los: int = 2, k_edges=None,
                     pos_b: Optional[torch.Tensor] = None, pos_b_prev: Optional[torch.Tensor] = None, order: int = 2,
                     interlace: bool = True, subtract_shot_noise: bool = True) -> Dict:
    """The multipoles ``P_0``, ``P_2``, ``P_4`` of the power spectrum of ``pos`` (``[N, 3]`` or ``[T, N, 3]``) about the
    box axis ``los``, in redshift space when ``pos_prev`` (the frame before, the same shape) and ``dt`` are given: every
    particle is first displaced along ``los`` by ``velocity_scale * minimum_image(pos - pos_prev) / dt``
    (``ops.redshift_positions``; ``velocity_scale`` is ``1 / (a H)`` in the caller's units).  Without ``pos_prev`` they are
    the real-space multipoles of ``pos``: ``P_2`` and ``P_4`` then hold only what the discrete shells leak (see
    ``legendre_mean_l``).  With ``pos_b`` (and ``pos_b_prev`` when ``pos_prev`` is given) also the second set's multipoles
    and the cross multipoles.  ``interlace`` (default on): a second mesh displaced by half a cell is combined with the
    first inside the reduction, which removes the odd aliases; without it ``P_4`` is wrong past a quarter of the mesh even
    on white noise.  Returns the dict of :func:`multipoles_from_sums`.  Everything is computed on the device of ``pos``
    without a host synchronisation and comes back in one transfer."""
    what = "power_multipoles"
    moving = pos_prev is not None
    if moving and dt is None:
        raise ValueError(f"{what}: pos_prev needs dt")
    mesh, k_edges, los = _check_multipole_arguments(what, box_size, mesh, k_edges, order, los, dt, velocity_scale, moving)
    if (pos_b_prev is not None) != (pos_b is not None and moving):
        raise ValueError(f"{what}: pos_b_prev is given exactly when pos_b and pos_prev both are")
    sets = []
    for name, cur, prev in (("pos", pos, pos_prev), ("pos_b", pos_b, pos_b_prev)):
        if cur is None:
            sets.append(None)
            continue
        frames = _f32_frames(cur, name, what)
        if cur.dim() != pos.dim() or frames.shape[0] != (pos.shape[0] if pos.dim() == 3 else 1):
            raise ValueError(f"{what}: {name} {tuple(cur.shape)} does not go with pos {tuple(pos.shape)}")
        if prev is not None:
            if tuple(prev.shape) != tuple(cur.shape):
                raise ValueError(f"{what}: {name}_prev {tuple(prev.shape)} and {name} {tuple(cur.shape)} differ in shape")
            frames = ops.redshift_positions(frames, _f32_frames(prev, name + "_prev", what).to(frames.device), dt,
                                            box_size, los, velocity_scale)
        sets.append(frames)
    modes, sums = _to_host(*_shell_sums(sets[0], sets[1], box_size, mesh, k_edges, order, los, bool(interlace)))
    if pos.dim() == 2:
        modes, sums = modes[0], sums[0]
    return multipoles_from_sums(modes, sums, sets[0].shape[1], None if sets[1] is None else sets[1].shape[1], box_size,
                                mesh, k_edges, subtract_shot_noise)


def rollout_redshift_spectra(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor],
                             box_size: float, mesh: int, dt: float, velocity_scale: float = 1.0, los: int = 2,
                             frames: Optional[Sequence[int]] = None, k_edges=None, order: int = 2,
                             interlace: bool = True) -> Dict:
    """Redshift-space statistics of a rollout against the truth, for the dicts ``rollout.rollout`` returns
    (``Coordinates [T, N, 3]``): whether the velocities are right where they matter.  Every judged frame of either side is
    displaced along ``los`` by its own velocity, ``minimum_image`` of its step from the frame before in the same dict,
    over ``dt`` and times ``velocity_scale`` (:func:`power_multipoles`).  ``frames``: the frame numbers to judge (default:
    every frame from 1 on that both hold); frame 0 has no predecessor and is ``nan``, as in :func:`rollout_gas_spectra`.
    Per selected frame (``[F, nb]``, CPU, float64), for ``l`` in 0, 2, 4:

    * ``power_pred_l``, ``power_true_l``: the multipoles of the two sides (the shot noise leaves ``l = 0``);
      ``cross_l``: their cross multipoles;
    * ``r``, ``transfer``: of the monopoles, as in :func:`rollout_power_spectra`;
    * ``quadrupole_ratio``: ``power_pred_2 / power_true_2``,

    plus ``frames``, ``k_lo``, ``k_hi``, ``k_mean``, ``legendre_mean_2``, ``legendre_mean_4`` (``[nb]``) and ``modes``
    (``[nb]``, int64).  No host synchronisation per frame; one transfer."""
    what = "rollout_redshift_spectra"
    mesh, k_edges, los = _check_multipole_arguments(what, box_size, mesh, k_edges, order, los, dt, velocity_scale, True)
    pc = rollout_data["Coordinates"]
    dev = pc.device
    truth = {"Coordinates": ground_truth["Coordinates"].to(dev)}       # moved once: the predecessors come from it too
    if frames is None:
        frames = range(1, min(len(pc), len(truth["Coordinates"])))
    cp, ct, sel = _rollout_frames(rollout_data, truth, frames, what)
    rows = [i for i, f in enumerate(sel) if f > 0]
    if not rows:
        raise ValueError(f"{what}: no selected frame has a predecessor (frames {sel})")
    nf, nb, n = len(sel), len(k_edges) - 1, cp.shape[1]
    prev = torch.tensor([sel[i] - 1 for i in rows], dtype=torch.int64).to(dev)
    at = torch.tensor(rows, dtype=torch.int64).to(dev)
    sides = []
    for cur, source in ((cp, pc), (ct, truth["Coordinates"])):
        sides.append(ops.redshift_positions(_f32_frames(cur.index_select(0, at), "Coordinates", what),
                                            _f32_frames(source.index_select(0, prev), "Coordinates", what), dt, box_size,
                                            los, velocity_scale))
    modes, sums = _shell_sums(sides[0], sides[1], box_size, mesh, k_edges, order, los, bool(interlace))
    if len(rows) != nf:        # frame 0: nan sums; the mode counts are every frame's
        block = torch.full((nf, _lib.POWER_MULTIPOLE_SUMS, nb), float("nan"), dtype=torch.float64, device=dev)
        block.index_copy_(0, at, sums)
        modes, sums = modes[:1].expand(nf, nb).contiguous(), block
    modes, sums = _to_host(modes, sums)
    sp = multipoles_from_sums(modes, sums, n, n, box_size, mesh, k_edges, True)
    out = {"frames": sel, "k_lo": sp["k_lo"], "k_hi": sp["k_hi"], "modes": sp["modes"][0].clone(),
           "r": sp["r"], "transfer": sp["transfer"], "quadrupole_ratio": sp["power_2"] / sp["power_b_2"]}
    first = rows[0]                 # a frame that was computed: the shells are every frame's
    for key in ("k_mean", "legendre_mean_2", "legendre_mean_4"):
        out[key] = sp[key][first].clone()
    for ell in MULTIPOLES:
        out[f"power_pred_{ell}"], out[f"power_true_{ell}"] = sp[f"power_{ell}"], sp[f"power_b_{ell}"]
        out[f"cross_{ell}"] = sp[f"cross_{ell}"]
    return out


# ---- redshift space below the mesh: xi(s, mu) from exact pair counts, and its multipoles -------------------------------
#
# ``ops.pair_counts_smu`` counts the pairs of a frame by separation and by mu = |cos| of the angle to the line of sight;
# what follows forms xi(s, mu) with the analytic random term of a periodic box and projects it on the Legendre
# polynomials.  (r_p, pi) counts and w_p, per-particle or wide-angle lines of sight, random catalogues and Landy-Szalay,
# weighted pairs, sharded, batched and owned-storage variants and a correlation-multipole loss are not built.

def default_mu_edges(n_mu: int = 20) -> torch.Tensor:
    """``linspace(0, 1, n_mu + 1)``: ``n_mu`` equal bins of mu = |cos| of the angle to the line of sight (float64)."""
    if isinstance(n_mu, bool) or int(n_mu) != n_mu or not 1 <= n_mu <= _lib.PAIR_COUNTS_SMU_MAX_AXIS:
        raise ValueError(f"default_mu_edges: n_mu must be an integer in [1, {_lib.PAIR_COUNTS_SMU_MAX_AXIS}], got {n_mu!r}")
    return torch.linspace(0.0, 1.0, int(n_mu) + 1, dtype=torch.float64)


def _mus(mu_edges, who: str) -> torch.Tensor:
    """The mu edges the kernel bins by (float32 values), as float64."""
    return torch.tensor(ops.check_mu_edges(default_mu_edges() if mu_edges is None else mu_edges, who),
                        dtype=torch.float64)


def legendre_bin_integrals(mu: torch.Tensor) -> torch.Tensor:
    """``[3, nmu]``: the integrals of ``L_0``, ``L_2``, ``L_4`` over each bin of the edges ``mu``, in closed form from
    the antiderivatives ``mu``, ``(mu^3 - mu) / 2`` and ``(7 mu^5 - 10 mu^3 + 3 mu) / 8``."""
    prim = torch.stack([mu, (mu ** 3 - mu) / 2.0, (7.0 * mu ** 5 - 10.0 * mu ** 3 + 3.0 * mu) / 8.0])
    return prim[:, 1:] - prim[:, :-1]


def correlation_multipoles_from_counts(counts, n_a: int, n_b: Optional[int], box_size: float, s_edges, mu_edges,
                                       auto: bool) -> Dict:
    """xi(s, mu) and its multipoles from the ``ns x nmu`` integers of ``ops.pair_counts_smu``, on the host in float64
    (``counts [ns, nmu]`` or ``[T, ns, nmu]``; everything comes back on the CPU).  The natural estimator with the
    analytic random term of a periodic box, as in :func:`correlation_from_counts`:

    * ``xi_smu = DD / RR - 1`` with ``RR[i, j] = pairs * 4 pi / 3 (s_{i+1}^3 - s_i^3) / L^3 * (mu_{j+1} - mu_j)`` and
      ``pairs = N (N - 1) / 2`` (auto; ``n_b`` is ignored) or ``N_a N_b`` (cross): mu is |cos| folded into [0, 1], so a
      mu-bin holds the fraction ``mu_{j+1} - mu_j`` of a shell;
    * ``xi_0``, ``xi_2``, ``xi_4`` (``[..., ns]``): ``xi_l[i] = (2 l + 1) sum_j xi_smu[i, j] int_{mu_j}^{mu_{j+1}} L_l(mu)
      dmu`` with the bin integrals in closed form (:func:`legendre_bin_integrals`).  They are exact for the bins and sum
      to (1, 0, 0) over [0, 1], so the -1 leaves ``l = 2, 4`` altogether, and ``xi_0`` is
      ``correlation_from_counts(counts.sum(-1), ...)`` to rounding;

    plus ``s_lo``, ``s_hi`` (``[ns]``), ``mu_lo``, ``mu_hi`` (``[nmu]``) -- the float32 values the kernel binned by, as
    float64 -- and ``counts`` (int64).  A bin that expects no pair at all (``N < 2``) gives ``nan``."""
    what = "correlation_multipoles_from_counts"
    s = _radii(s_edges, box_size, what)
    mu = _mus(mu_edges, what)
    ns, nmu = s.numel() - 1, mu.numel() - 1
    counts = torch.as_tensor(counts).detach().to(device="cpu")
    if counts.dim() < 2 or tuple(counts.shape[-2:]) != (ns, nmu):
        raise ValueError(f"{what}: counts {tuple(counts.shape)} for {ns} x {nmu} bins")
    shell = _shell_volumes(s) / float(box_size) ** 3
    pairs = n_a * (n_a - 1) / 2.0 if auto else float(n_a) * float(n_b)
    rr = pairs * shell[:, None] * (mu[1:] - mu[:-1])[None, :]
    xi = counts.to(torch.float64) / rr - 1.0
    out = {"s_lo": s[:-1].clone(), "s_hi": s[1:].clone(), "mu_lo": mu[:-1].clone(), "mu_hi": mu[1:].clone(),
           "counts": counts.to(torch.int64), "xi_smu": xi}
    for ell, w in zip(MULTIPOLES, legendre_bin_integrals(mu)):
        out[f"xi_{ell}"] = (2 * ell + 1) * (xi * w).sum(-1)
    return out


def _check_smu_arguments(what: str, box_size, s_edges, mu_edges, los, dt, velocity_scale, moving: bool):
    """The host refusals of the (s, mu) functions, before any device work; returns the mu edges to bin by and ``los``."""
    s = ops.check_pair_count_edges(s_edges, box_size, what)
    mu_edges = ops.check_mu_edges(default_mu_edges() if mu_edges is None else mu_edges, what)
    ns, nmu = len(s) - 1, len(mu_edges) - 1
    if ns > _lib.PAIR_COUNTS_SMU_MAX_AXIS or ns * nmu > _lib.PAIR_COUNTS_SMU_MAX_BINS:
        raise ValueError(f"{what}: {ns} x {nmu} bins exceed {_lib.PAIR_COUNTS_SMU_MAX_AXIS} per axis or "
                         f"{_lib.PAIR_COUNTS_SMU_MAX_BINS} in all")
    los = ops.check_los(los, what)
    if moving:
        ops.redshift_shift(dt, velocity_scale, what)
    return mu_edges, los


def correlation_multipoles(pos: torch.Tensor, box_size: float, s_edges, mu_edges=None,
                           pos_prev: Optional[torch.Tensor] = None, dt: Optional[float] = None,
                           velocity_scale: float = 1.0, los: int = 2, pos_b: Optional[torch.Tensor] = None,
                           pos_b_prev: Optional[torch.Tensor] = None) -> Dict:
    """xi(s, mu) and the multipoles ``xi_0``, ``xi_2``, ``xi_4`` of ``pos`` (``[N, 3]`` or ``[T, N, 3]``) about the box
    axis ``los`` from exact pair counts (``ops.pair_counts_smu``), in redshift space when ``pos_prev`` (the frame before,
    the same shape) and ``dt`` are given: every particle is first displaced along ``los`` by ``velocity_scale *
    minimum_image(pos - pos_prev) / dt`` (``ops.redshift_positions``), as in :func:`power_multipoles`.  Without
    ``pos_prev`` they are the real-space multipoles of ``pos``.  With ``pos_b`` (and ``pos_b_prev`` when ``pos_prev`` is
    given) the cross counts and cross multipoles of the two sets, and only those.  ``mu_edges`` defaults to
    :func:`default_mu_edges`.  Returns the dict of :func:`correlation_multipoles_from_counts`.  Everything is counted on
    the device of ``pos`` without a host synchronisation and comes back in one transfer."""
    what = "correlation_multipoles"
    moving = pos_prev is not None
    if moving and dt is None:
        raise ValueError(f"{what}: pos_prev needs dt")
    mu_edges, los = _check_smu_arguments(what, box_size, s_edges, mu_edges, los, dt, velocity_scale, moving)
    if (pos_b_prev is not None) != (pos_b is not None and moving):
        raise ValueError(f"{what}: pos_b_prev is given exactly when pos_b and pos_prev both are")
    sets = []
    for name, cur, prev in (("pos", pos, pos_prev), ("pos_b", pos_b, pos_b_prev)):
        if cur is None:
            sets.append(None)
            continue
        frames = _f32_frames(cur, name, what)
        if cur.dim() != pos.dim() or frames.shape[0] != (pos.shape[0] if pos.dim() == 3 else 1):
            raise ValueError(f"{what}: {name} {tuple(cur.shape)} does not go with pos {tuple(pos.shape)}")
        if prev is not None:
            if tuple(prev.shape) != tuple(cur.shape):
                raise ValueError(f"{what}: {name}_prev {tuple(prev.shape)} and {name} {tuple(cur.shape)} differ in shape")
            frames = ops.redshift_positions(frames, _f32_frames(prev, name + "_prev", what).to(frames.device), dt,
                                            box_size, los, velocity_scale)
        sets.append(frames)
    counts = ops.pair_counts_smu(sets[0], box_size, s_edges, mu_edges, sets[1], los=los).cpu()
    if pos.dim() == 2:
        counts = counts[0]
    return correlation_multipoles_from_counts(counts, sets[0].shape[1], None if sets[1] is None else sets[1].shape[1],
                                              box_size, s_edges, mu_edges, sets[1] is None)


def rollout_redshift_correlation(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor],
                                 box_size: float, s_edges, dt: float, velocity_scale: float = 1.0, los: int = 2,
                                 frames: Optional[Sequence[int]] = None, mu_edges=None) -> Dict:
    """Redshift-space correlation multipoles of a rollout against the truth, for the dicts ``rollout.rollout`` returns
    (``Coordinates [T, N, 3]``): :func:`rollout_redshift_spectra` below the scales a mesh can follow, where the virial
    motions inside halos stretch structures along the line of sight.  Every judged frame of either side is displaced
    along ``los`` by its own velocity, ``minimum_image`` of its step from the frame before in the same dict, over ``dt``
    and times ``velocity_scale`` (:func:`correlation_multipoles`).  ``frames``: the frame numbers to judge (default:
    every frame from 1 on that both hold); frame 0 has no predecessor: its multipoles are ``nan`` and its counts 0.
    Per selected frame (CPU), for ``l`` in 0, 2, 4:

    * ``xi_pred_l``, ``xi_true_l``: the multipoles of the two sides; ``xi_cross_l``: of their cross counts (float64
      ``[F, ns]``);
    * ``counts_pred``, ``counts_true``, ``counts_cross``: the pair counts behind them (int64 ``[F, ns, nmu]``);
    * ``quadrupole_ratio``: ``xi_pred_2 / xi_true_2``,

    plus ``frames``, ``s_lo``, ``s_hi`` (``[ns]``) and ``mu_lo``, ``mu_hi`` (``[nmu]``).  No host synchronisation per
    frame; one transfer."""
    what = "rollout_redshift_correlation"
    mu_edges, los = _check_smu_arguments(what, box_size, s_edges, mu_edges, los, dt, velocity_scale, True)
    pc = rollout_data["Coordinates"]
    dev = pc.device
    truth = {"Coordinates": ground_truth["Coordinates"].to(dev)}       # moved once: the predecessors come from it too
    if frames is None:
        frames = range(1, min(len(pc), len(truth["Coordinates"])))
    cp, ct, sel = _rollout_frames(rollout_data, truth, frames, what)
    rows = [i for i, f in enumerate(sel) if f > 0]
    if not rows:
        raise ValueError(f"{what}: no selected frame has a predecessor (frames {sel})")
    n = cp.shape[1]
    prev = torch.tensor([sel[i] - 1 for i in rows], dtype=torch.int64).to(dev)
    at = torch.tensor(rows, dtype=torch.int64).to(dev)
    sides = []
    for cur, source in ((cp, pc), (ct, truth["Coordinates"])):
        sides.append(ops.redshift_positions(_f32_frames(cur.index_select(0, at), "Coordinates", what),
                                            _f32_frames(source.index_select(0, prev), "Coordinates", what), dt, box_size,
                                            los, velocity_scale))
    counted = torch.stack([ops.pair_counts_smu(sides[0], box_size, s_edges, mu_edges, los=los),
                           ops.pair_counts_smu(sides[1], box_size, s_edges, mu_edges, los=los),
                           ops.pair_counts_smu(sides[0], box_size, s_edges, mu_edges, sides[1], los=los)]).cpu()
    counts = torch.zeros((3, len(sel)) + tuple(counted.shape[2:]), dtype=torch.int64)
    counts[:, rows] = counted
    out = {"frames": sel}
    no_prev = torch.tensor([f == 0 for f in sel])[:, None]             # frame 0: nan
    for i, (name, auto) in enumerate((("pred", True), ("true", True), ("cross", False))):
        res = correlation_multipoles_from_counts(counts[i], n, n, box_size, s_edges, mu_edges, auto)
        out[f"counts_{name}"] = res["counts"]
        for ell in MULTIPOLES:
            out[f"xi_{name}_{ell}"] = res[f"xi_{ell}"].masked_fill(no_prev, float("nan"))
    for key in ("s_lo", "s_hi", "mu_lo", "mu_hi"):
        out[key] = res[key]
    out["quadrupole_ratio"] = out["xi_pred_2"] / out["xi_true_2"]
    return out


# ---- pairwise velocities: the mean infall and the two dispersions by separation -------------------------------------------
#
# The redshift-space multipoles above are the real-space clustering convolved with the distribution of the pairwise
# line-of-sight velocity (the streaming picture); its first two moments by separation are the mean infall v12(r), the
# dispersion along the pair sigma_par(r) (the fingers of god) and across it sigma_perp(r).  ``ops.pair_velocity_sums``
# sums them in exact integers over the pair counter's pairs; what follows quantises velocities on one scale, and does
# the host arithmetic.  Line-of-sight pairwise velocities and the full pairwise velocity distribution, per-bin histograms
# of ``u``, weighted pairs in general, batched, sharded and owned-storage variants and a loss are not built.

def _moment_words(sums: torch.Tensor, m: int) -> torch.Tensor:
    """Moment ``m`` of ``sums [..., 3, 2]`` (int64 words lo, hi) as float64: ``hi * 2^32 + lo``, rounded once."""
    return sums[..., m, 1].to(torch.float64) * 4294967296.0 + sums[..., m, 0].to(torch.float64)


def pairwise_velocity_moments(counts, sums, value_scale, edges=None) -> Dict:
    """``v12``, ``sigma_par``, ``sigma_perp`` and ``mean_square_par`` per separation bin from the exact integers of
    ``ops.pair_velocity_sums``: ``counts [..., nb]`` and ``sums [..., nb, 3, 2]`` (the moments S1, R2, T2 as words lo,
    hi), host arithmetic in float64.  ``value_scale`` (a number, or a tensor that broadcasts against ``[..., nb]``) is
    the scale the velocities were quantised on; with ``step = value_scale / 2^20``

    * ``v12 = step S1 / counts``: the mean relative velocity along the pair, negative for infall;
    * ``sigma_par = step sqrt(R2 / counts - (S1 / counts)^2)``: the dispersion along the pair;
    * ``sigma_perp = step sqrt((T2 - R2) / (2 counts))``: the dispersion per axis across it (``T2 - R2`` is taken in
      the integer words and clipped at 0: the rounding of ``iu`` can leave it a few units negative);
    * ``mean_square_par = step^2 R2 / counts``.

    All ``nan`` where ``counts == 0``.  The dict carries ``counts`` too, and ``r_lo``, ``r_hi`` when ``edges`` (the
    ``nb + 1`` radii) are given."""
    what = "pairwise_velocity_moments"
    counts, sums = torch.as_tensor(counts).detach().cpu(), torch.as_tensor(sums).detach().cpu()
    if counts.dim() < 1 or tuple(sums.shape) != tuple(counts.shape) + (3, 2) or sums.dtype != torch.int64:
        raise ValueError(f"{what}: sums must be int64 {list(counts.shape) + [3, 2]} for counts {tuple(counts.shape)}, "
                         f"got {sums.dtype} {tuple(sums.shape)}")
    if torch.is_tensor(value_scale):
        scale = value_scale.detach().cpu().to(torch.float64)
    else:
        scale = torch.tensor(ops._check_value_scale(value_scale, what), dtype=torch.float64)
    if not bool((scale > 0).all()) or not bool(torch.isfinite(scale).all()):
        raise ValueError(f"{what}: value_scale must be positive and finite")
    step = scale / float(1 << _lib.WEIGHT_BITS)
    c = counts.to(torch.float64)
    c = torch.where(c > 0, c, torch.full_like(c, float("nan")))
    s1, r2 = _moment_words(sums, 0), _moment_words(sums, 1)
    across = ((sums[..., 2, 1] - sums[..., 1, 1]).to(torch.float64) * 4294967296.0
              + (sums[..., 2, 0] - sums[..., 1, 0]).to(torch.float64))
    mean = s1 / c
    out = {"counts": counts,
           "v12": step * mean,
           "sigma_par": step * torch.sqrt(torch.clamp(r2 / c - mean * mean, min=0.0)),
           "sigma_perp": step * torch.sqrt(torch.clamp(across, min=0.0) / (2.0 * c)),
           "mean_square_par": step * step * r2 / c}
    if edges is not None:
        r = torch.as_tensor(edges).detach().to(device="cpu", dtype=torch.float32).reshape(-1).to(torch.float64)
        if r.numel() != counts.shape[-1] + 1:
            raise ValueError(f"{what}: {r.numel()} edges for {counts.shape[-1]} bins")
        out["r_lo"], out["r_hi"] = r[:-1], r[1:]
    return out


def _check_pairwise_edges(what: str, box_size, edges):
    e = ops.check_pair_count_edges(edges, box_size, what)
    if len(e) - 1 > _lib.PAIR_VELOCITY_MAX_BINS:
        raise ValueError(f"{what}: edges must hold nb + 1 radii with 1 <= nb <= {_lib.PAIR_VELOCITY_MAX_BINS}, got "
                         f"{len(e)} values")
    return e


def _check_dt(what: str, dt) -> float:
    if isinstance(dt, bool) or not isinstance(dt, (int, float)) or not math.isfinite(dt) or not dt > 0:
        raise ValueError(f"{what}: dt must be a positive finite number, got {dt!r}")
    return float(dt)


def _step_velocities(pos: torch.Tensor, pos_prev: torch.Tensor, dt: float, box_size: float) -> torch.Tensor:
    """``minimum_image(pos - pos_prev) / dt`` in float64, the velocity of :func:`momentum_power_spectrum`."""
    box = float(box_size)
    d = (pos - pos_prev).to(torch.float64)
    return (d - box * torch.round(d / box)) / float(dt)


def _scale_on_device(value_scale, velocities, what: str):
    """The value scale of a call: the given one checked, or the largest ``|v|`` over all the given velocity tensors as
    a 0-d float64 device tensor (not read on the host)."""
    if value_scale is not None:
        return ops._check_value_scale(value_scale, what)
    m = torch.stack([ops._max_abs_scale(v) for v in velocities]).max()
    return m


def pairwise_velocities(pos: torch.Tensor, box_size: float, edges, vel: Optional[torch.Tensor] = None,
                        pos_prev: Optional[torch.Tensor] = None, dt: Optional[float] = None,
                        pos_b: Optional[torch.Tensor] = None, vel_b: Optional[torch.Tensor] = None,
                        pos_b_prev: Optional[torch.Tensor] = None, value_scale=None) -> Dict:
    """The mean pairwise velocity ``v12(r)`` and the dispersions ``sigma_par(r)``, ``sigma_perp(r)`` of ``pos`` (``[N, 3]``
    or ``[T, N, 3]``) over the pairs :func:`correlation_function` counts for ``edges`` (at most 64 bins), from the exact
    integer sums of ``ops.pair_velocity_sums``.  Exactly one of ``vel`` (velocities in the shape of ``pos``) or
    ``pos_prev`` with ``dt`` gives the velocities; the second form is ``minimum_image(pos - pos_prev) / dt`` in float64,
    as in :func:`momentum_power_spectrum`.  With ``pos_b`` (and ``vel_b`` or ``pos_b_prev``, matching the form) the
    cross pairs of the two sets, and only those: ``u`` is then the velocity of the ``pos_b`` particle relative to the
    ``pos`` one along their separation.  ``v12 < 0`` is infall.

    The velocities are quantised by ``ops.quantize_weights`` on ``value_scale`` (2^20 steps per scale); the default is
    the largest ``|v|`` of anything in the call, taken on the device.  One runaway particle therefore coarsens the step
    for all the others; a given ``value_scale`` is the remedy: velocities beyond it are clamped to it.  Returns the
    dict of :func:`pairwise_velocity_moments` with ``r_lo``, ``r_hi`` and ``value_scale`` (float64, 0-d).  Everything
    is summed on the device of ``pos`` without a host synchronisation and comes back in one transfer."""
    what = "pairwise_velocities"
    _check_pairwise_edges(what, box_size, edges)
    moving = pos_prev is not None
    if (vel is not None) == moving:
        raise ValueError(f"{what}: exactly one of vel or (pos_prev, dt) gives the velocities")
    if moving:
        dt = _check_dt(what, dt)
    elif dt is not None:
        raise ValueError(f"{what}: dt goes with pos_prev")
    if pos_b is None:
        if vel_b is not None or pos_b_prev is not None:
            raise ValueError(f"{what}: vel_b and pos_b_prev go with pos_b")
    elif (vel_b is not None) == moving or (pos_b_prev is not None) != moving:
        raise ValueError(f"{what}: pos_b takes vel_b when vel is given, pos_b_prev when pos_prev is")
    sets, vels = [], []
    for name, cur, v, prev in (("pos", pos, vel, pos_prev), ("pos_b", pos_b, vel_b, pos_b_prev)):
        if cur is None:
            sets.append(None)
            continue
        frames = _f32_frames(cur, name, what)
        if cur.dim() != pos.dim() or frames.shape[0] != (pos.shape[0] if pos.dim() == 3 else 1):
            raise ValueError(f"{what}: {name} {tuple(cur.shape)} does not go with pos {tuple(pos.shape)}")
        other = prev if moving else v
        if not torch.is_tensor(other) or tuple(other.shape) != tuple(cur.shape):
            raise ValueError(f"{what}: the {'previous positions' if moving else 'velocities'} of {name} must have its "
                             f"shape {tuple(cur.shape)}")
        other = other.to(frames.device).reshape(frames.shape)
        vels.append(_step_velocities(frames, _f32_frames(other, name + "_prev", what), dt, box_size) if moving
                    else other.to(torch.float64))
        sets.append(frames)
    scale = _scale_on_device(value_scale, vels, what)
    q = [ops.quantize_weights(v, scale) for v in vels]
    counts, sums = ops.pair_velocity_sums(sets[0], q[0], box_size, edges, sets[1], q[1] if len(q) > 1 else None)
    scale_t = scale.reshape(1).to(counts.device) if torch.is_tensor(scale) else \
        torch.tensor([scale], dtype=torch.float64).to(counts.device)
    counts, sums, scale_t = _to_host(counts, sums, scale_t.to(torch.float64))
    if pos.dim() == 2:
        counts, sums = counts[0], sums[0]
    out = pairwise_velocity_moments(counts, sums, scale_t[0], edges)
    out["value_scale"] = scale_t[0]
    return out


def rollout_pairwise_velocities(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor],
                                box_size: float, edges, dt: float, frames: Optional[Sequence[int]] = None,
                                value_scale=None) -> Dict:
    """Pairwise velocity statistics of a rollout against the truth, for the dicts ``rollout.rollout`` returns
    (``Coordinates [T, N, 3]``): what :func:`rollout_redshift_correlation`'s ``quadrupole_ratio`` leaves unexplained --
    whether the mean infall, the dispersion along the pair or the one across it is off, down to scales no mesh follows.
    Every judged frame of either side takes its velocities from its own step, ``minimum_image`` of the frame minus the
    frame before in the same dict, over ``dt`` (:func:`pairwise_velocities`).  ``frames``: the frame numbers to judge
    (default: every frame from 1 on that both hold); frame 0 has no predecessor: its statistics are ``nan`` and its
    counts 0.  One ``value_scale`` serves both sides and all frames (default: the largest ``|v|`` among them, on the
    device; a runaway predicted particle coarsens the step of everything, a given scale clamps it instead).  Per
    selected frame (CPU, float64 ``[F, nb]``):

    * ``v12_pred``, ``v12_true``, ``sigma_par_pred``, ``sigma_par_true``, ``sigma_perp_pred``, ``sigma_perp_true``;
    * ``counts_pred``, ``counts_true`` (int64 ``[F, nb]``);
    * ``infall_ratio``: ``v12_pred / v12_true``; ``dispersion_ratio``: ``sigma_par_pred / sigma_par_true``,

    plus ``frames``, ``r_lo``, ``r_hi`` (``[nb]``) and ``value_scale``.  No cross term: the relative velocity of a
    predicted and a true particle judges nothing.  No host synchronisation per frame; one transfer."""
    what = "rollout_pairwise_velocities"
    e = _check_pairwise_edges(what, box_size, edges)
    dt = _check_dt(what, dt)
    if value_scale is not None:
        ops._check_value_scale(value_scale, what)
    pc = rollout_data["Coordinates"]
    dev = pc.device
    truth = {"Coordinates": ground_truth["Coordinates"].to(dev)}       # moved once: the predecessors come from it too
    if frames is None:
        frames = range(1, min(len(pc), len(truth["Coordinates"])))
    cp, ct, sel = _rollout_frames(rollout_data, truth, frames, what)
    rows = [i for i, f in enumerate(sel) if f > 0]
    if not rows:
        raise ValueError(f"{what}: no selected frame has a predecessor (frames {sel})")
    prev = torch.tensor([sel[i] - 1 for i in rows], dtype=torch.int64).to(dev)
    at = torch.tensor(rows, dtype=torch.int64).to(dev)
    pos, vels = [], []
    for cur, source in ((cp, pc), (ct, truth["Coordinates"])):
        pos.append(_f32_frames(cur.index_select(0, at), "Coordinates", what))
        vels.append(_step_velocities(pos[-1], _f32_frames(source.index_select(0, prev), "Coordinates", what), dt,
                                     box_size))
    scale = _scale_on_device(value_scale, vels, what)
    counted = [ops.pair_velocity_sums(p, ops.quantize_weights(v, scale), box_size, edges) for p, v in zip(pos, vels)]
    scale_t = scale.reshape(1).to(dev) if torch.is_tensor(scale) else torch.tensor([scale], dtype=torch.float64).to(dev)
    got_c, got_s, scale_t = _to_host(torch.stack([c for c, _ in counted]), torch.stack([s for _, s in counted]),
                                     scale_t.to(torch.float64))
    nb = len(e) - 1
    counts = torch.zeros((2, len(sel), nb), dtype=torch.int64)
    sums = torch.zeros((2, len(sel), nb, 3, 2), dtype=torch.int64)
    counts[:, rows], sums[:, rows] = got_c, got_s
    out = {"frames": sel, "value_scale": scale_t[0]}
    for i, name in enumerate(("pred", "true")):
        res = pairwise_velocity_moments(counts[i], sums[i], scale_t[0], edges)     # frame 0: counts 0, hence nan
        out[f"counts_{name}"] = res["counts"]
        for key in ("v12", "sigma_par", "sigma_perp"):
            out[f"{key}_{name}"] = res[key]
    out["r_lo"], out["r_hi"] = res["r_lo"], res["r_hi"]
    out["infall_ratio"] = out["v12_pred"] / out["v12_true"]
    out["dispersion_ratio"] = out["sigma_par_pred"] / out["sigma_par_true"]
    return out


# ---- gas fields on the mesh: thermal and momentum spectra ---------------------------------------------------------------
#
# ``ops.mass_assign_weighted`` deposits per-particle values in exact integers; what follows forms the fields' spectra with
# the pieces above.  The weighted shot noise (sums over the particles) is formed on the device in float64 and travels
# with the shell sums in the one transfer.  Sharded and batched variants, an owned-storage variant (``dist.
# assemble_frames`` first), redshift-space gas fields and interlaced thermal and momentum spectra (the matter spectra have
# both: the section above) are not built.

def _scalar_values(values: torch.Tensor, frames: torch.Tensor, pos: torch.Tensor, name: str, what: str) -> torch.Tensor:
    """Scalar per-particle ``values`` (``[N]`` / ``[N, 1]`` for ``pos [N, 3]``, with a leading ``T`` for frames) -> ``[F, N]``."""
    lead = tuple(pos.shape[:-1])
    if not torch.is_tensor(values) or tuple(values.shape) not in (lead, lead + (1,)):
        raise ValueError(f"{what}: {name} must be {list(lead)} or {list(lead) + [1]} (one scalar per particle), got "
                         f"{tuple(values.shape) if torch.is_tensor(values) else values!r}")
    return values.reshape(frames.shape[:2])


def _frame_fields(pos: torch.Tensor, values: torch.Tensor, box_size: float, mesh: int, order: int) -> torch.Tensor:
    """The fields of ``values [F, N, C]`` at ``pos [F, N, 3]`` in value units (float64 ``[F, C, M, M, M]``, the cell mean is
    the mean value), every frame quantised over its own largest ``|value|``: a frame's field does not depend on the
    frames it is computed with."""
    v64 = values.to(torch.float64)
    scale = v64.abs().amax(dim=(1, 2))
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    q = ops.quantize_weights(v64 / scale[:, None, None], 1.0)
    grid = ops.mass_assign_weighted(pos, q, box_size, mesh, order)
    per = mesh ** 3 / (pos.shape[1] * _lib.MASS_ASSIGN_Q ** 3)
    return grid.to(torch.float64) * (scale * per)[:, None, None, None, None]


def _field_transform(pos: torch.Tensor, values: torch.Tensor, box_size: float, mesh: int, order: int, normalise: str):
    """-> (``rfftn`` of the scalar field of ``values [F, N]`` at ``pos [F, N, 3]``, complex128 ``[F, M, M, M/2 + 1]``; its
    shot noise float64 ``[F]``), on the device.  ``"mean"``: the field over its mean, minus one, ``L^3 sum a^2 / (sum
    a)^2``; ``"none"``: the field in value units (cell mean = mean value), ``L^3 sum value^2 / N^2``."""
    n, vol = pos.shape[1], float(box_size) ** 3
    v64 = values.to(torch.float64)
    s2, s1 = (v64 * v64).sum(dim=1), v64.sum(dim=1)
    field = _frame_fields(pos, values.unsqueeze(-1), box_size, mesh, order)[:, 0]
    if normalise == "mean":
        field = field / (s1 / float(n))[:, None, None, None] - 1.0
        shot = vol * s2 / (s1 * s1)
    else:
        shot = vol * s2 / float(n) ** 2
    return torch.fft.rfftn(field, dim=(-3, -2, -1)), shot


def field_sums_on_device(pos, values, pos_b, values_b, box_size: float, mesh: int, k_edges, order: int, normalise: str):
    """The device part of :func:`field_power_spectrum` for ``pos [F, N, 3]``, ``values [F, N]`` (and the second set, or
    ``None``): device tensors ``modes [F, nb]``, ``sums [F, 4, nb]`` (``ops.power_bins``) and the shot noise of the two
    fields ``[2, F]`` (the first twice without a second set).  No host synchronisation."""
    a, shot_a = _field_transform(pos, values, box_size, mesh, order, normalise)
    b, shot_b = (None, shot_a) if pos_b is None else _field_transform(pos_b, values_b, box_size, mesh, order, normalise)
    modes, sums = ops.power_bins(a, mesh, order, k_edges, b)
    return modes, sums, torch.stack([shot_a, shot_b])


def field_power_spectrum(pos: torch.Tensor, values: torch.Tensor, box_size: float, mesh: int, k_edges=None,
                         pos_b: Optional[torch.Tensor] = None, values_b: Optional[torch.Tensor] = None, order: int = 2,
                         normalise: str = "mean", subtract_shot_noise: bool = True) -> Dict:
    """The power spectrum of the field of scalar per-particle ``values`` (``[N]`` / ``[N, 1]`` at ``pos [N, 3]``, or with a
    leading ``T``): the thermal-energy field when the values are internal energies.  Deposited in exact integers
    (``ops.mass_assign_weighted``), deconvolved by the window of ``order``.  ``normalise="mean"``: the spectrum of ``field /
    mean(field) - 1`` (values of 1 give :func:`power_spectrum`), with the shot noise ``L^3 sum a_i^2 / (sum a_i)^2``;
    ``"none"``: the spectrum of the field in value units (its cell mean is the mean value), shot noise ``L^3 sum value_i^2
    / N^2``.  With ``pos_b`` and ``values_b`` also the second field's spectrum and the cross spectrum.  Returns the dict
    of :func:`power_spectrum` plus ``shot_noise`` (and ``shot_noise_b``), float64 ``[]`` or ``[T]``; the shot noise is
    subtracted from the auto spectra when ``subtract_shot_noise``, ``r`` comes from the spectra before the subtraction.
    Everything is computed on the device without a host synchronisation and comes back in one transfer."""
    what = "field_power_spectrum"
    mesh, k_edges = _check_spectrum_arguments(what, box_size, mesh, k_edges, order)
    if normalise not in ("mean", "none"):
        raise ValueError(f"{what}: normalise must be 'mean' or 'none', got {normalise!r}")
    if (pos_b is None) != (values_b is None):
        raise ValueError(f"{what}: pos_b and values_b go together")
    frames_a = _frames3(pos, "pos", what)
    val_a = _scalar_values(values, frames_a, pos, "values", what)
    frames_b = val_b = None
    if pos_b is not None:
        frames_b = _frames3(pos_b, "pos_b", what)
        if pos_b.dim() != pos.dim() or frames_b.shape[0] != frames_a.shape[0]:
            raise ValueError(f"{what}: pos_b {tuple(pos_b.shape)} does not go with pos {tuple(pos.shape)}")
        val_b = _scalar_values(values_b, frames_b, pos_b, "values_b", what)
    modes, sums, shot = _to_host(*field_sums_on_device(frames_a, val_a, frames_b, val_b, box_size, mesh, k_edges, order,
                                                       normalise))
    single = pos.dim() == 2
    if single:
        modes, sums = modes[0], sums[0]
    out = spectra_from_sums(modes, sums, 1, None if frames_b is None else 1, box_size, mesh, k_edges, False)
    sa, sb = (shot[0, 0], shot[1, 0]) if single else (shot[0], shot[1])
    out["shot_noise"] = sa.clone()
    if frames_b is not None:
        out["shot_noise_b"] = sb.clone()
    if subtract_shot_noise:
        out["power"] = out["power"] - (sa if single else sa[:, None])
        if frames_b is not None:
            out["power_b"] = out["power_b"] - (sb if single else sb[:, None])
            out["transfer"] = torch.sqrt(out["power"] / out["power_b"])
    return out


def _long_weights(mesh: int, device):
    """``n_c / |n|`` of every mode of the rfft array (float64 ``[3, M, M, M/2 + 1]``; 0 at ``n = 0``), over the signed
    integer frequencies of ``cgnn_power_bins``: ``n`` in ``(-M/2, M/2]`` on the two full axes, ``[0, M/2]`` on the last."""
    i = torch.arange(mesh, dtype=torch.float64, device=device)
    full = torch.where(i <= mesh // 2, i, i - mesh)
    half = torch.arange(mesh // 2 + 1, dtype=torch.float64, device=device)
    nx, ny, nz = full[:, None, None], full[None, :, None], half[None, None, :]
    norm = torch.sqrt(nx * nx + ny * ny + nz * nz)
    inv = torch.where(norm > 0, 1.0 / norm, torch.zeros_like(norm))
    return torch.stack([(nx * inv).expand_as(norm), (ny * inv).expand_as(norm), (nz * inv).expand_as(norm)])


def momentum_sums_on_device(pos_prev: torch.Tensor, pos: torch.Tensor, dt: float, box_size: float, mesh: int, k_edges, order: int):
    """The device part of :func:`momentum_power_spectrum`, without a host synchronisation.  For frames ``[F, N, 3]``: device tensors ``modes [F, nb]``, ``total [F, nb]`` and ``div [F, nb]`` (the shell sums of
    ``sum_c |p_c(k)|^2`` and of ``|a_L(k)|^2``), ``k_sums [F, nb]`` (row 3 of ``ops.power_bins``) and the shot noise ``[F]``."""
    box = float(box_size)
    d = (pos - pos_prev).to(torch.float64)
    vel = (d - box * torch.round(d / box)) / float(dt)                       # the minimum image
    shot = box ** 3 * (vel * vel).sum(dim=(1, 2)) / float(pos.shape[1]) ** 2
    field = _frame_fields(pos, vel, box_size, mesh, order)                      # [F, 3, M, M, M]
    pk = torch.fft.rfftn(field, dim=(-3, -2, -1))                               # [F, 3, M, M, M/2 + 1]
    del field
    plan = ops.PowerPlan.of(mesh, k_edges, pos.device)
    total = None
    for c in range(3):
        modes, sums = ops.power_bins(pk[:, c].contiguous(), mesh, order, k_edges, None, plan)
        total = sums[:, 0] if total is None else total + sums[:, 0]
    a_long = (pk * _long_weights(mesh, pos.device)).sum(dim=1)
    modes, sums = ops.power_bins(a_long.contiguous(), mesh, order, k_edges, None, plan)
    return modes, total, sums[:, 0], sums[:, 3], shot


def momentum_power_spectrum(pos_prev: torch.Tensor, pos: torch.Tensor, dt: float, box_size: float, mesh: int,
                            k_edges=None, order: int = 2, subtract_shot_noise: bool = True) -> Dict:
    """The power spectrum of the momentum field of a frame ``pos`` (``[N, 3]`` or ``[T, N, 3]``) whose velocities are
    ``minimum_image(pos - pos_prev) / dt``, and its split into the longitudinal (divergence) and the transverse (curl)
    part.  One three-channel deposit at ``pos`` (``ops.mass_assign_weighted``; the field in velocity units, its cell mean
    the mean velocity), three ``rfftn``.  Returns (CPU, float64 / int64, ``[nb]`` or ``[T, nb]``) ``k_lo``, ``k_hi``,
    ``k_mean``, ``modes`` and

    * ``power_total``: ``L^3 / M^6`` times the mean over the shell of ``sum_c |p_c(k)|^2 / W2``;
    * ``power_div``: likewise of ``|a_L|^2``, ``a_L = sum_c n_c p_c(k) / |n|`` over the signed integer frequencies
      (``a_L = 0`` at ``n = 0``, which is never counted);
    * ``power_curl = power_total - power_div``;
    * ``shot_noise``: ``L^3 sum |v_i|^2 / N^2``, subtracted from ``power_total`` (a third of it from ``power_div``, the
      rest from ``power_curl``) when ``subtract_shot_noise``.

    No host synchronisation; one transfer."""
    what = "momentum_power_spectrum"
    mesh, k_edges = _check_spectrum_arguments(what, box_size, mesh, k_edges, order)
    if isinstance(dt, bool) or not (float(dt) > 0.0 and math.isfinite(float(dt))):
        raise ValueError(f"{what}: dt must be positive and finite, got {dt!r}")
    frames = _frames3(pos, "pos", what)
    if tuple(pos_prev.shape) != tuple(pos.shape):
        raise ValueError(f"{what}: pos_prev {tuple(pos_prev.shape)} and pos {tuple(pos.shape)} differ in shape")
    prev = _frames3(pos_prev, "pos_prev", what)
    modes, total, div, k_sums, shot = momentum_sums_on_device(prev, frames, dt, box_size, mesh, k_edges, order)
    nan = torch.full_like(total, float("nan"))
    modes, sums, shot = _to_host(modes, torch.stack([total, div, nan, k_sums], dim=1), shot)
    return _momentum_spectra(modes, sums, shot, box_size, mesh, k_edges, subtract_shot_noise, pos.dim() == 2)


def _momentum_spectra(modes, sums, shot, box_size, mesh, k_edges, subtract_shot_noise: bool, single: bool) -> Dict:
    """Host arithmetic of :func:`momentum_power_spectrum` from ``modes [F, nb]``, ``sums [F, 4, nb]`` (rows: total, div,
    unused, ``sqrt(n2)``) and ``shot [F]``."""
    # the two rows go through spectra_from_sums as a pair of auto spectra
    sp = spectra_from_sums(modes, sums, 1, 1, box_size, mesh, k_edges, False)
    total, div = sp["power"], sp["power_b"]
    if subtract_shot_noise:
        total, div = total - shot[:, None], div - shot[:, None] / 3.0
    out = {"k_lo": sp["k_lo"], "k_hi": sp["k_hi"], "k_mean": sp["k_mean"], "modes": sp["modes"], "power_total": total,
           "power_div": div, "power_curl": total - div, "shot_noise": shot}
    if single:
        out = {k: (v if k in ("k_lo", "k_hi") else v[0].clone()) for k, v in out.items()}
    return out


def rollout_gas_spectra(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], box_size: float,
                        mesh: int, dt: Optional[float] = None, k_edges=None, frames: Optional[Sequence[int]] = None,
                        order: int = 2) -> Dict:
    """Gas statistics of a rollout against the truth in Fourier space, for the dicts ``rollout.rollout`` returns
    (``Coordinates [T, N, 3]``, ``InternalEnergy [T, N(, 1)]``).  ``frames``: the frame numbers to judge (default: every
    frame both hold).  Per selected frame (``[F, nb]``, CPU, float64):

    * ``thermal_power_pred``, ``thermal_power_true``: the shot-noise-subtracted spectra of the internal-energy-weighted
      field over its mean (:func:`field_power_spectrum`, ``normalise="mean"``), positions and weights of the same frame;
      ``thermal_cross``, ``thermal_r`` (``|r| <= 1``) and ``thermal_transfer`` (``sqrt(pred / true)``, ``nan`` where a
      subtracted spectrum is negative) of the predicted against the true field;
    * ``thermal_density_r_pred``, ``thermal_density_r_true``: the correlation coefficient of that field with the density
      contrast of the same frame ("is the hot gas where the dense gas is");
    * with ``dt``: ``momentum_div_pred``, ``momentum_div_true``, ``momentum_curl_pred``, ``momentum_curl_true``
      (:func:`momentum_power_spectrum`, shot noise subtracted), velocities from the frame before in the same dict;
      frame 0 has no predecessor and is ``nan``,

    plus ``frames``, ``k_lo``, ``k_hi``, ``k_mean`` and ``modes`` (``[nb]``).  Everything is computed on the device of the
    rollout without a host synchronisation per frame; the results come back in one transfer."""
    what = "rollout_gas_spectra"
    mesh, k_edges = _check_spectrum_arguments(what, box_size, mesh, k_edges, order)
    if dt is not None and (isinstance(dt, bool) or not (float(dt) > 0.0 and math.isfinite(float(dt)))):
        raise ValueError(f"{what}: dt must be positive and finite, got {dt!r}")
    pc = rollout_data["Coordinates"]
    dev = pc.device
    truth = {"Coordinates": ground_truth["Coordinates"].to(dev)}       # moved once: the predecessors come from it too
    pe, te = rollout_data["InternalEnergy"].to(dev), ground_truth["InternalEnergy"].to(dev)
    cp, ct, sel, ep, et = _rollout_frames(rollout_data, truth, frames, what, also=(pe, te))
    n, nf = cp.shape[1], len(sel)
    if pe.numel() != len(pe) * n or te.numel() != len(te) * n:
        raise ValueError(f"{what}: InternalEnergy does not hold one value per particle and frame")
    ep, et = ep.reshape(nf, n), et.reshape(nf, n)
    moving = None
    rows = [i for i, f in enumerate(sel) if f > 0]
    if dt is not None and rows:
        prev = torch.tensor([sel[i] - 1 for i in rows], dtype=torch.int64).to(dev)
        rows = torch.tensor(rows, dtype=torch.int64).to(dev)
        moving = (rows, pc.index_select(0, prev), truth["Coordinates"].index_select(0, prev))
    modes, sums, extra = _to_host(*gas_sums_on_device(cp, ct, ep, et, box_size, mesh, k_edges, order, dt, moving))
    return _gas_spectra(modes, sums, extra, sel, box_size, mesh, dt, k_edges)


def gas_sums_on_device(cp, ct, ep, et, box_size: float, mesh: int, k_edges, order: int, dt=None, moving=None):
    """The device part of :func:`rollout_gas_spectra` for the selected predicted and true frames ``cp``, ``ct [F, N, 3]``
    and their internal energies ``ep``, ``et [F, N]``: ``modes [F, nb]``, ``sums [3 or 5, F, 4, nb]`` (thermal pred x true,
    thermal x density of the predicted and of the true frames, and with ``moving`` the momentum rows of the two) and
    ``extra [2 or 4, F]`` (the shot noises).  ``moving``: ``None``, or ``(rows, prev_p, prev_t)``, the (device) indices of
    the selected frames that have a predecessor and those predecessors ``[len(rows), N, 3]``.  No host synchronisation."""
    dev = cp.device
    nf, nb = cp.shape[0], len(k_edges) - 1
    plan = ops.PowerPlan.of(mesh, k_edges, dev)
    fp, shot_p = _field_transform(cp, ep, box_size, mesh, order, "mean")
    ft, shot_t = _field_transform(ct, et, box_size, mesh, order, "mean")
    modes, thermal = ops.power_bins(fp, mesh, order, k_edges, ft, plan)
    _, with_p = ops.power_bins(fp, mesh, order, k_edges, _contrast_modes(cp, box_size, mesh, order), plan)
    _, with_t = ops.power_bins(ft, mesh, order, k_edges, _contrast_modes(ct, box_size, mesh, order), plan)
    sums, extra = [thermal, with_p, with_t], [shot_p, shot_t]
    if moving is not None:
        rows, prev_p, prev_t = moving
        for cur, prev in ((cp, prev_p), (ct, prev_t)):
            _, total, div, k_sums, shot = momentum_sums_on_device(prev, cur.index_select(0, rows), dt, box_size, mesh,
                                                                  k_edges, order)
            block = torch.full((nf, 4, nb), float("nan"), dtype=torch.float64, device=dev)
            block.index_copy_(0, rows, torch.stack([total, div, torch.full_like(total, float("nan")), k_sums], dim=1))
            shot_all = torch.full((nf,), float("nan"), dtype=torch.float64, device=dev)
            shot_all.index_copy_(0, rows, shot)
            sums.append(block)
            extra.append(shot_all)
    return modes, torch.stack(sums), torch.stack(extra)


def _gas_spectra(modes, sums, extra, sel, box_size, mesh, dt, k_edges) -> Dict:
    """Host arithmetic of :func:`rollout_gas_spectra`."""
    nf, nb = modes.shape
    sp = spectra_from_sums(modes, sums[0], 1, 1, box_size, mesh, k_edges, False)
    power_p, power_t = sp["power"] - extra[0][:, None], sp["power_b"] - extra[1][:, None]
    out = {"frames": sel, "k_lo": sp["k_lo"], "k_hi": sp["k_hi"], "k_mean": sp["k_mean"][0].clone(),
           "modes": sp["modes"][0].clone(), "thermal_power_pred": power_p, "thermal_power_true": power_t,
           "thermal_cross": sp["cross"], "thermal_r": sp["r"], "thermal_transfer": torch.sqrt(power_p / power_t),
           "thermal_shot_noise_pred": extra[0].clone(), "thermal_shot_noise_true": extra[1].clone()}
    for which, name in ((1, "pred"), (2, "true")):
        out["thermal_density_r_" + name] = spectra_from_sums(modes, sums[which], 1, 1, box_size, mesh, k_edges, False)["r"]
    if dt is not None:
        for which, name in ((3, "pred"), (4, "true")):
            if len(sums) > 3:
                mom = _momentum_spectra(modes, sums[which], extra[which - 1], box_size, mesh, k_edges, True, False)
                out["momentum_div_" + name], out["momentum_curl_" + name] = mom["power_div"], mom["power_curl"]
            else:
                nan = torch.full((nf, nb), float("nan"), dtype=torch.float64)
                out["momentum_div_" + name], out["momentum_curl_" + name] = nan, nan.clone()
    return out


def default_linking_length(n: int, box_size: float, b: float = 0.2) -> float:
    """``b`` mean interparticle spacings: ``b * box_size / n ** (1 / 3)``."""
    if int(n) < 1:
        raise ValueError(f"default_linking_length: n must be at least 1, got {n!r}")
    return float(b) * float(box_size) / float(n) ** (1.0 / 3.0)


def default_size_edges(n: int, min_members: int = 20) -> list:
    """Doubling group-size edges ``min_members, 2 min_members, 4 min_members, ...`` up to the first value above ``n``
    (at least two edges, so that there is a bin): no group of ``n`` particles lies beyond the last one."""
    if isinstance(min_members, bool) or int(min_members) != min_members or int(min_members) < 1:
        raise ValueError(f"default_size_edges: min_members must be a whole number of at least 1, got {min_members!r}")
    edges = [int(min_members)]
    while len(edges) < 2 or edges[-1] <= int(n):
        edges.append(2 * edges[-1])
    return edges


def halo_centres(root_pos, size, disp, box_size: float) -> torch.Tensor:
    """The centres of groups from the sums of ``ops.fof_catalogue``, on the host in float64: ``(pos[root] + disp / size *
    L / 2^30) mod L`` for ``root_pos [H, 3]``, ``size [H]``, ``disp [H, 3]`` (int64, displacements from the root under
    the minimum image in units of ``L / 2^30``), with ``L`` the float32 value of ``box_size`` the kernels use.  The
    mean of minimum-image displacements from one member is the centre of mass of a group that spans less than half
    the box, wherever it lies (a group across a box corner has its centre at the corner); a group that spans more
    than half the box has no meaningful centre."""
    box = float(torch.tensor(float(box_size), dtype=torch.float32))
    root_pos = torch.as_tensor(root_pos).detach().to(device="cpu", dtype=torch.float64).reshape(-1, 3)
    size = torch.as_tensor(size).detach().to(device="cpu", dtype=torch.float64).reshape(-1, 1)
    disp = torch.as_tensor(disp).detach().to(device="cpu", dtype=torch.float64).reshape(-1, 3)
    return torch.remainder(root_pos + disp / size * (box / _lib.FOF_DISP_UNITS), box)


def halo_catalogue(pos: torch.Tensor, box_size: float, linking_length: Optional[float] = None,
                   min_members: int = 20) -> Dict:
    """The friends-of-friends groups of one frame ``pos [N, 3]`` with at least ``min_members`` members
    (``linking_length``: default :func:`default_linking_length`, 0.2 mean spacings).  Returns on the CPU

    * ``labels`` int32 ``[N]``: every particle's group, named by its smallest member (``ops.fof_labels``);
    * ``root`` int64 ``[H]``, ``size`` int64 ``[H]``: the listed groups, sorted by size descending, then by root
      ascending;  ``centre`` float64 ``[H, 3]``: :func:`halo_centres` (a group that spans more than half the box has no
      meaningful centre).

    The number of groups is only known on the device: this function synchronises once (``nonzero``) after the kernels
    and before its single transfer.  Positions only: no velocities (unbinding: :func:`halo_binding`; profiles and spherical-overdensity
    masses: :func:`halo_profiles`); one box, no spatial shards (``dist.assemble_frames`` first)."""
    what = "halo_catalogue"
    if pos.dim() != 2 or pos.shape[-1] != 3 or pos.shape[0] < 1:
        raise ValueError(f"{what}: pos must be one frame [N, 3] with N >= 1, got {tuple(pos.shape)}")
    if isinstance(min_members, bool) or int(min_members) != min_members or int(min_members) < 1:
        raise ValueError(f"{what}: min_members must be a whole number of at least 1, got {min_members!r}")
    n = pos.shape[0]
    ll = default_linking_length(n, box_size) if linking_length is None else linking_length
    ops.check_linking_length(ll, box_size, what)
    labels = ops.fof_labels(pos, box_size, ll)
    size, disp, _ = ops.fof_catalogue(pos, labels, box_size)
    root = torch.nonzero(size >= int(min_members)).reshape(-1)                        # the one synchronisation
    rp = pos.index_select(0, root).to(torch.float32).contiguous()
    # one transfer: the float32 root positions travel as their bits among the integers
    packed = torch.cat([labels.to(torch.int64), root, size.index_select(0, root).to(torch.int64),
                        disp.index_select(0, root).reshape(-1), rp.view(torch.int32).to(torch.int64).reshape(-1)]).cpu()
    h = root.numel()
    labels_h = packed[:n].to(torch.int32)
    root_h, size_h = packed[n:n + h], packed[n + h:n + 2 * h]
    disp_h = packed[n + 2 * h:n + 5 * h].reshape(h, 3)
    rp_h = packed[n + 5 * h:].to(torch.int32).view(torch.float32).reshape(h, 3)
    order = sorted(range(h), key=lambda i: (-int(size_h[i]), int(root_h[i])))
    order = torch.tensor(order, dtype=torch.int64)
    return {"labels": labels_h, "root": root_h[order], "size": size_h[order],
            "centre": halo_centres(rp_h[order], size_h[order], disp_h[order], box_size)}


def halo_counts_on_device(frames: torch.Tensor, box_size: float, linking_length: float, size_edges) -> torch.Tensor:
    """The device part of :func:`halo_mass_function`: for ``frames [F, N, 3]`` an int64 ``[F, nb + 3]`` device tensor
    whose rows hold the ``nb`` group counts, then the number of groups with at least ``size_edges[0]`` members, the
    particles in them, and the size of the largest group.  No host synchronisation."""
    labels = ops.fof_labels(frames, box_size, linking_length)
    size, _, hist = ops.fof_catalogue(frames, labels, box_size, size_edges, want_disp=False)
    listed = size >= int(size_edges[0])
    members = torch.where(listed, size, torch.zeros_like(size)).sum(dim=1, dtype=torch.int64)
    return torch.cat([hist, listed.sum(dim=1, dtype=torch.int64).unsqueeze(1), members.unsqueeze(1),
                      size.max(dim=1).values.to(torch.int64).unsqueeze(1)], dim=1)


def _halo_arguments(n: int, box_size: float, linking_length, size_edges, what: str):
    ll = default_linking_length(n, box_size) if linking_length is None else linking_length
    ll = ops.check_linking_length(ll, box_size, what)
    return ll, ops.check_size_edges(default_size_edges(n) if size_edges is None else size_edges, what)


def halo_mass_function(pos: torch.Tensor, box_size: float, linking_length: Optional[float] = None,
                       size_edges=None) -> Dict:
    """The friends-of-friends mass function of ``pos [N, 3]`` (or of every frame of ``[T, N, 3]``): the number of groups
    by size.  ``linking_length``: default 0.2 mean spacings; ``size_edges``: ``nb + 1`` ascending whole numbers
    (default :func:`default_size_edges`, doubling from 20).  Returns on the CPU

    * ``size_lo``, ``size_hi`` int64 ``[nb]``; ``counts`` int64 ``[nb]`` (``[T, nb]``): the groups with ``size_lo <= size <
      size_hi``;
    * ``n_groups`` (int64) and ``fraction_in_groups`` (float64): the groups with at least ``size_edges[0]`` members
      (beyond the last edge too) and the fraction of the particles they hold;  ``largest``: the largest group.

    Everything is computed on the device of ``pos`` without a host synchronisation and comes back in one transfer.
    One box per call, positions only (no velocities -- unbinding: :func:`halo_binding`; no ``offsets``
    batches; no spatial shards: ``dist.assemble_frames`` first)."""
    what = "halo_mass_function"
    frames = _frames3(pos, "pos", what)
    n = frames.shape[1]
    ll, e = _halo_arguments(n, box_size, linking_length, size_edges, what)
    out = halo_counts_on_device(frames, box_size, ll, e).cpu()
    if pos.dim() == 2:
        out = out[0]
    nb = len(e) - 1
    edges = torch.tensor(e, dtype=torch.int64)
    return {"size_lo": edges[:-1].clone(), "size_hi": edges[1:].clone(), "counts": out[..., :nb].clone(),
            "n_groups": out[..., nb].clone(), "fraction_in_groups": out[..., nb + 1].to(torch.float64) / n,
            "largest": out[..., nb + 2].clone()}


def rollout_halo_statistics(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor],
                            box_size: float, linking_length: Optional[float] = None, size_edges=None,
                            frames: Optional[Sequence[int]] = None) -> Dict:
    """Halo statistics of a rollout against the truth, for the dicts ``rollout.rollout`` returns (``Coordinates [T, N,
    3]``).  ``frames``: the frame numbers to judge (default: every frame both hold).  Per selected frame (CPU):

    * ``counts_pred``, ``counts_true`` int64 ``[F, nb]``: the mass functions (:func:`halo_mass_function`);
    * ``n_groups_pred``, ``n_groups_true`` (int64 ``[F]``), ``fraction_pred``, ``fraction_true`` (float64): groups with
      at least ``size_edges[0]`` members and the fraction of the particles in them;
    * ``largest_pred``, ``largest_true`` (int64): the largest group,

    plus ``frames``, ``size_lo`` and ``size_hi``.  No synchronisation per frame; the results come back in one packed
    transfer.  The two frames' halos are not matched with each other here (:func:`rollout_halo_matching` does that); no
    velocities (whether the groups are bound: :func:`rollout_halo_binding`); one box, no spatial shards (an owned-storage rollout goes
    through ``dist.assemble_frames`` first)."""
    what = "rollout_halo_statistics"
    pc, tc, sel = _rollout_frames(rollout_data, ground_truth, frames, what)
    n = pc.shape[1]
    ll, e = _halo_arguments(n, box_size, linking_length, size_edges, what)
    out = torch.stack([halo_counts_on_device(pc, box_size, ll, e), halo_counts_on_device(tc, box_size, ll, e)]).cpu()
    nb = len(e) - 1
    edges = torch.tensor(e, dtype=torch.int64)
    res = {"frames": sel, "size_lo": edges[:-1].clone(), "size_hi": edges[1:].clone()}
    for which, name in enumerate(("pred", "true")):
        res["counts_" + name] = out[which, :, :nb].clone()
        res["n_groups_" + name] = out[which, :, nb].clone()
        res["fraction_" + name] = out[which, :, nb + 1].to(torch.float64) / n
        res["largest_" + name] = out[which, :, nb + 2].clone()
    return res


def _group_values(values, n: int, name: str, what: str):
    if values is None:
        return None
    if not torch.is_tensor(values) or values.dim() not in (1, 2) or values.shape[0] != n or values.is_complex() \
            or values.dtype == torch.bool or (values.dim() == 2 and not 1 <= values.shape[1] <= _lib.GROUP_SUMS_MAX_CHANNELS):
        raise ValueError(f"{what}: {name} must be a real tensor [{n}] or [{n}, C] with 1 <= C <= "
                         f"{_lib.GROUP_SUMS_MAX_CHANNELS}, got {tuple(values.shape) if torch.is_tensor(values) else values!r}")
    return values


def halo_matches(pos_a: torch.Tensor, pos_b: torch.Tensor, box_size: float, linking_length: Optional[float] = None,
                 min_members: int = 20, values_a: Optional[torch.Tensor] = None,
                 values_b: Optional[torch.Tensor] = None) -> Dict:
    """The friends-of-friends groups of frame ``pos_a [N, 3]`` (the truth, by convention) with at least ``min_members``
    members, each with its partner among the groups of ``pos_b [N, 3]``, a frame of the same particles under the same
    indices: the listed group of B that shares the most members with it (``ops.halo_match``; ties to the smaller root).
    Returns on the CPU, for every listed group of A sorted as :func:`halo_catalogue` sorts (size descending, then root
    ascending):

    * ``root``, ``size`` int64 ``[H]``, ``centre`` float64 ``[H, 3]``: as :func:`halo_catalogue`;
    * ``match_root`` int64 (-1 without a match), ``match_size`` and ``shared`` int64 (0 without), ``mutual`` bool: the
      partner, its size, the members the two share, and whether the group is its partner's best partner too;
    * ``match_centre`` float64 ``[H, 3]`` and ``centre_offset`` float64 ``[H]``: the partner's centre and the
      minimum-image distance of the two :func:`halo_centres`; ``nan`` without a match;
    * with ``values_a`` (``[N]`` or ``[N, C]``, ``C <= 4``, e.g. the temperature): ``mean_value`` float64 ``[H]`` (``[H,
      C]``), the mean over the group's members (``ops.fof_group_sums``: exact up to the quantisation to 2^-20 of the
      largest ``|value|``; int32 values are taken as quantised weights, in units of their scale); with ``values_b``:
      ``match_mean_value``, the partner's mean over its members in frame B, ``nan`` without a match.

    The number of groups is only known on the device: one synchronisation (``nonzero``) after the kernels and one
    transfer, as :func:`halo_catalogue`.  One box, one device, membership only (unbinding: :func:`halo_binding`), no merger trees over more than two frames; no spatial shards (``dist.assemble_frames`` first)."""
    what = "halo_matches"
    for pos, name in ((pos_a, "pos_a"), (pos_b, "pos_b")):
        if not torch.is_tensor(pos) or pos.dim() != 2 or pos.shape[-1] != 3 or pos.shape[0] < 1:
            raise ValueError(f"{what}: {name} must be one frame [N, 3] with N >= 1, got "
                             f"{tuple(pos.shape) if torch.is_tensor(pos) else pos!r}")
    if pos_a.shape != pos_b.shape:
        raise ValueError(f"{what}: the frames hold the same particles: pos_a is {tuple(pos_a.shape)}, pos_b "
                         f"{tuple(pos_b.shape)}")
    min_members = ops.check_min_members(min_members, what)
    n = pos_a.shape[0]
    ll = default_linking_length(n, box_size) if linking_length is None else linking_length
    ops.check_linking_length(ll, box_size, what)
    values = (_group_values(values_a, n, "values_a", what), _group_values(values_b, n, "values_b", what))
    pos_b = pos_b.to(pos_a.device)
    la, lb = ops.fof_labels(pos_a, box_size, ll), ops.fof_labels(pos_b, box_size, ll)
    sa, da, _ = ops.fof_catalogue(pos_a, la, box_size)
    sb, db, _ = ops.fof_catalogue(pos_b, lb, box_size)
    m_ab, s_ab, m_ba, _, _ = ops.halo_match(la, sa, lb, sb, min_members)
    sums = [None if v is None else ops.fof_group_sums(lab, v.to(pos_a.device))
            for lab, v in zip((la, lb), values)]
    root = torch.nonzero(sa >= min_members).reshape(-1)                               # the one synchronisation
    m = m_ab.index_select(0, root).to(torch.int64)
    has = m >= 0
    mc = m.clamp(min=0)
    mutual = has & (m_ba.index_select(0, mc).to(torch.int64) == root)
    h = root.numel()

    def bits(pos, idx):     # the float32 positions travel as their bits among the integers
        return pos.index_select(0, idx).to(torch.float32).contiguous().view(torch.int32)

    blocks = [("root", root), ("size", sa.index_select(0, root)), ("match_root", m),
              ("match_size", torch.where(has, sb.index_select(0, mc), torch.zeros_like(mc, dtype=torch.int32))),
              ("shared", s_ab.index_select(0, root)), ("mutual", mutual),
              ("disp_a", da.index_select(0, root)), ("disp_b", db.index_select(0, mc)),
              ("pos_a", bits(pos_a, root)), ("pos_b", bits(pos_b, mc))]
    scales = []             # of the value blocks, in their order: float64 bits behind the table
    for name, s, idx in (("sums_a", sums[0], root), ("sums_b", sums[1], mc)):
        if s is not None:
            blocks.append((name, s[0].reshape(n, -1).index_select(0, idx)))
            scales.append(torch.ones(1, dtype=torch.float64, device=root.device) if s[1] is None
                          else s[1].to(torch.float64).reshape(1))
    widths = [1 if t.dim() == 1 else t.shape[1] for _, t in blocks]
    table = torch.cat([t.to(torch.int64).reshape(h, w) for (_, t), w in zip(blocks, widths)], dim=1)
    packed = torch.cat([table.reshape(-1)] + [sc.view(torch.int64) for sc in scales]).cpu()     # the one transfer
    table_h = packed[:table.numel()].reshape(h, table.shape[1])
    scales_h = packed[table.numel():].view(torch.float64).tolist()
    order = sorted(range(h), key=lambda i: (-int(table_h[i, 1]), int(table_h[i, 0])))
    table_h = table_h[torch.tensor(order, dtype=torch.int64)]
    f, at = {}, 0
    for (name, _), w in zip(blocks, widths):
        f[name] = table_h[:, at:at + w]
        at += w

    def f32(b):
        return b.to(torch.int32).contiguous().view(torch.float32)

    size_h, msize_h = f["size"].reshape(h), f["match_size"].reshape(h)
    matched = (f["match_root"] >= 0).reshape(h, 1)
    nan = float("nan")
    centre = halo_centres(f32(f["pos_a"]), size_h, f["disp_a"], box_size)
    mcentre = halo_centres(f32(f["pos_b"]), msize_h.clamp(min=1), f["disp_b"], box_size)
    mcentre = torch.where(matched, mcentre, torch.full_like(mcentre, nan))
    box = float(torch.tensor(float(box_size), dtype=torch.float32))
    d = mcentre - centre
    d = d - box * torch.round(d / box)
    res = {"root": f["root"].reshape(h).clone(), "size": size_h.clone(), "centre": centre,
           "match_root": f["match_root"].reshape(h).clone(), "match_size": msize_h.clone(),
           "shared": f["shared"].reshape(h).clone(), "mutual": f["mutual"].reshape(h).to(torch.bool),
           "match_centre": mcentre, "centre_offset": torch.sqrt((d * d).sum(dim=1))}
    for v, block, name, count in ((values[0], "sums_a", "mean_value", size_h),
                                  (values[1], "sums_b", "match_mean_value", msize_h)):
        if v is None:
            continue
        mean = f[block].to(torch.float64) / count.clamp(min=1).to(torch.float64).unsqueeze(1) \
            * (scales_h.pop(0) / float(1 << _lib.WEIGHT_BITS))
        if name == "match_mean_value":
            mean = torch.where(matched, mean, torch.full_like(mean, nan))
        res[name] = mean.reshape(h) if v.dim() == 1 else mean
    return res


def halo_matching_on_device(true_frames: torch.Tensor, pred_frames: torch.Tensor, box_size: float, linking_length: float,
                            size_edges, min_members: int) -> torch.Tensor:
    """The device part of :func:`rollout_halo_matching`: for ``[F, N, 3]`` true and predicted frames an int64 ``[F, 6 nb
    + 3]`` device tensor whose rows hold the summary of ``ops.halo_match`` (A the truth), then the listed true groups,
    the listed predicted groups, and the mutual pairs among all of them.  No host synchronisation."""
    lt, lp = ops.fof_labels(true_frames, box_size, linking_length), ops.fof_labels(pred_frames, box_size, linking_length)
    st = ops.fof_catalogue(true_frames, lt, box_size, want_disp=False)[0]
    sp = ops.fof_catalogue(pred_frames, lp, box_size, want_disp=False)[0]
    m_ab, _, m_ba, _, summary = ops.halo_match(lt, st, lp, sp, min_members, size_edges=size_edges)
    m = m_ab.to(torch.int64)
    back = torch.gather(m_ba.to(torch.int64), 1, m.clamp(min=0))
    mutual = (m >= 0) & (back == torch.arange(m.shape[1], device=m.device).unsqueeze(0))
    return torch.cat([summary.reshape(summary.shape[0], -1),
                      (st >= min_members).sum(dim=1, dtype=torch.int64).unsqueeze(1),
                      (sp >= min_members).sum(dim=1, dtype=torch.int64).unsqueeze(1),
                      mutual.sum(dim=1, dtype=torch.int64).unsqueeze(1)], dim=1)


def rollout_halo_matching(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], box_size: float,
                          linking_length: Optional[float] = None, size_edges=None,
                          frames: Optional[Sequence[int]] = None, min_members: Optional[int] = None) -> Dict:
    """Whether a rollout forms the SAME halos as the truth, for the dicts ``rollout.rollout`` returns (``Coordinates [T,
    N, 3]``; both hold the same particles under the same indices).  Per selected frame the groups of the true frame
    with at least ``min_members`` members (default ``size_edges[0]``) are matched with those of the predicted frame
    (``ops.halo_match``, A the truth).  Per frame and per size bin of the TRUE groups (CPU):

    * ``n_true``, ``n_matched``, ``n_mutual`` int64 ``[F, nb]``: the listed true groups of the bin, those that share a
      member with a listed predicted group, and those whose best partner has them as its best partner too;
    * ``completeness`` float64: ``n_mutual / n_true`` (``nan`` for an empty bin);
    * ``shared_fraction``, ``size_ratio`` float64: over the mutual ones, the members shared / the true sizes, and the
      predicted sizes / the true sizes (``nan`` without a mutual pair),

    per frame ``n_groups_true``, ``n_groups_pred`` (int64 ``[F]``, the listed groups, beyond the last edge too) and
    ``n_unmatched_pred`` (the listed predicted groups without a mutual partner), plus ``frames``, ``size_lo`` and
    ``size_hi``.  The ratios are formed on the host from the integer sums.  No synchronisation per frame, one packed
    transfer.  Arguments and refusals are those of :func:`rollout_halo_statistics`.  One box, one device, membership
    only (unbinding: :func:`rollout_halo_binding`), no merger trees over more than two frames; an owned-storage
    rollout goes through ``dist.assemble_frames`` first."""
    what = "rollout_halo_matching"
    pc, tc, sel = _rollout_frames(rollout_data, ground_truth, frames, what)
    n = pc.shape[1]
    ll, e = _halo_arguments(n, box_size, linking_length, size_edges, what)
    min_members = e[0] if min_members is None else ops.check_min_members(min_members, what)
    out = halo_matching_on_device(tc, pc, box_size, ll, e, min_members).cpu()
    nb = len(e) - 1
    edges = torch.tensor(e, dtype=torch.int64)
    summary = out[:, :nb * _lib.HALO_MATCH_COLS].reshape(len(sel), nb, _lib.HALO_MATCH_COLS)
    n_true, n_matched, n_mutual = summary[..., 0].clone(), summary[..., 1].clone(), summary[..., 2].clone()
    shared, size_true, size_pred = (summary[..., c].to(torch.float64) for c in (3, 4, 5))
    base = nb * _lib.HALO_MATCH_COLS
    return {"frames": sel, "size_lo": edges[:-1].clone(), "size_hi": edges[1:].clone(),
            "n_true": n_true, "n_matched": n_matched, "n_mutual": n_mutual,
            "completeness": n_mutual.to(torch.float64) / n_true.to(torch.float64),
            "shared_fraction": shared / size_true, "size_ratio": size_pred / size_true,
            "n_groups_true": out[:, base].clone(), "n_groups_pred": out[:, base + 1].clone(),
            "n_unmatched_pred": out[:, base + 1] - out[:, base + 2]}


def default_radial_edges(n: int, box_size: float) -> torch.Tensor:
    """The default radii of the halo profiles: 0, then 24 log-spaced radii from 0.05 to 8 mean interparticle spacings
    ``box_size / n ** (1 / 3)``, without those above ``fl32(0.5 * box_size)`` (the profile kernel's reach); at least two
    edges remain, since 0.05 spacings never exceed a twentieth of the box.  Float32 values as float64, ascending."""
    if int(n) < 1:
        raise ValueError(f"default_radial_edges: n must be at least 1, got {n!r}")
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"default_radial_edges: box_size must be positive and finite, got {box_size!r}")
    spacing = float(box_size) / float(n) ** (1.0 / 3.0)
    r = (spacing * torch.logspace(math.log10(0.05), math.log10(8.0), 24, dtype=torch.float64)).to(torch.float32)
    r = r[r <= box * 0.5]
    return torch.cat([torch.zeros(1, dtype=torch.float32), r]).to(torch.float64)


def _profile_edges(edges, n: int, box_size: float, what: str):
    """The radii of a profile (default :func:`default_radial_edges`) as checked host floats and as float64; they start
    at 0, as the cumulative counts of :func:`so_masses` need."""
    e = ops.check_profile_edges(default_radial_edges(n, box_size) if edges is None else edges, box_size, what)
    if e[0] != 0.0:
        raise ValueError(f"{what}: edges[0] must be 0 (the spherical-overdensity mass counts every particle inside a "
                         f"radius), got {e[0]}")
    return e, torch.tensor(e, dtype=torch.float64)


def halo_centres_on_device(pos: torch.Tensor, size: torch.Tensor, disp: torch.Tensor, roots: torch.Tensor,
                           box_size: float):
    """:func:`halo_centres` on the device, for the kernels that take centres: ``(pos[root] + disp[root] / size[root] * L
    / 2^30) mod L`` in float64 (``L`` the float32 value of ``box_size``), rounded to float32.  ``pos [N, 3]``, ``size [N]``
    and ``disp [N, 3]`` as ``ops.fof_catalogue`` gives them, ``roots`` int64 ``[H]``; or all with one leading frame axis.
    Returns ``(centres, valid)``: float32 ``[H, 3]`` in ``[0, L]`` (the rounding may reach ``L``) and bool ``[H]``.  A row
    whose ``size[root] < 1`` (no root slot) has no centre: it is set to 0 and ``valid`` is false there, so that a kernel
    never sees a non-finite centre.  No host synchronisation."""
    box = float(torch.tensor(float(box_size), dtype=torch.float32))
    idx = roots.to(torch.int64)
    s = torch.take_along_dim(size, idx, dim=-1)
    valid = s >= 1
    idx3 = idx.unsqueeze(-1).expand(*idx.shape, 3)
    rp = torch.take_along_dim(pos, idx3, dim=-2).to(torch.float64)
    d = torch.take_along_dim(disp, idx3, dim=-2).to(torch.float64)
    c = torch.remainder(rp + d / s.clamp(min=1).to(torch.float64).unsqueeze(-1) * (box / _lib.FOF_DISP_UNITS), box)
    c = c.to(torch.float32)
    return torch.where(valid.unsqueeze(-1), c, torch.zeros_like(c)), valid


def so_masses(counts: torch.Tensor, n: int, box_size: float, edges, delta: float = 200.0):
    """Spherical-overdensity radius and mass from a radial profile: ``counts [..., nb]`` (the counts of
    ``ops.halo_profiles``; ``n`` particles in the box) -> ``(r_delta, m_delta)``, float64 ``[...]`` on the device of
    ``counts``, ``m_delta`` in particles.  ``edges[0]`` must be 0 (``ValueError``).  The rule:

    * ``N_i`` = the particles inside ``edges[i]`` (the cumulative sum of the counts), and for ``i >= 1`` the mean enclosed
      density over the mean density of the box, ``D_i = N_i / (n * 4/3 pi edges[i]^3 / L^3)``;
    * ``i*`` = the first ``i >= 1`` with ``D_i >= delta``, and ``k`` = the first ``k > i*`` with ``D_k < delta``;
    * ``r_delta`` lies between ``edges[k - 1]`` and ``edges[k]``, where ``D`` crosses ``delta`` on the straight line through
      ``(log r, log D)`` at the two edges; ``m_delta = delta * n / L^3 * 4/3 pi r_delta^3``.

    ``nan`` where there is no ``i*`` (the halo is too diffuse for ``delta`` at every edge) or no ``k`` (the profile does not
    reach out far enough).  An empty core (``D_1 < delta``) is passed over: the search for ``k`` begins at ``i*``.  The
    limit of the rule: everything inside a radius counts, so a heavier neighbour inside the last edge can keep ``D``
    above ``delta`` and move the crossing outward (bound or not: :func:`halo_binding` unbinds; no exclusion of other halos).  Cumulative sums and
    comparisons in float64 torch: no host synchronisation."""
    what = "so_masses"
    r = _radii(edges, box_size, what)
    if float(r[0]) != 0.0:
        raise ValueError(f"{what}: edges[0] must be 0 (N_i counts every particle inside edges[i]), got {float(r[0])}")
    if not (isinstance(delta, (int, float)) and not isinstance(delta, bool) and math.isfinite(delta) and delta > 0):
        raise ValueError(f"{what}: delta must be a positive finite number, got {delta!r}")
    if not torch.is_tensor(counts) or counts.dim() < 1 or counts.shape[-1] != r.numel() - 1:
        raise ValueError(f"{what}: counts must be [..., {r.numel() - 1}] for {r.numel()} edges, got "
                         f"{tuple(counts.shape) if torch.is_tensor(counts) else counts!r}")
    nb = r.numel() - 1
    r = r[1:].contiguous()                                                # edges[1 .. nb]: column j is edge j + 1
    if counts.is_cuda:                                                    # pinned + non_blocking: no synchronisation
        r = r.pin_memory().to(counts.device, non_blocking=True)
    rho = float(n) / float(box_size) ** 3
    dens = torch.cumsum(counts.to(torch.float64), dim=-1) / (rho * (4.0 / 3.0 * math.pi) * r ** 3)
    above = dens >= float(delta)
    seen = torch.cumsum(above.to(torch.int64), dim=-1) > 0                # at or behind i*
    cand = seen & ~above                                                  # behind i* and below delta
    k = (torch.cumsum(cand.to(torch.int64), dim=-1) == 0).sum(dim=-1)     # the columns ahead of the first one: k - 1
    found = k < nb
    if nb == 1:                                                           # one edge: never a k behind an i*
        r_delta = torch.full(dens.shape[:-1], float("nan"), dtype=torch.float64, device=dens.device)
        return r_delta, r_delta.clone()
    k = k.clamp(min=1, max=nb - 1).unsqueeze(-1)                          # k >= 1 where found; elsewhere any column
    d0, d1 = torch.gather(dens, -1, k - 1).squeeze(-1), torch.gather(dens, -1, k).squeeze(-1)
    lr = torch.log(r).expand(*dens.shape[:-1], nb)
    l0, l1 = torch.gather(lr, -1, k - 1).squeeze(-1), torch.gather(lr, -1, k).squeeze(-1)
    r_delta = torch.exp(l0 + (math.log(float(delta)) - torch.log(d0)) / (torch.log(d1) - torch.log(d0)) * (l1 - l0))
    r_delta = torch.where(found, r_delta, torch.full_like(r_delta, float("nan")))
    return r_delta, float(delta) * rho * (4.0 / 3.0 * math.pi) * r_delta ** 3


def halo_profiles(pos: torch.Tensor, box_size: float, edges=None, linking_length: Optional[float] = None,
                  min_members: int = 20, values: Optional[torch.Tensor] = None, delta: float = 200.0) -> Dict:
    """What is INSIDE the halos of one frame ``pos [N, 3]``: around the centre of every friends-of-friends group with at
    least ``min_members`` members (the steps of :func:`halo_catalogue`) the particles of the whole frame by radius
    (``ops.halo_profiles``; ``edges``: default :func:`default_radial_edges`, at most 32 bins, ``edges[0] == 0``), and from
    that profile the spherical-overdensity radius and mass (:func:`so_masses`).  Returns on the CPU, sorted as
    :func:`halo_catalogue` sorts (size descending, then root ascending):

    * ``root``, ``size`` int64 ``[H]``; ``centre`` float64 ``[H, 3]``: the float32 centres the kernel used
      (:func:`halo_centres_on_device`), widened;
    * ``r_lo``, ``r_hi`` float64 ``[nb]``; ``counts`` int64 ``[H, nb]``: the particles per shell, members or not;
    * ``density`` float64 ``[H, nb]``: the counts over ``n * V_shell / L^3``, the density in units of the mean density;
    * with ``values`` (``[N]`` or ``[N, C]``, ``C <= 4``, e.g. the temperature): ``mean_value`` float64 ``[H, nb]`` (``[H, nb,
      C]``), the mean over the particles of the shell, exact up to the quantisation to 2^-20 of the largest ``|value|``
      (int32 values are taken as quantised weights, in units of their scale); ``nan`` in an empty shell;
    * ``r_delta``, ``m_delta`` float64 ``[H]``: :func:`so_masses` for ``delta``, ``nan`` where undefined.

    The number of groups is only known on the device: one synchronisation (``nonzero``) and one transfer, as
    :func:`halo_catalogue`.  One box, one device; every particle inside a radius counts, bound or not (:func:`halo_binding`); no spatial
    shards (``dist.assemble_frames`` first), no ``offsets`` batches."""
    what = "halo_profiles"
    if not torch.is_tensor(pos) or pos.dim() != 2 or pos.shape[-1] != 3 or pos.shape[0] < 1:
        raise ValueError(f"{what}: pos must be one frame [N, 3] with N >= 1, got "
                         f"{tuple(pos.shape) if torch.is_tensor(pos) else pos!r}")
    min_members = ops.check_min_members(min_members, what)
    n = pos.shape[0]
    e, r = _profile_edges(edges, n, box_size, what)
    nb = len(e) - 1
    ll = default_linking_length(n, box_size) if linking_length is None else linking_length
    ops.check_linking_length(ll, box_size, what)
    values = _group_values(values, n, "values", what)
    so_masses(torch.zeros(nb), n, box_size, e, delta)                     # refuses a bad delta before device work
    labels = ops.fof_labels(pos, box_size, ll)
    size, disp, _ = ops.fof_catalogue(pos, labels, box_size)
    root = torch.nonzero(size >= min_members).reshape(-1)                 # the one synchronisation
    h = root.numel()
    c = 0 if values is None else (1 if values.dim() == 1 else values.shape[1])
    shell = n * _shell_volumes(r) / float(box_size) ** 3
    nan = float("nan")
    if h == 0:
        res = {"root": torch.zeros(0, dtype=torch.int64), "size": torch.zeros(0, dtype=torch.int64),
               "centre": torch.zeros((0, 3), dtype=torch.float64), "r_lo": r[:-1].clone(), "r_hi": r[1:].clone(),
               "counts": torch.zeros((0, nb), dtype=torch.int64), "density": torch.zeros((0, nb), dtype=torch.float64),
               "r_delta": torch.zeros(0, dtype=torch.float64), "m_delta": torch.zeros(0, dtype=torch.float64)}
        if values is not None:
            res["mean_value"] = torch.zeros((0, nb) if values.dim() == 1 else (0, nb, c), dtype=torch.float64)
        return res
    centres, _ = halo_centres_on_device(pos, size, disp, root, box_size)
    scale = None
    if values is None:
        counts = ops.halo_profiles(pos, centres, box_size, e)
    elif values.dtype == torch.int32:
        counts, sums = ops.halo_profiles(pos, centres, box_size, e, values.to(pos.device))
    else:
        values = values.to(pos.device)
        m = values.detach().abs().max().to(torch.float64)
        scale = torch.where(m > 0, m, torch.ones_like(m))                 # the scale ops.halo_profiles would take
        counts, sums = ops.halo_profiles(pos, centres, box_size, e, values, scale)
    r_delta, m_delta = so_masses(counts, n, box_size, e, delta)
    # one transfer: the float32 centres and the float64 results travel as their bits among the integers
    blocks = [root.reshape(h, 1), size.index_select(0, root).to(torch.int64).reshape(h, 1),
              centres.contiguous().view(torch.int32).to(torch.int64), counts,
              r_delta.view(torch.int64).reshape(h, 1), m_delta.view(torch.int64).reshape(h, 1)]
    if values is not None:
        blocks.append(sums.reshape(h, nb * c))
    table = torch.cat(blocks, dim=1)
    tail = [] if scale is None else [scale.reshape(1).view(torch.int64)]
    packed = torch.cat([table.reshape(-1)] + tail).cpu()
    table_h = packed[:table.numel()].reshape(h, table.shape[1])
    order = sorted(range(h), key=lambda i: (-int(table_h[i, 1]), int(table_h[i, 0])))
    table_h = table_h[torch.tensor(order, dtype=torch.int64)]
    counts_h = table_h[:, 5:5 + nb].clone()
    res = {"root": table_h[:, 0].clone(), "size": table_h[:, 1].clone(),
           "centre": table_h[:, 2:5].to(torch.int32).contiguous().view(torch.float32).to(torch.float64),
           "r_lo": r[:-1].clone(), "r_hi": r[1:].clone(), "counts": counts_h,
           "density": counts_h.to(torch.float64) / shell,
           "r_delta": table_h[:, 5 + nb].clone().view(torch.float64),
           "m_delta": table_h[:, 6 + nb].clone().view(torch.float64)}
    if values is not None:
        unit = (1.0 if scale is None else float(packed[table.numel():].view(torch.float64))) / float(1 << _lib.WEIGHT_BITS)
        sums_h = table_h[:, 7 + nb:].reshape(h, nb, c).to(torch.float64)
        mean = torch.where(counts_h.unsqueeze(-1) > 0, sums_h / counts_h.clamp(min=1).unsqueeze(-1) * unit,
                           torch.full_like(sums_h, nan))
        res["mean_value"] = mean.reshape(h, nb) if values.dim() == 1 else mean
    return res


_TEMPERATURE_KEYS = ("Temperature", "InternalEnergy")   # the rollout dicts carry the temperature as InternalEnergy


def halo_profile_stacks_on_device(frames: torch.Tensor, box_size: float, linking_length: float, size_edges, edges,
                                  max_halos: int, delta: float, temperature: Optional[torch.Tensor] = None):
    """The device part of :func:`rollout_halo_profiles` for one side: ``frames [F, N, 3]`` (``temperature``: the values
    ``[F, N]`` and their scale, a 0-d device tensor) -> ``(ints, floats)``, an int64 ``[F, 1 + sb (2 + nb (1 + t))]`` tensor whose
    rows hold the listed groups beyond
    ``max_halos``, then per size bin the profiled groups, those with a defined ``m_delta``, the stacked counts and (``t =
    1`` with a temperature) the stacked weight sums; and a float64 ``[F, 2 sb]`` tensor with the sums of ``m_delta`` and
    ``r_delta`` over the groups where they are defined.  The ``max_halos`` largest listed groups are a ``topk`` of the key
    ``size << 32 | (2^32 - 1 - root)``: ties go to the smaller root.  The sums over the groups are masked sums in a fixed
    order, not atomics: the same bits on every run.  No host synchronisation."""
    f, n = frames.shape[0], frames.shape[1]
    dev = frames.device
    nb, sb = len(edges) - 1, len(size_edges) - 1
    labels = ops.fof_labels(frames, box_size, linking_length)
    size, disp, _ = ops.fof_catalogue(frames, labels, box_size)
    listed = size >= int(size_edges[0])
    slot = torch.arange(n, dtype=torch.int64, device=dev)
    key = torch.where(listed, (size.to(torch.int64) << 32) | ((1 << 32) - 1 - slot), torch.full_like(slot, -1))
    kk = min(int(max_halos), n)
    top, root = torch.topk(key, kk, dim=1)
    taken = top >= 0                                                      # [F, K]: a listed group, not padding
    centres, _ = halo_centres_on_device(frames, size, disp, root, box_size)
    if temperature is None:
        counts, sums = ops.halo_profiles(frames, centres, box_size, edges), None
    else:
        counts, sums = ops.halo_profiles(frames, centres, box_size, edges, temperature[0], temperature[1])
    r_delta, m_delta = so_masses(counts, n, box_size, edges, delta)       # [F, K]
    sz = torch.gather(size, 1, root)
    in_bin = torch.stack([taken & (sz >= int(lo)) & (sz < int(hi)) for lo, hi in zip(size_edges[:-1], size_edges[1:])],
                         dim=-1)                                          # [F, K, sb]
    defined = in_bin & ~torch.isnan(m_delta).unsqueeze(-1)
    stack = (in_bin.unsqueeze(-1) * counts.unsqueeze(2)).sum(dim=1)       # [F, sb, nb] int64
    ints = [(listed.sum(dim=1, dtype=torch.int64) - kk).clamp(min=0).unsqueeze(1),
            in_bin.sum(dim=1, dtype=torch.int64), defined.sum(dim=1, dtype=torch.int64), stack.reshape(f, sb * nb)]
    if sums is not None:
        ints.append((in_bin.unsqueeze(-1) * sums.unsqueeze(2)).sum(dim=1).reshape(f, sb * nb))
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    floats = [torch.where(defined, v.unsqueeze(-1), zero).sum(dim=1) for v in (m_delta, r_delta)]
    return torch.cat(ints, dim=1), torch.cat(floats, dim=1)


def rollout_halo_profiles(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], box_size: float,
                          edges=None, linking_length: Optional[float] = None, size_edges=None, max_halos: int = 1024,
                          delta: float = 200.0, frames: Optional[Sequence[int]] = None) -> Dict:
    """Whether a rollout gets the INSIDE of its halos right, for the dicts ``rollout.rollout`` returns (``Coordinates [T,
    N, 3]``).  Per selected frame and per side (predicted, true) the ``max_halos`` largest friends-of-friends groups
    with at least ``size_edges[0]`` members (ties to the smaller root) are profiled around their centres
    (``ops.halo_profiles``; ``edges``: default :func:`default_radial_edges`) and stacked by size.  Per frame and per size
    bin of the groups (``size_edges``: default :func:`default_size_edges`), for ``pred`` and ``true`` (CPU):

    * ``n_halos_*`` int64 ``[F, sb]``: the profiled groups of the bin;
    * ``counts_*`` int64 ``[F, sb, nb]``: their summed counts;  ``density_*`` float64: the stacked profile ``counts / (n_halos
      n V_shell / L^3)`` in units of the mean density (``nan`` for an empty bin);
    * ``m_delta_*``, ``r_delta_*`` float64 ``[F, sb]``: the mean of :func:`so_masses` over the groups where it is defined
      (``nan`` without one), and ``n_delta_*`` int64: how many those are;
    * with a temperature in both dicts (``Temperature``, or the ``InternalEnergy [T, N(, 1)]`` the rollout dicts carry):
      ``temperature_*`` float64 ``[F, sb, nb]``, the mean temperature of the stacked shells (quantised to 2^-20 of the
      side's largest ``|T|``; ``nan`` in an empty shell),

    per frame ``not_profiled_pred``, ``not_profiled_true`` int64 ``[F]``: the listed groups beyond ``max_halos``, which are
    in none of the sums (a truncation is never silent), plus ``frames``, ``size_lo``, ``size_hi``, ``r_lo`` and ``r_hi``.  A
    group beyond the last size edge is profiled but in no bin.  No synchronisation per frame, one packed transfer.
    Out of scope: profiles of matched pairs (a true halo against its partner: :func:`rollout_halo_matching` pairs
    them; whether they are bound: :func:`rollout_halo_binding`), ``offsets`` batches, and sharded or owned-storage inputs (``dist.assemble_frames`` first)."""
    what = "rollout_halo_profiles"
    key = next((k for k in _TEMPERATURE_KEYS if k in rollout_data and k in ground_truth), None)
    dev = rollout_data["Coordinates"].device
    also = () if key is None else (rollout_data[key].to(dev), ground_truth[key].to(dev))
    got = _rollout_frames(rollout_data, ground_truth, frames, what, also)
    pc, tc, sel = got[:3]
    n = pc.shape[1]
    ll, se = _halo_arguments(n, box_size, linking_length, size_edges, what)
    e, r = _profile_edges(edges, n, box_size, what)
    if isinstance(max_halos, bool) or not isinstance(max_halos, int) or max_halos < 1:
        raise ValueError(f"{what}: max_halos must be a whole number of at least 1, got {max_halos!r}")
    nb, sb, nf = len(e) - 1, len(se) - 1, len(sel)
    so_masses(torch.zeros(nb), n, box_size, e, delta)                     # refuses a bad delta before device work
    parts, scales = [], []
    for side, frames_ in enumerate((pc, tc)):
        temp = None
        if key is not None:
            t = _scalar_values(got[3 + side], frames_, frames_, key, what)
            m = t.detach().abs().max().to(torch.float64)
            scales.append(torch.where(m > 0, m, torch.ones_like(m)).reshape(1))
            temp = (t, scales[-1].reshape(()))
        ints, floats = halo_profile_stacks_on_device(frames_, box_size, ll, se, e, max_halos, float(delta), temp)
        parts += [ints.reshape(-1), floats.contiguous().view(torch.int64).reshape(-1)]
    packed = torch.cat(parts + [s.view(torch.int64) for s in scales]).cpu()                      # the one transfer
    width_i = 1 + sb * (2 + nb * (1 + (key is not None)))
    shell = n * _shell_volumes(r) / float(box_size) ** 3
    sedges = torch.tensor(se, dtype=torch.int64)
    res = {"frames": sel, "size_lo": sedges[:-1].clone(), "size_hi": sedges[1:].clone(), "r_lo": r[:-1].clone(),
           "r_hi": r[1:].clone()}
    at = 0
    scales_h = packed[packed.numel() - len(scales):].view(torch.float64).tolist()
    for side, name in enumerate(("pred", "true")):
        ints = packed[at:at + nf * width_i].reshape(nf, width_i)
        at += nf * width_i
        floats = packed[at:at + nf * 2 * sb].view(torch.float64).reshape(nf, 2 * sb)
        at += nf * 2 * sb
        n_halos, n_def = ints[:, 1:1 + sb].clone(), ints[:, 1 + sb:1 + 2 * sb].clone()
        counts = ints[:, 1 + 2 * sb:1 + 2 * sb + sb * nb].reshape(nf, sb, nb).clone()
        res["not_profiled_" + name] = ints[:, 0].clone()
        res["n_halos_" + name], res["n_delta_" + name], res["counts_" + name] = n_halos, n_def, counts
        res["density_" + name] = counts.to(torch.float64) / (n_halos.to(torch.float64).unsqueeze(-1) * shell)
        res["m_delta_" + name] = floats[:, :sb] / n_def.to(torch.float64)
        res["r_delta_" + name] = floats[:, sb:] / n_def.to(torch.float64)
        if key is not None:
            sums = ints[:, 1 + 2 * sb + sb * nb:].reshape(nf, sb, nb).to(torch.float64)
            res["temperature_" + name] = sums / counts.to(torch.float64) * (scales_h[side] / float(1 << _lib.WEIGHT_BITS))
    return res


# ---- is a halo bound: potentials inside the groups, unbinding, virial ratios ---------------------------------------------
#
# A friends-of-friends group is a set of particles that are close together; it is a halo only if they are also
# gravitationally bound.  An emulator can put the right number of particles in the right places and still give them
# velocities that fly apart in the next frames: the mass function, the matching and the profiles above all call such
# a group a correct halo.  ``ops.halo_potentials`` gives every member its softened potential sum over the other members
# in exact integers; what follows is elementwise float64 arithmetic and integer group sums on top of it.
#
# Units: ``gm`` is G times the particle mass in length^3 / time^2 of the caller's positions and velocities; energies are
# specific (per unit particle mass).  Equal masses, direct sums over the members of a group only.  Out of scope: unequal
# masses, tree or mesh potentials, particles outside a group as sources, subhalo finding, re-accretion of removed
# particles, partial removal per pass, sharded, batched or owned-storage inputs (``dist.assemble_frames`` first), a loss.

BINDING_VELOCITY_BITS = _lib.WEIGHT_BITS   # a group's bulk velocity: integer sums of velocities in 2^-20 of the scale
BINDING_ENERGY_BITS = 32                   # group sums of energies: integers in 2^-32 of the largest term
BINDING_SPLIT_BITS = 20                    # a potential sum enters a group sum as two words, P >> 20 and P & (2^20 - 1)


def _check_gm(what: str, gm, hubble, iterations=None):
    for name, v, positive in (("gm", gm, True), ("hubble", hubble, False)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and not v > 0):
            raise ValueError(f"{what}: {name} must be a {'positive ' if positive else ''}finite number, got {v!r}")
    if iterations is not None and (isinstance(iterations, bool) or not isinstance(iterations, int) or
                                   not 1 <= iterations <= 64):
        raise ValueError(f"{what}: iterations must be a whole number in [1, 64], got {iterations!r}")


def _slot_sums(key: torch.Tensor, values: torch.Tensor, n: int) -> torch.Tensor:
    """Integer sums per root slot: ``out[r] = sum of values[i] over key[i] == r`` for int64 ``values [N]`` or ``[N, C]``,
    ``key`` in ``[0, n]`` (slot ``n`` collects what is in no group and is dropped).  Integer ``index_add``: the same bits
    on every run."""
    out = torch.zeros((n + 1,) + tuple(values.shape[1:]), dtype=torch.int64, device=values.device)
    out.index_add_(0, key, values)
    return out[:n]


def _quantised_slot_sums(key: torch.Tensor, values: torch.Tensor, mask: torch.Tensor, n: int):
    """Group sums of float64 ``values [N]`` over the particles of ``mask`` as integers: ``(sums int64 [n], scale)`` with
    ``scale`` the largest ``|value|`` under the mask (0-d float64, 1 where there is none) and a value entering as
    ``rint(value / scale * 2^32)``; the group's sum is ``sums * scale / 2^32``, each term off by at most half a step."""
    zero = torch.zeros((), dtype=torch.float64, device=values.device)
    v = torch.where(mask, values, zero)
    m = v.abs().max()
    scale = torch.where(m > 0, m, torch.ones_like(m))
    q = torch.round(v / scale * float(1 << BINDING_ENERGY_BITS)).to(torch.int64)
    return _slot_sums(key, q, n), scale


def binding_energies(psum: torch.Tensor, shift: int, gm: float, vel: torch.Tensor, labels: torch.Tensor,
                     active: torch.Tensor, dx: Optional[torch.Tensor] = None, hubble: float = 0.0,
                     internal_energy: Optional[torch.Tensor] = None, velocity_scale=None) -> Dict:
    """The specific energies of the particles of one frame from the integer potential sums of ``ops.halo_potentials``
    (``psum [N]``, ``shift``), elementwise in float64 on the device of ``psum``:

    * ``potential``: ``phi_i = -gm * psum_i * 2^-shift``, ``gm`` = G times the particle mass;
    * ``kinetic``: ``k_i = 1/2 |v_i - v_bulk + hubble * dx_i|^2 (+ internal_energy_i)`` with ``v_bulk`` the mean velocity
      of the active members of ``i``'s group (``labels [N]``, ``active [N]`` bool) and ``dx [N, 3]`` the minimum-image
      displacement from the group's centre (needed with ``hubble != 0``);
    * ``energy``: ``e_i = k_i + phi_i``; a member is bound iff ``e_i < 0``;
    * ``peculiar2``: ``|v_i - v_bulk|^2``; ``v_bulk`` float64 ``[N, 3]`` and ``n_active`` int64 ``[N]`` per root slot.

    ``v_bulk`` comes from integer sums: the velocities enter as ``rint(v / velocity_scale * 2^20)`` (default scale: the
    largest ``|v|`` component, taken on the device; components beyond a given scale are clamped), summed by integer
    ``index_add``: the same bits on every run.  The values at inactive particles are computed like the others (against
    their label's bulk velocity) and mean nothing.  No host synchronisation."""
    what = "binding_energies"
    _check_gm(what, gm, hubble)
    if not torch.is_tensor(psum) or psum.dtype != torch.int64 or psum.dim() != 1 or psum.shape[0] < 1:
        raise ValueError(f"{what}: psum must be an int64 tensor [N], got "
                         f"{(psum.dtype, tuple(psum.shape)) if torch.is_tensor(psum) else psum!r}")
    n = psum.shape[0]
    if isinstance(shift, bool) or not isinstance(shift, int) or not -200 < shift < 200:
        raise ValueError(f"{what}: shift must be the integer ops.halo_potentials returns, got {shift!r}")
    if not torch.is_tensor(vel) or tuple(vel.shape) != (n, 3) or not vel.is_floating_point():
        raise ValueError(f"{what}: vel must be a float tensor [{n}, 3]")
    if not torch.is_tensor(labels) or tuple(labels.shape) != (n,) or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"{what}: labels must be an integer tensor [{n}]")
    if not torch.is_tensor(active) or tuple(active.shape) != (n,) or active.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{what}: active must be a bool or uint8 tensor [{n}]")
    if dx is None and float(hubble) != 0.0:
        raise ValueError(f"{what}: hubble needs dx, the displacements from the group centres")
    if dx is not None and (not torch.is_tensor(dx) or tuple(dx.shape) != (n, 3)):
        raise ValueError(f"{what}: dx must be [{n}, 3]")
    if internal_energy is not None and (not torch.is_tensor(internal_energy) or tuple(internal_energy.shape) != (n,)):
        raise ValueError(f"{what}: internal_energy must be [{n}]")
    dev = psum.device
    v = vel.to(device=dev, dtype=torch.float64)
    lab = labels.to(device=dev, dtype=torch.int64)
    act = active.to(dev).bool() & (lab >= 0) & (lab < n)
    key = torch.where(act, lab, torch.full_like(lab, n))
    if velocity_scale is None:
        m = v.abs().max()
        scale = torch.where(m > 0, m, torch.ones_like(m))
    else:
        scale = ops._check_value_scale(velocity_scale, what)
        scale = scale.to(device=dev, dtype=torch.float64) if torch.is_tensor(scale) else scale
    unit = float(1 << BINDING_VELOCITY_BITS)
    q = torch.round(torch.clamp(v / scale, -1.0, 1.0) * unit).to(torch.int64)
    n_active = _slot_sums(key, torch.ones_like(key), n)
    v_bulk = _slot_sums(key, q, n).to(torch.float64) / n_active.clamp(min=1).to(torch.float64).unsqueeze(-1) * (scale / unit)
    u = v - v_bulk.index_select(0, lab.clamp(0, n - 1))
    peculiar2 = (u * u).sum(dim=-1)
    if dx is not None and float(hubble) != 0.0:
        u = u + float(hubble) * dx.to(device=dev, dtype=torch.float64)
    kinetic = 0.5 * (u * u).sum(dim=-1)
    if internal_energy is not None:
        kinetic = kinetic + internal_energy.to(device=dev, dtype=torch.float64)
    potential = psum.to(torch.float64) * (-float(gm) * 2.0 ** -shift)
    return {"kinetic": kinetic, "potential": potential, "energy": kinetic + potential, "peculiar2": peculiar2,
            "v_bulk": v_bulk, "n_active": n_active}


def binding_from_sums(size, n_bound, kinetic_q, kinetic_scale, peculiar_q, peculiar_scale, psum_hi, psum_lo, shift: int,
                      gm: float) -> Dict:
    """The per-group results of an unbinding from its integer group sums, float64, elementwise (on the device of the
    sums, or on the host): for groups of ``size`` members of which ``n_bound`` stayed,

    * ``bound_fraction = n_bound / size``;
    * ``kinetic = kinetic_q * kinetic_scale / 2^32``, the sum of the bound members' ``k_i``;
    * ``potential = -gm / 2 * (psum_hi * 2^20 + psum_lo) * 2^-shift``: ``W = 1/2 sum phi_i`` over the bound members, the
      potential sums having entered as two words, ``P >> 20`` and ``P & (2^20 - 1)`` (the sum of whole ``P`` over a group of
      10^5 members can pass int64);
    * ``virial_ratio = 2 kinetic / |potential|``, ``nan`` without a potential (fewer than two bound members);
    * ``sigma_v = sqrt(peculiar_q * peculiar_scale / 2^32 / n_bound)``, the three-dimensional velocity dispersion of the
      bound members about their mean, ``nan`` without a bound member."""
    f64 = torch.float64
    size, n_bound = torch.as_tensor(size), torch.as_tensor(n_bound)
    nb = n_bound.to(f64)
    step = 2.0 ** -BINDING_ENERGY_BITS
    kinetic = torch.as_tensor(kinetic_q).to(f64) * (torch.as_tensor(kinetic_scale).to(f64) * step)
    words = torch.as_tensor(psum_hi).to(f64) * float(1 << BINDING_SPLIT_BITS) + torch.as_tensor(psum_lo).to(f64)
    potential = words * (-0.5 * float(gm) * 2.0 ** -int(shift))
    nan = torch.full_like(kinetic, float("nan"))
    virial = torch.where(potential != 0, 2.0 * kinetic / potential.abs(), nan)
    pec = torch.as_tensor(peculiar_q).to(f64) * (torch.as_tensor(peculiar_scale).to(f64) * step)
    sigma = torch.where(n_bound > 0, torch.sqrt(pec / nb.clamp(min=1.0)), nan)
    return {"bound_fraction": nb / size.to(f64).clamp(min=1.0), "kinetic": kinetic, "potential": potential,
            "virial_ratio": virial, "sigma_v": sigma}


def binding_size_bins(size, n_bound, bound_fraction, virial_ratio, sigma_v, size_edges, min_members: int):
    """The groups of an unbinding by size, as masked sums in a fixed order: ``size``, ``n_bound`` (integers) and the three
    float64 results of :func:`binding_from_sums`, one entry per group or per root slot (an entry with ``size <
    min_members`` is no group and is in no sum).  With ``sb = len(size_edges) - 1`` bins ``size_edges[b] <= size <
    size_edges[b + 1]`` returns ``(ints, floats)`` on the device of ``size``:

    * ``ints`` int64 ``[5, sb]``: the groups of the bin; those left with fewer than ``min_members`` bound members (the
      spurious halos); the groups whose BOUND size lies in the bin (the bound mass function); the groups of the bin with
      a defined virial ratio; with a defined ``sigma_v``;
    * ``floats`` float64 ``[3, sb]``: the sums over the groups of the bin of the bound fraction, of the defined virial
      ratios and of the defined ``sigma_v``."""
    size = torch.as_tensor(size).to(torch.int64)
    n_bound = torch.as_tensor(n_bound).to(torch.int64).to(size.device)
    listed = size >= int(min_members)
    lo_hi = list(zip(size_edges[:-1], size_edges[1:]))
    in_bin = torch.stack([listed & (size >= int(lo)) & (size < int(hi)) for lo, hi in lo_hi], dim=0)        # [sb, G]
    bound_bin = torch.stack([listed & (n_bound >= int(lo)) & (n_bound < int(hi)) for lo, hi in lo_hi], dim=0)
    vir_ok, sig_ok = ~torch.isnan(virial_ratio), ~torch.isnan(sigma_v)
    ints = torch.stack([in_bin.sum(dim=1), (in_bin & (n_bound < int(min_members))).sum(dim=1), bound_bin.sum(dim=1),
                        (in_bin & vir_ok).sum(dim=1), (in_bin & sig_ok).sum(dim=1)])
    zero = torch.zeros((), dtype=torch.float64, device=size.device)
    floats = torch.stack([torch.where(in_bin, bound_fraction, zero).sum(dim=1),
                          torch.where(in_bin & vir_ok, virial_ratio, zero).sum(dim=1),
                          torch.where(in_bin & sig_ok, sigma_v, zero).sum(dim=1)])
    return ints.to(torch.int64), floats


def _binding_velocities(what: str, pos: torch.Tensor, vel, pos_prev, dt, box_size: float) -> torch.Tensor:
    """The float64 velocities of one frame, those of :func:`pairwise_velocities`: ``vel``, or ``minimum_image(pos -
    pos_prev) / dt``."""
    moving = pos_prev is not None
    if (vel is not None) == moving:
        raise ValueError(f"{what}: exactly one of vel or (pos_prev, dt) gives the velocities")
    if moving:
        dt = _check_dt(what, dt)
    elif dt is not None:
        raise ValueError(f"{what}: dt goes with pos_prev")
    other = pos_prev if moving else vel
    if not torch.is_tensor(other) or tuple(other.shape) != tuple(pos.shape) or not other.is_floating_point():
        raise ValueError(f"{what}: the {'previous positions' if moving else 'velocities'} must be a float tensor "
                         f"{tuple(pos.shape)} like pos")
    other = other.to(pos.device)
    return _step_velocities(pos.to(torch.float32), other.to(torch.float32), dt, box_size) if moving else other.to(torch.float64)


def halo_unbinding_on_device(pos: torch.Tensor, vel: torch.Tensor, box_size: float, gm: float, softening: float,
                             linking_length: float, min_members: int, hubble: float = 0.0,
                             internal_energy: Optional[torch.Tensor] = None, iterations: int = 3) -> Dict:
    """The device part of :func:`halo_binding` for one frame ``pos [N, 3]`` with float64 velocities ``vel [N, 3]``:
    friends-of-friends groups, then ``iterations`` unbinding passes -- each recomputes the bulk velocities and the
    potentials from the particles still active (``ops.halo_potentials``, :func:`binding_energies`) and drops every member
    with ``e_i >= 0`` -- and one evaluation pass over the members that stayed, from which the reported sums come.  Returns
    device tensors: ``labels``, ``size`` (of the catalogue), ``bound`` (bool ``[N]``), per root slot int64 ``[N]`` ``n_bound``,
    ``removed_last`` (the members the last pass dropped), ``kinetic_q``, ``peculiar_q``, ``psum_hi``, ``psum_lo``, the 0-d
    float64 ``kinetic_scale`` and ``peculiar_scale``, and the host integer ``shift``: the arguments of
    :func:`binding_from_sums`.  Fixed shapes and a fixed number of passes: no host synchronisation."""
    n = pos.shape[0]
    box = float(torch.tensor(float(box_size), dtype=torch.float32))
    labels = ops.fof_labels(pos, box_size, linking_length)
    size, disp, _ = ops.fof_catalogue(pos, labels, box_size, want_disp=float(hubble) != 0.0)
    members = ops.halo_member_order(labels, size, min_members)
    lab = labels.to(torch.int64)
    active = size.index_select(0, lab) >= int(min_members)
    dx = None
    if float(hubble) != 0.0:      # from the catalogue's centre (halo_centres), float64, under the minimum image
        p64 = pos.to(torch.float64)
        centre = p64.index_select(0, lab) + disp.index_select(0, lab).to(torch.float64) / \
            size.index_select(0, lab).clamp(min=1).to(torch.float64).unsqueeze(-1) * (box / _lib.FOF_DISP_UNITS)
        d = p64 - centre
        dx = d - box * torch.round(d / box)
    m = vel.abs().max()
    vscale = torch.where(m > 0, m, torch.ones_like(m))
    removed_last = torch.zeros(n, dtype=torch.int64, device=pos.device)
    shift = 0
    for it in range(int(iterations) + 1):
        psum, shift = ops.halo_potentials(pos, labels, size, box_size, softening, min_members, active, members=members)
        be = binding_energies(psum, shift, gm, vel, labels, active, dx, hubble, internal_energy, vscale)
        if it == int(iterations):
            break
        keep = active & (be["energy"] < 0)
        key = torch.where(active & ~keep, lab, torch.full_like(lab, n))
        removed_last = _slot_sums(key, torch.ones_like(key), n)
        active = keep
    key = torch.where(active, lab, torch.full_like(lab, n))
    kq, kscale = _quantised_slot_sums(key, be["kinetic"], active, n)
    sq, sscale = _quantised_slot_sums(key, be["peculiar2"], active, n)
    p = torch.where(active, psum, torch.zeros_like(psum))
    return {"labels": labels, "size": size, "bound": active, "n_bound": be["n_active"], "removed_last": removed_last,
            "kinetic_q": kq, "kinetic_scale": kscale, "peculiar_q": sq, "peculiar_scale": sscale,
            "psum_hi": _slot_sums(key, p >> BINDING_SPLIT_BITS, n),
            "psum_lo": _slot_sums(key, p & ((1 << BINDING_SPLIT_BITS) - 1), n), "shift": shift}


def _check_binding_arguments(what: str, n: int, box_size, gm, softening, linking_length, hubble, iterations):
    _check_gm(what, gm, hubble, iterations)
    ops.check_softening(softening, box_size, what)
    ll = default_linking_length(n, box_size) if linking_length is None else linking_length
    return ops.check_linking_length(ll, box_size, what)


def halo_binding(pos: torch.Tensor, box_size: float, gm: float, softening: float, vel: Optional[torch.Tensor] = None,
                 pos_prev: Optional[torch.Tensor] = None, dt: Optional[float] = None,
                 linking_length: Optional[float] = None, min_members: int = 20, hubble: float = 0.0,
                 internal_energy: Optional[torch.Tensor] = None, iterations: int = 3) -> Dict:
    """Which friends-of-friends groups of one frame ``pos [N, 3]`` are gravitationally BOUND, and how much of each: the
    groups with at least ``min_members`` members (the steps of :func:`halo_catalogue`), unbound by ``iterations`` passes.
    Velocities are those of :func:`pairwise_velocities`: ``vel [N, 3]``, or ``minimum_image(pos - pos_prev) / dt``.  A pass
    gives every active member ``e_i = k_i + phi_i`` (:func:`binding_energies`: ``phi_i = -gm * P_i * 2^-S`` from the exact
    integer sums of ``ops.halo_potentials`` with the Plummer ``softening``, ``k_i = 1/2 |v_i - v_bulk + hubble * dx_i|^2 +
    internal_energy_i``, ``v_bulk`` the mean velocity of the group's active members, ``dx_i`` the minimum-image displacement
    from the catalogue's centre) and drops every member with ``e_i >= 0``, all at once; a last evaluation over the members
    that stayed gives the reported sums.  ``gm`` is G times the particle mass in length^3 / time^2.  Returns on the CPU,
    sorted as :func:`halo_catalogue` sorts (size descending, then root ascending), per group:

    * ``root``, ``size`` int64 ``[H]``; ``n_bound`` int64, ``bound_fraction`` float64;
    * ``kinetic``, ``potential`` float64: ``K = sum k_i`` and ``W = 1/2 sum phi_i`` over the bound members, per unit particle
      mass; ``virial_ratio = 2 K / |W|`` (``nan`` with fewer than two bound members); ``sigma_v``: their three-dimensional
      velocity dispersion about ``v_bulk`` (``nan`` without one);
    * ``removed_last`` int64: the members the last pass dropped -- not 0 means that the unbinding has not converged in
      ``iterations`` passes, which is therefore never silent,

    and ``bound`` bool ``[N]``, the per-particle mask, with ``shift``, the ``S`` of the potentials.  Group sums are integer
    sums (:func:`binding_from_sums`): the same bits on every run.  One synchronisation (``nonzero``) and one transfer,
    as :func:`halo_profiles`.  Out of scope: unequal masses, tree or mesh potentials, particles outside a group as
    sources, subhalo finding, re-accretion of removed particles, partial removal per pass, sharded, batched or
    owned-storage inputs (``dist.assemble_frames`` first), a loss."""
    what = "halo_binding"
    if not torch.is_tensor(pos) or pos.dim() != 2 or pos.shape[-1] != 3 or pos.shape[0] < 1 or not pos.is_floating_point():
        raise ValueError(f"{what}: pos must be one frame [N, 3] of floats with N >= 1, got "
                         f"{tuple(pos.shape) if torch.is_tensor(pos) else pos!r}")
    n = pos.shape[0]
    min_members = ops.check_min_members(min_members, what)
    ll = _check_binding_arguments(what, n, box_size, gm, softening, linking_length, hubble, iterations)
    v = _binding_velocities(what, pos, vel, pos_prev, dt, box_size)
    u = _group_values(internal_energy, n, "internal_energy", what)
    if u is not None and (u.dim() != 1 or not u.is_floating_point()):
        raise ValueError(f"{what}: internal_energy must be a float tensor [{n}]")
    _lib.require_device(pos, "pos")
    d = halo_unbinding_on_device(pos, v, box_size, gm, softening, ll, min_members, hubble,
                                 None if u is None else u.to(pos.device), iterations)
    root = torch.nonzero(d["size"] >= min_members).reshape(-1)            # the one synchronisation
    h = root.numel()
    cols = [root] + [d[k].index_select(0, root).to(torch.int64) for k in
                     ("size", "n_bound", "removed_last", "kinetic_q", "peculiar_q", "psum_hi", "psum_lo")]
    scales = torch.stack([d["kinetic_scale"], d["peculiar_scale"]]).view(torch.int64)
    packed = torch.cat([torch.stack(cols, dim=1).reshape(-1), scales, d["bound"].to(torch.int64)]).cpu()   # one transfer
    table = packed[:8 * h].reshape(h, 8)
    order = sorted(range(h), key=lambda i: (-int(table[i, 1]), int(table[i, 0])))
    table = table[torch.tensor(order, dtype=torch.int64)]
    kscale, sscale = packed[8 * h:8 * h + 2].view(torch.float64)
    res = {"root": table[:, 0].clone(), "size": table[:, 1].clone(), "n_bound": table[:, 2].clone(),
           "removed_last": table[:, 3].clone(), "bound": packed[8 * h + 2:].to(torch.bool), "shift": d["shift"]}
    res.update(binding_from_sums(table[:, 1], table[:, 2], table[:, 4], kscale, table[:, 5], sscale, table[:, 6],
                                 table[:, 7], d["shift"], gm))
    return res


def rollout_halo_binding(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], box_size: float,
                         dt: float, gm: float, softening: float, linking_length: Optional[float] = None, size_edges=None,
                         hubble: float = 0.0, iterations: int = 3, frames: Optional[Sequence[int]] = None) -> Dict:
    """Whether a rollout's halos are BOUND, for the dicts ``rollout.rollout`` returns (``Coordinates [T, N, 3]``): per
    selected frame ``f >= 1`` (default: every frame from 1 on that both hold) and per side the friends-of-friends groups
    with at least ``size_edges[0]`` members are unbound as :func:`halo_binding` does, with the velocities
    ``minimum_image(pos[f] - pos[f - 1]) / dt`` and no internal energy.  All listed groups are processed, at fixed shapes:
    there is no ``max_halos``.  Per frame and per size bin of the FoF groups (``size_edges``: default
    :func:`default_size_edges`), for ``pred`` and ``true`` (CPU):

    * ``n_groups_*`` int64 ``[F, sb]``; ``spurious_*``: the groups of the bin left with fewer than ``size_edges[0]`` bound
      members; ``bound_counts_*``: the mass function of the BOUND sizes on ``size_edges``;
    * ``bound_fraction_*``, ``virial_ratio_*``, ``sigma_v_*`` float64 ``[F, sb]``: the means over the groups of the bin (the
      last two over the groups where they are defined, ``n_virial_*`` and ``n_sigma_*`` many; ``nan`` without one),

    the ratios ``bound_fraction_ratio`` and ``sigma_v_ratio`` (pred / true), plus ``frames``, ``size_lo``, ``size_hi``.  A group
    beyond the last size edge is unbound but in no bin.  The bins are masked sums in a fixed order.  No synchronisation
    per frame, one packed transfer.  Out of scope: as :func:`halo_binding`; the two sides' halos are not matched with
    each other (:func:`rollout_halo_matching`)."""
    what = "rollout_halo_binding"
    dt = _check_dt(what, dt)
    avail = min(len(rollout_data["Coordinates"]), len(ground_truth["Coordinates"]))
    sel = list(range(1, avail)) if frames is None else [int(f) for f in frames]
    if not sel or min(sel) < 1:
        raise ValueError(f"{what}: frames must be numbers in [1, {avail}) (a frame needs its predecessor), got {sel}")
    pc, tc, sel = _rollout_frames(rollout_data, ground_truth, sel, what)
    pp, tp, _ = _rollout_frames(rollout_data, ground_truth, [f - 1 for f in sel], what)
    n = pc.shape[1]
    ll, se = _halo_arguments(n, box_size, linking_length, size_edges, what)
    _check_binding_arguments(what, n, box_size, gm, softening, ll, hubble, iterations)
    sb, nf = len(se) - 1, len(sel)
    parts = []
    for cur, prev in ((pc, pp), (tc, tp)):
        for f in range(nf):
            pos = cur[f].to(torch.float32).contiguous()
            v = _step_velocities(pos, prev[f].to(torch.float32), dt, box_size)
            d = halo_unbinding_on_device(pos, v, box_size, gm, softening, ll, se[0], hubble, None, iterations)
            r = binding_from_sums(d["size"], d["n_bound"], d["kinetic_q"], d["kinetic_scale"], d["peculiar_q"],
                                  d["peculiar_scale"], d["psum_hi"], d["psum_lo"], d["shift"], gm)
            ints, floats = binding_size_bins(d["size"], d["n_bound"], r["bound_fraction"], r["virial_ratio"], r["sigma_v"],
                                             se, se[0])
            parts += [ints.reshape(-1), floats.contiguous().view(torch.int64).reshape(-1)]
    packed = torch.cat(parts).cpu().reshape(2, nf, 8 * sb)                # the one transfer
    sedges = torch.tensor(se, dtype=torch.int64)
    res = {"frames": sel, "size_lo": sedges[:-1].clone(), "size_hi": sedges[1:].clone()}
    for side, name in enumerate(("pred", "true")):
        ints = packed[side, :, :5 * sb].reshape(nf, 5, sb)
        floats = packed[side, :, 5 * sb:].contiguous().view(torch.float64).reshape(nf, 3, sb)
        res["n_groups_" + name], res["spurious_" + name] = ints[:, 0].clone(), ints[:, 1].clone()
        res["bound_counts_" + name] = ints[:, 2].clone()
        res["n_virial_" + name], res["n_sigma_" + name] = ints[:, 3].clone(), ints[:, 4].clone()
        res["bound_fraction_" + name] = floats[:, 0] / ints[:, 0].to(torch.float64)
        res["virial_ratio_" + name] = floats[:, 1] / ints[:, 3].to(torch.float64)
        res["sigma_v_" + name] = floats[:, 2] / ints[:, 4].to(torch.float64)
    res["bound_fraction_ratio"] = res["bound_fraction_pred"] / res["bound_fraction_true"]
    res["sigma_v_ratio"] = res["sigma_v_pred"] / res["sigma_v_true"]
    return res


# ---- k-nearest-neighbour distance distributions ----------------------------------------------------------------------
#
# Everything above is a two-point statistic or a statistic of collapsed objects; two frames can agree in all of it and
# differ in how empty their voids are or in any connected higher-order moment.  The kNN-CDFs (Banerjee & Abel 2021) are
# sensitive to every N-point function at once: from volume-filling query points, the empirical distribution of the
# distance to the k-th nearest particle (``ops.knn_distances``, ``ops.knn_cdf_counts``).  The void probability function
# is ``1 - CDF_1``, the counts-in-spheres distribution ``P(N = k | r) = CDF_k - CDF_{k+1}``, and the joint CDF of two
# particle sets seen from the same queries a cross-correlation beyond r(k).  One box per call; particle-centred
# distributions, batched, sharded and owned-storage variants, random default queries and a loss are not built.


def query_lattice(m: int, box_size: float, device=None) -> torch.Tensor:
    """The volume-filling default queries of the kNN-CDFs: the ``m^3`` cell centres ``fl32((i + 0.5) box_size / m)`` of
    a regular lattice as float32 ``[m^3, 3]``, x slowest.  Deterministic: no random numbers."""
    if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= 1024:
        raise ValueError(f"query_lattice: m must be a whole number in [1, 1024], got {m!r}")
    if not (math.isfinite(float(box_size)) and float(box_size) > 0.0):
        raise ValueError(f"query_lattice: box_size must be positive and finite, got {box_size!r}")
    c = ((torch.arange(m, dtype=torch.float64) + 0.5) * float(box_size) / m).to(torch.float32)
    q = torch.cartesian_prod(c, c, c).reshape(m ** 3, 3)
    return q if device is None else q.to(device)


def default_knn_radii(n: int, box_size: float) -> torch.Tensor:
    """The default radii of the kNN-CDFs: 24 log-spaced radii from 0.1 to 4 mean interparticle spacings ``box_size /
    n ** (1 / 3)``, without those above ``fl32(0.5 * box_size)`` (0.1 spacings never exceed a tenth of the box, so at
    least one remains).  Float32 values as float64, ascending."""
    if int(n) < 1:
        raise ValueError(f"default_knn_radii: n must be at least 1, got {n!r}")
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"default_knn_radii: box_size must be positive and finite, got {box_size!r}")
    spacing = float(box_size) / float(n) ** (1.0 / 3.0)
    r = (spacing * torch.logspace(math.log10(0.1), math.log10(4.0), 24, dtype=torch.float64)).to(torch.float32)
    return r[r <= box * 0.5].to(torch.float64)


def _cdf_counts_on_host(what: str, name: str, below, shape=None) -> torch.Tensor:
    b = torch.as_tensor(below).detach().to(device="cpu")
    if b.dtype.is_floating_point or b.dtype == torch.bool or b.dim() not in (2, 3):
        raise ValueError(f"{what}: {name} must hold integer counts [nk, nr] or [T, nk, nr], got {b.dtype} "
                         f"{tuple(b.shape)}")
    if shape is not None and tuple(b.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} {tuple(b.shape)} does not go with below {tuple(shape)}")
    return b.to(torch.float64)


def knn_cdfs_from_counts(below, n_queries: int, ks, radii, below_b=None, below_joint=None) -> Dict:
    """The kNN-CDFs from the integers of ``ops.knn_cdf_counts``, on the host in float64.  ``below [nk, nr]`` (or ``[T, nk,
    nr]``) for the ranks ``ks`` and the ``nr`` radii, counted over ``n_queries`` queries.  Returns (CPU, float64, in the
    shape of ``below``):

    * ``cdf = below / n_queries``: the fraction of the volume within ``r`` of at least ``k`` particles;
    * ``peaked_cdf = min(cdf, 1 - cdf)``, which shows both tails;
    * ``vpf = 1 - cdf[k = 1]`` (``[nr]`` or ``[T, nr]``), the void probability function, when 1 is among ``ks``;
    * ``counts_in_spheres``: a dict keyed by ``k`` with ``P(N = k | r) = cdf_k - cdf_{k+1}`` for every ``k`` with both
      ``k`` and ``k + 1`` among ``ks``;
    * with ``below_b`` and ``below_joint`` (a second particle set from the same queries, and the counts of the
      elementwise maximum of the two tables; both or neither): ``cdf_b``, ``joint_cdf`` and ``joint_excess = joint_cdf -
      cdf * cdf_b``, which is zero for independent sets,

    plus ``ks`` (a list) and ``radii`` (float64 ``[nr]``)."""
    what = "knn_cdfs_from_counts"
    ranks = ops.check_knn_ranks(ks, what)
    if isinstance(n_queries, bool) or int(n_queries) != n_queries or int(n_queries) < 1:
        raise ValueError(f"{what}: n_queries must be a whole number of at least 1, got {n_queries!r}")
    r = torch.as_tensor(radii).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    b = _cdf_counts_on_host(what, "below", below)
    if b.shape[-2] != len(ranks) or b.shape[-1] != r.numel():
        raise ValueError(f"{what}: below {tuple(b.shape)} for {len(ranks)} ranks and {r.numel()} radii")
    if (below_b is None) != (below_joint is None):
        raise ValueError(f"{what}: below_b and below_joint come together")
    nq = float(int(n_queries))
    cdf = b / nq
    out = {"ks": ranks, "radii": r.clone(), "cdf": cdf, "peaked_cdf": torch.minimum(cdf, 1.0 - cdf)}
    if 1 in ranks:
        out["vpf"] = 1.0 - cdf[..., ranks.index(1), :]
    out["counts_in_spheres"] = {k: cdf[..., i, :] - cdf[..., ranks.index(k + 1), :]
                                for i, k in enumerate(ranks) if k + 1 in ranks}
    if below_b is not None:
        out["cdf_b"] = _cdf_counts_on_host(what, "below_b", below_b, b.shape) / nq
        out["joint_cdf"] = _cdf_counts_on_host(what, "below_joint", below_joint, b.shape) / nq
        out["joint_excess"] = out["joint_cdf"] - cdf * out["cdf_b"]
    return out


def _check_knn_cdf_arguments(what: str, n: int, box_size, radii, ks, queries, n_query_axis, device):
    """Ranks, radii (default :func:`default_knn_radii`) and queries (default :func:`query_lattice`) of a kNN-CDF call,
    checked on the host before any device work."""
    ranks = ops.check_knn_ranks(ks, what)
    if ranks[-1] > 27 * n:
        raise ValueError(f"{what}: rank {ranks[-1]} exceeds the 27 N = {27 * n} periodic images")
    r = ops.check_knn_radii(default_knn_radii(n, box_size) if radii is None else radii, box_size, what)
    if queries is None:
        queries = query_lattice(int(round(n ** (1.0 / 3.0))) if n_query_axis is None else n_query_axis, box_size, device)
    elif n_query_axis is not None:
        raise ValueError(f"{what}: queries and n_query_axis exclude each other")
    elif not torch.is_tensor(queries) or queries.dim() != 2 or queries.shape[1] != 3 or queries.shape[0] < 1:
        raise ValueError(f"{what}: queries must be a tensor [nq, 3] with nq >= 1, got "
                         f"{tuple(queries.shape) if torch.is_tensor(queries) else type(queries).__name__}")
    return ranks, r, queries


def knn_cdfs(pos: torch.Tensor, box_size: float, radii=None, ks=(1, 2, 4, 8), queries: Optional[torch.Tensor] = None,
             n_query_axis: Optional[int] = None, pos_b: Optional[torch.Tensor] = None) -> Dict:
    """The kNN-CDFs of ``pos [N, 3]`` (or of every frame of ``[T, N, 3]``): the keys of :func:`knn_cdfs_from_counts`, plus
    ``below`` (the int64 counts behind ``cdf``) and ``n_queries``.  ``radii``: default :func:`default_knn_radii`;
    ``queries [nq, 3]``: default ``query_lattice(n_query_axis or round(N ** (1 / 3)))``, as many queries as particles.
    With ``pos_b`` (a second set in the shape of ``pos`` up to its number of particles) also ``cdf_b``, ``joint_cdf`` and
    ``joint_excess``, from the same queries.  The counts come back in one transfer."""
    what = "knn_cdfs"
    if not torch.is_tensor(pos):
        raise ValueError(f"{what}: pos must be a tensor, got {type(pos).__name__}")
    frames = _frames3(pos, "pos", what)
    n = frames.shape[1]
    ranks, r, queries = _check_knn_cdf_arguments(what, n, box_size, radii, ks, queries, n_query_axis, pos.device)
    if pos_b is not None:
        if not torch.is_tensor(pos_b) or pos_b.dim() != pos.dim() or _frames3(pos_b, "pos_b", what).shape[0] != frames.shape[0]:
            raise ValueError(f"{what}: pos_b must be frames like pos {tuple(pos.shape)}")
        if ranks[-1] > 27 * pos_b.shape[-2]:
            raise ValueError(f"{what}: rank {ranks[-1]} exceeds the 27 N = {27 * pos_b.shape[-2]} images of pos_b")
    d2 = ops.knn_distances(pos, queries, box_size, ranks)
    counts = [ops.knn_cdf_counts(d2, r, box_size)]
    if pos_b is not None:
        d2_b = ops.knn_distances(pos_b, queries, box_size, ranks)
        counts += [ops.knn_cdf_counts(d2_b, r, box_size), ops.knn_cdf_counts(d2, r, box_size, d2_b)]
    counts = torch.stack(counts).cpu()                                                  # the one transfer
    nq = queries.shape[0]
    out = knn_cdfs_from_counts(counts[0], nq, ranks, r, *(counts[1:] if pos_b is not None else ()))
    out["below"], out["n_queries"] = counts[0], nq
    return out


def rollout_knn_cdfs(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], box_size: float,
                     radii=None, ks=(1, 2, 4, 8), n_query_axis: Optional[int] = None,
                     frames: Optional[Sequence[int]] = None) -> Dict:
    """kNN-CDFs of a rollout against the truth, for the dicts ``rollout.rollout`` returns (``Coordinates [T, N, 3]``): what
    xi(r), P(k) and the halo statistics cannot tell -- whether the voids are as empty and the web as sharp as in the true
    frame.  Both sides are seen from the same lattice of queries (:func:`query_lattice`, ``n_query_axis`` per axis,
    default ``round(N ** (1 / 3))``).  Per selected frame (CPU, float64):

    * ``cdf_pred``, ``cdf_true`` (``[F, nk, nr]``);
    * ``joint_cdf``: the fraction of queries with the k-th neighbour of BOTH frames within ``r``, and ``joint_excess =
      joint_cdf - cdf_pred * cdf_true``;
    * ``vpf_pred``, ``vpf_true`` (``[F, nr]``), when 1 is among ``ks``;
    * ``max_cdf_difference`` (``[F, nk]``): the Kolmogorov distance ``max_r |cdf_pred - cdf_true|`` between the predicted
      and the true distribution per rank, over the given radii,

    plus ``frames``, ``ks``, ``radii`` and ``n_queries``.  No host synchronisation per frame; one transfer."""
    what = "rollout_knn_cdfs"
    n = rollout_data["Coordinates"].shape[-2]
    dev = rollout_data["Coordinates"].device
    ranks, r, queries = _check_knn_cdf_arguments(what, n, box_size, radii, ks, None, n_query_axis, dev)
    pc, tc, sel = _rollout_frames(rollout_data, ground_truth, frames, what)
    d2_p = ops.knn_distances(_f32_frames(pc, "Coordinates", what), queries, box_size, ranks)
    d2_t = ops.knn_distances(_f32_frames(tc, "Coordinates", what), queries, box_size, ranks)
    counts = torch.stack([ops.knn_cdf_counts(d2_p, r, box_size), ops.knn_cdf_counts(d2_t, r, box_size),
                          ops.knn_cdf_counts(d2_p, r, box_size, d2_t)]).cpu()           # [3, F, nk, nr], the one transfer
    nq = queries.shape[0]
    res = knn_cdfs_from_counts(counts[0], nq, ranks, r, counts[1], counts[2])
    out = {"frames": sel, "ks": ranks, "radii": res["radii"], "n_queries": nq, "cdf_pred": res["cdf"],
           "cdf_true": res["cdf_b"], "joint_cdf": res["joint_cdf"], "joint_excess": res["joint_excess"],
           "max_cdf_difference": (res["cdf"] - res["cdf_b"]).abs().amax(dim=-1)}
    if 1 in ranks:
        i = ranks.index(1)
        out["vpf_pred"], out["vpf_true"] = res["vpf"], 1.0 - res["cdf_b"][..., i, :]
    return out


# ---- the bispectrum --------------------------------------------------------------------------------------------------
#
# The three-point function in Fourier space, by the FFT estimator (Scoccimarro 2015).  For shell i of ``k_edges``,
# ``D_i(x) = sum over the shell's modes of delta_k / W e^{ikx}`` (``ops.bispectrum_shells``, ``ops.shell_fields``) and
# ``I_i(x)`` the same with 1 for ``delta_k / W``.  ``sum_x D_i D_j D_l / M^3`` is the sum of ``delta_k1 delta_k2 delta_k3``
# over every closed triangle ``k1 + k2 + k3 = 0`` with one mode in each shell, ``sum_x I_i I_j I_l / M^3`` their number
# (``ops.BispectrumPlan.counts``) -- as long as ``k1 + k2 + k3 = 0 (mod M)`` means ``= 0``: ``3 k_edges[-1] <= mesh``.
# Cross-bispectra of two fields, interlacing (every shell lies at or below a third of the mesh, where aliasing is
# mild), redshift-space multipoles of B, a float32 path, batched, sharded and owned-storage variants, a bispectrum
# loss and more than 32 shells are not built.


def default_bispectrum_edges(mesh: int, num_shells: Optional[int] = None) -> torch.Tensor:
    """Equal-width shells from 0.5 up to the largest edge at or below ``mesh / 3`` (float64, units of ``2 pi / L``):
    ``num_shells`` of them, by default ``min(16, floor(mesh / 3 - 0.5))`` and at least one.  The width is the largest
    whole number that fits, so the shells stay centred on whole frequencies (mesh 256: 16 shells of width 5 up to 80.5;
    mesh 32 with 4 shells: 0.5, 2.5, .., 8.5); where not even width 1 fits, the shells divide ``[0.5, mesh / 3]``."""
    mesh = ops.check_mesh(mesh, "default_bispectrum_edges")
    span = mesh / 3.0 - 0.5
    if num_shells is None:
        num_shells = max(1, min(16, int(math.floor(span))))
    if isinstance(num_shells, bool) or int(num_shells) != num_shells or not 1 <= num_shells <= _lib.BISPECTRUM_MAX_SHELLS:
        raise ValueError(f"default_bispectrum_edges: num_shells must be a whole number in [1, "
                         f"{_lib.BISPECTRUM_MAX_SHELLS}], got {num_shells!r}")
    num_shells = int(num_shells)
    width = float(math.floor(span / num_shells))
    if width < 1.0:
        width = span / num_shells
    edges = 0.5 + width * torch.arange(num_shells + 1, dtype=torch.float64)
    edges[-1] = min(float(edges[-1]), ops.bispectrum_top_edge(mesh))      # a fractional width may overshoot by an ulp
    return edges


def bispectrum_from_sums(counts, triangle_sums, triangles, modes, sums, n: int, box_size: float, mesh: int, k_edges,
                         subtract_shot_noise: bool = True) -> Dict:
    """The bispectrum from the triangle sums, on the host in float64: a pure function of ``counts [nt]`` (the closed
    triangles of modes per listed triple, ``ops.BispectrumPlan.counts``), ``triangle_sums [..., nt]`` (``sum_x D_i D_j
    D_l`` as ``ops.bispectrum_sums`` gives it), ``triangles [nt, 3]``, the ``modes [..., nb]`` and ``sums [..., 4, nb]``
    of ``ops.power_bins`` on the same edges, the number of particles ``n``, ``L = box_size`` and ``M = mesh``.  With
    ``P^_i = L^3 S_i / modes_i / M^6`` the shell power with its shot noise, ``nbar = n / L^3`` and ``N`` the count:

    * ``bispectrum``: ``B_meas = L^6 / M^9 (triangle_sums / M^3) / N``, and with ``subtract_shot_noise``
      ``B = B_meas - (P^_i + P^_j + P^_l) / nbar + 2 / nbar^2``; ``nan`` where ``N == 0``;
    * ``power`` ``[..., nb]``: ``P = P^ - 1 / nbar`` with ``subtract_shot_noise``, else ``P^``;
    * ``reduced_bispectrum``: ``Q = B / (P_i P_j + P_j P_l + P_l P_i)`` from that ``power``;
    * ``gaussian_sigma``: ``sqrt(s L^3 P^_i P^_j P^_l / N)`` with ``s`` = 6, 2 or 1 for three, two or no equal shell
      indices: the scatter of ``B`` for a Gaussian field of that power;
    * ``k1``, ``k2``, ``k3``: the mean ``|k|`` of the three shells (row 3 of ``power_bins``);

    plus ``triangles`` (int64 ``[nt, 3]``) and ``count`` (int64 ``[nt]``).  CPU, float64, ``[..., nt]``."""
    what = "bispectrum_from_sums"
    box, _, modes, sums, shell_modes, norm = _sums_on_host(what, modes, sums, 4, box_size, mesh, k_edges)
    nb = modes.shape[-1]
    tri = ops.check_triangles(torch.as_tensor(triangles).detach().cpu(), nb, what).to(torch.int64)
    count = torch.as_tensor(counts).detach().to(device="cpu", dtype=torch.int64).reshape(-1)
    ts = torch.as_tensor(triangle_sums).detach().to(device="cpu", dtype=torch.float64)
    if count.numel() != tri.shape[0] or ts.shape[-1] != tri.shape[0] or ts.shape[:-1] != modes.shape[:-1]:
        raise ValueError(f"{what}: counts {tuple(count.shape)}, triangle_sums {tuple(ts.shape)} and modes "
                         f"{tuple(modes.shape)} do not fit {tri.shape[0]} triangles")
    if isinstance(n, bool) or int(n) != n or int(n) < 1:
        raise ValueError(f"{what}: n must be a whole number of at least 1, got {n!r}")
    m = float(mesh)
    nbar = int(n) / box ** 3
    p_hat = norm * sums[..., 0, :] / shell_modes
    power = p_hat - 1.0 / nbar if subtract_shot_noise else p_hat
    i, j, l = tri[:, 0], tri[:, 1], tri[:, 2]
    num = count.to(torch.float64)
    num = torch.where(count > 0, num, torch.full_like(num, float("nan")))
    b = box ** 6 / m ** 9 * (ts / m ** 3) / num
    hi, hj, hl = p_hat[..., i], p_hat[..., j], p_hat[..., l]
    if subtract_shot_noise:
        b = b - (hi + hj + hl) / nbar + 2.0 / nbar ** 2
    pi, pj, pl = power[..., i], power[..., j], power[..., l]
    sym = torch.where((i == j) & (j == l), 6.0, torch.where((i == j) | (j == l), 2.0, 1.0)).to(torch.float64)
    k_mean = sums[..., 3, :] / shell_modes * (2.0 * math.pi / box)
    return {"triangles": tri, "count": count, "k1": k_mean[..., i], "k2": k_mean[..., j], "k3": k_mean[..., l],
            "bispectrum": b, "reduced_bispectrum": b / (pi * pj + pj * pl + pl * pi), "power": power,
            "gaussian_sigma": torch.sqrt(sym * box ** 3 * hi * hj * hl / num)}


def _check_bispectrum_arguments(what: str, box_size, mesh, k_edges, order):
    mesh = ops.check_mesh(mesh, what)
    mesh, k_edges = ops.check_bispectrum_edges(mesh, default_bispectrum_edges(mesh) if k_edges is None else k_edges, what)
    if isinstance(order, bool) or order not in (1, 2, 3):
        raise ValueError(f"{what}: order must be 1 (NGP), 2 (CIC) or 3 (TSC), got {order!r}")
    if not (float(box_size) > 0.0 and math.isfinite(float(box_size))):
        raise ValueError(f"{what}: box_size must be positive and finite, got {box_size!r}")
    return mesh, k_edges


def _triangle_sums(sets, box_size: float, mesh: int, k_edges, order: int):
    """For every set of frames ``[F, N, 3]`` in ``sets`` the device tensors ``(modes [F, nb], sums [F, 4, nb],
    triangle_sums [F, nt])`` of its density contrast, and the :class:`ops.BispectrumPlan`.  Frames go through in chunks
    that fit the free device memory: per frame and set ``nb 16 M^2 (M/2 + 1)`` bytes of filtered modes, ``nb 8 M^3`` of
    shell fields and the contrast, its transform and the int64 mesh of ``_shell_sums``, and as much again for the FFT's
    scratch.  The filtered modes of a chunk are gone before its triangle sums are made, its fields before the next chunk."""
    from .training import free_device_bytes
    n_frames, nb, dev = sets[0].shape[0], len(k_edges) - 1, sets[0].device
    half = mesh * mesh * (mesh // 2 + 1)
    per_frame = 2 * (nb * (16 * half + 8 * mesh ** 3) + 16 * mesh ** 3 + 16 * half) * len(sets)
    chunk = max(1, min(n_frames, free_device_bytes(dev) // per_frame))
    plan = ops.BispectrumPlan.of(mesh, k_edges, dev)
    power_plan = ops.PowerPlan.of(mesh, k_edges, dev)
    out = [([], [], []) for _ in sets]
    for f0 in range(0, n_frames, chunk):
        for pos, (modes, sums, tsums) in zip(sets, out):
            delta_k = _contrast_modes(pos[f0:f0 + chunk], box_size, mesh, order)
            m, s = ops.power_bins(delta_k, mesh, order, k_edges, None, power_plan)
            filtered = ops.bispectrum_shells(delta_k, mesh, order, k_edges, plan)
            del delta_k
            fields = ops.shell_fields(filtered, mesh)
            del filtered
            tsums.append(ops.bispectrum_sums(fields.reshape(fields.shape[0], nb, -1), plan.triangles))
            del fields
            modes.append(m)
            sums.append(s)
    return [tuple(p[0] if len(p) == 1 else torch.cat(p) for p in parts) for parts in out], plan


def bispectrum(pos: torch.Tensor, box_size: float, mesh: int, k_edges=None, order: int = 2,
               subtract_shot_noise: bool = True) -> Dict:
    """The bispectrum of ``pos [N, 3]`` (or of every frame of ``[T, N, 3]``) on a ``mesh^3`` grid, deposited with
    ``order`` (1 = NGP, 2 = CIC, 3 = TSC) and deconvolved by that window, for every triple of the shells ``k_edges``
    (``nb + 1 <= 33`` edges in units of ``2 pi / L`` with ``3 k_edges[-1] <= mesh``; default
    :func:`default_bispectrum_edges`) that can hold a closed triangle.  Returns the dict of :func:`bispectrum_from_sums`
    (CPU; ``[nt]`` or ``[T, nt]``, ``power`` ``[nb]`` or ``[T, nb]``).  Everything is computed on the device of ``pos``
    without a host synchronisation and comes back in one transfer."""
    what = "bispectrum"
    mesh, k_edges = _check_bispectrum_arguments(what, box_size, mesh, k_edges, order)
    frames = _frames3(pos, "pos", what)
    ((modes, sums, tsums),), plan = _triangle_sums([frames], box_size, mesh, k_edges, order)
    modes, sums, tsums, counts = _to_host(modes, sums, tsums, plan.counts)
    if pos.dim() == 2:
        modes, sums, tsums = modes[0], sums[0], tsums[0]
    return bispectrum_from_sums(counts, tsums, plan.triangles, modes, sums, frames.shape[1], box_size, mesh, k_edges,
                                subtract_shot_noise)


def rollout_bispectra(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], box_size: float,
                      mesh: int, k_edges=None, order: int = 2, frames: Optional[Sequence[int]] = None) -> Dict:
    """Bispectra of a rollout against the truth, for the dicts ``rollout.rollout`` returns (``Coordinates [T, N, 3]``):
    two frames can agree in P(k), r(k) and T(k) and still have the wrong filaments, and the amplitude and the shape
    dependence of B are where that shows first.  ``frames``: the frame numbers to judge (default: every frame both
    hold).  Per selected frame (CPU, float64, ``[F, nt]``; shot noise subtracted):

    * ``bispectrum_pred``, ``bispectrum_true``, ``reduced_bispectrum_pred``, ``reduced_bispectrum_true``;
    * ``power_pred``, ``power_true`` (``[F, nb]``): the shell power behind Q;
    * ``bispectrum_ratio = B_pred / B_true``;
    * ``gaussian_sigma_true`` and ``difference_sigma = (B_pred - B_true) / gaussian_sigma_true``,

    plus ``frames``, ``triangles`` (``[nt, 3]``), ``count`` (``[nt]``), ``k1``, ``k2``, ``k3`` (``[nt]``, of the first
    true frame: the shells' mean ``|k|`` depend on the mesh alone) and ``equilateral``, the indices of the ``i = j = l``
    triangles.  No host synchronisation per frame; one transfer at the end."""
    what = "rollout_bispectra"
    mesh, k_edges = _check_bispectrum_arguments(what, box_size, mesh, k_edges, order)
    pc, tc, sel = _rollout_frames(rollout_data, ground_truth, frames, what)
    n = pc.shape[1]
    (pred, true), plan = _triangle_sums([pc, tc], box_size, mesh, k_edges, order)
    host = _to_host(*pred, *true, plan.counts)
    counts = host[6]
    p = bispectrum_from_sums(counts, host[2], plan.triangles, host[0], host[1], n, box_size, mesh, k_edges)
    t = bispectrum_from_sums(counts, host[5], plan.triangles, host[3], host[4], n, box_size, mesh, k_edges)
    tri = t["triangles"]
    return {"frames": sel, "triangles": tri, "count": t["count"], "k1": t["k1"][0].clone(), "k2": t["k2"][0].clone(),
            "k3": t["k3"][0].clone(), "bispectrum_pred": p["bispectrum"], "bispectrum_true": t["bispectrum"],
            "reduced_bispectrum_pred": p["reduced_bispectrum"], "reduced_bispectrum_true": t["reduced_bispectrum"],
            "power_pred": p["power"], "power_true": t["power"], "gaussian_sigma_true": t["gaussian_sigma"],
            "bispectrum_ratio": p["bispectrum"] / t["bispectrum"],
            "difference_sigma": (p["bispectrum"] - t["bispectrum"]) / t["gaussian_sigma"],
            "equilateral": torch.nonzero((tri[:, 0] == tri[:, 1]) & (tri[:, 1] == tri[:, 2])).reshape(-1).tolist()}


# ---- the three-point correlation function ----------------------------------------------------------------------------
#
# The bispectrum's partner below the mesh: the connected three-point function in configuration space, as Legendre
# multipoles in the angle between the two sides of a triangle that meet at a primary,
#     zeta(r1, r2, u1 . u2) = sum_l zeta_l(r1, r2) P_l(u1 . u2),
# by the O(N neighbours) algorithm of Slepian & Eisenstein (2015): per primary and radial bin the sums of the monomials
# of the unit vectors to its neighbours, contracted over two bins of the same primary (``ops.triplet_moments``).  The
# device returns the power sums of ``(u1 . u2)^n``; the Legendre polynomials are finite combinations of those.  Not
# built: random catalogues and edge correction (a periodic box needs neither), ``l > 4`` and more than 16 bins, error
# bars for zeta, the redshift-space 3PCF, batched, sharded and owned-storage variants, a loss, and the accumulation of
# the moments on the float64 matrix instruction.

# c[l][n]: P_l(x) = sum_n c[l][n] x^n; every coefficient up to l = 4 is a dyadic rational, exact in float64
_LEGENDRE = ((1.0,), (0.0, 1.0), (-0.5, 0.0, 1.5), (0.0, -1.5, 0.0, 2.5), (0.375, 0.0, -3.75, 0.0, 4.375))


def legendre_coefficients(lmax: int) -> torch.Tensor:
    """``c [lmax + 1, lmax + 1]`` float64 with ``P_l(x) = sum_n c[l, n] x^n`` for ``0 <= lmax <= 4``."""
    if isinstance(lmax, bool) or not isinstance(lmax, int) or not 0 <= lmax <= _lib.THREE_POINT_MAX_L:
        raise ValueError(f"legendre_coefficients: lmax must be a whole number in [0, {_lib.THREE_POINT_MAX_L}], got {lmax!r}")
    c = torch.zeros((lmax + 1, lmax + 1), dtype=torch.float64)
    for l in range(lmax + 1):
        c[l, :l + 1] = torch.tensor(_LEGENDRE[l], dtype=torch.float64)
    return c


def default_three_point_edges(n: int, box_size: float) -> torch.Tensor:
    """The default radii of the three-point function: 8 equal bins from 0.5 to 4.5 mean interparticle spacings
    ``box_size / n ** (1 / 3)``, without the radii above ``fl32(0.5 * box_size)``.  At least one bin remains from 8
    particles on (one spacing is then at most half the box).  Float32 values as float64, ascending."""
    if int(n) < 8:
        raise ValueError(f"default_three_point_edges: n must be at least 8, got {n!r}")
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"default_three_point_edges: box_size must be positive and finite, got {box_size!r}")
    spacing = float(box_size) / float(n) ** (1.0 / 3.0)
    r = (spacing * torch.linspace(0.5, 4.5, 9, dtype=torch.float64)).to(torch.float32)
    return r[r <= box * 0.5].to(torch.float64)


def three_point_from_sums(T, n_primaries: int, n_partners: int, box_size: float, edges, unit_bits: int = 20,
                          pairs=None) -> Dict:
    """The Legendre multipoles of the triplet counts from the power sums of ``ops.triplet_moments``, on the host in
    float64.  ``T [lmax + 1, nb, nb]`` (or ``[F, lmax + 1, nb, nb]``) and, to take the degenerate triangles out, ``pairs
    [nb]`` (``[F, nb]``), counted over ``n_primaries`` primaries with ``n_partners`` neighbours in the box:

    * ``S_n = T[n] / 2^(2 unit_bits)`` for ``n >= 1`` and ``S_0 = T[0]``: the sums of ``(u1 . u2)^n``;
    * ``ddd[l] = sum_n c[l, n] S_n`` (:func:`legendre_coefficients`): the sum of ``P_l(u1 . u2)`` over every primary and
      its neighbours ``j`` in ``b1`` and ``k`` in ``b2``.  On the diagonal ``b1 == b2`` the sum includes ``j == k``, a
      triangle that is none and adds ``P_l(1) = 1``: with ``pairs`` the counted pairs of the bin are subtracted
      there, for every ``l``; without, nothing is;
    * ``triplet[l] = (2 l + 1) ddd[l] / (n_primaries nbar^2 V_b1 V_b2)`` with ``nbar = n_partners / L^3`` and ``V_b = 4 pi /
      3 (r_{b+1}^3 - r_b^3)`` from the float64 values of the float32 edges: the l-th multipole of the triplet density
      around a primary in units of the uncorrelated one (``triplet[0] = 1`` and the others 0 for neighbours without
      correlations).

    Returns ``{"ddd", "triplet", "r_lo", "r_hi"}`` (CPU, float64, in the shape of ``T``)."""
    what = "three_point_from_sums"
    t = torch.as_tensor(T).detach().to(device="cpu", dtype=torch.float64)
    if t.dim() not in (3, 4) or t.shape[-1] != t.shape[-2] or not 1 <= t.shape[-3] <= _lib.THREE_POINT_MAX_L + 1:
        raise ValueError(f"{what}: T must be [lmax + 1, nb, nb] or [F, lmax + 1, nb, nb] with lmax <= "
                         f"{_lib.THREE_POINT_MAX_L}, got {tuple(t.shape)}")
    lmax, nb = t.shape[-3] - 1, t.shape[-1]
    r = torch.tensor(ops.check_triplet_arguments(edges, box_size, lmax, unit_bits, what), dtype=torch.float64)
    if r.numel() - 1 != nb:
        raise ValueError(f"{what}: T holds {nb} bins, edges {r.numel() - 1}")
    for name, v in (("n_primaries", n_primaries), ("n_partners", n_partners)):
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise ValueError(f"{what}: {name} must be a whole number of at least 1, got {v!r}")
    scale = torch.ones(lmax + 1, dtype=torch.float64)
    scale[1:] = 2.0 ** (-2 * unit_bits)
    s = t * scale[:, None, None]
    ddd = torch.einsum("ln,...nab->...lab", legendre_coefficients(lmax), s)
    if pairs is not None:
        p = torch.as_tensor(pairs).detach().to(device="cpu")
        if p.dtype.is_floating_point or p.dtype == torch.bool or tuple(p.shape) != tuple(t.shape[:-3]) + (nb,):
            raise ValueError(f"{what}: pairs must hold integer counts {list(t.shape[:-3]) + [nb]}, got {p.dtype} "
                             f"{tuple(p.shape)}")
        ddd = ddd - torch.diag_embed(p.to(torch.float64)).unsqueeze(-3)
    vol = _shell_volumes(r)
    nbar = float(int(n_partners)) / float(box_size) ** 3
    norm = float(int(n_primaries)) * nbar * nbar * vol[:, None] * vol[None, :]
    ell = (2.0 * torch.arange(lmax + 1, dtype=torch.float64) + 1.0)[:, None, None]
    return {"ddd": ddd, "triplet": ell * ddd / norm, "r_lo": r[:-1].clone(), "r_hi": r[1:].clone()}


def three_point_zeta(T_data, pairs_data, T_queries, pairs_queries, n: int, n_queries: int, box_size: float, edges,
                     unit_bits: int = 20) -> Dict:
    """The connected multipoles from two calls of ``ops.triplet_moments`` on the same ``n`` particles, on the host in
    float64: the particles as primaries (auto) and ``n_queries`` volume-filling points as primaries (cross).  Around a
    particle the expected triplet density is ``1 + xi_1 + xi_2 + xi_3 + zeta``, around a random point ``1 + xi_3``:

        ``zeta_l = triplet_l(data) - triplet_l(queries) - delta_{l0} (xibar_b1 + xibar_b2)``

    with ``xibar_b = pairs_b / (n nbar V_b) - 1`` from the auto call's ``pairs``.  Returns ``zeta``, ``zeta_full`` (``=
    triplet_l(data) - delta_{l0}``), ``triplet_queries``, ``xi`` (``[nb]`` or ``[F, nb]``), ``pairs`` (the auto call's,
    int64), ``r_lo`` and ``r_hi``."""
    d = three_point_from_sums(T_data, n, n, box_size, edges, unit_bits, pairs_data)
    q = three_point_from_sums(T_queries, n_queries, n, box_size, edges, unit_bits, pairs_queries)
    p = torch.as_tensor(pairs_data).detach().to(device="cpu")
    vol = _shell_volumes(torch.cat([d["r_lo"], d["r_hi"][-1:]]))
    xi = p.to(torch.float64) / (float(n) * (float(n) / float(box_size) ** 3) * vol) - 1.0
    full = d["triplet"].clone()
    full[..., 0, :, :] -= 1.0
    zeta = d["triplet"] - q["triplet"]
    zeta[..., 0, :, :] -= xi[..., :, None] + xi[..., None, :]
    return {"zeta": zeta, "zeta_full": full, "triplet_queries": q["triplet"], "xi": xi, "pairs": p,
            "r_lo": d["r_lo"], "r_hi": d["r_hi"]}


def _check_three_point_arguments(what: str, n: int, box_size, edges, lmax, queries, n_query_axis, device):
    """Radii (default :func:`default_three_point_edges`) and queries (default :func:`query_lattice`) of a three-point
    call, checked on the host before any device work."""
    e = ops.check_triplet_arguments(default_three_point_edges(n, box_size) if edges is None else edges, box_size, lmax,
                                    _lib.THREE_POINT_MAX_UNIT_BITS, what)
    if queries is None:
        queries = query_lattice(max(1, int(round(n ** (1.0 / 3.0)))) if n_query_axis is None else n_query_axis, box_size,
                                device)
    elif n_query_axis is not None:
        raise ValueError(f"{what}: queries and n_query_axis exclude each other")
    elif not torch.is_tensor(queries) or queries.dim() != 2 or queries.shape[1] != 3 or queries.shape[0] < 1:
        raise ValueError(f"{what}: queries must be a tensor [nq, 3] with nq >= 1, got "
                         f"{tuple(queries.shape) if torch.is_tensor(queries) else type(queries).__name__}")
    return e, queries


def triplet_sums_on_device(frames: torch.Tensor, queries: torch.Tensor, box_size: float, e, lmax: int) -> torch.Tensor:
    """Both calls of a three-point estimate for ``frames [F, N, 3]`` as one int64 tensor ``[F, 2 ((lmax + 1) nb^2 + nb)]``:
    per call the bits of the float64 sums, then the pairs; the particles as primaries first, then the queries."""
    f = frames.shape[0]
    out = []
    for pos, pos_b in ((frames, None), (queries.to(frames.device).unsqueeze(0).expand(f, -1, -1), frames)):
        sums, pairs = ops.triplet_moments(pos, box_size, e, lmax, pos_b, return_pairs=True)
        out += [sums.reshape(f, -1).view(torch.int64), pairs]
    return torch.cat(out, dim=1)


def triplet_sums_on_host(packed: torch.Tensor, lmax: int, nb: int):
    """``(T_data, pairs_data, T_queries, pairs_queries)`` from the host copy of :func:`triplet_sums_on_device`."""
    m = (lmax + 1) * nb * nb
    shape = (packed.shape[0], lmax + 1, nb, nb)
    call = [packed[:, :m + nb], packed[:, m + nb:]]
    return tuple(x for c in call for x in (c[:, :m].contiguous().view(torch.float64).reshape(shape), c[:, m:]))


def three_point_correlation(pos: torch.Tensor, box_size: float, edges=None, lmax: int = 4,
                            queries: Optional[torch.Tensor] = None, n_query_axis: Optional[int] = None) -> Dict:
    """The multipoles ``zeta_l(r1, r2)``, ``l = 0 .. lmax``, of the connected three-point correlation function of ``pos
    [N, 3]`` (or of every frame of ``[T, N, 3]``): the dict of :func:`three_point_zeta` (CPU; ``zeta [lmax + 1, nb, nb]``
    with a leading ``T`` for frames), plus ``n_queries``.  ``edges``: default :func:`default_three_point_edges`, at most
    16 bins; ``queries [nq, 3]``: default ``query_lattice(n_query_axis or round(N ** (1 / 3)))``, about as many queries
    as particles.  Two device calls per frame -- the particles as primaries, and the queries as primaries against the
    particles -- without a host synchronisation; the sums come back in one transfer.  On the diagonal ``r1 == r2`` the
    degenerate triangles are taken out; the bins there still hold triangles with two sides in the same shell."""
    what = "three_point_correlation"
    if not torch.is_tensor(pos):
        raise ValueError(f"{what}: pos must be a tensor, got {type(pos).__name__}")
    frames = _frames3(pos, "pos", what)
    n = frames.shape[1]
    e, queries = _check_three_point_arguments(what, n, box_size, edges, lmax, queries, n_query_axis, pos.device)
    packed = triplet_sums_on_device(_f32_frames(frames, "pos", what), queries, box_size, e, lmax).cpu()   # the one transfer
    host = triplet_sums_on_host(packed, lmax, len(e) - 1)
    if pos.dim() == 2:
        host = tuple(x[0] for x in host)
    out = three_point_zeta(*host, n, queries.shape[0], box_size, e)
    out["n_queries"] = queries.shape[0]
    return out


def rollout_three_point(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], box_size: float,
                        edges=None, lmax: int = 4, frames: Optional[Sequence[int]] = None,
                        n_query_axis: Optional[int] = None) -> Dict:
    """Three-point multipoles of a rollout against the truth, for the dicts ``rollout.rollout`` returns (``Coordinates
    [T, N, 3]``): in which configurations, below the mesh, the predicted frame differs -- filaments raise ``zeta_2``
    against ``zeta_0``, round blobs do not.  Both sides are seen from the same lattice of queries (``n_query_axis`` per
    axis, default ``round(N ** (1 / 3))``).  Per selected frame (CPU, float64, ``[F, lmax + 1, nb, nb]``):

    * ``zeta_pred``, ``zeta_true``;
    * ``zeta_difference = zeta_pred - zeta_true`` and ``zeta_ratio = zeta_pred / zeta_true``;
    * ``xi_pred``, ``xi_true`` (``[F, nb]``), the shell-averaged two-point function behind the ``l = 0`` subtraction,

    plus ``frames``, ``r_lo``, ``r_hi`` and ``n_queries``.  No host synchronisation per frame; one transfer at the
    end."""
    what = "rollout_three_point"
    n = rollout_data["Coordinates"].shape[-2]
    dev = rollout_data["Coordinates"].device
    e, queries = _check_three_point_arguments(what, n, box_size, edges, lmax, None, n_query_axis, dev)
    pc, tc, sel = _rollout_frames(rollout_data, ground_truth, frames, what)
    packed = torch.stack([triplet_sums_on_device(_f32_frames(x, "Coordinates", what), queries, box_size, e, lmax)
                          for x in (pc, tc)]).cpu()                                     # the one transfer
    nb, nq = len(e) - 1, queries.shape[0]
    p = three_point_zeta(*triplet_sums_on_host(packed[0], lmax, nb), n, nq, box_size, e)
    t = three_point_zeta(*triplet_sums_on_host(packed[1], lmax, nb), n, nq, box_size, e)
    return {"frames": sel, "r_lo": t["r_lo"], "r_hi": t["r_hi"], "n_queries": nq, "zeta_pred": p["zeta"],
            "zeta_true": t["zeta"], "zeta_difference": p["zeta"] - t["zeta"], "zeta_ratio": p["zeta"] / t["zeta"],
            "xi_pred": p["xi"], "xi_true": t["xi"]}


# ---- morphology: the Minkowski functionals of the density field --------------------------------------------------------
#
# What none of the statistics above says: how much volume lies above a density threshold, how much surface bounds it, how
# curved that surface is and how connected the set is.  Two frames can agree in P(k) and roughly in B and still differ
# here -- in one the filaments percolate into a network, in the other they break into blobs.  The four Minkowski
# functionals V0 .. V3 of the excursion sets of the smoothed density field measure exactly this, and their departure from
# the Gaussian curves, as a function of the threshold, is sensitive to every order of correlation at once.  On a mesh
# they reduce to exact integer counts of the cubes, faces, edges and vertices of a cubical complex (Schmalzing & Buchert
# 1997, Crofton's formula): ``ops.excursion_counts`` reads the field once for all thresholds.  Not built: float32 fields,
# per-voxel masks, Minkowski tensors and the Betti numbers, marching-cubes / Koenderink estimators, a genus convention
# (``euler`` is reported; periodic conventions for the genus differ), error bars, redshift-space fields, batched, sharded
# and owned-storage variants, and a morphology loss.

def default_minkowski_thresholds() -> torch.Tensor:
    """The default thresholds of the Minkowski functionals: 25 values from -3 to 3 (float64), in units of the field's
    standard deviation under ``threshold_units="sigma"``."""
    return torch.linspace(-3.0, 3.0, 25, dtype=torch.float64)


def minkowski_from_counts(counts, mesh: int, box_size: float) -> Dict:
    """The Minkowski functionals per unit volume from the integers of ``ops.excursion_counts``, on the host in float64.
    ``counts [4, nt]`` (or ``[F, 4, nt]``): per threshold the vertices ``n0``, edges ``n1``, faces ``n2`` and cubes ``n3``
    of the excursion set on a periodic ``mesh^3`` grid of cells of side ``a = box_size / mesh``; with ``N = mesh^3``

    * ``v0 = n3 / N``: the volume fraction;
    * ``v1 = 2 (n2 - 3 n3) / (9 a N)``: a sixth of the surface per unit volume;
    * ``v2 = 2 (n1 - 2 n2 + 3 n3) / (9 a^2 N)``: the integrated mean curvature, over ``3 pi``, per unit volume;
    * ``v3 = (n0 - n1 + n2 - n3) / (a^3 N)``: the Euler characteristic per unit volume;
    * ``euler = n0 - n1 + n2 - n3`` (int64).  No genus: periodic conventions differ.

    The factors 2/9 are Crofton's average over the orientations of a cubic lattice, the convention under which the
    functionals of a mesh converge to those of the continuum for an isotropic field: a single cube therefore reports
    2/3 of its geometric surface, by design.  Returns ``{"v0", "v1", "v2", "v3", "euler", "counts"}`` (CPU, in the shape
    of ``counts`` without its axis of 4)."""
    what = "minkowski_from_counts"
    mesh = ops.check_mesh(mesh, what)
    if not (float(box_size) > 0.0 and math.isfinite(float(box_size))):
        raise ValueError(f"{what}: box_size must be positive and finite, got {box_size!r}")
    c = torch.as_tensor(counts).detach().to(device="cpu")
    if c.dtype.is_floating_point or c.dtype == torch.bool or c.dim() not in (2, 3) or c.shape[-2] != 4 or c.shape[-1] < 1:
        raise ValueError(f"{what}: counts must hold integers [4, nt] or [F, 4, nt], got {c.dtype} {tuple(c.shape)}")
    c = c.to(torch.int64)
    n0, n1, n2, n3 = c[..., 0, :], c[..., 1, :], c[..., 2, :], c[..., 3, :]
    a, cells = float(box_size) / mesh, float(mesh) ** 3
    euler = n0 - n1 + n2 - n3
    return {"v0": n3.to(torch.float64) / cells,
            "v1": 2.0 * (n2 - 3 * n3).to(torch.float64) / (9.0 * a * cells),
            "v2": 2.0 * (n1 - 2 * n2 + 3 * n3).to(torch.float64) / (9.0 * a * a * cells),
            "v3": euler.to(torch.float64) / (a ** 3 * cells), "euler": euler, "counts": c}


def gaussian_minkowski(nu, sigma0, sigma1) -> Dict:
    """What a Gaussian random field gives (Tomita 1986; Schmalzing & Buchert 1997), in float64 on the host: with ``lam =
    sqrt(sigma1^2 / (6 pi sigma0^2))``, ``sigma0^2`` the variance of the field and ``sigma1^2`` that of its gradient,

    * ``v0 = erfc(nu / sqrt 2) / 2``;
    * ``v1 = (2 / 3) (lam / sqrt(2 pi)) exp(-nu^2 / 2)``;
    * ``v2 = (2 / 3) (lam^2 / sqrt(2 pi)) nu exp(-nu^2 / 2)``;
    * ``v3 = (lam^3 / sqrt(2 pi)) (nu^2 - 1) exp(-nu^2 / 2)``

    in the normalisation of :func:`minkowski_from_counts`.  ``nu [nt]``: thresholds in units of ``sigma0``; ``sigma0``,
    ``sigma1``: numbers, or ``[F]`` for curves ``[F, nt]``.  Returns ``{"v0", "v1", "v2", "v3", "lam"}``."""
    what = "gaussian_minkowski"
    nu = torch.as_tensor(nu).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    s0 = torch.as_tensor(sigma0).detach().to(device="cpu", dtype=torch.float64)
    s1 = torch.as_tensor(sigma1).detach().to(device="cpu", dtype=torch.float64)
    if nu.numel() < 1 or not bool(torch.isfinite(nu).all()):
        raise ValueError(f"{what}: nu must hold at least one finite value")
    if s0.shape != s1.shape or s0.dim() > 1:
        raise ValueError(f"{what}: sigma0 and sigma1 must be two numbers or two tensors [F], got {tuple(s0.shape)} and "
                         f"{tuple(s1.shape)}")
    if bool((s0 <= 0).any()) or bool((s1 < 0).any()):
        raise ValueError(f"{what}: sigma0 must be positive and sigma1 not negative")
    lam = torch.sqrt(s1 * s1 / (6.0 * math.pi * s0 * s0))
    l = lam[..., None] if lam.dim() else lam
    g = torch.exp(-0.5 * nu * nu) / math.sqrt(2.0 * math.pi)
    return {"v0": (0.5 * torch.erfc(nu / math.sqrt(2.0))).expand(tuple(s0.shape) + nu.shape).clone(),
            "v1": (2.0 / 3.0) * l * g, "v2": (2.0 / 3.0) * l * l * nu * g, "v3": l ** 3 * (nu * nu - 1.0) * g, "lam": lam}


def _check_minkowski_arguments(what: str, box_size, mesh, smoothing, thresholds, order, threshold_units):
    """Mesh and thresholds (default :func:`default_minkowski_thresholds`) of a Minkowski call, checked on the host before
    any device work -> ``(mesh, thresholds as float64 host values)``."""
    mesh = ops.check_mesh(mesh, what)
    if isinstance(order, bool) or order not in (1, 2, 3):
        raise ValueError(f"{what}: order must be 1 (NGP), 2 (CIC) or 3 (TSC), got {order!r}")
    if not (float(box_size) > 0.0 and math.isfinite(float(box_size))):
        raise ValueError(f"{what}: box_size must be positive and finite, got {box_size!r}")
    if isinstance(smoothing, bool) or not math.isfinite(smoothing) or smoothing < 0:
        raise ValueError(f"{what}: smoothing must be a finite length >= 0, got {smoothing!r}")
    if threshold_units not in ("sigma", "contrast"):
        raise ValueError(f"{what}: threshold_units must be 'sigma' or 'contrast', got {threshold_units!r}")
    nu = ops.check_excursion_thresholds(default_minkowski_thresholds() if thresholds is None else thresholds, what)
    return mesh, nu


def _minkowski_filters(mesh: int, box_size: float, smoothing: float, dev):
    """``(kernel, k2w)`` on the modes of ``rfftn`` (float64 ``[M, M, M/2 + 1]``): the Gaussian of
    ``losses.gaussian_filter`` (``None`` without smoothing), and ``|k|^2`` times the number of modes a stored one stands
    for (the Hermitian weights of the half axis: 1 at ``n_z = 0`` and at the Nyquist plane of an even mesh, 2 between)."""
    from .losses import gaussian_filter
    n = torch.fft.fftfreq(mesh, 1.0 / mesh, dtype=torch.float64, device=dev)
    nz = torch.fft.rfftfreq(mesh, 1.0 / mesh, dtype=torch.float64, device=dev)
    k2 = ((n * n)[:, None, None] + (n * n)[None, :, None] + (nz * nz)[None, None, :]) * (2.0 * math.pi / float(box_size)) ** 2
    herm = 2.0 - ((nz == 0) | (2.0 * nz == float(mesh))).to(torch.float64)
    return (gaussian_filter(mesh, box_size, smoothing, dev) if smoothing > 0 else None), k2 * herm


def _smoothed_frame(pos: torch.Tensor, box_size: float, mesh: int, order: int, threshold_units: str, kernel, k2w):
    """One frame ``pos [N, 3]`` of :func:`smoothed_contrast`: ``(field [M, M, M], sigma0, sigma1)``."""
    delta = ops.grid_contrast(ops.mass_assign(pos, box_size, mesh, order), pos.shape[0])
    modes = torch.fft.rfftn(delta)
    if kernel is not None:
        modes = modes * kernel
        delta = torch.fft.irfftn(modes, s=(mesh,) * 3)
    sigma0 = torch.sqrt((delta * delta).mean())
    sigma1 = torch.sqrt((k2w * (modes.real * modes.real + modes.imag * modes.imag)).sum()) / float(mesh) ** 3
    return (delta / sigma0 if threshold_units == "sigma" else delta).contiguous(), sigma0, sigma1


def smoothed_contrast(pos: torch.Tensor, box_size: float, mesh: int, smoothing: float, order: int = 2,
                      threshold_units: str = "sigma"):
    """The field whose excursion sets :func:`minkowski_functionals` counts, for frames ``pos [F, N, 3]``, on the device:
    ``(field [F, M, M, M], sigma0 [F], sigma1 [F])`` in float64.  The exact deposit (``ops.mass_assign``,
    ``ops.grid_contrast``), smoothed with the Gaussian ``exp(-|k|^2 R^2 / 2)`` of ``losses.gaussian_filter`` between
    ``torch.fft.rfftn`` and ``irfftn`` (``smoothing = 0``: no FFT for the field); ``sigma0^2`` is the mean square of the
    smoothed field and ``sigma1^2`` that of its gradient, ``sum |k|^2 |u_k|^2`` over the modes with the Hermitian
    weights of the half axis.  With ``"sigma"`` the field is divided by its own ``sigma0``.  No host synchronisation."""
    kernel, k2w = _minkowski_filters(mesh, box_size, smoothing, pos.device)
    parts = [_smoothed_frame(pos[f], box_size, mesh, order, threshold_units, kernel, k2w) for f in range(pos.shape[0])]
    return tuple(torch.stack([p[i] for p in parts]) for i in range(3))


def minkowski_counts_on_device(frames: torch.Tensor, box_size: float, mesh: int, smoothing: float, nu, order: int = 2,
                               threshold_units: str = "sigma") -> torch.Tensor:
    """What a Minkowski estimate of ``frames [F, N, 3]`` brings back from the device, as one int64 tensor ``[F, 4 nt + 2]``:
    the counts of ``ops.excursion_counts`` on the frames of :func:`smoothed_contrast`, then the bits of ``sigma0`` and
    ``sigma1``.  One frame's field and transforms are alive at a time.  No host synchronisation."""
    kernel, k2w = _minkowski_filters(mesh, box_size, smoothing, frames.device)
    out = []
    for f in range(frames.shape[0]):
        field, s0, s1 = _smoothed_frame(frames[f], box_size, mesh, order, threshold_units, kernel, k2w)
        out.append(torch.cat([ops.excursion_counts(field, nu).reshape(-1), torch.stack([s0, s1]).view(torch.int64)]))
    return torch.stack(out)


def minkowski_on_host(packed: torch.Tensor, nt: int):
    """``(counts [F, 4, nt], sigma0 [F], sigma1 [F])`` from the host copy of :func:`minkowski_counts_on_device`."""
    sig = packed[:, 4 * nt:].contiguous().view(torch.float64)
    return packed[:, :4 * nt].reshape(-1, 4, nt), sig[:, 0].clone(), sig[:, 1].clone()


def _minkowski_result(counts, s0, s1, mesh: int, box_size: float, nu, threshold_units: str) -> Dict:
    out = minkowski_from_counts(counts, mesh, box_size)
    out.update(sigma0=s0, sigma1=s1, thresholds=torch.tensor(nu, dtype=torch.float64))
    if threshold_units == "sigma":
        g = gaussian_minkowski(nu, s0, s1)
        out.update({"gaussian_v%d" % d: g["v%d" % d] for d in range(4)})
    return out


def minkowski_functionals(pos: torch.Tensor, box_size: float, mesh: int, smoothing: float, thresholds=None, order: int = 2,
                          threshold_units: str = "sigma") -> Dict:
    """The Minkowski functionals of the excursion sets of the density field of ``pos [N, 3]`` (or of every frame of ``[T,
    N, 3]``): deposited on a ``mesh^3`` grid with ``order`` (1 = NGP, 2 = CIC, 3 = TSC), smoothed with a Gaussian of
    length ``smoothing`` (in the units of ``box_size``; 0: the raw mesh) and cut at ``thresholds`` (default
    :func:`default_minkowski_thresholds`) -- with ``threshold_units="sigma"`` in units of the smoothed field's own
    standard deviation (the field is divided by it on the device), with ``"contrast"`` values of delta.  Returns the dict
    of :func:`minkowski_from_counts` (``[nt]`` or ``[T, nt]``) plus ``sigma0``, ``sigma1`` (of the smoothed contrast),
    ``thresholds`` and, with ``"sigma"``, the curves ``gaussian_v0`` .. ``gaussian_v3`` of :func:`gaussian_minkowski`
    for that ``sigma0`` and ``sigma1``.  The counts are exact integers of the field the device made; everything is
    computed on the device of ``pos`` without a host synchronisation and comes back in one transfer."""
    what = "minkowski_functionals"
    mesh, nu = _check_minkowski_arguments(what, box_size, mesh, smoothing, thresholds, order, threshold_units)
    if not torch.is_tensor(pos):
        raise ValueError(f"{what}: pos must be a tensor, got {type(pos).__name__}")
    frames = _frames3(pos, "pos", what)
    packed = minkowski_counts_on_device(_f32_frames(frames, "pos", what), box_size, mesh, smoothing, nu, order,
                                        threshold_units).cpu()                          # the one transfer
    counts, s0, s1 = minkowski_on_host(packed, len(nu))
    if pos.dim() == 2:
        counts, s0, s1 = counts[0], s0[0], s1[0]
    return _minkowski_result(counts, s0, s1, mesh, box_size, nu, threshold_units)


def rollout_minkowski(rollout_data: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], box_size: float,
                      mesh: int, smoothing: float, thresholds=None, order: int = 2, threshold_units: str = "sigma",
                      frames: Optional[Sequence[int]] = None) -> Dict:
    """Minkowski functionals of a rollout against the truth, for the dicts ``rollout.rollout`` returns (``Coordinates [T,
    N, 3]``): whether the predicted cosmic web has the volume, the surface, the curvature and the connectivity of the
    true one at every density threshold.  ``frames``: the frame numbers to judge (default: every frame both hold).  Per
    selected frame (CPU, ``[F, nt]``):

    * ``v0_pred`` .. ``v3_pred``, ``v0_true`` .. ``v3_true`` and ``v0_difference`` .. ``v3_difference`` (pred - true);
    * ``euler_pred``, ``euler_true`` (int64) and ``counts_pred``, ``counts_true`` (int64 ``[F, 4, nt]``);
    * ``sigma0_pred``, ``sigma0_true``, ``sigma1_pred``, ``sigma1_true`` (``[F]``);
    * with ``threshold_units="sigma"``: ``gaussian_v0_true`` .. ``gaussian_v3_true``,

    plus ``frames`` and ``thresholds``.  With ``"sigma"`` each side is cut in units of its own standard deviation.  No
    host synchronisation per frame; one transfer at the end."""
    what = "rollout_minkowski"
    mesh, nu = _check_minkowski_arguments(what, box_size, mesh, smoothing, thresholds, order, threshold_units)
    pc, tc, sel = _rollout_frames(rollout_data, ground_truth, frames, what)
    packed = torch.stack([minkowski_counts_on_device(_f32_frames(x, "Coordinates", what), box_size, mesh, smoothing, nu,
                                                     order, threshold_units) for x in (pc, tc)]).cpu()   # the one transfer
    p = _minkowski_result(*minkowski_on_host(packed[0], len(nu)), mesh, box_size, nu, threshold_units)
    t = _minkowski_result(*minkowski_on_host(packed[1], len(nu)), mesh, box_size, nu, threshold_units)
    out = {"frames": sel, "thresholds": t["thresholds"]}
    for key in ("v0", "v1", "v2", "v3"):
        out.update({key + "_pred": p[key], key + "_true": t[key], key + "_difference": p[key] - t[key]})
        if threshold_units == "sigma":
            out["gaussian_" + key + "_true"] = t["gaussian_" + key]
    for key in ("euler", "counts", "sigma0", "sigma1"):
        out.update({key + "_pred": p[key], key + "_true": t[key]})
    return out
